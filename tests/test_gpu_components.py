"""GPU tests of the lesion-wise detection scores: ops.label_components, ops.component_areas, ops.lesion_match and
functions.LesionScores against their numpy restatements (tests/components_ref.py), and the launcher's `-p -m detect` with
detect.lesionwise.  Run with `pytest -m gpu` on an MI355X.

Everything here is integers: labels are canonical (numbered by first pixel), so every comparison is torch.equal / array_equal, and
every call's error word is 0.  The tile of the labelling kernel is 32 rows x 64 columns; the shapes put pixels on every side of its
seams and corners."""
import math
import os

import numpy as np
import pytest
import torch

from run_helpers import read_csv, run_launcher, write_config
import components_ref as R
import prior_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONN = [4, 8]


def _label(x, threshold=None, connectivity=8):
    from hipops import ops
    labels, counts, err = ops.label_components(torch.as_tensor(x).to(DEV), threshold, connectivity)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.shape == tuple(np.shape(x)) and counts.shape == (np.shape(x)[0],)
    assert int(err) == 0, "error word %d" % int(err)
    return labels, counts


def _check(x, connectivity, threshold=None, what=""):
    """Labels, counts and areas of x against the restatement; -> (labels, counts) on the device."""
    from hipops import ops
    want_l, want_c = R.label(x, threshold, connectivity)
    labels, counts = _label(x, threshold, connectivity)
    assert np.array_equal(counts.cpu().numpy(), want_c), (what, counts.cpu().tolist(), want_c.tolist())
    assert np.array_equal(labels.cpu().numpy(), want_l), what
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    areas = ops.component_areas(labels, counts, connectivity, err)
    N, H, W = want_l.shape
    assert areas.shape == (N, R.cap(H, W, connectivity)) and areas.dtype == torch.int32 and int(err) == 0
    assert np.array_equal(areas.cpu().numpy(), R.areas(want_l, want_c, connectivity)), what          # zeros past counts[n] included
    return labels, counts


# ------------------------------------------------------------------------------------------------ labelling: small shapes
def _runs(n):
    """Alternating runs of growing length: 1 on, 1 off, 2 on, 2 off, ..."""
    out, k, on = [], 1, 1
    while len(out) < n:
        out += [on] * k
        k, on = k + (1 - on), 1 - on
    return np.array(out[:n], dtype=np.uint8)


@pytest.mark.parametrize("connectivity", CONN)
def test_label_shapes_below_one_tile(connectivity):
    _check(np.ones((1, 1, 1), np.uint8), connectivity, what="one foreground pixel")
    _check(np.zeros((1, 1, 1), np.uint8), connectivity, what="one background pixel")
    _check(_runs(37).reshape(1, 1, 37) * 200, connectivity, what="a row of runs")          # any non-zero byte is foreground
    _check(_runs(37).reshape(1, 37, 1), connectivity, what="a column of runs")
    g = np.random.default_rng(8)
    for d in (0.3, 0.5, 0.7):
        _check((g.uniform(size=(1, 8, 8)) < d).astype(np.uint8), connectivity, what="8 x 8 at %g" % d)


# ------------------------------------------------------------------------------------------------ labelling: tiles and seams
SHAPES = [(2, 33, 65), (1, 64, 128), (3, 96, 160)]          # ragged tiles and two images; 2 x 2 whole tiles; 3 x 3 tiles (the last column ragged)
PATTERNS = ["ones", "zeros", "checkerboard", "spiral", "comb", "rings", "bern0.407", "bern0.5", "bern0.593"]


def _pattern(name, shape):
    N, H, W = shape
    if name == "ones":
        return np.ones(shape, np.uint8)
    if name == "zeros":
        return np.zeros(shape, np.uint8)
    if name.startswith("bern"):
        g = np.random.default_rng(1000 + H + int(1000 * float(name[4:])))
        x = (g.uniform(size=shape) < float(name[4:])).astype(np.uint8)
        if N > 1:          # image 0 ends in foreground and image 1 begins with it: nothing joins across images
            x[0, -1, -4:] = 1
            x[1, 0, :4] = 1
        return x
    one = getattr(R, name)(H, W)
    # further images: the pattern mirrored, then turned upside down - first pixels and merge orders differ
    return np.stack([(one, one[:, ::-1], one[::-1])[n % 3] for n in range(N)]).copy()


@pytest.mark.parametrize("connectivity", CONN)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_label_patterns_across_tiles(name, shape, connectivity):
    x = _pattern(name, shape)
    labels, counts = _check(x, connectivity, what="%s %s" % (name, shape))
    N, H, W = shape
    if name == "ones":
        assert counts.cpu().tolist() == [1] * N
    if name == "checkerboard":
        assert counts.cpu().tolist() == [R.cap(H, W, 4) if connectivity == 4 else 1] * N
    if name == "spiral":
        assert counts.cpu().tolist() == [1] * N          # one component, the longest parent chains
    again = _label(x, None, connectivity)
    assert torch.equal(again[0], labels) and torch.equal(again[1], counts), "two runs differ"


PAIRS = [
    ("corner NW/SE", ((31, 63), (32, 64)), 1),          # across the four-tile corner, both diagonals
    ("corner NE/SW", ((31, 64), (32, 63)), 1),
    ("vertical seam NE/SW", ((10, 64), (11, 63)), 1),   # a left-column pixel's SW neighbour, away from any corner
    ("vertical seam NW/SE", ((10, 63), (11, 64)), 1),
    ("vertical seam W/E", ((10, 63), (10, 64)), 0),
    ("horizontal seam N/S", ((31, 20), (32, 20)), 0),
    ("horizontal seam diagonal", ((31, 20), (32, 21)), 1),
]


@pytest.mark.parametrize("connectivity", CONN)
def test_label_two_pixels_across_a_seam(connectivity):
    for what, pixels, diagonal in PAIRS:
        x = np.zeros((1, 64, 128), np.uint8)
        for p in pixels:
            x[0][p] = 1
        labels, counts = _check(x, connectivity, what=what)
        assert int(counts[0]) == (2 if diagonal and connectivity == 4 else 1), what


FULL = {4: 0.593, 8: 0.407}          # the percolation thresholds: the largest and most ragged components


@pytest.mark.parametrize("connectivity", CONN)
def test_label_full_size_at_the_percolation_threshold(connectivity):
    g = np.random.default_rng(512 + connectivity)
    x = (g.uniform(size=(1, 512, 512)) < FULL[connectivity]).astype(np.uint8)
    labels, counts = _check(x, connectivity, what="512 x 512")
    assert int(counts[0]) > 1000
    again = _label(x, None, connectivity)
    assert torch.equal(again[0], labels) and torch.equal(again[1], counts), "two runs differ"


@pytest.mark.parametrize("connectivity", CONN)
def test_label_float_route(connectivity):
    g = np.random.default_rng(3)
    s = g.uniform(0, 1, (2, 33, 65)).astype(np.float32)
    thr = float(s[0, 5, 7])          # a value exactly at the threshold is foreground
    s[1, 3, 3] = s[0, 32, 64] = np.nan          # a NaN is background
    s[1, 4, 4] = np.inf
    labels, counts = _check(s, connectivity, threshold=thr, what="float route")
    assert int(labels[0, 5, 7]) > 0 and int(labels[1, 3, 3]) == 0 and int(labels[0, 32, 64]) == 0 and int(labels[1, 4, 4]) > 0
    with np.errstate(invalid="ignore"):
        mask = (s >= np.float32(thr)).astype(np.uint8)
    by_mask = _label(mask, None, connectivity)
    assert torch.equal(by_mask[0], labels) and torch.equal(by_mask[1], counts)
    bools = _label(mask.astype(bool), None, connectivity)
    assert torch.equal(bools[0], labels)
    _check(s, connectivity, threshold=0.0, what="threshold 0: everything but the NaNs")
    _check(s, connectivity, threshold=2.0, what="a threshold above every finite score")


@pytest.mark.parametrize("connectivity", CONN)
def test_label_back_to_back_calls_share_no_state(connectivity):
    """Several patterns of one shape, one call after the other with nothing read in between, then compared: a call leaves nothing
    in a workspace that the next one could pick up."""
    shape = (3, 96, 160)
    names = ["spiral", "bern0.593", "ones", "checkerboard", "zeros", "comb", "bern0.407", "rings"]
    from hipops import ops
    got = [ops.label_components(torch.as_tensor(_pattern(n, shape)).to(DEV), None, connectivity) for n in names]
    for n, (labels, counts, err) in zip(names, got):
        want_l, want_c = R.label(_pattern(n, shape), None, connectivity)
        assert int(err) == 0 and np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(counts.cpu().numpy(), want_c), n


def test_operators_refuse_bad_arguments():
    from hipops import ops
    x = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="connectivity=6 must be 4 or 8"):
        ops.label_components(x, None, 6)
    with pytest.raises(RuntimeError, match="empty"):
        ops.label_components(x[:0])
    with pytest.raises(RuntimeError, match="torch.uint8"):
        ops.label_components(x.float())
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.label_components(x, 0.5)
    with pytest.raises(RuntimeError, match="NaN"):
        ops.label_components(x.float(), float("nan"))
    labels, counts, _ = ops.label_components(x)
    areas = ops.component_areas(labels, counts)
    acc = ops.new_lesion_acc(DEV, 1)[0]
    with pytest.raises(RuntimeError, match="different shapes"):
        ops.lesion_match(labels, counts, areas, labels[:, :4], counts, 1, acc)
    with pytest.raises(RuntimeError, match="min_size=0"):
        ops.lesion_match(labels, counts, areas, labels, counts, 0, acc)
    with pytest.raises(RuntimeError, match="torch.int32"):
        ops.component_areas(labels.long(), counts)
    assert not bool(acc.any())
    # a label beyond the cap of the connectivity named is dropped and flagged, never written
    board = torch.as_tensor(R.checkerboard(8, 8)[None]).to(DEV)
    l4, c4, _ = ops.label_components(board, None, 4)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    a8 = ops.component_areas(l4, c4, 8, err)
    assert int(err) == 8 and a8.shape == (1, 16) and a8.cpu().tolist() == [[1] * 16]


# ------------------------------------------------------------------------------------------------ matching and scores
def _scores(maps, gt, thresholds, min_size, connectivity):
    from functions import LesionScores
    acc = LesionScores(thresholds, min_size, connectivity)
    acc.update(torch.as_tensor(maps).to(DEV), torch.as_tensor(gt).to(DEV))
    return acc


def _rows(result):
    return [[r[k] for k in R.ACC] for r in result]


def _same_scores(result, want_rows):
    assert _rows(result) == want_rows
    for r, w in zip(result, want_rows):
        assert r["err"] == 0
        for k, v in R.scores(w).items():
            assert (math.isnan(r[k]) and math.isnan(v)) or r[k] == v, (k, r[k], v)


_disc_cache = {}


def _disc_case():
    """Synthetic discs as the ground truth against a noisy smooth map of them, (4, 96, 160), shared by the tests below."""
    if not _disc_cache:
        from dataio import synthetic_lesions
        H, W = 96, 160
        g = np.random.default_rng(41)
        gt, maps = [], []
        for n in range(4):
            delta, mask = synthetic_lesions(5, n, W, 3, 14.0, 0.8)
            delta, mask = delta[0, :H].numpy(), mask[0, :H].numpy()          # the upper part of a square slice: some discs are cut
            gt.append(mask)
            maps.append((0.25 * delta * (n != 2) + np.abs(g.normal(0, 0.04, (H, W)))).astype(np.float32))          # slice 2: lesions missed
        _disc_cache["v"] = (np.stack(maps), np.stack(gt))
    return _disc_cache["v"]


THRESHOLDS = [0.0, 0.05, 0.1, 0.15, 0.3]


@pytest.mark.parametrize("connectivity", CONN)
def test_lesion_scores_on_synthetic_discs(connectivity):
    maps, gt = _disc_case()
    want = R.lesion_scores(maps, gt, THRESHOLDS, 3, connectivity)
    assert want[0][3] == 4 and want[0][2] == want[0][1] > 4 and 0 < want[2][2] < want[2][1] and want[2][4] > 0          # the case has hits, misses and false alarms
    result = _scores(maps, gt, THRESHOLDS, 3, connectivity).result()
    assert [r["threshold"] for r in result] == THRESHOLDS
    _same_scores(result, want)
    assert _rows(_scores(maps, gt, THRESHOLDS, 3, connectivity).result()) == want, "two runs differ"
    # two updates equal one update on the concatenation
    acc = _scores(maps[:1], gt[:1], THRESHOLDS, 3, connectivity)
    acc.update(torch.as_tensor(maps[1:]).to(DEV), torch.as_tensor(gt[1:, None]).to(DEV))          # (N, 1, H, W) labels too
    _same_scores(acc.result(), want)


def _draw(H, W, boxes):
    x = np.zeros((1, H, W), np.uint8)
    for y0, y1, x0, x1 in boxes:
        x[0, y0:y1, x0:x1] = 1
    return x


def test_lesion_match_min_size_bridges_and_doubles():
    gt = _draw(40, 140, [(4, 12, 4, 12), (4, 12, 100, 108)])          # two lesions of 64 pixels, in different tiles
    # a blob of exactly 12 pixels on lesion 1: kept at min_size 11 and 12, dropped at 13
    blob = _draw(40, 140, [(6, 8, 2, 8)]).astype(np.float32)
    for min_size, kept in ((11, 1), (12, 1), (13, 0)):
        want = R.lesion_scores(blob, gt, [0.5], min_size, 8)
        assert want == [[1, 2, kept, kept, 0, 8 * kept, 12 * kept, 128]]
        _same_scores(_scores(blob, gt, [0.5], min_size, 8).result(), want)
    # one blob bridging both lesions detects both and is one matched component
    bridge = _draw(40, 140, [(8, 10, 10, 102)]).astype(np.float32)
    want = R.lesion_scores(bridge, gt, [0.5], 1, 8)
    assert want == [[1, 2, 2, 1, 0, 8, 184, 128]]
    _same_scores(_scores(bridge, gt, [0.5], 1, 8).result(), want)
    # two blobs on one lesion detect it once and are two matched components; a third one elsewhere is false
    doubles = _draw(40, 140, [(4, 6, 4, 6), (9, 11, 9, 11), (30, 33, 60, 70)]).astype(np.float32)
    want = R.lesion_scores(doubles, gt, [0.5], 1, 8)
    assert want == [[1, 2, 1, 3, 1, 8, 38, 128]]
    res = _scores(doubles, gt, [0.5], 1, 8).result()
    _same_scores(res, want)
    assert res[0]["sensitivity"] == 0.5 and res[0]["fp_per_slice"] == 1.0 and res[0]["precision"] == 2 / 3


def test_lesion_scores_empty_ground_truth_and_empty_prediction():
    maps, gt = _disc_case()
    none = np.zeros_like(gt)
    want = R.lesion_scores(maps, none, [0.1], 1, 8)
    assert want[0][1] == want[0][2] == want[0][7] == 0 and want[0][3] == want[0][4] > 0
    res = _scores(maps, none, [0.1], 1, 8).result()
    _same_scores(res, want)
    assert math.isnan(res[0]["sensitivity"]) and math.isnan(res[0]["f1"]) and res[0]["precision"] == 0.0 and res[0]["dice_filtered"] == 0.0
    want = R.lesion_scores(maps, gt, [10.0], 1, 8)          # nothing reaches the threshold
    assert want[0][3] == want[0][6] == 0 and want[0][1] > 0
    res = _scores(maps, gt, [10.0], 1, 8).result()
    _same_scores(res, want)
    assert res[0]["sensitivity"] == 0.0 and math.isnan(res[0]["precision"]) and math.isnan(res[0]["f1"]) and res[0]["fp_per_slice"] == 0.0
    res = _scores(np.zeros_like(maps), none, [10.0], 1, 8).result()          # neither
    assert _rows(res) == [[4, 0, 0, 0, 0, 0, 0, 0]] and math.isnan(res[0]["dice_filtered"])


def test_lesion_match_accumulates_into_acc():
    from hipops import ops
    maps, gt = _disc_case()
    pl, pc = _label(maps, 0.1, 8)
    gl, gc = _label(gt, None, 4)          # the ground truth under another connectivity: its cap is the larger one
    areas = ops.component_areas(pl, pc, 8)
    acc = ops.new_lesion_acc(DEV, 2)
    ops.lesion_match(pl, pc, areas, gl, gc, 2, acc[1])
    once = R.match(R.label(maps, 0.1, 8)[0], R.label(gt, None, 4)[0], 2)
    assert acc.cpu().tolist() == [[0] * 8, once]
    ops.lesion_match(pl, pc, areas, gl, gc, 2, acc[1])
    assert acc.cpu().tolist() == [[0] * 8, [2 * v for v in once]]


# ------------------------------------------------------------------------------------------------ the launcher
LESIONWISE = dict(thresholds=[0, 0.02, 0.1], min_size=2, connectivity=8)


def test_launcher_writes_lesion_scores_and_a_seed_repeats_every_byte(tmp_path):
    from dataio import get_data_loader
    save = os.path.join(str(tmp_path), "run")
    run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), P.prior_run_config(save)), "-p")
    ckpt = os.path.join(save, "study", "version_0", "ckpt-epoch=0000-total_loss=0.00.ckpt")
    raw = P.prior_run_config(save, resume_checkpoint=ckpt)
    lesions = dict(n=2, radius=5, contrast=0.8)
    raw["detect"] = dict(n_slices=0, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0,
                         against="image", weight="mask", labels={"synthetic": lesions}, lesionwise=LESIONWISE)
    cfg = write_config(os.path.join(str(tmp_path), "detect.json"), raw)
    files = {}
    for version in (1, 2):
        out = run_launcher(cfg, "-p", "-m", "detect")
        assert "Detection results are saved" in out
        rdir = os.path.join(save, "study", "version_%d" % version)
        mine = sorted(f for f in os.listdir(rdir) if f.startswith("detect"))
        assert mine == ["detect.csv", "detect_0000.png", "detect_0001.png", "detect_lesions.csv", "detect_result.csv"]
        files[version] = {f: open(os.path.join(rdir, f), "rb").read() for f in mine}
    assert files[1] == files[2], "the same seed writes the same bytes"
    rdir = os.path.join(save, "study", "version_1")
    header, rows = read_csv(os.path.join(rdir, "detect_lesions.csv"))
    assert header == ["threshold", "slices", "gt_lesions", "gt_detected", "sensitivity", "pred_components", "pred_false", "fp_per_slice",
                      "precision", "f1", "dice_filtered"]
    assert [r[0] for r in rows] == ["0", "0.02", "0.1"]          # one row per threshold
    # the loader's own labels, under the restatement
    batches = list(get_data_loader(mode="test", dataset_name="synthetic", root_dir_path=None, batch_size=4, num_workers=0, image_size=32,
                                   n_samples=4, seed=raw["run"]["seed"], lesions=lesions))
    gt = torch.cat([b["label"] for b in batches])[:, 0].numpy()
    n_slices, H, W = gt.shape
    positives = [int(r[5]) for r in read_csv(os.path.join(rdir, "detect.csv"))[1]]
    assert positives == gt.reshape(n_slices, -1).sum(1).tolist()          # these are the slices the launcher scored
    _, counts = R.label(gt, None, 8)
    G = int(gt.sum())
    for r in rows:
        assert int(r[1]) == n_slices == 4 and int(r[2]) == int(counts.sum())
        assert 0 <= int(r[3]) <= int(r[2]) and 0 <= int(r[6]) <= int(r[5])
    # threshold 0 takes every pixel: one component per slice, every lesion found; these follow from the definitions alone
    zero = rows[0]
    assert int(zero[5]) == n_slices and int(zero[3]) == int(zero[2])
    assert int(zero[6]) == int((counts == 0).sum())
    assert float(zero[10]) == 2 * G / (n_slices * H * W + G)
    assert float(zero[4]) == 1.0 and float(zero[7]) == int(zero[6]) / n_slices
    # the pixel-wise files are those of the run without the section
    del raw["detect"]["lesionwise"]
    run_launcher(write_config(os.path.join(str(tmp_path), "plain.json"), raw), "-p", "-m", "detect")
    rdir3 = os.path.join(save, "study", "version_3")
    plain = sorted(f for f in os.listdir(rdir3) if f.startswith("detect"))
    assert plain == ["detect.csv", "detect_0000.png", "detect_0001.png", "detect_result.csv"]          # no detect_lesions.csv
    for f in plain:
        assert open(os.path.join(rdir3, f), "rb").read() == files[1][f], f
