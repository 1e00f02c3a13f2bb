"""GPU tests of anomaly detection with the code prior: ops.anomaly_map, ops.score_histogram and ops.detection_scores against their
restatements (tests/detect_ref.py), PriorTrainer.detect on TINY_VQGAN with the p64 GPT, and the launcher's `-p -m detect`.  Run
with `pytest -m gpu` on an MI355X.

Tolerances.  anomaly_map: the project's gate - its distance from the float64 restatement is at most twice the fp32 restatement's
(relative L2).  score_histogram: integer counts, bit-equal to np.bincount of the restated keys.  detection_scores: rtol 1e-10
against the sort-based restatement (65 536 double additions at 2^-53 each, with margin); the hand cases are exact."""
import math
import os

import numpy as np
import pytest
import torch

from run_helpers import read_csv, run_launcher, write_config
import detect_ref as D
import gpt_ref as G
import prior_ref as P
from test_gpu_vqgan_blocks import _gate          # the gate rule, written once

pytestmark = pytest.mark.gpu
DEV = "cuda"
BINS = 65536


# ------------------------------------------------------------------------------------------------ anomaly_map
# (N, H, W, C, h, w, sigma, with a cell mask).  A workgroup owns a 32 x 64 tile of the map; the halo is ceil(3 sigma) pixels.
MAP_CASES = [
    (1, 8, 8, 1, 2, 2, 0.5, True),             # smaller than one tile: the halo lies beyond every edge
    (2, 36, 60, 1, 3, 5, 1.0, True),           # ragged tiles, factor 12, two images: the batch offset
    (1, 64, 64, 3, 16, 16, 2.0, True),         # the mean over three channels, K = 13
    (1, 96, 160, 1, 6, 10, 4.0, True),         # K = 25, the widest halo sigma <= 4 asks for; 3 x 3 tiles
    (1, 36, 60, 1, 3, 5, 0.0, True),           # no blur
    (1, 36, 60, 1, 3, 5, 1.0, False),          # no cell mask: no up-sampling
]
_map_cache = {}


def _map_inputs(case):
    N, H, W, C, h, w, sigma, masked = case
    g = torch.Generator().manual_seed(1000 + H + 7 * W + C)
    a, b = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    mask = (torch.rand(N, h, w, generator=g) < 0.5).to(torch.uint8) * 3 if masked else None          # any non-zero byte is set
    return a, b, mask


def _map_refs(case):
    if case not in _map_cache:
        a, b, mask = _map_inputs(case)
        _map_cache[case] = (D.anomaly_map_ref(a, b, mask, case[6], torch.float64), D.anomaly_map_ref(a, b, mask, case[6], torch.float32))
    return _map_cache[case]


def _run_map(a, b, mask, sigma):
    from hipops import ops
    return ops.anomaly_map(a.to(DEV), b.to(DEV), None if mask is None else mask.to(DEV), sigma)


@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: "N%d_%dx%d_C%d_h%dw%d_s%g_%s" % (c[:7] + ("mask" if c[7] else "nomask",)))
def test_anomaly_map_against_float64(case):
    a, b, mask = _map_inputs(case)
    truth, ref32 = _map_refs(case)
    got = _run_map(a, b, mask, case[6])
    assert got.shape == truth.shape and got.dtype == torch.float32
    _gate(got.cpu(), truth, ref32, "anomaly_map %s" % (case,))
    assert torch.equal(_run_map(a, b, mask, case[6]), got), "two runs differ"
    # channels_last inputs are the same tensor
    cl = torch.channels_last
    assert torch.equal(_run_map(a.contiguous(memory_format=cl), b.contiguous(memory_format=cl), mask, case[6]), got)


def test_anomaly_map_all_zero_mask_is_exactly_zero():
    a, b, mask = _map_inputs(MAP_CASES[1])
    got = _run_map(a, b, torch.zeros_like(mask), 1.0)
    assert got.shape == (2, 36, 60) and not bool(got.any())
    # and a mask of all ones is the plain blurred residual
    ones, plain = _run_map(a, b, torch.ones_like(mask), 1.0), _run_map(a, b, None, 1.0)
    assert torch.equal(ones, plain)
    # forward only: an input on the tape leaves no tape behind
    from hipops import ops
    assert not ops.anomaly_map(a.to(DEV).requires_grad_(True), b.to(DEV), mask.to(DEV), 1.0).requires_grad


def test_anomaly_map_refuses_what_the_tile_cannot_hold():
    a, b, mask = _map_inputs(MAP_CASES[1])
    with pytest.raises(RuntimeError, match="K=37 taps.*at most 33"):          # sigma 6: a halo of 18 pixels
        _run_map(a, b, mask, 6.0)
    _run_map(a, b, mask, 5.33)                                                 # K = 33: the widest
    with pytest.raises(RuntimeError, match="integer multiples of the cell grid h=5, w=5"):
        _run_map(a, b, torch.ones(2, 5, 5, dtype=torch.uint8), 1.0)
    with pytest.raises(RuntimeError, match="torch.uint8"):
        _run_map(a, b, torch.ones(2, 3, 5), 1.0)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        _run_map(a, b[:, :, :30], mask, 1.0)
    with pytest.raises(RuntimeError, match="empty"):
        _run_map(a[:0], b[:0], mask[:0], 1.0)


# ------------------------------------------------------------------------------------------------ score_histogram
def _bincount(scores, labels):
    keys, lab = D.keys_ref(scores), (np.asarray(labels).reshape(-1) != 0).astype(np.int64)
    ok = keys >= 0
    h = np.bincount(lab[ok] * BINS + keys[ok], minlength=2 * BINS).reshape(2, BINS)
    return h, int((~ok).sum())


def _histogram(scores, labels, hist=None, err=None):
    from hipops import ops
    if hist is None:
        hist, err = ops.new_score_histogram(DEV)
    ops.score_histogram(torch.as_tensor(scores).to(DEV), torch.as_tensor(labels).to(DEV), hist, err)
    return hist, err


def _random_scores(n, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0, 2, n).astype(np.float32), (g.uniform(0, 1, n) < 0.3).astype(np.uint8) * 7


@pytest.mark.parametrize("n", [1, 255, 4097, 2 ** 20])
def test_score_histogram_equals_bincount(n):
    s, y = _random_scores(n, n)
    want, bad = _bincount(s, y)
    hist, err = _histogram(s, y)
    assert hist.dtype == torch.long and np.array_equal(hist.cpu().numpy(), want) and int(err) == bad == 0
    assert int(hist.sum()) == n
    if n > 1:          # two calls on halves accumulate to one call on the whole; and a second run gives the same counts
        h2, e2 = _histogram(s[:n // 2], y[:n // 2])
        _histogram(s[n // 2:], y[n // 2:], h2, e2)
        assert torch.equal(h2, hist) and int(e2) == 0
        # a view that starts 4 bytes into the buffer: the one-score-per-load route
        dev_s, dev_y = torch.as_tensor(s).to(DEV), torch.as_tensor(y).to(DEV)
        from hipops import ops
        h3, e3 = ops.new_score_histogram(DEV)
        ops.score_histogram(dev_s[1:], dev_y[1:], h3, e3)
        assert np.array_equal(h3.cpu().numpy(), _bincount(s[1:], y[1:])[0])


def test_score_histogram_constant_map_fills_one_bin():
    n = 2 ** 20
    for value in (0.0, 0.37):          # outside every window (key 0) and inside it
        s = np.full(n, value, dtype=np.float32)
        y = (np.arange(n) % 5 == 0).astype(np.uint8)
        hist, err = _histogram(s, y)
        want, _ = _bincount(s, y)
        assert np.array_equal(hist.cpu().numpy(), want) and int(err) == 0
        key = int(D.keys_ref(s[:1])[0])
        assert int(hist[0, key]) + int(hist[1, key]) == n and int(hist[1, key]) == int(y.sum())


def test_score_histogram_wide_range_leaves_the_window():
    """Scores over 60 exponents: most keys lie outside a workgroup's 24-exponent LDS window and go to the global counters."""
    g = np.random.default_rng(3)
    n = 50000
    s = (2.0 ** g.uniform(-40, 20, n)).astype(np.float32)
    y = (g.uniform(0, 1, n) < 0.5).astype(np.uint8)
    hist, err = _histogram(s, y)
    assert np.array_equal(hist.cpu().numpy(), _bincount(s, y)[0]) and int(err) == 0


def test_score_histogram_counts_what_it_cannot_bin():
    tiny = np.array([1], dtype=np.uint32).view(np.float32)[0]          # the smallest denormal
    s = np.array([np.nan, 0.5, np.inf, -1.0, -0.0, tiny, 1.5, -np.inf, -tiny, 0.0, 3e38], dtype=np.float32)
    y = np.array([1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1], dtype=np.uint8)
    want, bad = _bincount(s, y)
    assert bad == 5 and want.sum() == 6
    hist, err = _histogram(s, y)
    assert int(err) == 5 and np.array_equal(hist.cpu().numpy(), want)
    assert int(hist[1, 0]) == 1 and int(hist[0, 0]) == 2          # -0 (positive), the denormal and 0 (negatives) share key 0
    _histogram(s, y, hist, err)                                   # err accumulates too
    assert int(err) == 10 and np.array_equal(hist.cpu().numpy(), 2 * want)
    from hipops import ops
    assert float(ops.detection_scores(hist, err)[6]) == 0.0 and float(ops.detection_scores(hist)[6]) == 1.0


# ------------------------------------------------------------------------------------------------ detection_scores
def _scores(hist, err=None):
    from hipops import ops
    out = ops.detection_scores(torch.as_tensor(np.asarray(hist, dtype=np.int64)).to(DEV), err)
    assert out.dtype == torch.float64 and out.shape == (8,) and out.is_cuda
    return out.cpu().tolist()


def _empty():
    return np.zeros((2, BINS), dtype=np.int64)


def test_detection_scores_hand_cases():
    h = _empty()
    h[1, 0x7F00], h[0, 0x3000] = 5, 7                              # separable
    assert _scores(h) == [1.0, 1.0, 1.0, 1.0, 5.0, 7.0, 1.0, 0.0]
    h = _empty()
    h[0, 0x7F00], h[1, 0x3000] = 7, 5                              # reversed: the best Dice takes every pixel
    got = _scores(h)
    assert got[0] == 0.0 and got[1] == pytest.approx(5 / 12, rel=1e-14) and got[2] == 10 / 17 and got[3] == D.key_floor(0x3000) and got[4:6] == [5.0, 7.0]
    h = _empty()
    h[1, 0x4123], h[0, 0x4123] = 3, 9                              # one shared bin
    got = _scores(h)
    assert got[0] == 0.5 and got[1] == 0.25 and got[2] == 6 / 15 and got[3] == D.key_floor(0x4123)
    h = _empty()
    h[1, BINS - 1], h[0, 0] = 1, 1                                 # the two ends of the key range
    assert _scores(h)[:3] == [1.0, 1.0, 1.0]


def test_detection_scores_without_positives_or_negatives_are_nan():
    for lab in (0, 1):
        h = _empty()
        h[lab, 100], h[lab, 60000] = 4, 2
        got = _scores(h)
        assert all(math.isnan(v) for v in got[:4]) and got[4:] == [6.0 * lab, 6.0 * (1 - lab), 1.0, 0.0]
    got = _scores(_empty())
    assert all(math.isnan(v) for v in got[:4]) and got[4:6] == [0.0, 0.0]


_random_cache = {}


def _random_case():
    if not _random_cache:
        g = np.random.default_rng(17)
        n = 2 ** 20
        y = (g.uniform(0, 1, n) < 0.1).astype(np.uint8)
        s = (np.abs(g.normal(0, 0.2, n)) + 0.3 * y * g.uniform(0, 1, n)).astype(np.float32)          # positives score higher, with overlap
        _random_cache["v"] = (s, y, D.scores_sorted(D.keys_ref(s), y))
    return _random_cache["v"]


def test_detection_scores_of_a_million_pixels_against_the_sorted_restatement():
    s, y, want = _random_case()
    hist, err = _histogram(s, y)
    got = _scores(hist.cpu().numpy(), err)
    print("auroc %.12f ap %.12f dice %.12f at %.6g; the sorted restatement %.12f %.12f %.12f at %.6g" % (tuple(got[:4]) + tuple(want[:4])))
    assert 0.6 < want[0] < 1.0
    assert np.allclose(got[:3], want[:3], rtol=1e-10, atol=0) and got[3] == want[3] and got[4:6] == want[4:6] and got[6] == 1.0
    assert _scores(hist.cpu().numpy(), err) == got, "two runs differ"


def test_detection_scores_counts_near_2_to_the_40():
    """Products of two counts pass 2^64 and running sums pass 2^32: against exact rational arithmetic."""
    g = np.random.default_rng(23)
    h = _empty()
    bins = g.choice(BINS, size=40, replace=False)
    h[0, bins] = (2 ** 40 - g.integers(0, 2 ** 20, 40)) * (g.uniform(0, 1, 40) < 0.8)
    h[1, bins] = (2 ** 40 - g.integers(0, 2 ** 20, 40)) * (np.argsort(bins).argsort() > g.integers(0, 40, 40))          # more positives up high
    h[1, bins[0]] += 3
    want = D.scores_exact(h.tolist())
    got = _scores(h)
    assert want[4] > 2 ** 42 and want[5] > 2 ** 42 and 0.0 < want[0] < 1.0
    assert np.allclose(got[:3], want[:3], rtol=1e-10, atol=0) and got[3] == want[3] and got[4:6] == want[4:6]


def test_detection_scores_best_threshold_tie_goes_to_the_highest_bin():
    h = _empty()
    h[1, 300], h[0, 300], h[1, 200], h[0, 200] = 1, 1, 1, 3          # Dice 2/4 at bin 300 and 4/8 at bin 200
    got = _scores(h)
    assert got[2] == 0.5 and got[3] == D.key_floor(300)
    h = _empty()                                                      # the same tie across two threads' ranges and with large counts
    h[1, 40000], h[0, 40000], h[1, 150], h[0, 150] = 2 ** 40, 2 ** 40, 2 ** 40, 3 * 2 ** 40
    got = _scores(h)
    assert got[2] == 0.5 and got[3] == D.key_floor(40000)
    h[0, 150] -= 1                                                    # one pixel fewer: the lower bin now wins, by 1 part in 2^43
    assert _scores(h)[3] == D.key_floor(150) and D.scores_exact(h.tolist())[3] == D.key_floor(150)


# ------------------------------------------------------------------------------------------------ PriorTrainer.detect
_tr = {}


def _trainer():
    """test_gpu_prior_edit.py's tiny pair, built here: TINY_VQGAN (8 x 8 pictures, a 4 x 4 latent of 64 codes) and the p64 GPT."""
    if "tr" not in _tr:
        from networks import GPT, VQGAN
        from trainers import PriorTrainer
        torch.manual_seed(77)
        vqgan = VQGAN(**P.TINY_VQGAN)
        seed = P.SEEDS["p64"]
        torch.manual_seed(seed)
        gpt = G.init_gpt_(GPT(**P.gpt_kwargs("p64")), seed)
        _tr["tr"] = PriorTrainer(vqgan, gpt, device=DEV)
        _tr["image"] = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    return _tr["tr"], _tr["image"]


def _gen(seed=9):
    return torch.Generator(device=DEV).manual_seed(seed)


def test_detect_is_anomaly_map_of_edits_own_outputs():
    from hipops import ops
    tr, image = _trainer()
    nll = tr.token_nll({"image": image})
    thr = float(nll.median())
    kw = dict(n_candidates=3, temperature=1.0, top_k=16, top_p=0.95)
    ed = tr.edit({"image": image}, nll_threshold=thr, generator=_gen(), **kw)
    assert 0 < int(ed["cellmask"].sum()) < 32
    rows = torch.arange(2, device=DEV)
    for against, a, b in (("image", image, ed["composite"]), ("reconstruction", ed["recon"], ed["edit"])):
        for weight, mask in (("mask", ed["cellmask"]), ("none", None)):
            out = tr.detect({"image": image}, thr, sigma=1.0, against=against, weight=weight, generator=_gen(), **kw)
            assert sorted(out) == ["cellmask", "map", "n_resampled", "nll", "restored", "score"]
            assert torch.equal(out["map"], ops.anomaly_map(a, b, mask, 1.0)), (against, weight)
            assert out["map"].shape == (2, 8, 8) and bool(out["map"].any())
            assert torch.equal(out["restored"], b) and torch.equal(out["nll"], nll) and torch.equal(out["cellmask"], ed["cellmask"])
            assert torch.equal(out["score"], ed["scores"][rows, ed["best"]]) and out["score"].dtype == torch.float64
            assert torch.equal(out["n_resampled"], ed["cellmask"].reshape(2, -1).sum(1)) and out["n_resampled"].dtype == torch.long
    again = tr.detect({"image": image}, thr, sigma=1.0, generator=_gen(), **kw)
    first = tr.detect({"image": image}, thr, sigma=1.0, generator=_gen(), **kw)
    for k in again:
        assert torch.equal(again[k], first[k]), k
    assert tr.gpt.training
    # edit's results are what they were: the selector by mask gives the same dict as the selector by threshold
    by_mask = tr.edit({"image": image}, mask=(nll > thr).cpu().numpy(), generator=_gen(), **kw)
    assert sorted(by_mask) == sorted(ed) and all(torch.equal(by_mask[k], ed[k]) for k in ed)


def test_detect_leaves_an_untouched_slice_with_an_all_zero_map():
    tr, image = _trainer()
    nll = tr.token_nll({"image": image})
    thr = float(nll[1].max())          # nothing of slice 1 exceeds it; slice 0 keeps the codes above it, if any
    if not bool((nll[0] > thr).any()):
        thr = float(nll.max())
    out = tr.detect({"image": image}, thr, n_candidates=2, generator=_gen())
    assert int(out["n_resampled"][1]) == 0 and not bool(out["map"][1].any())
    assert torch.equal(out["restored"][1], image[1])
    ids_only = tr.detect({"ids": tr.codes({"image": image})}, thr, n_candidates=2, against="reconstruction", generator=_gen())
    assert not bool(ids_only["map"][1].any())
    with pytest.raises(ValueError, match="against='image' needs a batch with an image"):
        tr.detect({"ids": tr.codes({"image": image})}, thr, n_candidates=2, generator=_gen())


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_detects_and_a_seed_repeats_every_byte(tmp_path):
    from utils import png
    save = os.path.join(str(tmp_path), "run")
    run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), P.prior_run_config(save)), "-p")
    ckpt = os.path.join(save, "study", "version_0", "ckpt-epoch=0000-total_loss=0.00.ckpt")
    raw = P.prior_run_config(save, resume_checkpoint=ckpt)
    # a barely trained prior over 8 codes: token_nll sits around log 8 = 2.08, so about half of the codes are restored
    raw["detect"] = dict(n_slices=0, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0,
                         against="image", weight="mask", labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})
    cfg = write_config(os.path.join(str(tmp_path), "detect.json"), raw)
    files = {}
    for version in (1, 2):
        out = run_launcher(cfg, "-p", "-m", "detect")
        assert "Loading model from" in out and "Detection results are saved" in out
        rdir = os.path.join(save, "study", "version_%d" % version)
        mine = sorted(f for f in os.listdir(rdir) if f.startswith("detect"))
        assert mine == ["detect.csv", "detect_0000.png", "detect_0001.png", "detect_result.csv"]
        files[version] = {f: open(os.path.join(rdir, f), "rb").read() for f in mine}
    assert files[1] == files[2], "the same seed writes the same bytes"
    rdir = os.path.join(save, "study", "version_1")
    pixels, _ = png.load(os.path.join(rdir, "detect_0000.png"))
    assert pixels.shape == (32, 3 * 32) and pixels.dtype == np.uint8
    header, rows = read_csv(os.path.join(rdir, "detect.csv"))
    assert header == ["slice", "n_resampled", "mean_nll", "max_map", "score", "positives"] and len(rows) == 4
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3] and all(0 <= int(r[1]) <= 256 and float(r[4]) < 0 and int(r[5]) > 0 for r in rows)
    assert all((float(r[3]) > 0) == (int(r[1]) > 0) for r in rows) and any(int(r[1]) > 0 for r in rows)
    header, rows = read_csv(os.path.join(rdir, "detect_result.csv"))
    assert header == ["auroc", "ap", "best_dice", "best_threshold", "P", "N", "err_free", "err"] and len(rows) == 1
    auroc, ap, dice, thr, Pn, Nn, ok, err = (float(v) for v in rows[0])
    assert Pn > 0 and Nn > 0 and Pn + Nn == 4 * 32 * 32 and ok == 1 and err == 0          # the value of the AUROC is not asserted:
    assert math.isfinite(auroc) and 0 <= auroc <= 1 and 0 <= ap <= 1 and 0 <= dice <= 1   # the prior is barely trained
    assert Pn == sum(int(r[5]) for r in read_csv(os.path.join(rdir, "detect.csv"))[1])
