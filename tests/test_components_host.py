"""CPU-side checks of the lesion-wise detection scores (no GPU): the numpy restatement (tests/components_ref.py) on hand-drawn cases
and against scipy.ndimage.label, the C ABI and operator plumbing of vqw_label_components, vqw_component_areas and vqw_lesion_match
with their refusals before any device work, the cap formula, detect_lesionwise / check_detect_config, the committed config, and the
NaN rules of the derived scores."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import components_ref as R
import prior_ref as P

NEW_SYMBOLS = ("vqw_label_components_ws_ints", "vqw_label_components", "vqw_component_areas", "vqw_lesion_match_ws_bytes", "vqw_lesion_match")


# ------------------------------------------------------------------------------------------------ the restatement
def _img(rows):
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)[None]


def test_reference_labels_hand_drawn_cases():
    x = _img(["1010",
              "0100",
              "0001"])
    l8, c8 = R.label(x, None, 8)
    l4, c4 = R.label(x, None, 4)
    assert c8.tolist() == [2] and l8[0].tolist() == [[1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 2]]          # the V joins through its diagonals
    assert c4.tolist() == [4] and l4[0].tolist() == [[1, 0, 2, 0], [0, 3, 0, 0], [0, 0, 0, 4]]
    # numbering by FIRST pixel: the U's left arm starts before the dot, its right arm joins it only at the bottom
    x = _img(["10101",
              "10001",
              "11111"])
    for conn in (4, 8):
        l, c = R.label(x, None, conn)
        assert c.tolist() == [2] and l[0].tolist() == [[1, 0, 2, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]]
    # per image, never across: image 0 ends in foreground and image 1 begins with it
    x = np.stack([_img(["01", "11"])[0], _img(["11", "00"])[0]])
    l, c = R.label(x, None, 4)
    assert c.tolist() == [1, 1] and l.tolist() == [[[0, 1], [1, 1]], [[1, 1], [0, 0]]]
    # the float route: a value at the threshold is foreground, a NaN is background
    s = np.array([[[0.5, np.nan, 0.49999997, 0.7]]], dtype=np.float32)
    l, c = R.label(s, 0.5, 8)
    assert l.tolist() == [[[1, 0, 0, 2]]] and c.tolist() == [2]
    assert R.label(np.zeros((1, 3, 3), np.uint8))[1].tolist() == [0] and R.label(np.ones((1, 1, 1), np.uint8))[0].tolist() == [[[1]]]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_against_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3)) if connectivity == 8 else None
    g = np.random.default_rng(connectivity)
    cases = [(g.uniform(size=shape) < d).astype(np.uint8) for shape in ((1, 1), (1, 17), (33, 65), (64, 128)) for d in (0.2, 0.407, 0.5, 0.593, 0.8)]
    cases += [R.spiral(64, 128), R.comb(33, 65), R.rings(33, 65), R.checkerboard(33, 65)]
    for x in cases:
        want, n = ndi.label(x, structure=structure)
        got, c = R.label(x[None], None, connectivity)
        assert np.array_equal(got[0], want) and int(c[0]) == n
        a = R.areas(got, c, connectivity)
        assert np.array_equal(a[0, :n], np.bincount(want.reshape(-1), minlength=n + 1)[1:]) and not a[0, n:].any()


def test_patterns_are_what_the_gpu_tests_take_them_for():
    for H, W in ((64, 128), (96, 160), (33, 65)):
        for conn in (4, 8):
            assert R.label(R.spiral(H, W)[None], None, conn)[1].tolist() == [1]
            assert R.label(R.comb(H, W)[None], None, conn)[1].tolist() == [1]
            l, c = R.label(R.rings(H, W)[None], None, conn)
            assert c.tolist() == [2] and l[0, 0, 0] == 1 and l[0, 3, 3] == 2
        assert int(R.spiral(H, W).sum()) > H * W // 3


def test_cap_is_reached_by_a_checkerboard_and_a_dot_grid():
    from hipops import ops
    for H, W in ((1, 1), (1, 17), (2, 2), (8, 8), (33, 65), (7, 10)):
        assert ops.component_cap(H, W, 4) == R.cap(H, W, 4) == int(R.label(R.checkerboard(H, W)[None], None, 4)[1][0])
        dots = np.zeros((H, W), dtype=np.uint8)
        dots[::2, ::2] = 1
        assert ops.component_cap(H, W, 8) == R.cap(H, W, 8) == int(R.label(dots[None], None, 8)[1][0])
        if H > 1 and W > 1:          # the diagonals join a checkerboard into one
            assert R.label(R.checkerboard(H, W)[None], None, 8)[1].tolist() == [1]
        assert ops.component_cap(H, W, 4) >= ops.component_cap(H, W, 8)
    with pytest.raises(RuntimeError, match="connectivity=6 must be 4 or 8"):
        ops.component_cap(4, 4, 6)


def test_reference_match_on_hand_cases():
    gt = _img(["1100011",
               "1100011",
               "0000000",
               "0000000"])
    gl, gc = R.label(gt, None, 8)
    assert gc.tolist() == [2]
    bridge = _img(["0111110", "0000000", "0000000", "0000000"])          # one blob over both lesions
    assert R.match(R.label(bridge)[0], gl, 1) == [1, 2, 2, 1, 0, 2, 5, 8]
    two = _img(["1000000", "0000000", "0100000", "0000011"])             # one pixel on lesion 1, one stray pixel and a stray pair
    pl, pc = R.label(two, None, 4)
    assert pc.tolist() == [3] and R.match(pl, gl, 1) == [1, 2, 1, 3, 2, 1, 4, 8]
    assert R.match(pl, gl, 2) == [1, 2, 0, 1, 1, 0, 2, 8]                 # min_size 2 keeps only the pair, which is false
    assert R.match(pl, gl, 3) == [1, 2, 0, 0, 0, 0, 0, 8]
    on_one = _img(["1000000", "0100000", "0000000", "0000000"])          # under 4: two blobs on lesion 1, detected once
    assert R.match(R.label(on_one, None, 4)[0], gl, 1) == [1, 2, 1, 2, 0, 2, 2, 8]


# ------------------------------------------------------------------------------------------------ the derived scores
def test_derived_scores_and_their_nan_rules():
    from functions import LesionScores, derived_scores, lesion_csv_row, LESION_CSV
    from hipops import ops
    assert ops.LESION_ACC == tuple(R.ACC)
    s = derived_scores([4, 10, 8, 5, 1, 30, 50, 70])
    assert s == R.scores([4, 10, 8, 5, 1, 30, 50, 70])
    assert s["sensitivity"] == 0.8 and s["fp_per_slice"] == 0.25 and s["precision"] == 0.8 and s["dice_filtered"] == 0.5
    assert s["f1"] == pytest.approx(0.8, rel=1e-15)
    s = derived_scores([3, 0, 0, 2, 2, 0, 9, 0])          # no ground truth: sensitivity and f1 undefined, the false alarms count
    assert math.isnan(s["sensitivity"]) and math.isnan(s["f1"]) and s["precision"] == 0.0 and s["fp_per_slice"] == 2 / 3 and s["dice_filtered"] == 0.0
    s = derived_scores([3, 4, 0, 0, 0, 0, 0, 20])         # no prediction: precision and f1 undefined
    assert s["sensitivity"] == 0.0 and math.isnan(s["precision"]) and math.isnan(s["f1"]) and s["fp_per_slice"] == 0.0 and s["dice_filtered"] == 0.0
    s = derived_scores([0] * 8)
    assert all(math.isnan(v) for v in s.values())
    s = derived_scores([1, 2, 0, 3, 3, 0, 5, 5])          # both zero: the harmonic mean has no denominator
    assert s["sensitivity"] == 0.0 and s["precision"] == 0.0 and math.isnan(s["f1"])
    acc = LesionScores([0, 0.25], 2, 4)
    rows = acc.result()                                    # nothing accumulated: the one defined answer
    assert [r["threshold"] for r in rows] == [0.0, 0.25] and all(r["slices"] == 0 and math.isnan(r["f1"]) and r["err"] == 0 for r in rows)
    assert lesion_csv_row(dict(rows[1], slices=3, sensitivity=0.1)) == "0.25,3,0,0,0.10000000000000001,0,0,nan,nan,nan,nan"
    assert LESION_CSV[0] == "threshold" and len(LESION_CSV) == 11
    for bad in (dict(thresholds=[]), dict(thresholds=[-1.0]), dict(thresholds=[float("nan")]), dict(thresholds=[float("inf")])):
        with pytest.raises(ValueError, match="thresholds"):
            LesionScores(**bad)
    with pytest.raises(ValueError, match="min_size=0"):
        LesionScores([0.1], 0)
    with pytest.raises(ValueError, match="connectivity=6"):
        LesionScores([0.1], 1, 6)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES, s
    for s in ("vqw_label_components", "vqw_component_areas", "vqw_lesion_match"):
        assert s in ops_
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES["vqw_label_components_ws_ints"] == (l, [i, i, i])
    assert _lib.SIGNATURES["vqw_label_components"] == (i, [p, p, f, p, p, p, p, l, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_component_areas"] == (i, [p, p, p, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_lesion_match_ws_bytes"] == (l, [i, i, i])
    assert _lib.SIGNATURES["vqw_lesion_match"] == (i, [p, p, p, p, p, p, p, l, i, i, i, i, i, i, p])
    sch = str(torch.ops.vqw.label_components.default._schema)
    assert "Tensor? mask" in sch and "Tensor? scores" in sch and "float threshold" in sch and "Tensor(a!)? labels" in sch
    assert "Tensor(b!)? counts" in sch and "Tensor(c!)? err" in sch and "Tensor(d!)? ws" in sch and "int connectivity" in sch
    sch = str(torch.ops.vqw.component_areas.default._schema)
    assert "Tensor? labels" in sch and "Tensor(a!)? areas" in sch and "Tensor(b!)? err" in sch and "int cap" in sch
    sch = str(torch.ops.vqw.lesion_match.default._schema)
    assert "Tensor? pred_areas" in sch and "Tensor? gt_counts" in sch and "Tensor(a!)? acc" in sch and "int min_size" in sch


def test_workspace_queries():
    from hipops import _lib
    L = _lib.load()
    assert L.vqw_label_components_ws_ints(1, 1, 1) == 1 + 2 and L.vqw_label_components_ws_ints(4, 512, 512) == 4 * 512 * 512 + 2 * 4 * 256
    assert L.vqw_label_components_ws_ints(2, 33, 65) == 2 * 33 * 65 + 2 * 2 * 3          # 2145 pixels: three chunks of 1024
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (2, 32768, 32768)):
        assert L.vqw_label_components_ws_ints(*bad) == 0
    assert L.vqw_lesion_match_ws_bytes(2, 3, 4) == 16 and L.vqw_lesion_match_ws_bytes(2, 8, 9) == 48 and L.vqw_lesion_match_ws_bytes(0, 1, 1) == 0


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    P_ = 4096          # an aligned non-null stand-in for every pointer
    err = lambda: L.vqw_last_error()  # noqa: E731

    def lab(N=1, H=8, W=8, conn=8, mask=P_, scores=None, thr=0.0, labels=P_, counts=P_, e=P_, ws=P_, ws_ints=1 << 20):
        return L.vqw_label_components(mask, scores, thr, labels, counts, e, ws, ws_ints, N, H, W, conn, None)

    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert lab(**kw) != 0 and b"vqw_label_components" in err() and b"empty" in err()
    for conn in (0, 6, 5, -8):
        assert lab(conn=conn) != 0 and b"connectivity=%d must be 4 or 8" % conn in err()
    assert lab(N=2, H=32768, W=32768) != 0 and b"below 2^31" in err()
    assert lab(N=1, H=65536, W=32768) != 0 and b"below 2^31" in err()
    assert lab(mask=None) != 0 and b"exactly one of mask" in err()
    assert lab(scores=P_) != 0 and b"exactly one of mask" in err()
    for kw in (dict(labels=None), dict(counts=None), dict(e=None), dict(ws=None)):
        assert lab(**kw) != 0 and b"null pointer" in err()
    assert lab(mask=None, scores=P_, thr=float("nan")) != 0 and b"threshold is NaN" in err()
    for kw in (dict(mask=None, scores=P_ + 2), dict(labels=P_ + 1), dict(counts=P_ + 2), dict(e=P_ + 3), dict(ws=P_ + 2)):
        assert lab(**kw) != 0 and b"4-byte aligned" in err()
    assert lab(ws_ints=8 * 8 + 1) != 0 and b"a workspace of 65 ints, 66 are needed" in err()

    def areas(N=1, H=8, W=8, cap=16, labels=P_, a=P_, e=P_):
        return L.vqw_component_areas(labels, a, e, N, H, W, cap, None)

    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert areas(**kw) != 0 and b"vqw_component_areas" in err() and b"empty" in err()
    assert areas(N=2, H=32768, W=32768) != 0 and b"below 2^31" in err()
    assert areas(cap=0) != 0 and b"cap=0 must be at least 1" in err()
    for kw in (dict(labels=None), dict(a=None), dict(e=None)):
        assert areas(**kw) != 0 and b"null pointer" in err()
    for kw in (dict(labels=P_ + 2), dict(a=P_ + 1), dict(e=P_ + 2)):
        assert areas(**kw) != 0 and b"4-byte aligned" in err()

    def match(N=1, H=8, W=8, pcap=16, gcap=32, min_size=1, pl=P_, pc=P_, pa=P_, gl=P_, gc=P_, acc=P_, ws=P_, ws_bytes=1 << 20):
        return L.vqw_lesion_match(pl, pc, pa, gl, gc, acc, ws, ws_bytes, N, H, W, pcap, gcap, min_size, None)

    for kw in (dict(N=0), dict(H=0), dict(W=0)):
        assert match(**kw) != 0 and b"vqw_lesion_match" in err() and b"empty" in err()
    assert match(N=2, H=32768, W=32768) != 0 and b"below 2^31" in err()
    for m in (0, -3):
        assert match(min_size=m) != 0 and b"min_size=%d must be at least 1" % m in err()
    for kw in (dict(pcap=0), dict(gcap=0)):
        assert match(**kw) != 0 and b"must be at least 1" in err()
    for kw in (dict(pl=None), dict(pc=None), dict(pa=None), dict(gl=None), dict(gc=None), dict(acc=None), dict(ws=None)):
        assert match(**kw) != 0 and b"null pointer" in err()
    for kw in (dict(pl=P_ + 2), dict(pc=P_ + 1), dict(pa=P_ + 2), dict(gl=P_ + 2), dict(gc=P_ + 2), dict(acc=P_ + 4)):
        assert match(**kw) != 0 and b"aligned" in err()
    assert match(ws_bytes=47) != 0 and b"a workspace of 47 bytes, 48 are needed" in err()


def test_operators_have_no_cpu_route_and_check_their_arguments():
    from hipops import ops
    m, lab, cnt = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_components(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.component_areas(lab, cnt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lesion_match(lab, cnt, torch.zeros(1, 4, dtype=torch.int32), lab, cnt, 1, torch.zeros(8, dtype=torch.long))
    assert ops.new_lesion_acc("cpu", 3).shape == (3, 8) and ops.new_lesion_acc("cpu", 3).dtype == torch.long
    assert len(ops.LESION_ACC) == 8


# ------------------------------------------------------------------------------------------------ the config
DETECT = dict(n_slices=0, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0, against="image",
              weight="mask", labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})
LESIONWISE = dict(thresholds=[0, 0.05, 0.1], min_size=4, connectivity=8)


def _cfg(tmp_path, lesionwise=LESIONWISE, **detect):
    from utils import load_json
    raw = P.prior_run_config(tmp_path / "out", resume_checkpoint="prior.ckpt")
    raw["detect"] = dict(DETECT, **detect)
    if lesionwise is not None:
        raw["detect"]["lesionwise"] = lesionwise
    return load_json(write_config(tmp_path / "c.json", raw))


def test_detect_lesionwise_reads_good_sections_and_names_what_is_wrong(tmp_path):
    from trainers import check_detect_config, detect_lesionwise
    assert detect_lesionwise(_cfg(tmp_path)) == dict(thresholds=[0.0, 0.05, 0.1], min_size=4, connectivity=8)
    check_detect_config(_cfg(tmp_path))
    for off in (None, False):          # absent or false: off
        assert detect_lesionwise(_cfg(tmp_path, lesionwise=off)) is None
        check_detect_config(_cfg(tmp_path, lesionwise=off))
    assert detect_lesionwise(_cfg(tmp_path, lesionwise=dict(LESIONWISE, connectivity=4, thresholds=[1]))) == dict(thresholds=[1.0], min_size=4, connectivity=4)
    for key in LESIONWISE:
        bad = {k: v for k, v in LESIONWISE.items() if k != key}
        with pytest.raises(NotImplementedError, match=r"detect\.lesionwise\.\{thresholds, min_size, connectivity\}; missing: %s$" % key):
            check_detect_config(_cfg(tmp_path, lesionwise=bad))
    for thresholds in ([], [0.1, -0.5], [float("nan")], [float("inf")], 0.1, [True], ["0.1"]):
        with pytest.raises(ValueError, match=r"detect\.lesionwise\.thresholds"):
            check_detect_config(_cfg(tmp_path, lesionwise=dict(LESIONWISE, thresholds=thresholds)))
    for min_size in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match=r"detect\.lesionwise\.min_size"):
            check_detect_config(_cfg(tmp_path, lesionwise=dict(LESIONWISE, min_size=min_size)))
    for conn in (6, 0, "8", True):
        with pytest.raises(ValueError, match=r"detect\.lesionwise\.connectivity"):
            check_detect_config(_cfg(tmp_path, lesionwise=dict(LESIONWISE, connectivity=conn)))
    with pytest.raises(ValueError, match="needs detect.labels"):
        check_detect_config(_cfg(tmp_path, labels=False))
    check_detect_config(_cfg(tmp_path, labels="seg"))


def test_committed_lesionwise_config_parses():
    import json
    from utils import load_json
    from trainers import check_detect_config, detect_lesionwise
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_detect_lesionwise.json")
    c = load_json(path)
    check_detect_config(c)
    assert detect_lesionwise(c) == dict(thresholds=[0.0, 0.02, 0.05, 0.1, 0.2], min_size=4, connectivity=8)
    mine, base = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "prior_vqgan_512_detect.json")))
    assert mine["model"]["dis"]["normalization"] == "batchnorm"
    del mine["detect"]["lesionwise"]
    for k in ("run", "dataset", "model", "prior_optim", "detect"):          # the detect config plus the section
        assert mine[k] == base[k], k
    assert "prior_vqgan_512_detect_lesionwise.json" in open(os.path.join(ROOT, "configs", "README.md")).read()
