"""CPU-side checks of anomaly detection with the code prior (no GPU): the C ABI and operator plumbing of vqw_anomaly_map,
vqw_score_histogram and vqw_detection_scores with their refusals before any device work, the quantiser and the sort-based metric
restatement (tests/detect_ref.py) on cases one computes by hand, dataio's opt-in labels (synthetic_lesions, label_modality),
check_detect_config, and the launcher's `-m detect`."""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import detect_ref as D
import prior_ref as P

NEW_SYMBOLS = ("vqw_anomaly_map", "vqw_score_histogram", "vqw_detection_scores")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and s in ops_, s
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES["vqw_anomaly_map"] == (ctypes.c_int, [p, p, p, p, p, i, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_score_histogram"] == (ctypes.c_int, [p, p, p, p, l, p])
    assert _lib.SIGNATURES["vqw_detection_scores"] == (ctypes.c_int, [p, p, p, p])
    sch = str(torch.ops.vqw.anomaly_map.default._schema)
    assert "Tensor? a" in sch and "Tensor? cellmask" in sch and "Tensor? taps" in sch and "Tensor(a!)? map" in sch and "int K" in sch
    sch = str(torch.ops.vqw.score_histogram.default._schema)          # hist and err are mutated
    assert "Tensor? scores" in sch and "Tensor? labels" in sch and "Tensor(a!)? hist" in sch and "Tensor(b!)? err" in sch and "int n" in sch
    sch = str(torch.ops.vqw.detection_scores.default._schema)
    assert "Tensor? hist" in sch and "Tensor? err" in sch and "Tensor(a!)? out" in sch


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    P_ = 4096          # a 16-byte aligned non-null stand-in for every pointer

    def amap(N=1, H=8, W=8, C=1, h=2, w=2, K=3, a=P_, b=P_, mask=P_, taps=P_, out=P_):
        return L.vqw_anomaly_map(a, b, mask, taps, out, N, H, W, C, h, w, K, None)

    for kw in (dict(a=None), dict(b=None), dict(taps=None), dict(out=None)):
        assert amap(**kw) != 0 and b"vqw_anomaly_map" in L.vqw_last_error() and b"null pointer" in L.vqw_last_error()
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(C=0)):
        assert amap(**kw) != 0 and b"empty" in L.vqw_last_error()
    for K in (0, 2, 35, 99):          # 33 taps is the widest: a halo of 16 pixels
        assert amap(K=K) != 0 and b"at most 33" in L.vqw_last_error() and b"halo of 16" in L.vqw_last_error(), K
    for kw in (dict(h=3), dict(w=3), dict(h=0), dict(w=16)):
        assert amap(**kw) != 0 and b"integer multiples of the cell grid" in L.vqw_last_error()
    for kw in (dict(a=P_ + 4), dict(b=P_ + 8), dict(out=P_ + 4), dict(taps=P_ + 4)):
        assert amap(**kw) != 0 and b"16-byte aligned" in L.vqw_last_error()
    assert amap(N=65536) != 0 and b"65535" in L.vqw_last_error()

    def hist(n=10, scores=P_, labels=P_, h=P_, err=P_):
        return L.vqw_score_histogram(scores, labels, h, err, n, None)

    for kw in (dict(scores=None), dict(labels=None), dict(h=None), dict(err=None)):
        assert hist(**kw) != 0 and b"vqw_score_histogram" in L.vqw_last_error() and b"null pointer" in L.vqw_last_error()
    for n in (0, -1, 2 ** 40 + 1):
        assert hist(n=n) != 0 and b"1 <= n <= 2^40" in L.vqw_last_error()
    for kw in (dict(scores=P_ + 2), dict(h=P_ + 4), dict(err=P_ + 4)):
        assert hist(**kw) != 0 and b"aligned" in L.vqw_last_error()

    assert L.vqw_detection_scores(None, None, P_, None) != 0 and b"vqw_detection_scores" in L.vqw_last_error()
    assert L.vqw_detection_scores(P_, None, None, None) != 0 and b"null pointer" in L.vqw_last_error()
    assert L.vqw_detection_scores(P_ + 4, None, P_, None) != 0 and b"8-byte aligned" in L.vqw_last_error()


def test_operators_have_no_cpu_route_and_check_their_arguments():
    from hipops import ops
    a = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.anomaly_map(a, a, torch.zeros(1, 2, 2, dtype=torch.uint8), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_histogram(torch.zeros(4), torch.zeros(4, dtype=torch.uint8), torch.zeros(2, 65536, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detection_scores(torch.zeros(2, 65536, dtype=torch.long))
    for sigma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            ops.gauss_taps(sigma)
    assert ops.DETECTION_SCORES[:6] == ("auroc", "ap", "best_dice", "best_threshold", "P", "N")


def test_gauss_taps_are_the_restatements():
    from hipops import ops
    assert torch.equal(ops.gauss_taps(0), torch.ones(1))
    for sigma, K in ((0.5, 5), (1.0, 7), (2.0, 13), (4.0, 25), (1.3, 9)):
        t = ops.gauss_taps(sigma)
        assert t.dtype == torch.float32 and t.numel() == K == 2 * math.ceil(3 * sigma) + 1
        assert torch.equal(t, D.taps_ref(sigma, torch.float32)) and abs(float(t.double().sum()) - 1) < 1e-6
        assert torch.equal(t, t.flip(0)) and int(t.argmax()) == K // 2


# ------------------------------------------------------------------------------------------------ the quantiser
def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_quantiser_special_values_and_bin_edges():
    assert D.keys_ref(np.array([0.0, -0.0], dtype=np.float32)).tolist() == [0, 0]
    # denormals: exponent field 0, the key is the top 8 mantissa bits
    assert D.keys_ref(_f([1, 0x7FFF, 0x8000, 0x7FFFFF])).tolist() == [0, 0, 1, 0xFF]
    assert D.keys_ref(np.array([1.0, 2.0, 0.5], dtype=np.float32)).tolist() == [0x7F00, 0x8000, 0x7E00]
    # a bin [key << 15, (key + 1) << 15): its lower edge, its last float, the next bin's first
    assert D.keys_ref(_f([0x3F808000 - 1, 0x3F808000, 0x3F810000 - 1, 0x3F810000])).tolist() == [0x7F00, 0x7F01, 0x7F01, 0x7F02]
    assert D.keys_ref(np.array([np.finfo(np.float32).max], dtype=np.float32)).tolist() == [0xFEFF]
    bad = np.array([np.nan, np.inf, -np.inf, -1.0, -1e-45], dtype=np.float32)
    assert D.keys_ref(bad).tolist() == [-1] * 5 and D.keys_ref(_f([0xFFC00000])).tolist() == [-1]          # a NaN with the sign set
    assert D.key_floor(0x7F00) == 1.0 and D.key_floor(0) == 0.0 and D.key_floor(0x7F01) == 1.0 + 2.0 ** -8


def test_quantiser_is_monotone_with_relative_resolution_2_to_the_minus_8():
    g = np.random.default_rng(5)
    s = np.sort(np.concatenate([g.uniform(0, 2, 20000), 10.0 ** g.uniform(-44, 38, 20000), [0.0]]).astype(np.float32))
    k = D.keys_ref(s)
    assert (k >= 0).all() and (np.diff(k) >= 0).all()
    lo = np.array([D.key_floor(v) for v in k], dtype=np.float64)
    normal = s >= np.finfo(np.float32).tiny
    assert (lo <= s).all() and ((s[normal] - lo[normal]) < s[normal] * 2.0 ** -8).all()


# ------------------------------------------------------------------------------------------------ the metrics
def _hist(keys, labels):
    h = np.zeros((2, 65536), dtype=np.int64)
    np.add.at(h, (np.asarray(labels, dtype=np.int64), np.asarray(keys, dtype=np.int64)), 1)
    return h


def test_metric_restatements_on_hand_computable_cases():
    k = lambda *v: D.keys_ref(np.array(v, dtype=np.float32))  # noqa: E731
    # separable: both positives above both negatives
    got = D.scores_sorted(k(0.9, 0.8, 0.2, 0.1), [1, 1, 0, 0])
    assert got[:3] == [1.0, 1.0, 1.0] and got[3] == D.key_floor(k(0.8)[0]) and got[4:] == [2.0, 2.0]
    # reversed: AUROC 0; AP = (1/2)(1/3) + (1/2)(2/4); the best Dice takes everything: 2 * 2 / (2 + 2 + 2)
    got = D.scores_sorted(k(0.1, 0.2, 0.8, 0.9), [1, 1, 0, 0])
    assert got[0] == 0.0 and abs(got[1] - (1 / 6 + 1 / 4)) < 1e-15 and abs(got[2] - 2 / 3) < 1e-15 and got[3] == D.key_floor(k(0.1)[0])
    # one shared bin: AUROC 1/2, AP = the prevalence
    got = D.scores_sorted(k(0.5, 0.5, 0.5, 0.5, 0.5), [1, 0, 0, 0, 0])
    assert got[0] == 0.5 and got[1] == 0.2 and abs(got[2] - 2 / 6) < 1e-15
    # interleaved by hand: scores 4 3 2 1 with labels 1 0 1 0 -> U = 2 + 1 = 3 of 4; AP = (1/2)(1) + (1/2)(2/3)
    got = D.scores_sorted(k(4, 3, 2, 1), [1, 0, 1, 0])
    assert got[0] == 0.75 and abs(got[1] - (0.5 + 1 / 3)) < 1e-15 and abs(got[2] - 0.8) < 1e-15 and got[3] == 2.0
    # a tie between a positive and a negative counts half: scores 2 (pos), 1 (pos), 1 (neg) -> (1 + 1/2) / 2
    assert D.scores_sorted(k(2, 1, 1), [1, 1, 0])[0] == 0.75
    for labels in ([0, 0, 0], [1, 1, 1]):
        got = D.scores_sorted(k(1, 2, 3), labels)
        assert all(math.isnan(v) for v in got[:4]) and got[4] + got[5] == 3.0
    # an unbinned score takes no part
    assert D.scores_sorted(np.array([D.keys_ref(np.float32(4))[0], -1, *k(3, 2, 1)]), [1, 1, 0, 1, 0])[:2] == D.scores_sorted(k(4, 3, 2, 1), [1, 0, 1, 0])[:2]


def test_sorted_and_exact_restatements_agree_and_ties_go_to_the_highest_bin():
    g = np.random.default_rng(11)
    s = g.uniform(0, 2, 5000).astype(np.float32) ** 3
    y = (g.uniform(0, 1, 5000) < 0.2 + 0.3 * (s > 1)).astype(np.int64)
    keys = D.keys_ref(s)
    a, b = D.scores_sorted(keys, y), D.scores_exact(_hist(keys, y))
    assert np.allclose(a[:3], b[:3], rtol=1e-12, atol=0) and a[3:] == b[3:]
    # Dice 2 * 1 / (1 + 1 + 2) at the upper bin = 2 * 2 / (2 + 4 + 2) at the lower one: exactly 1/2 both
    h = np.zeros((2, 65536), dtype=np.int64)
    h[1, 300], h[0, 300], h[1, 200], h[0, 200] = 1, 1, 1, 3
    got = D.scores_exact(h)
    assert got[2] == 0.5 and got[3] == D.key_floor(300)
    keys, labels = [300, 300, 200, 200, 200, 200], [1, 0, 1, 0, 0, 0]
    assert D.scores_sorted(keys, labels)[2:4] == [0.5, D.key_floor(300)]


# ------------------------------------------------------------------------------------------------ dataio
def test_synthetic_lesions_are_a_pure_function_and_the_mask_matches_the_delta():
    from dataio import synthetic_lesions, synthetic_slice, SyntheticSliceDataset
    d1, m1 = synthetic_lesions(3, 7, 64, 3, 10.0, 0.8)
    d2, m2 = synthetic_lesions(3, 7, 64, 3, 10.0, 0.8)
    assert torch.equal(d1, d2) and torch.equal(m1, m2)
    assert d1.shape == (1, 64, 64) and d1.dtype == torch.float32 and m1.shape == (1, 64, 64) and m1.dtype == torch.uint8
    assert not torch.equal(d1, synthetic_lesions(3, 8, 64, 3, 10.0, 0.8)[0]) and not torch.equal(d1, synthetic_lesions(4, 7, 64, 3, 10.0, 0.8)[0])
    assert 0 < int(m1.sum()) <= 3 * math.pi * 10.5 ** 2 and float(d1.max()) == pytest.approx(0.8) and float(d1.min()) == 0.0
    # the mask is the half-height set of the delta; the edge is smooth: some pixels lie strictly between 0 and the contrast
    assert bool((d1[m1 == 1] >= 0.4 - 1e-6).all()) and bool((d1[m1 == 0] < 0.4 + 1e-6).all())
    assert bool(((d1 > 0) & (d1 < 0.8 - 1e-6)).any())
    dn, mn = synthetic_lesions(3, 7, 64, 2, 6.0, -0.5)          # a dark lesion: the same rule on |delta|
    assert float(dn.max()) == 0.0 and bool((dn[mn == 1] <= -0.25 + 1e-6).all()) and bool((dn[mn == 0] > -0.25 - 1e-6).all())
    # the dataset: opt-in, the slice underneath is untouched
    plain = SyntheticSliceDataset("test", 64, 4, seed=3)
    with_l = SyntheticSliceDataset("test", 64, 4, seed=3, lesions=dict(n=3, radius=10.0, contrast=0.8))
    s0, s1 = plain[2], with_l[2]
    assert sorted(s0) == ["image", "patient_id", "slice_num"] and sorted(s1) == ["image", "label", "patient_id", "slice_num"]
    assert torch.equal(s0["image"], synthetic_slice(3 * 3 + 2, 2, 64))
    delta, mask = synthetic_lesions(3 * 3 + 2, 2, 64, 3, 10.0, 0.8)
    assert torch.equal(s1["label"], mask) and torch.equal(s1["image"], (s0["image"] + delta).clamp(-1, 1))
    assert torch.equal(s1["image"][mask == 0][delta[mask == 0] == 0], s0["image"][mask == 0][delta[mask == 0] == 0])


def _brats_tree(root):
    g = np.random.default_rng(0)
    for p in ("patA", "patB"):
        os.makedirs(os.path.join(root, p))
        for s in (3, 4):
            np.save(os.path.join(root, p, "%s_t1_%d.npy" % (p, s)), g.uniform(0, 255, (8, 8)).astype(np.float32))
            seg = np.zeros((8, 8), dtype=np.int16)
            seg[2:4, s:s + 2] = 4 if s == 3 else 1
            np.save(os.path.join(root, p, "%s_seg_%d.npy" % (p, s)), seg)
    return root


def test_label_modality_none_leaves_the_loader_unchanged_and_a_name_adds_the_label(tmp_path):
    from dataio import get_data_loader
    root = _brats_tree(str(tmp_path / "brats"))
    kw = dict(mode="test", dataset_name="MICCAIBraTSDataset", root_dir_path=root, batch_size=2, num_workers=0, modality="t1")
    before = list(get_data_loader(**kw))
    same = list(get_data_loader(label_modality=None, **kw))
    labelled = list(get_data_loader(label_modality="seg", **kw))
    assert len(before) == len(same) == len(labelled) == 2
    for b0, b1, b2 in zip(before, same, labelled):
        assert sorted(b0) == sorted(b1) == ["image", "image_path", "modality", "patient_id", "slice_num"]
        assert sorted(b2) == sorted(list(b0) + ["label"])
        for k in b0:
            eq = torch.equal if torch.is_tensor(b0[k]) else (lambda x, y: x == y)
            assert eq(b0[k], b1[k]) and eq(b0[k], b2[k]), k
        assert b2["label"].shape == (2, 1, 8, 8) and b2["label"].dtype == torch.uint8
        for i, path in enumerate(b2["image_path"]):
            seg = np.load(path.replace("_t1_", "_seg_"))
            assert np.array_equal(b2["label"][i, 0].numpy(), (seg != 0).astype(np.uint8)) and int(b2["label"][i].sum()) == 4
    with pytest.raises(NotImplementedError, match="label_modality"):
        get_data_loader(mode="test", dataset_name="synthetic", root_dir_path=None, batch_size=2, num_workers=0, label_modality="seg")
    with pytest.raises(NotImplementedError, match="lesions"):
        get_data_loader(lesions=dict(n=1, radius=2, contrast=1), **kw)
    syn = dict(mode="test", dataset_name="synthetic", root_dir_path=None, batch_size=2, num_workers=0, image_size=16, n_samples=2, seed=1)
    plain, les = next(iter(get_data_loader(**syn))), next(iter(get_data_loader(lesions=dict(n=1, radius=3, contrast=1.0), **syn)))
    assert "label" not in plain and les["label"].shape == (2, 1, 16, 16) and int(les["label"].sum()) > 0


# ------------------------------------------------------------------------------------------------ the config and the launcher
DETECT = dict(n_slices=0, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0, against="image",
              weight="mask", labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})


def _raw(tmp_path, detect=DETECT, **run):
    raw = P.prior_run_config(tmp_path / "out", **dict(dict(resume_checkpoint="prior.ckpt"), **run))
    if detect is not None:
        raw["detect"] = dict(detect)
    return raw


def _args(**kw):
    a = dict(config="x.json", mode="detect", multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)
    a.update(kw)
    return argparse.Namespace(**a)


def test_check_detect_config_names_what_is_missing(tmp_path):
    from utils import load_json
    from trainers import check_detect_config
    from trainers.config import detect_labels
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    check_detect_config(cfg(_raw(tmp_path)))
    for key in DETECT:
        bad = dict(DETECT)
        del bad[key]
        with pytest.raises(NotImplementedError, match=r"detect\.\{.*\}; missing: %s$" % key):
            check_detect_config(cfg(_raw(tmp_path, detect=bad)))
    with pytest.raises(NotImplementedError, match="missing: n_slices, n_candidates, temperature, top_k, top_p, seed, nll_threshold, sigma, against, weight, labels"):
        check_detect_config(cfg(_raw(tmp_path, detect=None)))
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        check_detect_config(cfg(_raw(tmp_path, resume_checkpoint=False)))
    with pytest.raises(NotImplementedError, match="missing: detect.nll_threshold"):          # a JSON false is no threshold
        check_detect_config(cfg(_raw(tmp_path, detect=dict(DETECT, nll_threshold=False))))
    with pytest.raises(NotImplementedError, match="detect.against is one of 'image', 'reconstruction'"):
        check_detect_config(cfg(_raw(tmp_path, detect=dict(DETECT, against="recon"))))
    with pytest.raises(NotImplementedError, match="detect.weight is one of 'mask', 'none'"):
        check_detect_config(cfg(_raw(tmp_path, detect=dict(DETECT, weight=False))))
    with pytest.raises(NotImplementedError, match="missing: detect.labels.synthetic.radius"):
        check_detect_config(cfg(_raw(tmp_path, detect=dict(DETECT, labels={"synthetic": dict(n=2, contrast=0.8)}))))
    with pytest.raises(NotImplementedError, match="missing: detect.labels.synthetic.n, "):
        check_detect_config(cfg(_raw(tmp_path, detect=dict(DETECT, labels={"other": 1}))))
    assert detect_labels(cfg(_raw(tmp_path))) == (None, dict(n=2, radius=5, contrast=0.8))
    assert detect_labels(cfg(_raw(tmp_path, detect=dict(DETECT, labels=False)))) == (None, None)
    assert detect_labels(cfg(_raw(tmp_path, detect=dict(DETECT, labels="seg")))) == ("seg", None)
    raw = _raw(tmp_path)
    del raw["model"]["prior"]["pkeep"]
    with pytest.raises(NotImplementedError, match=r"model\.prior.*missing: pkeep"):          # check_prior_config's keys come first
        check_detect_config(cfg(raw))


def test_launcher_accepts_detect_only_with_the_prior(tmp_path):
    import importlib
    from utils import load_json
    rv = importlib.import_module("run_vqwnet")
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    assert rv.build_parser().parse_args(["-c", "x.json", "-p", "-m", "detect"]).mode == "detect"
    assert rv.check_arguments(cfg(_raw(tmp_path)), _args()) == ("second_step", 1)
    with pytest.raises(ValueError, match="-m detect: .* needs -p"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(prior=False))
    with pytest.raises(ValueError, match="-p with -v"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(vqgan=True))
    with pytest.raises(ValueError, match="-m detect: .* needs -p"):          # -v alone
        rv.check_arguments(cfg(_raw(tmp_path)), _args(prior=False, vqgan=True))
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        rv.check_arguments(cfg(_raw(tmp_path, resume_checkpoint=False)), _args())
    with pytest.raises(NotImplementedError, match=r"detect\.\{.*\}; missing: sigma$"):
        rv.check_arguments(cfg(_raw(tmp_path, detect={k: v for k, v in DETECT.items() if k != "sigma"})), _args())
    # every refusal pinned before stays a refusal
    with pytest.raises(ValueError, match="'train' or 'test'"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="fit"))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="test"))
    with pytest.raises(ValueError, match="data-parallel training of the prior is not built"):
        rv.check_arguments(cfg(_raw(tmp_path, num_gpus=2)), _args())
    assert rv.check_arguments(cfg(_raw(tmp_path, detect=None)), _args(mode="train")) == ("second_step", 1)          # training needs no detect section
    assert "-m detect" in rv.__doc__


def test_committed_detect_config_parses():
    from utils import load_json
    from trainers import check_detect_config
    from trainers.config import detect_labels
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_detect.json")
    c = load_json(path)
    check_detect_config(c)
    assert detect_labels(c) == (None, dict(n=3, radius=24, contrast=0.8)) and c.dataset.dataset_name == "synthetic"
    assert set(json.load(open(path))["detect"]) == {"n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed", "nll_threshold",
                                                    "sigma", "against", "weight", "labels"}
    assert "prior_vqgan_512_detect.json" in open(os.path.join(ROOT, "configs", "README.md")).read()


def test_detect_refuses_bad_arguments_before_any_kernel():
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    tr = PriorTrainer(VQGAN(**P.TINY_VQGAN), GPT(**P.gpt_kwargs("p64")), device="cpu")
    image = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="nll_threshold"):
        tr.detect({"image": image}, None)
    with pytest.raises(ValueError, match="against='pixels'"):
        tr.detect({"image": image}, 1.0, against="pixels")
    with pytest.raises(ValueError, match="weight='soft'"):
        tr.detect({"image": image}, 1.0, weight="soft")
    with pytest.raises(ValueError, match="sigma"):
        tr.detect({"image": image}, 1.0, sigma=-1.0)
