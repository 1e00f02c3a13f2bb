"""CPU-side checks of editing with the code prior (no GPU): the C ABI and operator plumbing of vqw_sample_filtered and
vqw_paste_cells, their refusals before any device work, the float64 restatement (tests/prior_edit_ref.py) against brute force on
the GPU test's own cases, every refusal of GPT.generate_masked and PriorTrainer.edit that comes before a kernel, the host reduction
of a pixel mask to cells, and the launcher's `-m edit`."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import gpt_ref as G
import prior_ref as P
import prior_edit_ref as R

NEW_SYMBOLS = ("vqw_sample_filtered", "vqw_paste_cells")


def _gpt(name="p64", **kw):
    from networks import GPT
    args = P.gpt_kwargs(name)
    args.update(kw)
    return GPT(**args)


def _trainer():
    from networks import VQGAN
    from trainers import PriorTrainer
    return PriorTrainer(VQGAN(**P.TINY_VQGAN), _gpt(), device="cpu")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and s in ops_, s
    res, args = _lib.SIGNATURES["vqw_sample_filtered"]
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert res is ctypes.c_int and args == [p, p, p, p, p, i, i, f, i, f, p]
    names = [n for _, n, _ in _lib.parse_header()["vqw_sample_filtered"][1]]
    assert names == ["logits", "u", "forced", "out", "logp", "B", "V", "temperature", "top_k", "top_p", "stream"]
    sch = str(torch.ops.vqw.sample_filtered.default._schema)
    assert "Tensor? logits" in sch and "Tensor? u" in sch and "Tensor? forced" in sch and "Tensor(a!)? out" in sch and "Tensor(b!)? logp" in sch
    assert "float temperature" in sch and "int top_k" in sch and "float top_p" in sch
    assert _lib.SIGNATURES["vqw_paste_cells"][1] == [p, p, p, p, i, i, i, i, i, i, p]
    sch = str(torch.ops.vqw.paste_cells.default._schema)
    assert "Tensor? image" in sch and "Tensor? edit" in sch and "Tensor? cellmask" in sch and "Tensor(a!)? out" in sch and "int h" in sch


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    P_ = 4096          # a 16-byte aligned non-null stand-in for every pointer

    def samp(B=2, V=10, temp=1.0, k=0, top_p=1.0, logits=P_, u=P_, out=P_):
        return L.vqw_sample_filtered(logits, u, None, out, None, B, V, temp, k, top_p, None)

    for V in (0, -3, 65537):
        assert samp(V=V) != 0 and b"vqw_sample_filtered" in L.vqw_last_error() and b"1 <= V <= 65536" in L.vqw_last_error()
    assert samp(B=0) != 0 and b"B=0" in L.vqw_last_error()
    for temp in (0.0, -1.0, float("nan")):
        assert samp(temp=temp) != 0 and b"temperature" in L.vqw_last_error() and b"positive" in L.vqw_last_error()
    assert samp(k=-1) != 0 and b"top_k=-1" in L.vqw_last_error()
    for top_p in (0.0, -0.1, float("nan")):
        assert samp(top_p=top_p) != 0 and b"top_p" in L.vqw_last_error() and b"positive" in L.vqw_last_error()
    for kw in (dict(logits=None), dict(u=None), dict(out=None)):
        assert samp(**kw) != 0 and b"null pointer" in L.vqw_last_error()

    def paste(N=2, H=8, W=8, C=1, h=4, w=4, image=P_, edit=P_, mask=P_, out=P_):
        return L.vqw_paste_cells(image, edit, mask, out, N, H, W, C, h, w, None)

    for kw in (dict(image=None), dict(edit=None), dict(mask=None), dict(out=None)):
        assert paste(**kw) != 0 and b"null pointer" in L.vqw_last_error()
    for kw in (dict(h=3), dict(w=3), dict(h=0), dict(w=16)):
        assert paste(**kw) != 0 and b"multiples of the cell grid" in L.vqw_last_error()
    assert paste(N=0) != 0 and b"positive" in L.vqw_last_error()
    assert paste(N=65536, H=256, W=256, h=4, w=4) != 0 and b"32-bit" in L.vqw_last_error()


def test_operators_have_no_cpu_route_and_trace_under_fake_tensors():
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_filtered(torch.zeros(2, 10), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.paste_cells(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 2, dtype=torch.uint8))
    with FakeTensorMode():
        z, u = torch.empty(3, 64, device="cuda"), torch.empty(3, device="cuda")
        tok, lp = ops.sample_filtered(z, u, torch.empty(3, dtype=torch.long, device="cuda"), 0.5, 10, 0.9)
        assert tok.shape == (3,) and tok.dtype == torch.long and lp.shape == (3,) and lp.dtype == torch.float32
        assert ops.sample_filtered(z, u, return_logp=False)[1] is None
        x = torch.empty(2, 1, 8, 8, device="cuda")
        assert ops.paste_cells(x, x, torch.empty(2, 4, 4, dtype=torch.uint8, device="cuda")).shape == (2, 1, 8, 8)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("V,k", [(1, 0), (100, 0), (100, 10), (1000, 100)])
def test_filter_ref_against_brute_force(V, k):
    """The sort-based strictly-greater mass against the O(V^2) definition; top_p >= 1 is gpt_ref.sample_ref's kept set; the share
    of unclear rows of every case stays within the cap before anything about the device."""
    for temp in G.SAMPLE_TEMPS:
        logits, u = G.sample_inputs(V, k, temp)
        _, _, k1 = G.sample_ref(logits, u, temp, k)
        assert torch.equal(R.filter_ref(logits, temp, k, 1.0)[0], k1)
        s = logits.double() / temp
        p = torch.where(k1, torch.exp(s - s.max(dim=1, keepdim=True).values), torch.zeros_like(s))
        g = (p[:, None, :] * (s[:, None, :] > s[:, :, None])).sum(-1) / p.sum(-1, keepdim=True)
        for top_p in (0.3, 0.9, R.TINY_TOP_P):
            kept, margin = R.filter_ref(logits, temp, k, top_p)
            sure = (g - top_p).abs() > 1e-12
            assert torch.equal((kept == (k1 & (g <= top_p)))[sure], torch.ones_like(kept)[sure])
            assert bool(kept.any(dim=1).all()) and bool((kept & ~k1).sum() == 0)
            assert bool((kept | (s < s.max(dim=1, keepdim=True).values)).all()), "the largest entry always stays"
            pick, lp, clear, _ = R.sample_filtered_ref(logits, u, None, temp, k, top_p)
            assert int((~clear).sum()) <= G.SAMPLE_UNCLEAR_CAP * G.SAMPLE_B and bool(kept.gather(1, pick[:, None]).all())


def test_the_largest_case_stays_within_the_cap():
    for temp in G.SAMPLE_TEMPS:
        logits, u = G.sample_inputs(16384, 100, temp)
        for top_p in R.TOP_PS:
            clear = R.sample_filtered_ref(logits, u, None, temp, 100, top_p)[2]
            assert int((~clear).sum()) <= G.SAMPLE_UNCLEAR_CAP * G.SAMPLE_B


def test_forced_rows_of_the_restatement():
    logits, u = G.sample_inputs(100, 10, 1.0)
    forced = torch.full((G.SAMPLE_B,), -7, dtype=torch.long)
    forced[0], forced[1], forced[2] = 5, 100, 99
    free = R.sample_filtered_ref(logits, u, None, 1.0, 10, 0.9)
    pick, lp, clear, _ = R.sample_filtered_ref(logits, u, forced, 1.0, 10, 0.9)
    assert int(pick[0]) == 5 and int(pick[2]) == 99 and torch.equal(pick[3:], free[0][3:]) and int(pick[1]) == int(free[0][1])
    assert bool(torch.isnan(lp[1])) and bool(torch.isfinite(lp[[0, 2]]).all()) and float(lp[0]) == float(torch.log_softmax(logits[0].double(), 0)[5])


# ------------------------------------------------------------------------------------------------ generate_masked's refusals
def test_generate_masked_refuses_before_any_kernel():
    m = _gpt().eval()
    idx, known = torch.zeros(2, 1, dtype=torch.long), torch.zeros(2, 16, dtype=torch.long)
    every = np.ones(16, dtype=bool)
    with pytest.raises(RuntimeError, match="inference only, the model is in training mode"):
        _gpt().train().generate_masked(idx, known, every)
    with pytest.raises(RuntimeError, match=r"a prompt of 2 tokens \+ 16 positions - 1 exceeds block_size=16"):
        m.generate_masked(torch.zeros(2, 2, dtype=torch.long), known, every)
    for bad in (np.ones(15, dtype=bool), np.ones((3, 16), dtype=bool), np.ones(16, dtype=np.int64), torch.ones(16)):
        with pytest.raises(ValueError, match="resample must be a host bool array"):
            m.generate_masked(idx, known, bad)
    with pytest.raises(ValueError, match="known .B, S. torch.long"):
        m.generate_masked(idx, known[:1], every)
    with pytest.raises(ValueError, match="known .B, S. torch.long"):
        m.generate_masked(idx, known.int(), every)
    for top_p in (0, 0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="top_p=.* must lie in \\(0, 1\\]"):
            m.generate_masked(idx, known, every, top_p=top_p)
    with pytest.raises(ValueError, match="temperature"):
        m.generate_masked(idx, known, every, temperature=0.0)
    late = np.arange(16) >= 6
    with pytest.raises(ValueError, match=r"uniforms of shape \(16, 2\), \(S - j0, B\) = \(10, 2\) expected"):
        m.generate_masked(idx, known, late, uniforms=torch.zeros(16, 2))
    p96 = _gpt("p96").eval()
    with pytest.raises(RuntimeError, match="n_unmasked=3 exceeds the 2 tokens of the prefill"):
        p96.generate_masked(idx, known, np.arange(16) >= 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # everything else is in order: the first kernel refuses the CPU
        p96.generate_masked(idx, known, np.arange(16) >= 2)


# ------------------------------------------------------------------------------------------------ edit's host side
def test_cell_mask_reduces_on_the_host():
    tr = _trainer()
    assert (tr.h, tr.w) == (4, 4)
    px = np.zeros((8, 8), dtype=bool)
    px[5, 2] = True
    want = np.zeros((4, 4), dtype=bool)
    want[2, 1] = True
    got = tr.cell_mask(3, mask=px)
    assert got.shape == (3, 4, 4) and got.dtype == np.bool_ and all(np.array_equal(g, want) for g in got)
    assert np.array_equal(tr.cell_mask(3, mask=want), got) and np.array_equal(tr.cell_mask(3, mask=want.astype(np.uint8) * 7), got)
    per_row = np.zeros((2, 8, 8), dtype=bool)
    per_row[1, 7, 7] = True
    got = tr.cell_mask(2, mask=per_row)
    assert not got[0].any() and got[1].sum() == 1 and got[1, 3, 3]
    box = tr.cell_mask(2, box=(1, 3, 4, 5))          # pixel rows 1..2, column 4: the cells (0, 2) and (1, 2)
    assert box.sum() == 4 and box[0, 0, 2] and box[0, 1, 2]
    assert not tr.cell_mask(2, box=(3, 3, 0, 8)).any()          # an empty box
    assert tr.cell_mask(1, box=(0, 8, 0, 8)).all()
    for bad in (np.zeros((3, 8), dtype=bool), np.zeros((3, 8, 8), dtype=bool), np.zeros((2, 2, 8, 8), dtype=bool)):
        with pytest.raises(ValueError, match="mask of shape"):
            tr.cell_mask(2, mask=bad)
    with pytest.raises(ValueError, match="box"):
        tr.cell_mask(2, box=(0, 9, 0, 8))


def test_edit_refuses_two_selectors_or_none_before_any_kernel():
    tr = _trainer()
    batch = {"ids": torch.zeros(2, 16, dtype=torch.long)}
    m = np.zeros((4, 4), dtype=bool)
    for kw in (dict(), dict(mask=m, box=(0, 2, 0, 2)), dict(mask=m, nll_threshold=1.0), dict(box=(0, 2, 0, 2), nll_threshold=1.0),
               dict(mask=m, box=(0, 2, 0, 2), nll_threshold=1.0)):
        with pytest.raises(ValueError, match="exactly one of mask, box and nll_threshold"):
            tr.edit(batch, **kw)
    with pytest.raises(ValueError, match="n_candidates=0"):
        tr.edit(batch, mask=m, n_candidates=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.edit(batch, mask=m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.token_nll(batch)
    assert tr.gpt.training


# ------------------------------------------------------------------------------------------------ the launcher
def _launcher():
    import importlib
    return importlib.import_module("run_vqwnet")


def _args(**kw):
    a = dict(config="x.json", mode="edit", multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)
    a.update(kw)
    return argparse.Namespace(**a)


EDIT = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[24, 32, 8, 24])


def _raw(tmp_path, edit=EDIT, **run):
    raw = P.prior_run_config(tmp_path / "out", **dict(dict(resume_checkpoint="prior.ckpt"), **run))
    if edit is not None:
        raw["edit"] = dict(edit)
    return raw


def test_launcher_accepts_edit_only_with_the_prior(tmp_path):
    from utils import load_json
    rv = _launcher()
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    assert rv.build_parser().parse_args(["-c", "x.json", "-p", "-m", "edit"]).mode == "edit"
    assert rv.check_arguments(cfg(_raw(tmp_path)), _args()) == ("second_step", 1)
    with pytest.raises(ValueError, match="-m edit: .* needs -p"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(prior=False))
    with pytest.raises(ValueError, match="-m edit: .* needs -p"):
        rv.check_arguments(cfg(_raw(tmp_path)), argparse.Namespace(config="x.json", mode="edit", multiwindow=False, vqgan=False, rank=None, seed=None))
    # every message pinned before stays
    with pytest.raises(ValueError, match="'train' or 'test'"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="fit"))
    with pytest.raises(ValueError, match="'train' or 'test'"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="fit", prior=False))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="test"))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step and no inference export"):
        rv.check_arguments(cfg(_raw(tmp_path, training_mode="inference")), _args())
    with pytest.raises(ValueError, match="-p with -v"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(vqgan=True))
    with pytest.raises(ValueError, match="data-parallel training of the prior is not built"):
        rv.check_arguments(cfg(_raw(tmp_path, num_gpus=2)), _args())
    assert rv.check_arguments(cfg(_raw(tmp_path, edit=None)), _args(mode="train")) == ("second_step", 1)          # training needs no edit section
    assert "-m edit" in rv.__doc__


def test_check_edit_config_names_what_is_missing(tmp_path):
    from utils import load_json
    from trainers import check_edit_config
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    check_edit_config(cfg(_raw(tmp_path)))
    for key in ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed"):
        bad = dict(EDIT)
        del bad[key]
        with pytest.raises(NotImplementedError, match=r"edit\.\{.*\}; missing: %s$" % key):
            check_edit_config(cfg(_raw(tmp_path, edit=bad)))
    with pytest.raises(NotImplementedError, match="missing: n_slices, n_candidates, temperature, top_k, top_p, seed"):
        check_edit_config(cfg(_raw(tmp_path, edit=None)))
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        check_edit_config(cfg(_raw(tmp_path, resume_checkpoint=False)))
    none = {k: v for k, v in EDIT.items() if k != "box"}
    with pytest.raises(NotImplementedError, match="exactly one of edit.{box, mask_path, nll_threshold}; given: none"):
        check_edit_config(cfg(_raw(tmp_path, edit=none)))
    with pytest.raises(NotImplementedError, match="given: box, nll_threshold"):
        check_edit_config(cfg(_raw(tmp_path, edit=dict(EDIT, nll_threshold=2.5))))
    check_edit_config(cfg(_raw(tmp_path, edit=dict(none, nll_threshold=2.5, box=False))))          # a JSON false is no selector
    check_edit_config(cfg(_raw(tmp_path, edit=dict(none, mask_path="mask.npy"))))
    raw = _raw(tmp_path)
    del raw["model"]["prior"]["pkeep"]
    with pytest.raises(NotImplementedError, match=r"model\.prior.*missing: pkeep"):          # check_prior_config's keys come first
        check_edit_config(cfg(raw))


def test_committed_edit_config_parses():
    from utils import load_json
    from trainers import check_edit_config, configure_prior
    rv = _launcher()
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_edit.json")
    config = load_json(path)
    assert rv.check_arguments(config, _args(config=path)) == ("second_step", 1)
    check_edit_config(config)
    raw, ref = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "prior_vqgan_512.json")))
    assert raw["model"] == ref["model"] and raw["prior_optim"] == ref["prior_optim"] and raw["dataset"] == ref["dataset"]
    e = raw["edit"]
    assert (e["n_slices"], e["n_candidates"], e["temperature"], e["top_k"], e["top_p"], e["seed"]) == (4, 8, 1.0, 32, 0.95, 0)
    y0, y1, x0, x1 = e["box"]          # whole cells of 32 x 32 pixels: a quarter of the 16 x 16 latent
    assert all(v % 32 == 0 for v in e["box"]) and (y1 - y0) // 32 * ((x1 - x0) // 32) == 64
    assert configure_prior(config).block_size == 256
    assert "prior_vqgan_512_edit.json" in open(os.path.join(ROOT, "configs", "README.md")).read()
