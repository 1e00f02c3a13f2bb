"""The pseudo-likelihood map of the masked prior without a GPU: the lattice of tests/pseudo_nll_ref.py (the groups partition the grid,
the chunked restatement equals the unchunked one), the header and the C ABI's refusals, the config checks of detect.pseudo and
edit.pnll_threshold - the accepting branch, each new refusal, and the old refusals with the old keys - and the refusals of the new
model and trainer arguments."""
import argparse
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import gpt_ref as G
import prior_ref as P
import pseudo_nll_ref as PN

NEW_SYMBOLS = ("vqw_lattice_inputs", "vqw_lattice_gather_ln")


# ------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("h,w", [(4, 4), (3, 5)])
def test_groups_partition_the_grid(h, w):
    for sy, sx in ((1, 1), (2, 2), (3, 2), (4, 4), (h, w)):
        if sy > h or sx > w:
            continue
        g = PN.groups(h, w, sy, sx)
        S = sy * sx
        assert g.shape == (h * w,) and g.min() == 0 and g.max() == S - 1, (h, w, sy, sx)
        counts = np.bincount(g, minlength=S)
        assert counts.sum() == h * w and (counts >= 1).all(), (h, w, sy, sx)          # every position in one group, no group empty
        ids = np.arange(1, h * w + 1)[None]
        inp = PN.lattice_inputs(ids, h, w, sy, sx, 0, S, 0)
        assert ((inp == 0).sum(0) == 1).all()                                          # every position is masked in exactly one pass
        assert np.array_equal((inp == 0).argmax(0), g)                                 # and that pass is its group
        if (sy, sx) == (h, w):
            assert np.array_equal(g, np.arange(h * w))                                 # one masked position per pass
        if (sy, sx) == (1, 1):
            assert (inp == 0).all()
    # two members of a group are never neighbours at stride (2, 2): every masked code sees its eight neighbours
    g = PN.groups(h, w, 2, 2).reshape(h, w)
    for y in range(h):
        for x in range(w):
            for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
                if y + dy < h and 0 <= x + dx < w:
                    assert g[y, x] != g[y + dy, x + dx], (y, x, dy, dx)


def test_chunked_reference_equals_the_unchunked_one():
    from networks import MaskedGPT
    kw = dict(vocab_size=32, block_size=16, n_layer=2, n_head=2, n_embed=64)
    torch.manual_seed(5)
    st = PN.state64(G.init_gpt_(MaskedGPT(**kw), 5))
    ids = torch.randint(0, 32, (2, 16), generator=torch.Generator().manual_seed(6))
    for sy, sx in ((2, 2), (3, 2), (4, 4)):
        whole, z = PN.pseudo_nll_ref(ids, st, 2, 2, 4, 4, sy, sx, 32)
        assert whole.shape == (2, 4, 4) and z.shape == (2, 16, 32) and bool((whole > 0).all())
        for chunk in (1, 3, 5):
            part, zc = PN.pseudo_nll_ref(ids, st, 2, 2, 4, 4, sy, sx, 32, chunk=chunk)
            assert torch.equal(part, whole) and torch.equal(zc, z), (sy, sx, chunk)          # a sample's pass does not see the other rows
    # stride (h, w): position t is the cross-entropy of the forward with only t masked
    exact = PN.pseudo_nll_ref(ids, st, 2, 2, 4, 4, 4, 4, 32)[0].reshape(2, 16)
    for t in (0, 7, 15):
        inp = ids.clone()
        inp[:, t] = 32
        z = G.gpt_ref(inp, st, 2, 2)[0][:, t]
        assert torch.allclose(exact[:, t], torch.logsumexp(z, -1) - z.gather(-1, ids[:, t:t + 1])[:, 0], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_two_entry_points():
    from hipops import _lib, library, ops
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and s in ops_, s
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES["vqw_lattice_inputs"] == (i, [p, p, i, i, i, i, i, i, i, l, p])
    assert _lib.SIGNATURES["vqw_lattice_gather_ln"] == (i, [p, p, p, p, i, i, i, i, i, i, i, i, f, p])
    sch = str(torch.ops.vqw.lattice_inputs.default._schema)
    assert "Tensor? ids" in sch and "Tensor(a!)? inp" in sch and "int mask_token" in sch and "int s0" in sch and "int ns" in sch
    sch = str(torch.ops.vqw.lattice_gather_ln.default._schema)
    assert all("Tensor? %s" % n in sch for n in ("x", "gamma", "beta")) and "Tensor(a!)? y" in sch and "float eps" in sch
    assert callable(ops.lattice_inputs) and callable(ops.lattice_gather_ln)


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    A = 4096          # an aligned non-null stand-in for every pointer

    def refused(fn, args, pattern):
        assert fn(*args) != 0, pattern
        msg = (L.vqw_last_error() or b"").decode()
        assert pattern in msg, (pattern, msg)

    def li(ids=A, inp=2 * A, B=2, h=4, w=4, sy=2, sx=2, s0=0, ns=4, mask_token=32):
        return (ids, inp, B, h, w, sy, sx, s0, ns, mask_token, None)

    def gl(x=A, gamma=A, beta=A, y=2 * A, B=2, h=4, w=4, E=64, sy=2, sx=2, s0=0, ns=4, eps=1e-5):
        return (x, gamma, beta, y, B, h, w, E, sy, sx, s0, ns, ctypes.c_float(eps), None)

    for fn, mk in ((L.vqw_lattice_inputs, li), (L.vqw_lattice_gather_ln, gl)):
        refused(fn, mk(B=0), "B=0, h=4, w=4 must be at least 1")
        refused(fn, mk(h=0), "must be at least 1")
        refused(fn, mk(sy=0), "stride (sy=0, sx=2) must lie in [1, h=4] x [1, w=4]")
        refused(fn, mk(sy=5), "stride (sy=5, sx=2) must lie in")
        refused(fn, mk(sx=5), "stride (sy=2, sx=5) must lie in")
        refused(fn, mk(s0=-1), "the chunk [s0=-1")
        refused(fn, mk(ns=0), "the chunk [s0=0, s0 + ns=0)")
        refused(fn, mk(s0=2, ns=3), "must be a non-empty part of the S = sy sx = 4 passes")
        refused(fn, mk(h=300, w=300), "T = h w = 90000 must not exceed 65536")
        refused(fn, mk(B=40000, h=256, w=256, sy=1, sx=1, ns=1), "are too many")
    refused(L.vqw_lattice_inputs, li(mask_token=-1), "mask_token=-1 must not be negative")
    refused(L.vqw_lattice_inputs, li(ids=None), "null pointer")
    refused(L.vqw_lattice_inputs, li(inp=None), "null pointer")
    refused(L.vqw_lattice_inputs, li(ids=A + 4), "8-byte aligned")
    refused(L.vqw_lattice_inputs, li(inp=A), "inp must not be ids itself")
    for E in (0, 6, 4100):
        refused(L.vqw_lattice_gather_ln, gl(E=E), "E=%d must be a multiple of 4 with 4 <= E <= 4096" % E)
    for name in ("x", "gamma", "beta", "y"):
        refused(L.vqw_lattice_gather_ln, gl(**{name: None}), "null pointer")
        refused(L.vqw_lattice_gather_ln, gl(**{name: A + 8}), "16-byte aligned")
    refused(L.vqw_lattice_gather_ln, gl(y=A), "y must not be x itself")


def test_operators_refuse_cpu_tensors_and_bad_shapes():
    from hipops import ops
    ids = torch.zeros(2, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.lattice_inputs(ids, (4, 4), (2, 2), 0, 4, 32)
    with pytest.raises(RuntimeError, match="ids"):
        ops.lattice_inputs(ids.int(), (4, 4), (2, 2), 0, 4, 32)
    with pytest.raises(ValueError, match="must be pairs of integers"):
        ops.lattice_inputs(ids, (4, 4), 2, 0, 4, 32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.lattice_gather_ln(torch.zeros(8, 16, 64), torch.ones(64), torch.zeros(64), torch.zeros(2, 16, 64), (4, 4), (2, 2), 0, 4)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.lattice_gather_ln(torch.zeros(8, 16, 64, requires_grad=True), torch.ones(64), torch.zeros(64), torch.zeros(2, 16, 64), (4, 4), (2, 2), 0, 4)


# ------------------------------------------------------------------------------------------------ the config
EDIT = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5)
DETECT = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=False, sigma=1.0, against="image",
              weight="mask", labels=False)
MASKED = dict(n_steps=4, choice_temperature=4.5, mask_seed=3)
COND = dict(source="label", n_labels=2, labels={"synthetic": dict(n=3, radius=4, contrast=0.5)})


def _raw(tmp_path, masked=True, edit=None, detect=None):
    raw = P.prior_run_config(tmp_path / "out", resume_checkpoint="prior.ckpt")
    if masked:
        raw["model"]["prior"]["masked"] = dict(MASKED) if masked is True else masked
    if edit is not None:
        raw["edit"] = dict(EDIT, **edit)
    if detect is not None:
        raw["detect"] = dict(DETECT, **detect)
    return raw


def _cfg(tmp_path, raw):
    from utils import load_json
    return load_json(write_config(tmp_path / "c.json", raw))


def _launcher():
    spec = importlib.util.spec_from_file_location("run_vqwnet_pseudo", os.path.join(ROOT, "medical-image-editing_amd", "run_vqwnet.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    return rv


def _args(mode):
    return argparse.Namespace(config="x.json", mode=mode, multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)


PSEUDO = dict(threshold=3.5, stride=[2, 2])


def test_detect_pseudo_is_accepted_with_the_masked_prior(tmp_path):
    from trainers import check_detect_config, detect_pseudo
    c = _cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=PSEUDO)))
    check_detect_config(c)
    assert detect_pseudo(c) == {"threshold": 3.5, "stride": (2, 2)}
    assert _launcher().check_arguments(c, _args("detect")) == ("second_step", 1)
    c = _cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=dict(threshold=2, stride=[16, 16]))))
    assert detect_pseudo(c) == {"threshold": 2.0, "stride": (16, 16)}
    for absent in ({}, dict(pseudo=False)):          # absent or `false`: no pseudo detection
        assert detect_pseudo(_cfg(tmp_path, _raw(tmp_path, detect=absent))) is None


def test_detect_without_pseudo_keeps_the_present_refusal(tmp_path):
    rv = _launcher()
    c = _cfg(tmp_path, _raw(tmp_path, detect=dict(nll_threshold=2.0)))
    with pytest.raises(NotImplementedError, match="-m detect with model.prior.masked: detection selects the codes to restore by a "
                                                  "raster-order likelihood, which the masked prior does not define"):
        rv.check_arguments(c, _args("detect"))
    assert "detect.pseudo" in rv.__doc__ and "edit.pnll_threshold" in rv.__doc__


def test_detect_pseudo_wants_nll_threshold_false(tmp_path):
    from trainers import check_detect_config
    with pytest.raises(ValueError, match=r"detect\.nll_threshold=2\.0 beside detect\.pseudo.*set detect\.nll_threshold to false"):
        check_detect_config(_cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=PSEUDO, nll_threshold=2.0))))


def test_detect_pseudo_needs_the_masked_prior(tmp_path):
    from trainers import check_detect_config
    with pytest.raises(ValueError, match=r"detect\.pseudo .* needs model\.prior\.masked"):
        check_detect_config(_cfg(tmp_path, _raw(tmp_path, masked=False, detect=dict(pseudo=PSEUDO))))


def test_detect_pseudo_refuses_the_conditional_masked_prior(tmp_path):
    from trainers import check_detect_config
    raw = _raw(tmp_path, masked=dict(MASKED, cond=COND), detect=dict(pseudo=PSEUDO))
    with pytest.raises(NotImplementedError, match=r"detect\.pseudo with model\.prior\.masked\.cond"):
        check_detect_config(_cfg(tmp_path, raw))
    with pytest.raises(NotImplementedError):
        _launcher().check_arguments(_cfg(tmp_path, raw), _args("detect"))


def test_detect_pseudo_names_missing_keys_and_bad_values(tmp_path):
    from trainers import check_detect_config
    for key in ("threshold", "stride"):
        bad = dict(PSEUDO)
        del bad[key]
        with pytest.raises(NotImplementedError, match=r"detect\.pseudo\.\{threshold, stride\}; missing: %s$" % key):
            check_detect_config(_cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=bad))))
    for stride in ([2], [2, 0], [2, 2.5], [1, 2, 3], 2):
        with pytest.raises(ValueError, match=r"detect\.pseudo\.stride=.* must be \[sy, sx\], two integers >= 1"):
            check_detect_config(_cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=dict(PSEUDO, stride=stride)))))
    with pytest.raises(ValueError, match=r"detect\.pseudo\.threshold='high' must be a number"):
        check_detect_config(_cfg(tmp_path, _raw(tmp_path, detect=dict(pseudo=dict(PSEUDO, threshold="high")))))


def test_old_detect_refusals_stay_with_the_old_keys(tmp_path):
    from trainers import check_detect_config
    ok = dict(nll_threshold=2.0)
    check_detect_config(_cfg(tmp_path, _raw(tmp_path, masked=False, detect=ok)))          # the autoregressive prior's config still parses
    with pytest.raises(NotImplementedError, match="needs a number for detect.nll_threshold, the token_nll above which a code is restored; "
                                                  "missing: detect.nll_threshold"):
        check_detect_config(_cfg(tmp_path, _raw(tmp_path, masked=False, detect={})))
    bad = dict(DETECT, **ok)
    del bad["sigma"]
    raw = _raw(tmp_path, masked=False)
    raw["detect"] = bad
    with pytest.raises(NotImplementedError, match=r"detect\.\{.*\}; missing: sigma$"):
        check_detect_config(_cfg(tmp_path, raw))
    with pytest.raises(NotImplementedError, match="detect.against is one of 'image', 'reconstruction'"):
        check_detect_config(_cfg(tmp_path, _raw(tmp_path, masked=False, detect=dict(ok, against="both"))))
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        raw = _raw(tmp_path, masked=False, detect=ok)
        raw["run"]["resume_checkpoint"] = False
        check_detect_config(_cfg(tmp_path, raw))


def test_edit_pnll_threshold_is_a_selector_of_the_masked_prior(tmp_path):
    from trainers import check_edit_config, edit_pnll
    c = _cfg(tmp_path, _raw(tmp_path, edit=dict(pnll_threshold=3.0)))
    check_edit_config(c)
    assert edit_pnll(c) == (3.0, None)
    c = _cfg(tmp_path, _raw(tmp_path, edit=dict(pnll_threshold=3.0, stride=[4, 4], n_steps=6)))
    check_edit_config(c)
    assert edit_pnll(c) == (3.0, (4, 4))
    assert _launcher().check_arguments(c, _args("edit")) == ("second_step", 1)
    assert edit_pnll(_cfg(tmp_path, _raw(tmp_path, edit=dict(box=[8, 16, 8, 24])))) is None
    check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(box=[8, 16, 8, 24], pnll_threshold=False))))          # a JSON false is no selector
    check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=dict(MASKED, cond=COND), edit=dict(pnll_threshold=3.0))))      # the conditional trainer's fourth


def test_edit_pnll_threshold_refusals(tmp_path):
    from trainers import check_edit_config
    with pytest.raises(NotImplementedError, match=r"exactly one of edit\.\{box, mask_path, nll_threshold, pnll_threshold\}; given: box, pnll_threshold"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(box=[8, 16, 8, 24], pnll_threshold=3.0))))
    with pytest.raises(NotImplementedError, match=r"pnll_threshold\}; given: none"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit={})))
    with pytest.raises(ValueError, match=r"edit\.pnll_threshold .* needs model\.prior\.masked"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=False, edit=dict(pnll_threshold=3.0))))
    with pytest.raises(ValueError, match=r"edit\.stride .* needs model\.prior\.masked"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=False, edit=dict(box=[8, 16, 8, 24], stride=[2, 2]))))
    with pytest.raises(ValueError, match=r"edit\.stride=\[2, 2\] is the lattice of edit\.pnll_threshold and needs it"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(box=[8, 16, 8, 24], stride=[2, 2]))))
    with pytest.raises(ValueError, match=r"edit\.stride=\[0, 2\] must be \[sy, sx\]"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(pnll_threshold=3.0, stride=[0, 2]))))
    with pytest.raises(ValueError, match=r"edit\.pnll_threshold='x' must be a number"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(pnll_threshold="x"))))


def test_old_edit_refusals_stay_verbatim(tmp_path):
    from trainers import check_edit_config
    with pytest.raises(NotImplementedError, match=r"needs exactly one of edit\.\{box, mask_path, nll_threshold\}; given: none$"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=False, edit={})))
    with pytest.raises(NotImplementedError, match=r"needs exactly one of edit\.\{box, mask_path, nll_threshold\}; given: box, nll_threshold$"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=False, edit=dict(box=[8, 16, 8, 24], nll_threshold=2.5))))
    with pytest.raises(NotImplementedError, match="edit.nll_threshold selects by a raster-order likelihood, which the masked prior does not define; "
                                                  "use edit.box or edit.mask_path"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, edit=dict(nll_threshold=2.5))))
    with pytest.raises(ValueError, match=r"edit\.n_steps=12 .* needs model\.prior\.masked"):
        check_edit_config(_cfg(tmp_path, _raw(tmp_path, masked=False, edit=dict(box=[8, 16, 8, 24], n_steps=12))))


def test_committed_configs_parse():
    from utils import load_json
    from networks import MaskedGPT
    from trainers import check_detect_config, check_edit_config, configure_prior, detect_pseudo, edit_pnll, prior_masked
    rv = _launcher()
    detect, edit = (os.path.join(ROOT, "configs", n) for n in ("prior_vqgan_512_masked_detect.json", "prior_vqgan_512_masked_pnll_edit.json"))
    c = load_json(detect)
    check_detect_config(c)
    assert rv.check_arguments(c, _args("detect")) == ("second_step", 1)
    assert detect_pseudo(c)["stride"] == (2, 2) and c.detect.nll_threshold is None and isinstance(configure_prior(c), MaskedGPT)
    c = load_json(edit)
    check_edit_config(c)
    assert rv.check_arguments(c, _args("edit")) == ("second_step", 1) and edit_pnll(c)[1] == (2, 2)
    raw = {n: json.load(open(os.path.join(ROOT, "configs", n + ".json"))) for n in
           ("prior_vqgan_512_masked", "prior_vqgan_512_masked_detect", "prior_vqgan_512_masked_pnll_edit", "prior_vqgan_512_detect")}
    for new in ("prior_vqgan_512_masked_detect", "prior_vqgan_512_masked_pnll_edit"):
        a, b = raw[new], raw["prior_vqgan_512_masked"]
        assert a["model"] == b["model"] and a["prior_optim"] == b["prior_optim"] and a["dataset"] == b["dataset"]
        assert a["save"]["study_name"] == new and prior_masked(load_json(os.path.join(ROOT, "configs", new + ".json"))) is not None
    d, old = dict(raw["prior_vqgan_512_masked_detect"]["detect"]), dict(raw["prior_vqgan_512_detect"]["detect"])
    assert d.pop("pseudo") == {"threshold": old.pop("nll_threshold"), "stride": [2, 2]} and d.pop("nll_threshold") is False
    assert d == old          # every other key of the autoregressive prior's detection
    readme = open(os.path.join(ROOT, "configs", "README.md")).read()
    assert "prior_vqgan_512_masked_detect.json" in readme and "prior_vqgan_512_masked_pnll_edit.json" in readme


# ------------------------------------------------------------------------------------------------ the model and the trainers
def test_masked_gpt_pseudo_nll_refusals_on_the_cpu():
    from networks import MaskedGPT
    m = MaskedGPT(vocab_size=32, block_size=16, n_layer=2, n_head=2, n_embed=64)
    ids = torch.zeros(2, 16, dtype=torch.long)
    for bad, pattern in ((ids.int(), r"ids \(B, T\) torch\.long"), (ids[:, :15], r"T = h w = 4 x 4"), (ids[0], r"ids \(B, T\)")):
        with pytest.raises(ValueError, match=pattern):
            m.pseudo_nll(bad, (4, 4))
    with pytest.raises(ValueError, match=r"T = h w = 4 x 8 <= block_size=16"):
        m.pseudo_nll(torch.zeros(2, 32, dtype=torch.long), (4, 8))
    with pytest.raises(ValueError, match=r"grid=4 must be a pair"):
        m.pseudo_nll(ids, 4)
    for stride in ((0, 2), (5, 1), (2, 5), (2,), 2, (2.5, 2), (1, 2, 3)):
        with pytest.raises(ValueError, match=r"stride=.* must be a pair \(sy, sx\) of integers in \[1, h = 4\] x \[1, w = 4\]"):
            m.pseudo_nll(ids, (4, 4), stride=stride)
    for max_rows in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match=r"max_rows=.* must be an integer >= 1"):
            m.pseudo_nll(ids, (4, 4), max_rows=max_rows)
    with pytest.raises(ValueError, match=r"cond tokens \(B, T\) = \(2, 16\)"):
        m.pseudo_nll(ids, (4, 4), cond=(ids[:, :4], torch.zeros(3, 64), None))
    m.train()
    with pytest.raises(RuntimeError, match="ROCm device"):          # a CPU tensor reaches no kernel: there is no fallback
        m.pseudo_nll(ids, (4, 4))
    assert m.training          # the training flag is restored
    assert "NOT a likelihood" in MaskedGPT.pseudo_nll.__doc__


def test_trainer_refusals_on_the_cpu():
    from networks import LabelCondition, MaskedGPT, VQGAN
    from trainers import ConditionalMaskedPriorTrainer, MaskedPriorTrainer
    kw = dict(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64)
    vqgan = VQGAN(**P.TINY_VQGAN)
    tr = MaskedPriorTrainer(vqgan, MaskedGPT(**kw), n_steps=4, mask_seed=5, device="cpu")
    ids = {"ids": torch.zeros(2, 16, dtype=torch.long)}
    # the old refusals, word for word
    for call in (lambda: tr.token_nll(ids), lambda: tr.detect(ids, nll_threshold=1.0), lambda: tr.edit(ids, nll_threshold=1.0)):
        with pytest.raises(NotImplementedError, match="raster-order likelihood is not defined"):
            call()
    with pytest.raises(ValueError, match="MaskedPriorTrainer.edit: exactly one of mask and box selects the region"):
        tr.edit(ids)
    # the new ones
    with pytest.raises(ValueError, match="exactly one of mask and box selects the region"):
        tr.edit(ids, box=(0, 4, 0, 4), pnll_threshold=2.0)
    with pytest.raises(ValueError, match=r"stride=\(2, 2\) is the lattice of pnll_threshold and needs it"):
        tr.edit(ids, box=(0, 4, 0, 4), stride=(2, 2))
    with pytest.raises(ValueError, match="pnll_threshold='x' must be a number"):
        tr.edit(ids, pnll_threshold="x")
    with pytest.raises(ValueError, match=r"stride=\(5, 1\) must be a pair"):
        tr.pseudo_nll(ids, stride=(5, 1))
    with pytest.raises(ValueError, match="max_rows=0"):
        tr.pseudo_nll(ids, max_rows=0)
    with pytest.raises(ValueError, match="sequences of h w = 16 codes expected, got 8"):
        tr.pseudo_nll({"ids": torch.zeros(2, 8, dtype=torch.long)})
    with pytest.raises(ValueError, match="pnll_threshold selects the codes to restore and is required"):
        tr.detect_pseudo(ids, None)
    with pytest.raises(ValueError, match="MaskedPriorTrainer.detect_pseudo: against='both'"):
        tr.detect_pseudo(ids, 2.0, against="both")
    with pytest.raises(ValueError, match="MaskedPriorTrainer.detect_pseudo: weight='cells'"):
        tr.detect_pseudo(ids, 2.0, against="reconstruction", weight="cells")
    with pytest.raises(ValueError, match=r"MaskedPriorTrainer.detect_pseudo: against='image' needs a batch with an image"):
        tr.detect_pseudo(ids, 2.0)
    assert "Not a likelihood" in MaskedPriorTrainer.pseudo_nll.__doc__
    ctr = ConditionalMaskedPriorTrainer(vqgan, MaskedGPT(**kw), LabelCondition(2, 64, 4, 4), n_steps=4, mask_seed=5, device="cpu")
    batch = dict(ids, cond=torch.zeros(2, 16, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="told where the lesion is"):
        ctr.detect_pseudo(batch, 2.0)
    for call in (lambda: ctr.token_nll(batch), lambda: ctr.detect(batch, nll_threshold=1.0), lambda: ctr.edit(batch, nll_threshold=1.0)):
        with pytest.raises(NotImplementedError, match="raster-order likelihood is not defined"):
            call()
    with pytest.raises(ValueError, match="exactly one of mask, box and new_label selects the region"):
        ctr.edit(batch)
    with pytest.raises(ValueError, match="exactly one of mask, box and new_label"):
        ctr.edit(batch, box=(0, 4, 0, 4), pnll_threshold=1.0)
    with pytest.raises(ValueError, match="is the lattice of pnll_threshold and needs it"):
        ctr.edit(batch, box=(0, 4, 0, 4), stride=(2, 2))
