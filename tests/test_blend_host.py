"""CPU-side checks of the seamless composite (no GPU): the restatement of multi-band blending (tests/blend_ref.py) against brute
force and against the properties its definition promises, the C ABI and operator plumbing of vqw_blend_cells with the refusals that
need no device, the config helpers edit.{blend, blend_levels, blend_source} (and synth's), and the trainers' keyword checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import blend_ref as R
import prior_ref as P

NEW_SYMBOLS = ("vqw_blend_cells", "vqw_blend_cells_workspace")


def _case(B, C, H, W, h, w, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    image, edit, recon = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) for _ in range(3))
    mask = (torch.rand(B, h, w, generator=g) < p).to(torch.uint8)
    return image, edit, recon, mask


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape,cells,levels", [((1, 1, 8, 8), (2, 2), 1), ((2, 2, 16, 24), (4, 3), 2)])
def test_restatement_against_brute_force(shape, cells, levels):
    image, edit, recon, mask = _case(*shape, *cells, seed=3)
    mask[0, 0, 0], mask[0, -1, -1] = 1, 0          # both values occur, and a masked cell touches a corner (every clamp is taken)
    for rc in (None, recon):
        got = R.blend_ref(image, edit, mask, levels, rc, torch.float64)
        want = R.blend_brute(image.numpy(), edit.numpy(), mask.numpy(), levels, None if rc is None else rc.numpy())
        assert got.shape == image.shape and np.abs(got.numpy() - want).max() < 1e-13
    # the fp32 restatement is the same computation rounded: 2^-24 per operation, a few dozen operations per band
    got32 = R.blend_ref(image.float(), edit.float(), mask, levels, None, torch.float32)
    assert got32.dtype == torch.float32
    assert (got32.double() - R.blend_ref(image.float(), edit.float(), mask, levels, None, torch.float64)).abs().max() < 1e-5


def test_reduce_and_expand_on_hand_computable_cases():
    ones = torch.ones(1, 1, 8, 12, dtype=torch.float64)
    assert torch.equal(R.reduce(ones), torch.ones(1, 1, 4, 6, dtype=torch.float64))          # the taps sum to 1, borders included
    assert torch.equal(R.expand(ones), torch.ones(1, 1, 16, 24, dtype=torch.float64))
    ramp = torch.arange(8, dtype=torch.float64).reshape(1, 1, 1, 8).expand(1, 1, 2, 8)
    r = R.reduce(ramp)          # a linear ramp is reproduced at the even samples away from the clamped border
    assert r.shape == (1, 1, 1, 4) and r[0, 0, 0].tolist()[1:3] == [2.0, 4.0]
    assert r[0, 0, 0, 0] == (1 * 0 + 4 * 0 + 6 * 0 + 4 * 1 + 1 * 2) / 16          # x[-2], x[-1] clamp to x[0]
    e = R.expand(torch.tensor([[[[0.0, 8.0]]]], dtype=torch.float64))
    assert e.shape == (1, 1, 2, 4) and e[0, 0, 0].tolist() == [1.0, 4.0, 7.0, 8.0] and torch.equal(e[0, 0, 0], e[0, 0, 1])


def test_masks_of_all_zeros_and_all_ones():
    image, edit, recon, _ = _case(2, 1, 64, 64, 8, 8, seed=5)
    zeros, ones = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.ones(2, 8, 8, dtype=torch.uint8)
    for dtype in (torch.float64, torch.float32):
        for rc in (None, recon):
            assert torch.equal(R.blend_ref(image, edit, zeros, 3, rc, dtype), image.to(dtype))          # bit for bit
    assert (R.blend_ref(image, edit, ones, 3) - edit).abs().max() < 1e-13                       # image + d, the pyramid of d collapsed
    assert (R.blend_ref(image, edit, ones, 3, recon) - (image + edit - recon)).abs().max() < 1e-13


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_a_constant_difference_comes_out_as_the_smoothed_mask(levels):
    """d = c: every Laplacian band of d is 0 (REDUCE and EXPAND keep constants), so R_0 = c EXPAND^L(REDUCE^L(M_0)), with values
    in [0, c].  The mixing zone of L levels is a smooth ramp about 2^(L+1) pixels wide, so its largest neighbour-to-neighbour jump
    is about c / 2^(L+1) (a straight edge gives 0.273, 0.119, 0.058, 0.029 c): held to 0.6 c / 2^L.  A hard paste jumps by c."""
    c = 3.0
    image = torch.randn(1, 1, 64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    mask = torch.zeros(1, 8, 8, dtype=torch.uint8)
    mask[0, 2:5, 3:6] = 1
    out, corr = R.blend_ref(image, image + c, mask, levels, return_correction=True)
    m = R.mask_pixels(mask, 64, 64, torch.float64)
    for _ in range(levels):
        m = R.reduce(m)
    for _ in range(levels):
        m = R.expand(m)
    assert (corr - c * m).abs().max() < 1e-13
    assert float(corr.min()) >= -1e-13 and float(corr.max()) <= c + 1e-13
    jump = max(float((corr[..., 1:] - corr[..., :-1]).abs().max()), float((corr[..., 1:, :] - corr[..., :-1, :]).abs().max()))
    print("levels %d: the largest jump of the blended constant is %.4f c" % (levels, jump / c))
    assert 0 < jump <= 0.6 * c / 2 ** levels
    assert R.boundary_jump(image + c * R.mask_pixels(mask, 64, 64, torch.float64) - image, mask) == c


def test_delta_with_recon_equal_to_image_is_the_edit_source():
    image, edit, _, mask = _case(1, 2, 32, 48, 4, 6, seed=7)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(R.blend_ref(image, edit, mask, 2, image.clone(), dtype), R.blend_ref(image, edit, mask, 2, None, dtype))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES, s
    assert "vqw_blend_cells" in ops_ and "vqw_blend_cells_workspace" not in ops_          # a tensor-free host query stays a C call
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES["vqw_blend_cells"] == (ctypes.c_int, [p, p, p, p, p, p, l, i, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_blend_cells_workspace"] == (ctypes.c_long, [i, i, i, i, i])
    names = [n for _, n, _ in _lib.parse_header()["vqw_blend_cells"][1]]
    assert names == ["image", "edit", "recon", "cellmask", "out", "workspace", "workspace_floats", "N", "H", "W", "C", "h", "w", "levels", "stream"]
    sch = str(torch.ops.vqw.blend_cells.default._schema)
    assert "Tensor? image" in sch and "Tensor? edit" in sch and "Tensor? recon" in sch and "Tensor? cellmask" in sch
    assert "Tensor(a!)? out" in sch and "Tensor(b!)? workspace" in sch and "int workspace_floats" in sch and "int levels" in sch
    assert "blend.hip" in open(os.path.join(ROOT, "medical-image-editing_amd", "csrc", "Makefile")).read()


def test_workspace_query():
    from hipops import _lib
    L = _lib.load()
    # G and M of the levels 1..L as C + 1 planes, R of the levels 1..L-1 as C planes
    assert L.vqw_blend_cells_workspace(1, 8, 8, 1, 1) == 2 * 16
    assert L.vqw_blend_cells_workspace(4, 512, 512, 1, 3) == 4 * (2 * (256 ** 2 + 128 ** 2 + 64 ** 2) + 256 ** 2 + 128 ** 2)
    assert L.vqw_blend_cells_workspace(2, 48, 80, 3, 4) == 2 * (4 * (24 * 40 + 12 * 20 + 6 * 10 + 3 * 5) + 3 * (24 * 40 + 12 * 20 + 6 * 10))
    for bad in ((0, 8, 8, 1, 1), (1, 8, 8, 0, 1), (1, 8, 8, 1, 0), (1, 8, 8, 1, 13), (65536, 256, 256, 1, 1)):
        assert L.vqw_blend_cells_workspace(*bad) == 0, bad


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    P_ = 4096          # a 16-byte aligned non-null stand-in for every pointer

    def blend(N=2, H=16, W=16, C=1, h=4, w=4, levels=2, ws_floats=1 << 20, image=P_, edit=P_, recon=None, mask=P_, out=P_, ws=P_):
        return L.vqw_blend_cells(image, edit, recon, mask, out, ws, ws_floats, N, H, W, C, h, w, levels, None)

    def msg():
        return L.vqw_last_error()

    for kw in (dict(image=None), dict(edit=None), dict(mask=None), dict(out=None), dict(ws=None)):
        assert blend(**kw) != 0 and b"vqw_blend_cells" in msg() and b"null pointer" in msg()
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(C=0)):
        assert blend(**kw) != 0 and b"must be positive" in msg()
    for levels in (0, -1, 13):
        assert blend(levels=levels) != 0 and ("levels=%d must lie in [1, 12]" % levels).encode() in msg()
    for kw in (dict(h=3), dict(w=3), dict(h=0), dict(w=32)):
        assert blend(**kw) != 0 and b"multiples of the cell grid" in msg()
    assert blend(levels=5) != 0 and b"2^levels = 32 must divide H=16 and W=16" in msg()
    assert blend(H=24, h=4, levels=4) != 0 and b"2^levels = 16 must divide H=24" in msg()
    assert blend(N=65536, H=2, W=2, h=1, w=1, levels=1) != 0 and b"N=65536 exceeds the 65535" in msg()
    assert blend(N=65535, H=256, W=256) != 0 and b"32-bit" in msg()
    need = L.vqw_blend_cells_workspace(2, 16, 16, 1, 2)
    assert need == 2 * (2 * (64 + 16) + 64)
    assert blend(ws_floats=need - 1) != 0 and ("workspace of %d floats, %d needed" % (need - 1, need)).encode() in msg()
    for kw in (dict(image=P_ + 4), dict(edit=P_ + 8), dict(recon=P_ + 4), dict(out=P_ + 4), dict(ws=P_ + 12)):
        assert blend(**kw) != 0 and b"16-byte aligned" in msg()


def test_operator_has_no_cpu_route_and_checks_its_arguments():
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    x, m = torch.zeros(1, 1, 8, 8), torch.zeros(1, 2, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.blend_cells(x, x, m, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.blend_cells(x, x, m, 1, recon=x)
    with FakeTensorMode():
        x = torch.empty(2, 1, 8, 8, device="cuda")
        m = torch.empty(2, 4, 4, dtype=torch.uint8, device="cuda")
        for levels in (1.0, True, None, "2"):
            with pytest.raises(RuntimeError, match="levels=.* must be an integer"):
                ops.blend_cells(x, x, m, levels)
        with pytest.raises(RuntimeError, match="shape mismatch"):
            ops.blend_cells(x, x[:, :, :4], m, 1)
        with pytest.raises(RuntimeError, match="shape mismatch .* vs recon"):
            ops.blend_cells(x, x, m, 1, recon=x[:1])
        with pytest.raises(RuntimeError, match="cellmask"):
            ops.blend_cells(x, x, m.bool(), 1)
        with pytest.raises(RuntimeError, match="cellmask"):
            ops.blend_cells(x, x, m[:1], 1)
        with pytest.raises(RuntimeError, match="multiples of the cell grid 3 x 4"):
            ops.blend_cells(x, x, torch.empty(2, 3, 4, dtype=torch.uint8, device="cuda"), 1)
        with pytest.raises(RuntimeError, match="fp32"):
            ops.blend_cells(x.double(), x.double(), m, 1)
        out = ops.blend_cells(x, x, m, 1, recon=x)
        assert out.shape == (2, 1, 8, 8) and out.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ the config helpers
EDIT = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[24, 32, 8, 24])


def _raw(tmp_path, edit=EDIT, **run):
    raw = P.prior_run_config(tmp_path / "out", **dict(dict(resume_checkpoint="prior.ckpt"), **run))
    raw["edit"] = dict(edit)
    return raw


def test_default_blend_levels():
    from trainers.config import default_blend_levels
    assert [default_blend_levels(f, f) for f in (2, 4, 8, 16, 32, 6, 12, 24)] == [1, 2, 3, 3, 3, 1, 2, 3]
    assert default_blend_levels(32, 4) == 2 and default_blend_levels(4, 32) == 2 and default_blend_levels(8, 2) == 1
    for fy, fx in ((1, 1), (3, 8), (8, 5), (7, 7)):
        with pytest.raises(ValueError, match="odd side and no pyramid"):
            default_blend_levels(fy, fx)


def test_blend_keys_of_a_config(tmp_path):
    from utils import load_json
    from trainers import check_edit_config
    from trainers.config import blend, check_blend
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    off = {"blend": None, "blend_levels": None, "blend_source": "edit"}
    assert blend(cfg(_raw(tmp_path)), "edit") == off          # absent keys mean off
    assert blend(cfg(_raw(tmp_path, edit=dict(EDIT, blend=False, blend_levels=False, blend_source=False))), "edit") == off
    assert blend(cfg(_raw(tmp_path)), "synth") == off          # no section at all
    on = dict(EDIT, blend="pyramid", blend_levels=3, blend_source="delta")
    assert blend(cfg(_raw(tmp_path, edit=on)), "edit") == {"blend": "pyramid", "blend_levels": 3, "blend_source": "delta"}
    assert blend(cfg(_raw(tmp_path, edit=dict(EDIT, blend="paste"))), "edit") == dict(off, blend="paste")
    check_edit_config(cfg(_raw(tmp_path, edit=on)))
    for key, bad, match in (("blend", "feather", r"edit\.blend='feather' is None, 'paste' or 'pyramid'"), ("blend", 1, r"edit\.blend=1 "),
                            ("blend", True, r"edit\.blend=True "),
                            ("blend_levels", 0, r"edit\.blend_levels=0 must be an integer in \[1, 12\]"), ("blend_levels", 13, r"edit\.blend_levels=13 "),
                            ("blend_levels", 2.0, r"edit\.blend_levels=2\.0 "), ("blend_levels", True, r"edit\.blend_levels=True "),
                            ("blend_levels", "3", r"edit\.blend_levels='3' "),
                            ("blend_source", "recon", r"edit\.blend_source='recon' is 'edit' or 'delta'"), ("blend_source", 2, r"edit\.blend_source=2 ")):
        with pytest.raises(ValueError, match=match):
            check_edit_config(cfg(_raw(tmp_path, edit=dict(on, **{key: bad}))))
    # the same three under synth, checked by check_synth_config's helper; the keyword form names the keywords
    raw = _raw(tmp_path)
    raw["synth"] = dict(blend="pyramid", blend_levels=99)
    with pytest.raises(ValueError, match=r"synth\.blend_levels=99 "):
        blend(cfg(raw), "synth")
    assert check_blend(None, None, "edit") == (None, None, "edit") and check_blend("pyramid", 2, "delta") == ("pyramid", 2, "delta")
    with pytest.raises(ValueError, match="^blend='x' "):
        check_blend("x", None, "edit")


def test_check_synth_config_checks_the_blend_keys(tmp_path):
    import inspect
    from trainers import config
    assert 'blend(config, "synth")' in inspect.getsource(config.check_synth_config)
    assert 'blend(config, "edit")' in inspect.getsource(config.check_edit_config)


def test_committed_blend_config_is_the_edit_config_with_the_three_keys():
    from utils import load_json
    from trainers import check_edit_config
    from trainers.config import blend
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_edit_blend.json")
    config = load_json(path)
    check_edit_config(config)
    assert blend(config, "edit") == {"blend": "pyramid", "blend_levels": 3, "blend_source": "delta"}
    raw, ref = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "prior_vqgan_512_edit.json")))
    assert "pyramid" in raw["comment"] and "delta" in raw["comment"]
    extra = {k: raw["edit"].pop(k) for k in ("blend", "blend_levels", "blend_source")}
    assert extra == {"blend": "pyramid", "blend_levels": 3, "blend_source": "delta"}
    for section in ref:
        if section not in ("comment", "save"):
            assert raw[section] == ref[section], section
    assert raw["save"] == dict(ref["save"], study_name="prior_vqgan_512_edit_blend")
    assert "prior_vqgan_512_edit_blend.json" in open(os.path.join(ROOT, "configs", "README.md")).read()


# ------------------------------------------------------------------------------------------------ the trainers
def _trainers():
    from networks import GPT, MaskedGPT, VQGAN
    from trainers import MaskedPriorTrainer, PriorTrainer
    yield PriorTrainer(VQGAN(**P.TINY_VQGAN), GPT(**P.gpt_kwargs("p64")), device="cpu")
    yield MaskedPriorTrainer(VQGAN(**P.TINY_VQGAN), MaskedGPT(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64), n_steps=4, mask_seed=21,
                             device="cpu")


def test_edit_refuses_bad_blend_values_before_any_kernel():
    image = {"image": torch.zeros(1, 1, 8, 8)}
    for tr in _trainers():
        for kw, match in ((dict(blend="feather"), "blend='feather'"), (dict(blend="pyramid", blend_levels=0), "blend_levels=0"),
                          (dict(blend="pyramid", blend_levels=1.5), "blend_levels=1.5"), (dict(blend_source="recon"), "blend_source='recon'"),
                          (dict(blend="paste", blend_levels=13), "blend_levels=13"),
                          (dict(blend="pyramid", blend_levels=4), "2\\^4 does not divide the picture's 8 x 8")):
            with pytest.raises(ValueError, match=match):
                tr.edit(image, box=(0, 4, 0, 4), **kw)
        # the tiny VQGAN's cell is 2 x 2 pixels: the default depth is 1; a picture whose cells are odd has none
        assert tr._blending(image, "pyramid", None, "delta") == (1, "delta") and tr._blending(image, "pyramid", 3, "edit") == (3, "edit")
        assert tr._blending(image, None, None, "edit") is None and tr._blending(image, "paste", 3, "delta") is None
        assert tr._blending({"ids": torch.zeros(1, 4, dtype=torch.long)}, "pyramid", None, "edit") is None          # no composite
        tr.h, tr.w = 8, 8
        with pytest.raises(ValueError, match="odd side and no pyramid"):
            tr._blending(image, "pyramid", None, "edit")
        # good values pass the checks and reach the device code, which has no CPU route
        tr.h, tr.w = 4, 4
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tr.edit(image, box=(0, 4, 0, 4), blend="pyramid", blend_source="delta")


def test_detect_does_not_take_the_keywords():
    import inspect
    from trainers import ConditionalMaskedPriorTrainer, ConditionalPriorTrainer, MaskedPriorTrainer, PriorTrainer
    assert "blend" not in inspect.signature(PriorTrainer.detect).parameters
    assert "blend" not in inspect.signature(MaskedPriorTrainer.detect_pseudo).parameters
    for cls in (PriorTrainer, MaskedPriorTrainer, ConditionalPriorTrainer, ConditionalMaskedPriorTrainer):
        p = inspect.signature(cls.edit).parameters
        assert (p["blend"].default, p["blend_levels"].default, p["blend_source"].default) == (None, None, "edit")
