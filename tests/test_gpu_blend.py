"""GPU tests of the seamless composite: ops.blend_cells (csrc/blend.hip) against the float64 restatement of multi-band blending
(tests/blend_ref.py), and the blend keywords of the trainers' edit() and of the launcher's `-p -m edit`.

Tolerance: the project's gate - the relative L2 distance of the kernel's output from the float64 restatement is at most twice that
of the fp32 restatement, which follows the kernel's order operation by operation.  Everything else is bit for bit: two runs, both
memory formats, the pixels whose correction is a structural zero, an all-zero mask, the trainers' composites and the launcher's
files."""
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, rel_err
from run_helpers import run_launcher, write_config
import blend_ref as R
import gpt_ref as G
import prior_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, H, W, C, h, w, levels).  A reduce workgroup owns 16 x 32 outputs of the level above, a collapse workgroup 16 x 64 of its own.
CASES = [
    (1, 8, 8, 1, 4, 4, 1),             # the TINY_VQGAN shape: smaller than a tile, every halo beyond every edge
    (1, 32, 32, 1, 1, 1, 5),           # one cell, the lowest level 1 x 1
    (2, 48, 80, 1, 3, 5, 4),           # factor 16, the lowest level 3 x 5, ragged tiles, the batch offset
    (1, 64, 64, 3, 16, 16, 2),         # channels
    (1, 96, 160, 1, 6, 10, 3),         # several tiles, non-square
    (1, 512, 512, 1, 16, 16, 5),       # the shipped shape: every level
]
SOURCES = ("edit", "delta")
_cache = {}


def _inputs(case):
    N, H, W, C, h, w, L = case
    g = torch.Generator().manual_seed(2000 + H + 7 * W + C + L)
    image, edit, recon = (torch.randn(N, C, H, W, generator=g) for _ in range(3))
    mask = (torch.rand(N, h, w, generator=g) < 0.5).to(torch.uint8) * 3          # any non-zero byte is set
    if h * w == 1:
        mask[:] = 1
    return image, edit, recon, mask


def _refs(case, source):
    """(float64, fp32) restatements: computed once, shared, never changed"""
    if (case, source) not in _cache:
        image, edit, recon, mask = _inputs(case)
        rc = recon if source == "delta" else None
        _cache[case, source] = (R.blend_ref(image, edit, mask, case[6], rc, torch.float64), R.blend_ref(image, edit, mask, case[6], rc, torch.float32))
    return _cache[case, source]


def _run(image, edit, mask, levels, recon=None):
    from hipops import ops
    return ops.blend_cells(image.to(DEV), edit.to(DEV), mask.to(DEV), levels, None if recon is None else recon.to(DEV))


def _gate(got, truth, ref32, what):
    """|got - truth| <= 2 |ref32 - truth| (relative L2), figures printed first."""
    spread, e = rel_err(ref32, truth), rel_err(got, truth)
    print("%-44s %.3e from float64, the fp32 restatement %.3e (ratio %.2f)" % (what, e, spread, e / max(spread, 1e-300)))
    assert_close(got, truth, 2.0 * spread, what)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_%dx%d_C%d_h%dw%d_L%d" % c)
def test_blend_cells_against_float64(case, source):
    image, edit, recon, mask = _inputs(case)
    rc = recon if source == "delta" else None
    truth, ref32 = _refs(case, source)
    got = _run(image, edit, mask, case[6], rc)
    assert got.shape == truth.shape and got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    # the correction is as large as the picture: about half the cells are set, d has variance 2
    assert rel_err(truth, image) > 0.3
    _gate(got.cpu(), truth, ref32, "blend_cells %s %s" % (case, source))
    assert torch.equal(_run(image, edit, mask, case[6], rc), got), "two runs differ"
    cl = torch.channels_last
    fmt = lambda t: None if t is None else t.contiguous(memory_format=cl)  # noqa: E731
    assert torch.equal(_run(fmt(image), fmt(edit), mask, case[6], fmt(rc)), got), "channels_last inputs give another tensor"
    # an all-zero mask returns the picture bit for bit
    assert torch.equal(_run(image, edit, torch.zeros_like(mask), case[6], rc).cpu(), image)


@pytest.mark.parametrize("source", SOURCES)
def test_structural_zeros_leave_the_picture_bit_for_bit(source):
    N, H, W, C, h, w, L = CASES[4]
    image, edit, recon, _ = _inputs(CASES[4])
    mask = torch.zeros(N, h, w, dtype=torch.uint8)
    mask[0, 2:4, 3:5] = 1          # one 2 x 2 block of cells
    rc = recon if source == "delta" else None
    truth, corr = R.blend_ref(image, edit, mask, L, rc, torch.float64, return_correction=True)
    zero = corr == 0
    share = float(zero.double().mean())
    print("structural zeros: %.1f %% of the pixels" % (100 * share))
    assert 0.1 < share < 0.9          # the mask pyramid vanishes far from the block: no tap of any level reaches those pixels
    got = _run(image, edit, mask, L, rc).cpu()
    assert torch.equal(got[zero], image[zero])
    assert not torch.equal(got[~zero], image[~zero])
    _gate(got, truth, R.blend_ref(image, edit, mask, L, rc, torch.float32), "blend_cells one block %s" % source)


def test_blend_cells_leaves_no_tape_and_masks_of_ones():
    from hipops import ops
    image, edit, recon, mask = _inputs(CASES[2])
    out = ops.blend_cells(image.to(DEV).requires_grad_(True), edit.to(DEV).requires_grad_(True), mask.to(DEV), 4, recon.to(DEV).requires_grad_(True))
    assert not out.requires_grad
    # every cell set: the pyramid of d collapses back to d, up to the rounding of its bands (a few 2^-24 of |d| per level)
    ones = _run(image, edit, torch.ones_like(mask), 4).cpu()
    assert (ones - edit).abs().max() < 1e-5
    # recon == image: source 'delta' is source 'edit', bit for bit
    assert torch.equal(_run(image, edit, mask, 4, image.clone()), _run(image, edit, mask, 4))


def test_blend_cells_refusals_name_the_value():
    from hipops import ops
    L = ops._L()
    x = torch.zeros(2, 1, 16, 16, device=DEV)
    m = torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV)
    for levels in (0, -2, 13):
        with pytest.raises(RuntimeError, match=r"levels=%d must lie in \[1, 12\]" % levels):
            ops.blend_cells(x, x, m, levels)
    with pytest.raises(RuntimeError, match=r"2\^levels = 32 must divide H=16 and W=16"):
        ops.blend_cells(x, x, m, 5)
    with pytest.raises(RuntimeError, match=r"2\^levels = 16 must divide H=24 and W=16"):
        ops.blend_cells(torch.zeros(1, 1, 24, 16, device=DEV), torch.zeros(1, 1, 24, 16, device=DEV), torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV), 4)
    with pytest.raises(RuntimeError, match="multiples of the cell grid 3 x 4"):
        ops.blend_cells(x, x, torch.zeros(2, 3, 4, dtype=torch.uint8, device=DEV), 1)
    many = torch.zeros(65536, 1, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="N=65536 exceeds the 65535"):
        ops.blend_cells(many, many, torch.zeros(65536, 1, 1, dtype=torch.uint8, device=DEV), 1)
    # the entry point itself: what the operator never passes on
    out, ws = torch.empty_like(x), torch.empty(1024, device=DEV)
    need = int(L.vqw_blend_cells_workspace(2, 16, 16, 1, 2))
    assert need == 2 * (2 * (64 + 16) + 64)
    with pytest.raises(RuntimeError, match="workspace of %d floats, %d needed" % (need - 1, need)):
        L.vqw_blend_cells(x, x, None, m, out, ws, need - 1, 2, 16, 16, 1, 4, 4, 2)
    with pytest.raises(RuntimeError, match=r"H=16, W=16 must be multiples of the cell grid h=3, w=4"):
        L.vqw_blend_cells(x, x, None, m, out, ws, 1024, 2, 16, 16, 1, 3, 4, 2)
    with pytest.raises(RuntimeError, match=r"65535 \* 256 \* 256 \* 2 elements need 32-bit indices"):
        L.vqw_blend_cells(x, x, None, m, out, ws, 1024, 65535, 256, 256, 1, 4, 4, 2)
    for kw in (dict(image=None), dict(edit=None), dict(cellmask=None), dict(out=None), dict(workspace=None)):
        args = dict(image=x, edit=x, recon=None, cellmask=m, out=out, workspace=ws)
        args.update(kw)
        with pytest.raises(RuntimeError, match="null pointer"):
            L.vqw_blend_cells(*args.values(), 1024, 2, 16, 16, 1, 4, 4, 2)
    off = torch.empty(2 * 256 + 4, device=DEV)[1:1 + 512].reshape(2, 1, 16, 16)          # 4 bytes off a 16-byte boundary
    for kw in (dict(image=off), dict(edit=off), dict(recon=off), dict(out=off), dict(workspace=torch.empty(1028, device=DEV)[1:])):
        args = dict(image=x, edit=x, recon=None, cellmask=m, out=out, workspace=ws)
        args.update(kw)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            L.vqw_blend_cells(*args.values(), 1024, 2, 16, 16, 1, 4, 4, 2)


# ------------------------------------------------------------------------------------------------ the trainers
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
    return _tr["tr"]


def _masked_trainer():
    """test_gpu_masked_prior.py's tiny pair, built here: TINY_VQGAN and a two-layer MaskedGPT."""
    if "masked" not in _tr:
        from networks import MaskedGPT, VQGAN
        from trainers import MaskedPriorTrainer
        torch.manual_seed(77)
        vqgan = VQGAN(**P.TINY_VQGAN)
        torch.manual_seed(611)
        gpt = G.init_gpt_(MaskedGPT(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64), 611)
        _tr["masked"] = MaskedPriorTrainer(vqgan, gpt, n_steps=4, mask_seed=21, lr=3e-3, betas=P.OPTIM["betas"], weight_decay=P.OPTIM["weight_decay"],
                                           grad_norm_clip=1.0, seed=17, device=DEV)
    return _tr["masked"]


def _gen(seed=9):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("which", ["gpt", "masked"])
def test_edit_blend_changes_the_composite_alone(which):
    from hipops import ops
    tr = _trainer() if which == "gpt" else _masked_trainer()
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    kw = dict(box=(2, 6, 0, 4), n_candidates=3, temperature=1.0, top_k=16, top_p=0.95)
    plain = tr.edit({"image": image}, generator=_gen(), **kw)
    paste = tr.edit({"image": image}, generator=_gen(), blend="paste", blend_levels=2, blend_source="delta", **kw)
    assert sorted(paste) == sorted(plain)
    for key in plain:
        assert torch.equal(plain[key], paste[key]), key          # 'paste' is today's call and today's bits
    assert torch.equal(plain["composite"], ops.paste_cells(image, plain["edit"], plain["cellmask"]))
    # the default depth on cells of 2 x 2 pixels is 1
    for extra, levels, recon in ((dict(), 1, None), (dict(blend_source="delta"), 1, "recon"), (dict(blend_levels=2), 2, None),
                                 (dict(blend_levels=3, blend_source="delta"), 3, "recon")):
        out = tr.edit({"image": image}, generator=_gen(), blend="pyramid", **extra, **kw)
        assert sorted(out) == sorted(plain)
        for key in plain:
            if key != "composite":
                assert torch.equal(plain[key], out[key]), (key, extra)
        want = ops.blend_cells(image, out["edit"], out["cellmask"], levels, None if recon is None else out[recon])
        assert torch.equal(out["composite"], want), extra
        assert not torch.equal(out["composite"], plain["composite"]), extra
        assert rel_err(out["composite"], R.blend_ref(image, out["edit"], out["cellmask"], levels, None if recon is None else out[recon])) < 1e-5
    # a {'ids'} batch still has no composite
    ids = tr.codes({"image": image})
    assert "composite" not in tr.edit({"ids": ids}, generator=_gen(), blend="pyramid", **kw)
    with pytest.raises(ValueError, match="blend='feather'"):
        tr.edit({"image": image}, generator=_gen(), blend="feather", **kw)


def test_edit_through_the_label_map_takes_the_keywords():
    """The fourth selector, new_label, on the conditional masked prior (test_gpu_masked_cond.py's tiny trainer, built here)."""
    from hipops import ops
    from networks import LabelCondition, MaskedGPT, VQGAN
    from trainers import ConditionalMaskedPriorTrainer
    import masked_cond_ref as MC
    torch.manual_seed(77)
    vqgan = VQGAN(**dict(P.TINY_VQGAN, dict_size=MC.TINY["vocab_size"]))
    torch.manual_seed(811)
    gpt = G.init_gpt_(MaskedGPT(**MC.TINY), 811)
    cond = LabelCondition(MC.N_LABELS, MC.TINY["n_embed"], 4, 4, null_token=True)
    tr = ConditionalMaskedPriorTrainer(vqgan, gpt, cond, n_steps=4, mask_seed=21, lr=3e-3, betas=P.OPTIM["betas"],
                                       weight_decay=P.OPTIM["weight_decay"], grad_norm_clip=1.0, seed=17, device=DEV)
    label = torch.randint(0, MC.N_LABELS, (2, 8, 8), generator=torch.Generator().manual_seed(78)).to(DEV)
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(79)).to(DEV)
    new = label.clone()
    new[0, 2:5, 2:6] = (new[0, 2:5, 2:6] + 1) % MC.N_LABELS
    kw = dict(new_label=new, n_candidates=3, n_steps=4, top_k=8, top_p=0.95)
    plain = tr.edit({"image": image, "label": label}, generator=_gen(), **kw)
    out = tr.edit({"image": image, "label": label}, generator=_gen(), blend="pyramid", blend_levels=2, blend_source="delta", **kw)
    assert sorted(out) == sorted(plain) and int(out["cellmask"][0].sum()) == 4 and int(out["cellmask"][1].sum()) == 0
    for key in plain:
        if key != "composite":
            assert torch.equal(plain[key], out[key]), key
    assert torch.equal(out["composite"], ops.blend_cells(image, out["edit"], out["cellmask"], 2, out["recon"]))
    assert not torch.equal(out["composite"][0], plain["composite"][0])
    assert torch.equal(out["composite"][1], image[1])          # no cell of slice 1 changed: its composite is the slice, bit for bit


def test_detect_keeps_the_hard_paste():
    from hipops import ops
    tr = _trainer()
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    thr = float(tr.token_nll({"image": image}).median())
    kw = dict(n_candidates=3, temperature=1.0, top_k=16, top_p=0.95)
    ed = tr.edit({"image": image}, nll_threshold=thr, generator=_gen(), **kw)
    out = tr.detect({"image": image}, thr, sigma=1.0, generator=_gen(), **kw)
    assert torch.equal(out["restored"], ops.paste_cells(image, ed["edit"], ed["cellmask"]))
    assert torch.equal(out["map"], ops.anomaly_map(image, out["restored"], ed["cellmask"], 1.0))
    outside = ~ed["cellmask"].bool().repeat_interleave(2, 1).repeat_interleave(2, 2)[:, None]
    assert torch.equal(out["restored"][outside], image[outside])          # outside the restored cells the residual is exactly 0
    with pytest.raises(TypeError, match="blend"):
        tr.detect({"image": image}, thr, blend="pyramid")


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_blends_the_composite_tile_and_nothing_else(tmp_path):
    from utils import png
    save = os.path.join(str(tmp_path), "run")
    run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), P.prior_run_config(save)), "-p")
    ckpt = os.path.join(save, "study", "version_0", "ckpt-epoch=0000-total_loss=0.00.ckpt")
    raw = P.prior_run_config(save, resume_checkpoint=ckpt)
    raw["edit"] = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[24, 32, 8, 24])
    plain = write_config(os.path.join(str(tmp_path), "edit.json"), raw)
    raw["edit"].update(blend="pyramid", blend_levels=1, blend_source="delta")          # cells of 2 x 2 pixels: one level
    blended = write_config(os.path.join(str(tmp_path), "edit_blend.json"), raw)
    files = {}
    for version, cfg in ((1, blended), (2, blended), (3, plain)):
        out = run_launcher(cfg, "-p", "-m", "edit")
        assert "Edited slices are saved" in out
        edir = os.path.join(save, "study", "version_%d" % version, "edit")
        assert sorted(os.listdir(edir)) == ["codes_0000.npy", "codes_0001.npy", "edit.csv", "slice_0000.png", "slice_0001.png"]
        files[version] = {f: open(os.path.join(edir, f), "rb").read() for f in os.listdir(edir)}
    assert files[1] == files[2], "the same seed writes the same bytes"
    for f in ("edit.csv", "codes_0000.npy", "codes_0001.npy"):
        assert files[1][f] == files[3][f], f
    a, _ = png.load(os.path.join(save, "study", "version_1", "edit", "slice_0000.png"))
    b, _ = png.load(os.path.join(save, "study", "version_3", "edit", "slice_0000.png"))
    assert a.shape == b.shape == (32, 4 * 32)
    assert np.array_equal(a[:, :96], b[:, :96]) and not np.array_equal(a[:, 96:], b[:, 96:])          # the composite tile alone
    assert np.array_equal(a[:16, 96:], b[:16, 96:])          # far above the box the blended composite is the slice as well
