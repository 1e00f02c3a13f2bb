"""The kernels of csrc/loss.hip and csrc/extras.hip against float64 (tests/loss_ref.py) on every route they can take.
Run with `pytest -m gpu tests/test_gpu_losses.py -s` on an MI355X; -s shows the measured error of every comparison.

Every case draws fp32 inputs from a seeded generator, runs the HIP path through hipops.ops and evaluates loss_ref on the
same fp32 values cast to float64, so a difference is the kernel's and not input rounding.  Gradients of the float64 side
come from autograd.

Tolerances (the project's own, header of test_gpu_parity.py / test_losses_golden / test_extras_golden):
  single-kernel outputs and gradients ... 2e-5 relative L2, and elementwise with atol = 2e-5 * max|ref|
  scalar losses ......................... 1e-5 relative; the dice loss additionally 1e-6 absolute (8 fp32 ulps at 1.0: the
                                          value is 1 - 2I/D and can be near 0)
  seg-loss gradients .................... 1e-4 relative L2
  dense form vs label form, same sums ... 1e-6
  keep masks, pixel shuffle, one-hot, flip: exact

The routes named in the case comments follow from csrc/loss.hip and common.h:
  cl_splits(B, HW) = min(ceil(1024 / B), max(HW / 512, 1), 64); a split has ceil(HW / splits) pixels, walked 256 at a time
  codebook in LDS (label form forward): D % 4 == 0 and K * D <= 4096, else read from global memory
  k_cross_bwd4 (lg = log2(D / 4)): D % 4 == 0 and D / 4 a power of two, else the flat k_cross_bwd
  stream_grid caps a launch at 2048 * 256 = 524288 threads: a grid-stride loop over more elements takes a second trip ("wraps")

Measured on an MI355X (largest error per group; bound in brackets):
  cross loss, label form .... loss 5.2e-8 [1e-5], e.grad 1.6e-7 relative L2 and elementwise [2e-5], coef 1.2e-7 [2e-5]
  cross loss, dense form .... loss 2.2e-8 [1e-5], e.grad 1.3e-7 [2e-5]; dense vs label form: loss 0, e.grad 5.3e-8 [1e-6]
  K = 4096 / 5120 ........... loss 5.1e-8 [1e-5], e.grad 5.2e-7 relative L2, 1.1e-6 elementwise [2e-5], coef 7.9e-8 [2e-5]
  SoftDice / Focal .......... dice 4.3e-8 [1e-5 + 1e-6], focal 6.6e-8 [1e-5], logits.grad 2.2e-7 [1e-4]
  DropBlock ................. scale 5.6e-8, apply forward / backward 2.6e-8 [1e-6]; keep masks exact
  No case needed the wider fp32-reference bound.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as LR
from helpers import rel_err, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNEL_TOL = 2e-5
LOSS_TOL = 1e-5
SEG_GRAD_TOL = 1e-4
DICE_ATOL = 1e-6
SAME_SUMS_TOL = 1e-6
F32 = lambda v: float(np.float32(v))      # a scalar argument as the kernel receives it


def _ops():
    from hipops import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(group, what, got, ref, tol, atol=0.0, elementwise=False):
    """Print the measured error, then assert |got - ref|_2 <= tol |ref|_2 (+ atol), and elementwise
    max|got - ref| <= tol max|ref| where asked."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    line = "[%s] %s: rel %.2e (bound %.0e)" % (group, what, rel_err(got, ref), tol)
    if elementwise:
        worst = float((got.reshape(-1) - ref.reshape(-1)).abs().max()) / (float(ref.abs().max()) + 1e-300)
        line += ", max|diff| / max|ref| %.2e" % worst
    print(line)
    assert_close(got, ref, tol, what, atol=atol)
    if elementwise:
        assert worst <= tol, "%s: elementwise %.3e > %.0e of max|ref|" % (what, worst, tol)


# --------------------------------------------------------------------------------------------------
# cross loss, label form
# --------------------------------------------------------------------------------------------------
def _label_map(B, H, W, K, g):
    """About 10 % zeros (out of frame); class 2 absent from image 0 and present in the last image (B = 1: absent altogether);
    class 3 in exactly one pixel of the whole batch; label K itself present."""
    lab = torch.randint(1, K + 1, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = 0
    lab[lab == 3] = 1
    lab[0][lab[0] == 2] = 1
    if B > 1:
        lab[B - 1, 0, 0] = 2
    lab[B - 1, H // 2, W // 2] = 3
    lab[0, 0, 1] = K
    return lab.int()


def _cross_inputs(B, H, W, D, K, seed):
    g = _gen(seed)
    return torch.randn(B, D, H, W, generator=g), torch.randn(K, D, generator=g), g


def _cross_ref(fn, e32, other, cb32, upstream):
    e = e32.double().requires_grad_(True)
    loss = fn(e, other, cb32.double())
    (loss * upstream).backward()
    return loss.detach(), e.grad


def _cross_hip(fn, e32, other, cb32, upstream):
    e = e32.to(DEV).requires_grad_(True)
    loss = fn(e, other.to(DEV), cb32.to(DEV))
    (loss * upstream).backward()
    return loss.detach(), e.grad


CROSS_LABEL_CASES = [
    # B, H, W, D, K
    (1, 64, 64, 16, 10),        # 8 splits of 512; LDS codebook; bwd4 lg = 2; no wrap
    (2, 40, 40, 16, 180),       # 3 splits of 534 (22 mod 256; the last has 532); LDS codebook at K * D = 2880; bwd4 lg = 2
    (2, 37, 29, 7, 50),         # D % 4 != 0: global codebook + flat backward; HW = 1073: 2 ragged splits of 537 / 536
    (2, 32, 32, 12, 64),        # LDS codebook (D % 4 == 0, K * D = 768) but flat backward (D / 4 = 3); 2 splits of 512
    (1, 48, 48, 256, 1024),     # config-4 codebook: K * D > 4096 -> global codebook; bwd4 lg = 6; 4 splits of 576
    (40, 128, 128, 4, 6),       # splits limited by B: ceil(1024 / 40) = 26 of 631 (the last 609); LDS codebook; bwd4 lg = 0
    (1, 256, 128, 16, 10),      # HW / 512 = 64: the 64-split cap; LDS codebook; bwd4 lg = 2
    (3, 33, 31, 16, 10),        # 1 split of 1023 pixels (255 mod 256); LDS codebook; bwd4 lg = 2
    (1, 128, 128, 256, 12),     # bwd4 (lg = 6) wraps: HW * D / 4 = 1048576 > 524288; global codebook; 32 splits
    (1, 192, 192, 20, 12),      # flat k_cross_bwd (D / 4 = 5) wraps: 737280 elements; LDS codebook (K * D = 240); 64 splits of 576
]
# An embed that is not 16-byte aligned (the scalar fallback of the cb_lds / bwd4 conditions) cannot be passed through ops:
# nhwc() hands the kernels a fresh channels-last allocation.  It is not forced here.


def _check_cross_labels(B, H, W, D, K, lab, seed, group="cross/labels"):
    ops = _ops()
    from hipops import functional  # noqa: F401  (registers torch.ops.vqw.embed_cross_loss)
    e32, cb32, _ = _cross_inputs(B, H, W, D, K, seed)
    tag = "(%d,%d,%d,%d,%d)" % (B, H, W, D, K)
    ref_loss, ref_grad = _cross_ref(LR.cross_loss_labels, e32, lab, cb32, 0.37)
    loss, grad = _cross_hip(ops.cross_loss_labels, e32, lab, cb32, 0.37)
    _report(group, "loss " + tag, loss, ref_loss, LOSS_TOL)
    _report(group, "e.grad " + tag, grad, ref_grad, KERNEL_TOL, elementwise=True)
    # coef[b, k] = 1 / ((cnt + 1e-6) n_present), 0 where the class is absent; cnt counted exactly on the host
    loss2, coef = torch.ops.vqw.embed_cross_loss(e32.to(DEV), lab.to(DEV), cb32.to(DEV))
    cnt = torch.stack([torch.bincount(lab[b].reshape(-1).long(), minlength=K + 1)[1:K + 1] for b in range(B)]).double()
    n_present = int((cnt > 0).sum())
    want = torch.where(cnt > 0, 1.0 / ((cnt + 1e-6) * n_present), torch.zeros_like(cnt))
    coef = coef.cpu().reshape(B, K)
    assert bool((coef[cnt == 0] == 0).all()), "coef is not 0 for absent classes"
    _report(group, "coef " + tag, coef, want, KERNEL_TOL, elementwise=True)
    _report(group, "loss (vqw::embed_cross_loss) " + tag, loss2, ref_loss, LOSS_TOL)


@pytest.mark.parametrize("B,H,W,D,K", CROSS_LABEL_CASES)
def test_cross_loss_labels(B, H, W, D, K):
    lab = _label_map(B, H, W, K, _gen(100 + D + K))
    cnt = torch.bincount(lab.reshape(-1).long(), minlength=K + 1)
    assert cnt[3] == 1 and cnt[K] >= 1 and int((lab[0] == 2).sum()) == 0 and 0.05 < float((lab == 0).float().mean()) < 0.15
    _check_cross_labels(B, H, W, D, K, lab, 200 + D + K)


def test_cross_loss_labels_all_out_of_frame():
    """No class present anywhere: the loss is NaN like torch's mean of an empty selection, the gradient all zeros."""
    ops = _ops()
    e32, cb32, _ = _cross_inputs(2, 40, 40, 16, 10, 7)
    lab = torch.zeros(2, 40, 40, dtype=torch.int32)
    ref_loss, ref_grad = _cross_ref(LR.cross_loss_labels, e32, lab, cb32, 0.37)
    assert math.isnan(float(ref_loss)) and float(ref_grad.abs().max()) == 0.0
    loss, grad = _cross_hip(ops.cross_loss_labels, e32, lab, cb32, 0.37)
    assert math.isnan(float(loss))
    assert float(grad.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------
# cross loss, dense form
# --------------------------------------------------------------------------------------------------
def _soft_weights(B, K, H, W, g):
    """Uniform (0, 1) weights, about 70 % of them exactly 0, the (0, 1) plane wholly zero (an absent class)."""
    r = torch.rand(B, K, H, W, generator=g)
    r[torch.rand(B, K, H, W, generator=g) < 0.7] = 0
    r[0, 1] = 0
    return r


CROSS_DENSE_CASES = [
    (2, 40, 40, 16, 10),        # 3 splits of 534 (the last 532)
    (1, 64, 64, 7, 5),          # 8 splits of 512, odd D
    (1, 64, 32, 16, 37),        # 4 splits of 512, K neither a power of two nor a multiple of the wave
    (1, 192, 192, 16, 6),       # k_cross_bwd_dense wraps: 589824 elements > 524288; 64 splits of 576
]


def _check_cross_dense(B, H, W, D, K, seed, group="cross/dense"):
    ops = _ops()
    e32, cb32, g = _cross_inputs(B, H, W, D, K, seed)
    r = _soft_weights(B, K, H, W, g)
    tag = "(%d,%d,%d,%d,%d)" % (B, H, W, D, K)
    ref_loss, ref_grad = _cross_ref(LR.cross_loss_dense, e32, r.double(), cb32, 0.37)
    loss, grad = _cross_hip(ops.cross_loss_dense, e32, r, cb32, 0.37)
    _report(group, "loss " + tag, loss, ref_loss, LOSS_TOL)
    _report(group, "e.grad " + tag, grad, ref_grad, KERNEL_TOL, elementwise=True)


@pytest.mark.parametrize("B,H,W,D,K", CROSS_DENSE_CASES)
def test_cross_loss_dense_soft_weights(B, H, W, D, K):
    _check_cross_dense(B, H, W, D, K, 300 + D + K)


@pytest.mark.parametrize("B,H,W,D,K", [(2, 40, 40, 16, 10), (2, 37, 29, 7, 50)])
def test_cross_loss_dense_equals_labels_on_onehot(B, H, W, D, K):
    """One-hot weights built from a label map: both forms add the same per-pixel terms (in a different order across the
    kernels' lanes), so they agree far inside the float64 bound."""
    ops = _ops()
    e32, cb32, g = _cross_inputs(B, H, W, D, K, 400 + K)
    lab = _label_map(B, H, W, K, g)
    r = LR.onehot(lab, K + 1)[:, 1:].float().contiguous()
    ll, gl = _cross_hip(ops.cross_loss_labels, e32, lab, cb32, 0.37)
    ld, gd = _cross_hip(ops.cross_loss_dense, e32, r, cb32, 0.37)
    _report("cross/dense-vs-labels", "loss (%d,%d,%d,%d,%d)" % (B, H, W, D, K), ld, ll, SAME_SUMS_TOL)
    _report("cross/dense-vs-labels", "e.grad (%d,%d,%d,%d,%d)" % (B, H, W, D, K), gd, gl, SAME_SUMS_TOL)


# --------------------------------------------------------------------------------------------------
# the K bound: 32 K bytes of LDS per workgroup, 160 KiB at most -> K <= 5120; the opt-in above 64 KiB (K > 2048)
# --------------------------------------------------------------------------------------------------
CL_MAX_K = 5120


def _sparse_codes_map(B, H, W, K, g, n_codes=50):
    codes = torch.cat([torch.tensor([1, K]), torch.randperm(K - 2, generator=g)[:n_codes - 2] + 2])
    lab = codes[torch.randint(0, n_codes, (B, H, W), generator=g)]
    lab[torch.rand(B, H, W, generator=g) < 0.1] = 0
    lab[0, 0, 0], lab[0, 0, 1] = 1, K
    return lab.int()


def test_cross_loss_labels_large_dictionary():
    """(1, 32, 32, 8, 4096): 128 KiB of LDS, global codebook, 2 splits of 512, bwd4 lg = 1.  About 50 distinct codes, 1 and
    4096 among them."""
    B, H, W, D, K = 1, 32, 32, 8, 4096
    lab = _sparse_codes_map(B, H, W, K, _gen(11))
    assert 40 <= len(torch.unique(lab[lab > 0])) <= 50
    _check_cross_labels(B, H, W, D, K, lab, 12, group="cross/large-K")


def test_cross_loss_labels_largest_dictionary():
    """K = 5120, the largest admitted: the whole 160 KiB of a compute unit's LDS in one workgroup."""
    B, H, W, D, K = 1, 32, 32, 4, CL_MAX_K
    _check_cross_labels(B, H, W, D, K, _sparse_codes_map(B, H, W, K, _gen(13)), 14, group="cross/large-K")


def test_cross_loss_dense_large_dictionary():
    """(1, 32, 32, 8, 4096) in the dense form (r is 16 MiB; well under a second on the device and in float64)."""
    _check_cross_dense(1, 32, 32, 8, 4096, 15, group="cross/large-K")


def test_cross_loss_rejects_k_over_the_lds_bound():
    """The first K that cannot launch is stopped by the argument check, which names K."""
    ops = _ops()
    K = CL_MAX_K + 1
    e = torch.randn(1, 4, 8, 8, device=DEV)
    cb = torch.randn(K, 4, device=DEV)
    with pytest.raises(RuntimeError, match=r"vqw_cross_loss_fwd: K = %d too large" % K):
        ops.cross_loss_labels(e, torch.zeros(1, 8, 8, dtype=torch.int32, device=DEV), cb)
    with pytest.raises(RuntimeError, match=r"vqw_cross_loss_dense_fwd: K = %d too large" % K):
        ops.cross_loss_dense(e, torch.zeros(1, K, 8, 8, device=DEV), cb)


# --------------------------------------------------------------------------------------------------
# SoftDice / Focal
# --------------------------------------------------------------------------------------------------
S_FIX, S_RAG, S_CAP = (2, 5, 9, 9), (3, 4, 23, 17), (2, 5, 264, 256)
S_C1, S_C64, S_VOL, S_WRAP = (2, 1, 16, 16), (1, 64, 24, 24), (1, 3, 6, 10, 12), (1, 2, 768, 704)
# S_FIX:  the golden fixture's shape, 162 pixels: one workgroup
# S_RAG:  1173 pixels: 5 workgroups, the last ragged; k_seg_finalize folds 5 partials
# S_CAP:  135168 pixels > 512 * 256: k_seg_partial at its 512-block cap, every thread takes a second pixel (and 32 a third)
# S_C1:   one class (softmax == 1: every gradient is analytically 0);  S_C64: C = SEG_MAXC;  S_VOL: a 3-D volume
# S_WRAP: 540672 pixels > 2048 * 256: k_seg_bwd's grid-stride loop wraps (S_CAP does not reach it: it runs one thread per pixel)
SEG_CASES = [
    # shape, ignore_index, gamma, target, logit scale, smooth, (a, b) upstream weights on (dice, focal)
    (S_FIX, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_FIX, 0, 2.0, "hard", 1, "small", (1, 0)),
    (S_FIX, -1, 2.0, "hard", 1, "small", (0, 1)),
    (S_FIX, 2, 0.5, "soft", 30, "small", (0.7, -1.3)),
    (S_FIX, 4, 0.0, "holes", 1, "clamped", (0.7, -1.3)),
    (S_RAG, -1, 5.0, "soft", 1, "small", (0.7, -1.3)),
    (S_RAG, 3, 2.0, "holes", 30, "small", (0.7, -1.3)),
    (S_RAG, 1, 0.5, "hard", 1, "clamped", (1, 0)),
    (S_RAG, 0, 0.0, "hard", 30, "small", (0, 1)),
    (S_CAP, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_CAP, 2, 0.5, "soft", 30, "small", (0.7, -1.3)),
    (S_CAP, 4, 5.0, "holes", 1, "clamped", (0.7, -1.3)),
    (S_C1, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_C1, 0, 2.0, "hard", 1, "small", (0.7, -1.3)),       # the only class ignored: I = D = 0, the clamped branch, dice = 1
    (S_C1, -1, 0.0, "holes", 1, "small", (0, 1)),
    (S_C64, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_C64, 63, 0.5, "soft", 30, "small", (0.7, -1.3)),
    (S_C64, 31, 5.0, "holes", 1, "clamped", (1, 0)),
    (S_C64, 0, 0.0, "hard", 1, "small", (0, 1)),
    (S_VOL, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_VOL, 1, 0.5, "soft", 30, "clamped", (0.7, -1.3)),
    (S_VOL, 2, 5.0, "holes", 1, "small", (0, 1)),
    (S_VOL, 0, 0.0, "hard", 30, "small", (1, 0)),
    (S_WRAP, -1, 2.0, "hard", 1, "small", (0.7, -1.3)),
    (S_WRAP, 1, 0.5, "soft", 30, "small", (0.7, -1.3)),
]


def _seg_target(shape, kind, g):
    B, C = shape[:2]
    sp = tuple(shape[2:])
    if kind == "soft":            # each pixel's class weights: a row of a random stochastic matrix
        t = torch.rand((B,) + sp + (C,), generator=g)
        t = t / t.sum(-1, keepdim=True)
    else:
        t = F.one_hot(torch.randint(0, C, (B,) + sp, generator=g), C).float()
        if kind == "holes":       # some pixels carry no class at all
            t[torch.rand((B,) + sp, generator=g) < 0.2] = 0
    return t.movedim(-1, 1).contiguous()


def _weighted(dice, focal, a, b):
    """a * dice + b * focal with a zero weight leaving that output out of the graph altogether"""
    terms = [w * l for w, l in ((a, dice), (b, focal)) if w != 0]
    return sum(terms[1:], terms[0])


@pytest.mark.parametrize("shape,ignore,gamma,tkind,zscale,smooth,up", SEG_CASES)
def test_seg_losses(shape, ignore, gamma, tkind, zscale, smooth, up):
    ops = _ops()
    g = _gen(500 + shape[1] + len(shape) + int(10 * gamma) + zscale)
    z32 = torch.randn(shape, generator=g) * zscale
    t32 = _seg_target(shape, tkind, g)
    eps = F32(1e-6)
    if smooth == "clamped":       # 10 x the case's own denominator, from float64: the D <= smooth branch
        p = torch.softmax(z32.double(), 1)
        kept = [c for c in range(shape[1]) if c != ignore]
        sm = F32(10.0 * float((p[:, kept].sum() + t32.double()[:, kept].sum())))
    else:
        sm = F32(1e-6)
    z = z32.double().requires_grad_(True)
    ref_d, ref_f = LR.soft_dice(z, t32.double(), ignore, sm), LR.focal(z, t32.double(), gamma, eps)
    _weighted(ref_d, ref_f, *up).backward()
    zd = z32.to(DEV).requires_grad_(True)
    dice, foc = ops.seg_losses(zd, t32.to(DEV), ignore_index=ignore, smooth=sm, gamma=gamma, eps=eps)
    _weighted(dice, foc, *up).backward()
    tag = "%s ign %d gamma %g %s x%d %s %s" % (shape, ignore, gamma, tkind, zscale, smooth, up)
    _report("seg", "dice " + tag, dice, ref_d, LOSS_TOL, atol=DICE_ATOL)
    _report("seg", "focal " + tag, foc, ref_f, LOSS_TOL)
    _report("seg", "logits.grad " + tag, zd.grad, z.grad, SEG_GRAD_TOL)


def test_seg_losses_reject_too_many_classes():
    with pytest.raises(RuntimeError, match="vqw_seg_losses_fwd"):
        _ops().seg_losses(torch.zeros(1, 65, 4, 4, device=DEV), torch.zeros(1, 65, 4, 4, device=DEV))


# --------------------------------------------------------------------------------------------------
# DropBlock
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,blocks", [
    ((2, 12, 12), (1, 2, 3, 4, 7, 15)),      # 288 pixels: one per thread at most; block 15 is larger than the map
    ((3, 37, 29), (1, 2, 3, 4, 7)),          # 3219 pixels: 3 full strides of the 1024 threads and a ragged fourth
    ((4, 64, 64), (1, 2, 3, 4, 7)),          # 16384 pixels: every thread takes 16
])
def test_dropblock_mask(shape, blocks):
    ops = _ops()
    seed = (torch.rand(shape, generator=_gen(600 + shape[1])) < 0.05).float()
    for block in blocks:
        ref_keep, ref_scale = LR.dropblock_keep(seed.double(), block)
        keep, scale = ops.dropblock_mask(seed.to(DEV), block)
        assert np.array_equal(keep.cpu().numpy(), ref_keep.numpy()), "keep %s block %d" % (shape, block)
        _report("dropblock", "scale %s block %d" % (shape, block), scale.reshape(()), ref_scale, 1e-6)
    keep, scale = ops.dropblock_mask(torch.zeros(shape, device=DEV), 3)
    assert float(scale) == 1.0 and bool((keep == 1).all())


@pytest.mark.parametrize("shape", [(4, 40, 64, 64), (3, 1, 37, 29)])     # 655360 elements: k_dropblock_apply wraps; C = 1
def test_dropblock_apply(shape):
    ops = _ops()
    g = _gen(700 + shape[1])
    seed = (torch.rand((shape[0],) + shape[2:], generator=g) < 0.05).float()
    x32, up32 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    keep, scale = ops.dropblock_mask(seed.to(DEV), 4)
    x = x32.double().requires_grad_(True)
    ref = LR.dropblock_apply(x, keep.cpu().double(), scale.cpu().double())      # the kernel's own fp32 scale: apply alone is measured
    (ref * up32.double()).sum().backward()
    xd = x32.to(DEV).requires_grad_(True)
    y = ops.dropblock_apply(xd, keep, scale)
    (y * up32.to(DEV)).sum().backward()
    _report("dropblock", "apply y %s" % (shape,), y, ref, 1e-6)
    _report("dropblock", "apply x.grad %s" % (shape,), xd.grad, x.grad, 1e-6)


# --------------------------------------------------------------------------------------------------
# exact maps
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 20, 6, 4), (1, 64, 96, 96)])     # the last: 589824 outputs, the loop wraps
def test_pixel_shuffle2_exact(shape):
    """Random input (a ramp would hide a transposed (i, j)), forward and backward.  test_extras_golden's pixel-shuffle block
    would also move under a swapped (i, j) - its convolution weights are not symmetric - but only through a convolution at
    1e-4 and at one even, power-of-two shape; this adds exactness, odd H and W, a channel count that is no power of two
    and the second trip of the grid-stride loop."""
    ops = _ops()
    g = _gen(800 + shape[1])
    x32 = torch.randn(shape, generator=g)
    up32 = torch.randn(shape[0], shape[1] // 4, 2 * shape[2], 2 * shape[3], generator=g)
    x = x32.clone().requires_grad_(True)
    ref = LR.pixel_shuffle2(x)
    ref.backward(up32)            # a random upstream: under all ones the backward of any permutation is all ones
    xd = x32.to(DEV).requires_grad_(True)
    y = ops.pixel_shuffle2(xd)
    assert tuple(y.shape) == tuple(ref.shape)
    y.backward(up32.to(DEV))
    assert np.array_equal(y.detach().cpu().numpy(), ref.detach().numpy())
    assert np.array_equal(xd.grad.cpu().numpy(), x.grad.numpy())


@pytest.mark.parametrize("shape,n_classes", [((2, 13, 11), 7), ((1, 16, 16), 1025), ((2, 300, 300), 4)])   # the last: 720000 outputs wrap
def test_onehot_exact(shape, n_classes):
    lab = torch.randint(-2, n_classes + 2, shape, generator=_gen(900 + n_classes), dtype=torch.int32)   # some outside [0, n): all-zero columns
    lab.view(-1)[:3] = torch.tensor([-1, n_classes, n_classes + 1], dtype=torch.int32)
    out = _ops().onehot(lab.to(DEV), n_classes)
    assert out.dtype == torch.float32 and tuple(out.shape) == (shape[0], n_classes) + shape[1:]
    assert np.array_equal(out.cpu().numpy(), LR.onehot(lab, n_classes).numpy())


@pytest.mark.parametrize("shape,borders", [
    ((3, 17, 23), (0, 1, 3, 9)),             # W odd; border 9 >= H / 2: everything zero
    ((2, 600, 512), (0, 1, 3, 300)),         # W even; 614400 elements: the loop wraps
])
def test_flip_labels_exact(shape, borders):
    ids = torch.randint(0, 70000, shape, generator=_gen(1000 + shape[2]), dtype=torch.int64)
    for border in borders:
        out = _ops().flip_labels(ids.to(DEV), border)
        assert out.dtype == torch.int32
        ref = LR.flip_labels(ids, border)
        assert np.array_equal(out.cpu().numpy(), ref.numpy()), "flip %s border %d" % (shape, border)
        if 2 * border >= min(shape[1:]):
            assert int(ref.abs().sum()) == 0
