"""GPU tests of the U-Net discriminator and its second training step: every new kernel against the float64 restatement
(tests/unet_dis_ref.py) at the smallest shapes that can go wrong, the D_ch=4 module and the two-step run against the reference's
fixtures (tests/golden/unet_dis_*.npz, made by tests/golden/make_golden_unet_dis.py), a block-level case at matrix-core widths,
run-to-run bit-identity, a one-rank process group, and a run through the launcher.  Run with `pytest -m gpu` on an MI355X.

Tolerances of the kernel tests.  A tail output is a sum of at most 9 fp32 terms and a gradient of at most 5: relative error below
9 * 2^-24 = 5.4e-7 per element, held to 1e-6 of the tensor's norm.  Head and losses accumulate in double and round once to fp32
(the head after a 16-term fp32 sum): 1e-6 as well.  The spectral-norm kernels keep t = W^T u, s = W v and sigma as fp32 between
three launches, each a double accumulation: three roundings of 6e-8 chained through two normalisations - 1e-5 leaves two orders
of magnitude to an indexing error, which is of order 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, grad_gate, check_init
import unet_dis_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = 2.0 ** -24


def _nhwc(t):
    """(N, C, H, W) float64 -> dense (N, H, W, C) fp32 device array"""
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def _nchw(a):
    return a.permute(0, 3, 1, 2).double().cpu()


def _L():
    from hipops import ops
    return ops._L()


# ------------------------------------------------------------------------------------------------ tails
@pytest.mark.parametrize("absent", ["none", "out", "relu"])
@pytest.mark.parametrize("C", [4, 36, 3])          # float4 path (C % 4 == 0) / scalar path
def test_down_tail_kernels(C, absent):
    N, H, W = 2, 6, 10
    g = torch.Generator().manual_seed(C * 10)
    a = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    s = torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64).requires_grad_(True)
    go, gr = (torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64) for _ in range(2))
    out = F.avg_pool2d(a, 2) + s
    ((out * go).sum() * (absent != "out") + (F.relu(out) * gr).sum() * (absent != "relu")).backward()
    d_out = torch.full((N, H // 2, W // 2, C), -7.0, device=DEV) if absent != "out" else None
    d_relu = torch.full((N, H // 2, W // 2, C), -7.0, device=DEV) if absent != "relu" else None
    _L().vqw_unet_dtail_fwd(_nhwc(a), _nhwc(s), d_out, d_relu, N, H, W, C)
    if d_out is not None:
        assert_close(_nchw(d_out), out, 1e-6, "out")
    if d_relu is not None:
        assert_close(_nchw(d_relu), F.relu(out), 1e-6, "relu(out)")
    g_full = torch.full((N, H, W, C), -7.0, device=DEV)
    g_low = torch.full((N, H // 2, W // 2, C), -7.0, device=DEV)
    _L().vqw_unet_dtail_bwd(d_relu, _nhwc(go) if d_out is not None else None, _nhwc(gr) if d_relu is not None else None, g_full, g_low,
                            N, H, W, C)
    torch.cuda.synchronize()
    assert_close(_nchw(g_full), a.grad, 1e-6, "g_a")
    assert_close(_nchw(g_low), s.grad, 1e-6, "g_s")
    # without a shortcut: the pooling of a block's input
    pooled = torch.full((N, H // 2, W // 2, C), -7.0, device=DEV)
    _L().vqw_unet_dtail_fwd(_nhwc(a), None, pooled, None, N, H, W, C)
    torch.cuda.synchronize()
    assert_close(_nchw(pooled), F.avg_pool2d(a, 2), 1e-6, "avgpool2")


@pytest.mark.parametrize("absent", ["none", "out", "cat"])
@pytest.mark.parametrize("C,Cr", [(4, 8), (36, 8), (4, 3), (36, 3)])          # float4 path / scalar path
def test_up_tail_kernels(C, Cr, absent):
    """The rectified output lands at channel stride C + Cr, the rectified residual at channel offset C of the same buffer."""
    N, H, W = 2, 6, 10
    g = torch.Generator().manual_seed(C * 10 + Cr)
    h = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    s = torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(N, Cr, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    gc = torch.randn(N, C + Cr, H, W, generator=g, dtype=torch.float64)
    out = h + F.interpolate(s, scale_factor=2, mode="nearest")
    cat = torch.cat((F.relu(out), F.relu(res)), 1)
    ((out * go).sum() * (absent != "out") + (cat * gc).sum() * (absent != "cat")).backward()
    with_cat = absent != "cat"
    d_out = torch.full((N, H, W, C), -7.0, device=DEV) if absent != "out" else None
    d_cat = torch.full((N, H, W, C + Cr), -7.0, device=DEV) if with_cat else None
    _L().vqw_unet_utail_fwd(_nhwc(h), _nhwc(s), _nhwc(res) if with_cat else None, d_out, d_cat, N, H, W, C, Cr if with_cat else 0)
    if d_out is not None:
        assert_close(_nchw(d_out), out, 1e-6, "out")
    if with_cat:
        assert_close(_nchw(d_cat), cat, 1e-6, "cat")
    g_h = torch.full((N, H, W, C), -7.0, device=DEV)
    g_s = torch.full((N, H // 2, W // 2, C), -7.0, device=DEV)
    g_res = torch.full((N, H, W, Cr), -7.0, device=DEV) if with_cat else None
    _L().vqw_unet_utail_bwd(d_cat, _nhwc(go) if d_out is not None else None, _nhwc(gc) if with_cat else None, g_h, g_s, g_res, N, H, W,
                            C, Cr if with_cat else 0)
    torch.cuda.synchronize()
    assert_close(_nchw(g_h), h.grad, 1e-6, "g_h")
    assert_close(_nchw(g_s), s.grad, 1e-6, "g_s")
    if with_cat:
        assert_close(_nchw(g_res), res.grad, 1e-6, "g_res")


def test_tail_operators_differentiate():
    """ops.unet_down_tail / unet_up_tail through autograd, an unused output's gradient arriving as None."""
    from hipops import ops
    g = torch.Generator().manual_seed(5)
    a = torch.randn(2, 8, 6, 10, generator=g, dtype=torch.float64).requires_grad_(True)
    s = torch.randn(2, 8, 3, 5, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(2, 4, 6, 10, generator=g, dtype=torch.float64).requires_grad_(True)
    out = F.avg_pool2d(a, 2) + s
    up = a + F.interpolate(out, scale_factor=2, mode="nearest")
    cat = torch.cat((F.relu(up), F.relu(res)), 1)
    wc = U.weight_pattern(cat.shape)
    ((F.relu(out) * U.weight_pattern(out.shape)).sum() + (cat * wc).sum()).backward()
    a32, s32, r32 = (t.detach().float().to(DEV).requires_grad_(True) for t in (a, s, res))
    o, r = ops.unet_down_tail(a32, s_low=s32)
    u, c = ops.unet_up_tail(a32, o, res=r32)
    ((r * U.weight_pattern(out.shape).float().to(DEV)).sum() + (c * wc.float().to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert_close(c, cat, 1e-6, "cat")
    for name, t32, t64 in (("a", a32, a), ("s", s32, s), ("res", r32, res)):
        assert_close(t32.grad, t64.grad, 2e-6, "grad " + name)


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [64, 1024])
def test_bottleneck_head(C, N, bias):
    from hipops import ops
    g = torch.Generator().manual_seed(C + N)
    h = torch.randn(N, C, 4, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.randn(1, C, generator=g, dtype=torch.float64) / C ** 0.5).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(N, 1, generator=g, dtype=torch.float64)
    y = F.linear(F.relu(h).sum((2, 3)), w, b if bias else None)
    (y * gy).sum().backward()
    h32, w32, b32 = (t.detach().float().to(DEV).requires_grad_(True) for t in (h, w, b))
    y32 = ops.unet_bottleneck_head(h32, w32, b32 if bias else None)
    (y32 * gy.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert y32.shape == (N, 1)
    assert_close(y32, y, 1e-6, "bottleneck")
    for name, t32, t64 in (("h", h32, h), ("w", w32, w)) + ((("bias", b32, b),) if bias else ()):
        assert_close(t32.grad, t64.grad, 1e-6, "grad " + name)
    assert bias or b32.grad is None


# ------------------------------------------------------------------------------------------------ CutMix and the losses
BOXES = {"interior": ((3, 8), (5, 15)), "borders": ((0, 5), (12, 20)), "empty": ((2, 9), (6, 6)), "whole": ((0, 12), (0, 20))}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_cutmix_select_and_losses(box, flip):
    from hipops import ops
    B, H, W = 2, 12, 20
    bx = BOXES[box]
    g = torch.Generator().manual_seed(len(box) + flip)
    image, recon = (torch.randn(B, 1, H, W, generator=g) for _ in range(2))
    got = ops.cutmix_select(image.to(DEV), recon.to(DEV), bx, flip)
    assert torch.equal(got.cpu(), U.cutmix_images_ref(image, recon, bx, flip))            # a select: exact
    maps = [torch.randn(B, 1, H, W, generator=g, dtype=torch.float64).mul_(1.5).requires_grad_(True) for _ in range(3)]
    bots = [torch.randn(B, 1, generator=g, dtype=torch.float64).mul_(1.5).requires_grad_(True) for _ in range(3)]
    wts = (0.7, 1.3, 2.1)
    ref = U.dis_losses_ref(*maps, *bots, bx, flip)
    sum(w * l for w, l in zip(wts, ref)).backward()
    m32 = [t.detach().float().to(DEV).requires_grad_(True) for t in maps]
    b32 = [t.detach().float().to(DEV).requires_grad_(True) for t in bots]
    got = ops.unet_dis_losses(*m32, *b32, bx, flip)
    ops.weighted_sum(list(got), wts).backward()
    torch.cuda.synchronize()
    for name, a, r in zip(("dis", "cutmix", "consistency"), got, ref):
        assert a.dim() == 0
        assert_close(a, r, 1e-6, "l_" + name)
    for name, t32, t64 in zip(("r_map", "f_map", "c_map", "r_bottle", "f_bottle", "c_bottle"), m32 + b32, maps + bots):
        assert_close(t32.grad, t64.grad, 1e-6, "grad " + name, atol=1e-12)


# ------------------------------------------------------------------------------------------------ BigGAN spectral norm
@pytest.mark.parametrize("shape", [(1, 64), (36, 8, 3, 3)])
def test_biggan_spectral_norm(shape):
    from hipops import ops
    g = torch.Generator().manual_seed(shape[0])
    w = torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_(True)
    u0 = torch.randn(1, shape[0], generator=g, dtype=torch.float64)
    G = torch.randn(*shape, generator=g, dtype=torch.float64)
    u_ref, sv_ref = u0.clone(), torch.ones(1, dtype=torch.float64)
    wn = U.sn_weight_ref(w, u_ref, sv_ref, True)
    (wn * G).sum().backward()

    def dev(t):
        t = t.detach().float()
        return (t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t).to(DEV)
    w32 = dev(w).requires_grad_(True)
    u32, sv32 = dev(u0), torch.ones(1, device=DEV)
    # eval first: iterates on a copy, stores nothing
    with torch.no_grad():
        (we,) = ops.spectral_norm_weights([w32], [u32], None, False, svs=[sv32], biggan=True)
    assert torch.equal(u32.cpu(), u0.float()) and float(sv32) == 1.0
    (wt,) = ops.spectral_norm_weights([w32], [u32], None, True, svs=[sv32], biggan=True)
    (wt * dev(G)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(we, wt), "the eval forward must use this forward's iterated u', v"
    assert wt.shape == w.shape
    assert_close(wt, wn, 1e-5, "weight / sv")
    assert_close(u32, u_ref, 1e-5, "u0 after")
    assert_close(sv32, sv_ref, 1e-5, "sv0 after")
    if shape[0] > 1:
        assert not torch.equal(u32.cpu(), u0.float())
    assert_close(w32.grad, w.grad, 1e-5, "grad weight", atol=1e-7)


# ------------------------------------------------------------------------------------------------ module, D_ch = 4
def _module_state(golden, tag="mod", file="unet_dis_ch4.npz"):
    return {k[2:]: v for k, v in golden(file).group(tag).items() if k.startswith("P.")}


def _restatement_grads(state, x, dtype, fmt=None):
    st = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    for k, v in st.items():
        if k.endswith((".weight", ".bias")):
            if fmt is not None and v.dim() == 4:
                v = v.contiguous(memory_format=fmt)
            st[k] = v.requires_grad_(True)
    xin = x.detach().clone().to(dtype)
    if fmt is not None:
        xin = xin.contiguous(memory_format=fmt)
    xin.requires_grad_(True)
    out, bottle, feats = U.unet_discriminator_ref(xin, st, True)
    sum((o * U.weight_pattern(o.shape, dtype)).sum() for o in [out, bottle] + feats).backward()
    grads = {k: v.grad for k, v in st.items() if v.requires_grad and v.grad is not None}
    grads["input"] = xin.grad
    return grads


_gate_cache = {}


def _gate_inputs(golden):
    """fp64 truth and three fp32 evaluations of the restatement (8 threads, 1 thread, channels_last), computed once."""
    if not _gate_cache:
        state, x = _module_state(golden), golden("unet_dis_ch4.npz").t("mod/in.0")
        _gate_cache["truth"] = _restatement_grads(state, x, torch.float64)
        n = torch.get_num_threads()
        variants = [_restatement_grads(state, x, torch.float32)]
        torch.set_num_threads(1)
        try:
            variants.append(_restatement_grads(state, x, torch.float32))
        finally:
            torch.set_num_threads(n)
        variants.append(_restatement_grads(state, x, torch.float32, torch.channels_last))
        _gate_cache["variants"] = variants
    return _gate_cache["truth"], _gate_cache["variants"]


def test_module_golden(golden):
    """Outputs and state against the reference module at _run_block's tolerances (1e-4 forward, 1e-5 state); gradients through
    helpers.grad_gate against the fp64 restatement."""
    from networks import UNetDiscriminator
    g = golden("unet_dis_ch4.npz")
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    dis.load_state_dict(_module_state(golden), strict=True)
    dis.to(DEV).train()
    x = g.t("mod/in.0", DEV).requires_grad_(True)
    out, bottle, feats = dis(x)
    assert out.shape == (1, 1, 512, 512) and bottle.shape == (1, 1) and len(feats) == 7
    sum((o * U.weight_pattern(o.shape, torch.float32).to(DEV)).sum() for o in [out, bottle] + list(feats)).backward()
    torch.cuda.synchronize()
    assert_close(U.subset(out), g["mod/out.0"], 1e-4, "out")
    assert_close(bottle, g["mod/bottleneck"], 1e-4, "bottleneck")
    for i, f in enumerate(feats):
        assert_close(U.subset(f), g["mod/feat.%d" % i], 1e-4, "feat.%d" % i)
    n = 0
    for k, v in dis.state_dict().items():
        key = "mod/after." + k
        if key in g.files:
            assert_close(v.float(), g[key].astype(np.float32), 1e-5, key)
            n += 1
    assert n == 2 * 44          # u0 / sv0 of the 43 layers in use and of `linear`, which stays as loaded
    assert torch.equal(dis.linear.u0.cpu(), g.t("mod/P.linear.u0")) and dis.linear.weight.grad is None
    truth, variants = _gate_inputs(golden)
    test = {k: p.grad for k, p in dis.named_parameters() if p.grad is not None}
    test["input"] = x.grad
    assert set(test) == set(truth)
    grad_gate(truth, variants, test, what="UNetDiscriminator D_ch=4")


def test_module_eval_golden(golden):
    from networks import UNetDiscriminator
    g = golden("unet_dis_ch4.npz")
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    state = _module_state(golden)
    dis.load_state_dict(state, strict=True)
    dis.to(DEV).eval()
    with torch.no_grad():
        out, bottle, _ = dis(g.t("mod/in.0", DEV))
    torch.cuda.synchronize()
    assert_close(U.subset(out), g["eval/out.0"], 1e-4, "out")
    assert_close(bottle, g["eval/bottleneck"], 1e-4, "bottleneck")
    for k, v in dis.state_dict().items():
        if k.endswith(("u0", "sv0")):
            assert torch.equal(v.cpu(), state[k]), k


def test_narrow_module_forward():
    """D_wide=False (the down blocks' hidden width is their input width) against the float64 restatement: outputs at
    _run_block's forward tolerance, the spectral-norm state at its state tolerance, and every parameter in use gets a gradient."""
    from networks import UNetDiscriminator
    torch.manual_seed(11)
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=False, D_attn='0', resolution=512, unconditional=True)
    assert dis.blocks[1][0].conv1.weight.shape == (4, 4, 3, 3)
    st = {k: v.detach().clone().double() for k, v in dis.state_dict().items()}
    x = torch.randn(1, 1, 512, 512)
    with torch.no_grad():
        out64, bottle64, feats64 = U.unet_discriminator_ref(x.double(), st, True)
    dis.to(DEV).train()
    out, bottle, feats = dis(x.to(DEV))
    sum(o.sum() for o in [out, bottle] + list(feats)).backward()
    torch.cuda.synchronize()
    assert_close(out, out64, 1e-4, "out")
    assert_close(bottle, bottle64, 1e-4, "bottleneck")
    for i, (a, b) in enumerate(zip(feats, feats64)):
        assert_close(a, b, 1e-4, "feat.%d" % i)
    for k, v in dis.state_dict().items():
        if k.endswith(("u0", "sv0")):
            assert_close(v, st[k], 1e-5, k)
    for k, p in dis.named_parameters():
        assert (p.grad is None) == k.startswith("linear."), k
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), k


# ------------------------------------------------------------------------------------------------ blocks at matrix-core widths
def test_blocks_d_ch16_gate():
    """A down block 64 -> 128 and an up block reading a concat (256 -> 64) at 16 x 16, N = 2 - the widths of D_ch = 16, where the
    convolutions take the matrix-core paths - between a second down block and a first up block that produce their inputs;
    gradients through helpers.grad_gate against the restatement."""
    from networks import unet_discriminator as M
    torch.manual_seed(3)
    blocks = {"d1": M.DBlock(64, 128, preactivation=False), "d2": M.DBlock(128, 128, preactivation=True),
              "u1": M.GBlock2(128, 128), "u2": M.GBlock2(256, 64)}
    net = torch.nn.ModuleDict(blocks)
    M._channels_last_(net)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 64, 16, 16)

    def ref(dtype, fmt=None):
        st = {k: v.detach().clone().to(dtype) for k, v in state.items()}
        for k in st:
            if k.endswith((".weight", ".bias")):
                st[k] = (st[k].contiguous(memory_format=fmt) if fmt is not None and st[k].dim() == 4 else st[k]).requires_grad_(True)
        xin = x.detach().clone().to(dtype).requires_grad_(True)
        a = U.dblock_ref(xin, st, "d1.", True, False)
        b = U.dblock_ref(a, st, "d2.", True, True)
        c = U.gblock_ref(b, st, "u1.", True)
        d = U.gblock_ref(torch.cat((c, a), 1), st, "u2.", True)
        (d * U.weight_pattern(d.shape, dtype)).sum().backward()
        out = {k: v.grad for k, v in st.items() if v.requires_grad}
        out["input"] = xin.grad
        return d.detach(), out, st

    d64, truth, st64 = ref(torch.float64)
    variants = [ref(torch.float32)[1]]
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        variants.append(ref(torch.float32)[1])
    finally:
        torch.set_num_threads(n)
    variants.append(ref(torch.float32, torch.channels_last)[1])
    net.to(DEV).train()
    layers = [c for b in blocks.values() for c in (b.conv1, b.conv2, b.conv_sc)]
    W = M.sn_weights(layers, True)
    xin = x.to(DEV).requires_grad_(True)
    a, ra = M.down_block(blocks["d1"], W, xin, None)
    b, rb = M.down_block(blocks["d2"], W, a, ra)
    c, rc = M.up_block(blocks["u1"], W, b, rb, None, a)
    d, _ = M.up_block(blocks["u2"], W, c, rc, a, None, want_cat=False)
    (d * U.weight_pattern(d.shape, torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert_close(d, d64, 1e-4, "output")
    for k, v in net.state_dict().items():
        if k.endswith(("u0", "sv0")):
            assert_close(v, st64[k], 1e-5, k)
    test = {k: p.grad for k, p in net.named_parameters()}
    test["input"] = xin.grad
    grad_gate(truth, variants, test, what="blocks at D_ch=16 widths")


# ------------------------------------------------------------------------------------------------ the two-step fixture
def _step_trainer(golden, **kw):
    from helpers import build_models
    from networks import UNetDiscriminator
    from trainers import UNetSecondStepTrainer, UNetGanLossWeights
    g = golden("unet_dis_step.npz")
    cfg = {k: g["step/cfg/" + k] for k in ("enc_filters", "dec_filters", "K", "momentum", "seed")}
    enc, dec = build_models(cfg)
    sums = {k[len("step/"):]: g[k] for k in g.files if k.startswith("step/init_sum/")}
    check_init(sums, enc, dec)
    K = int(cfg["K"])
    with torch.no_grad():
        enc.vq.embed.mul_(0.7)
        enc.vq.cluster_size.fill_(512 * 512 / K)
        enc.vq.embed_avg.copy_(enc.vq.embed.t() * enc.vq.cluster_size[None, :])
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    dis.load_state_dict(_module_state(golden, "step", "unet_dis_step.npz"), strict=True)
    w = UNetGanLossWeights(**{k: float(g["step/cfg/w." + k]) for k in UNetGanLossWeights._fields})
    boxes = []
    for s in range(2):
        y0, y1, x0, x1 = (int(v) for v in g["step/box%d" % s])
        boxes.append((((y0, y1), (x0, x1)), bool(int(g["step/flip%d" % s]))))
    it = iter(boxes)
    return UNetSecondStepTrainer(enc, dec, dis, loss_weight=w, lr=float(g["step/cfg/lr"]), betas=tuple(float(b) for b in g["step/cfg/betas"]),
                                 device=DEV, use_unet_perceptual_loss=True, cutmix_box=lambda: next(it), **kw)


def _run_two_steps(golden, **kw):
    g = golden("unet_dis_step.npz")
    tr = _step_trainer(golden, **kw)
    outs = []
    for s in range(2):
        out = tr.training_step({"image": g.t("step/image%d" % s, DEV)})
        outs.append({k: v.detach().clone() for k, v in out.items()})
    torch.cuda.synchronize()
    return tr, outs


def test_two_steps_golden(golden):
    """All ten logged losses of both steps within 2 x the fixture's own fp32-against-fp64 spread (+ fp32 storage rounding) of
    the largest of them, as tests/test_gan_norms_host.py holds the discriminator-update fixture; the state after as
    test_discriminator_update_golden_spectral_actnorm compares it (2e-3 of the norm, atol 2e-4).  The fixture's Adam runs at
    lr 1e-6 (see make_golden_unet_dis.py), which that state tolerance does not resolve, so the UPDATE of the discriminator and of
    the decoder (after - before) is also held to the reference run's, within twice the fixture's own fp32-against-fp64 distance
    of that update: a skipped optimiser step is 100 % off, a wrong-signed or missing loss term of the generator half far more
    than the decoder's 11 %."""
    g = golden("unet_dis_step.npz")
    before = _module_state(golden, "step", "unet_dis_step.npz")
    tr = _step_trainer(golden)
    dec_before = {k: v.detach().cpu().clone() for k, v in tr.decoder.state_dict().items()}
    outs = []
    for s in range(2):
        out = tr.training_step({"image": g.t("step/image%d" % s, DEV)})
        outs.append({k: v.detach().clone() for k, v in out.items()})
    torch.cuda.synchronize()
    sp = float(g["step/spread.loss"])
    worst = []
    for s, out in enumerate(outs):
        ref = torch.from_numpy(g["step/loss%d" % s]).double()
        got = torch.stack([out[k].double().cpu() if k in out else torch.zeros((), dtype=torch.float64) for k in U.LOSS_NAMES])
        scale = float(ref.abs().max())
        for k, a, r in zip(U.LOSS_NAMES, got.tolist(), ref.tolist()):
            print("step %d %-16s %.8g  reference %.8g  |diff| / largest %.3e  (spread %.1e)" % (s, k, a, r, abs(a - r) / scale, sp))
        worst.append((float((got - ref).abs().max()), (2.0 * sp + F32_EPS) * scale))
        assert "freq" not in out and "perceptual" not in out
    for file, pre, m in (("unet_dis_step_after.npz", "dis", tr.dis), ("unet_dis_step_dec.npz", "dec", tr.decoder)):
        ga = golden(file)
        for k, v in m.state_dict().items():
            ref = ga["step/after.%s.%s" % (pre, k)]
            if v.is_floating_point():
                assert_close(v.float(), ref.astype(np.float32), 2e-3, "after.%s.%s" % (pre, k), atol=2e-4)
            else:
                assert int(v) == int(ref), k
    # the updates themselves (after - before, all parameters of a network as one vector) against the reference run's: both
    # that run and this one are fp32 evaluations, each within the fixture's fp32-against-fp64 distance of the fp64 update
    # (spread.update_*: 5.4e-2 for the decoder, whose biases in front of an InstanceNorm have pure rounding noise for a
    # gradient, which Adam turns into steps; 1.3e-3 for the discriminator), hence within twice that of each other
    for file, pre, m, prior in (("unet_dis_step_after.npz", "dis", tr.dis, before), ("unet_dis_step_dec.npz", "dec", tr.decoder, dec_before)):
        ga, sd = golden(file), m.state_dict()
        names = [k for k, _ in m.named_parameters()]
        upd = torch.cat([(sd[k].cpu().double() - prior[k].double()).reshape(-1) for k in names])
        upd_ref = torch.cat([(ga.t("step/after.%s.%s" % (pre, k)).double() - prior[k].double()).reshape(-1) for k in names])
        e, bound = float((upd - upd_ref).norm() / upd_ref.norm()), 2.0 * float(g["step/spread.update_" + pre])
        print("%s update: %.3e from the reference's (norm %.3e over %d entries; bound %.3e)" % (pre, e, float(upd_ref.norm()), upd.numel(), bound))
        assert float(upd_ref.norm()) > 0 and e <= bound, "%s update %.3e > %.3e" % (pre, e, bound)
    for k in ("linear.weight", "linear.bias"):
        assert torch.equal(tr.dis.state_dict()[k].cpu(), before[k]), k
    for s, (err, bound) in enumerate(worst):
        assert err <= bound, "step %d: max |diff| %.3e > %.3e" % (s, err, bound)


def test_two_steps_are_deterministic(golden):
    a, oa = _run_two_steps(golden)
    b, ob = _run_two_steps(golden)
    for x, y in zip(oa, ob):
        assert list(x) == list(y)
        for k in x:
            assert torch.equal(x[k], y[k]), k
    for ma, mb in ((a.decoder, b.decoder), (a.dis, b.dis)):
        for (k, v), (_, v2) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, v2), k


def test_two_inner_loops_equal_two_discriminator_updates(golden):
    """n_inner_loops = 2: the second loop draws a second rectangle and runs the discriminator on the u0 the first loop left -
    bit for bit what one step with a single loop followed by one more discriminator_update on the same image and
    reconstruction gives."""
    g = golden("unet_dis_step.npz")
    image = g.t("step/image0", DEV)
    a, b = _step_trainer(golden, n_inner_loops=2), _step_trainer(golden)
    out_a = a.training_step({"image": image})
    out_b = b.training_step({"image": image})
    last = b.discriminator_update(image, out_b["recon_image"])
    torch.cuda.synchronize()
    for k, v in zip(("dis_total", "dis", "cutmix", "consistency"), last):
        assert torch.equal(out_a[k], v), k
        assert not torch.equal(out_a[k], out_b[k]), k + ": the second loop changed nothing"
    for k in ("gen_total", "recon", "gen", "unet_perceptual"):
        assert torch.equal(out_a[k], out_b[k]), k
    for (k, v), (_, v2) in zip(a.dis.state_dict().items(), b.dis.state_dict().items()):
        assert torch.equal(v, v2), k
    assert all(st["step"] == 2 for st in a.dis_optim.state.values()) and len(a.dis_optim.state) == len(list(a.dis.parameters())) - 2


WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "medical-image-editing_amd")); sys.path.insert(0, os.path.join(root, "tests"))
forced = os.environ.get("VQW_DP_FORCE", "0") == "1"      # one rank, every collective issued all the same (hipops.ops)
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1)
from conftest import load_golden
import test_gpu_unet_dis as T
tr, outs = T._run_two_steps(load_golden, data_parallel=forced)
torch.save({"losses": [{k: v.cpu() for k, v in o.items()} for o in outs],
            "state": {n: {k: v.cpu() for k, v in m.state_dict().items()} for n, m in (("dec", tr.decoder), ("dis", tr.dis))}}, out)
if forced:
    dist.barrier(); dist.destroy_process_group()
'''


def test_one_rank_process_group_equals_plain_run(tmp_path):
    """With one rank the gradient all-reduce is the identity: the two steps under a process group (reducers on, `linear.*` kept
    out of the discriminator's) equal the plain run bit for bit."""
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    res = []
    for tag, port, extra in (("plain", 29651, {}), ("group", 29652, {"VQW_DP_FORCE": "1"})):
        out = str(tmp_path / tag)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", **extra)
        p = subprocess.Popen([sys.executable, str(script), ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        o = p.communicate(timeout=500)[0].decode()
        assert p.returncode == 0, o[-3000:]
        res.append(torch.load(out))
    plain, group = res
    for a, b in zip(plain["losses"], group["losses"]):
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for n in plain["state"]:
        for k in plain["state"][n]:
            assert torch.equal(plain["state"][n][k], group["state"][n][k]), (n, k)


# ------------------------------------------------------------------------------------------------ through the launcher
UNET_DIS = dict(model_name="UNetDiscriminator", D_ch=4, D_wide=True, D_attn="0", resolution=512, normalization="batchnorm")
NEW_COLUMNS = ["unet_perceptual", "cutmix", "consistency"]


def _launch(tmp, name, n_epochs, resume=None):
    from run_helpers import MONITORED, raw_config, run_launcher, write_config
    save = os.path.join(str(tmp), name)
    raw = raw_config(save, None, run=dict(training_mode="second_step", n_epochs=n_epochs, monitoring_metrics=MONITORED + NEW_COLUMNS),
                     dataset=dict(dataset_name="synthetic", image_size=512, batch_size=1, n_samples_train=2, n_samples_val=1),
                     model=dict(dis=dict(UNET_DIS), vqmodel=dict(enc_filters=[4, 8, 16, 32, 64], dec_filters=[8, 16, 32, 64, 128])),
                     loss=dict(use_unet_perceptual_loss=True, loss_weight=dict(gen=0.5, dis=1.0, unet_perceptual=0.25, cutmix=0.75, consistency=2.0)),
                     save=dict(n_save_images=1))
    if resume:
        raw["run"]["resume_checkpoint"] = resume
    run_launcher(write_config(os.path.join(str(tmp), name + "%d.json" % n_epochs), raw))
    return save


def _ckpt(save, epoch, n=0):
    return os.path.join(save, "study", "version_%d" % n, "ckpt-epoch=%04d-total_loss=0.00.ckpt" % epoch)


def test_launcher_trains_logs_checkpoints_and_resumes(tmp_path):
    """`run_vqwnet.py` in second_step mode at 512 x 512, batch 1, D_ch = 4 on two synthetic samples: log.csv carries the new
    columns, the checkpoint's dis.* keys load strictly, and a run resumed from the first epoch's checkpoint ends bit-identical to
    the uninterrupted one (in the manner of tests/test_gpu_run.py; the CutMix draws come from the saved generator states)."""
    from run_helpers import MONITORED, read_csv
    from networks import UNetDiscriminator
    from utils.checkpoint import load_discriminator_from_ckpt
    from test_gpu_run import _differences
    full = _launch(tmp_path, "full", 2)
    header, rows = read_csv(os.path.join(full, "study", "version_0", "log.csv"))
    assert header == MONITORED + NEW_COLUMNS and len(rows) == 4
    for row in rows:
        rec = dict(zip(header, row))
        for k in ("total", "gen_total", "recon", "gen", "unet_perceptual", "dis_total", "dis", "cutmix", "consistency"):
            assert np.isfinite(float(rec[k])), (k, rec[k])
        assert float(rec["cutmix"]) > 0.0 and float(rec["unet_perceptual"]) > 0.0
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn="0", resolution=512)
    before = {k: v.clone() for k, v in dis.state_dict().items()}
    load_discriminator_from_ckpt(_ckpt(full, 1), dis)                       # strict
    assert not torch.equal(dis.blocks[0][0].conv1.u0, before["blocks.0.0.conv1.u0"])
    part = _launch(tmp_path, "part", 1)
    assert not _differences(_ckpt(part, 0), _ckpt(full, 0))
    _launch(tmp_path, "part", 2, resume=_ckpt(part, 0))
    diff = _differences(_ckpt(part, 1, n=1), _ckpt(full, 1))
    assert not diff, "resumed run differs from the uninterrupted one in %d tensors, e.g. %s" % (len(diff), diff[:8])
    _, rows_resumed = read_csv(os.path.join(part, "study", "version_1", "log.csv"))
    assert rows_resumed == rows[2:]
