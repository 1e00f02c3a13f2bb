"""The normalisation kernels (csrc/norm.hip) against a float64 restatement on the CPU, at the sizes and shapes that select each
dispatch form.

Every case builds its fp32 inputs on the CPU, hands the SAME values (cast to double) to plain ATen ops - F.instance_norm,
F.batch_norm, F.leaky_relu, F.max_pool2d and arithmetic - and takes the reference gradients from float64 autograd against a
fixed random cotangent r.  Errors are relative L2 (helpers.rel_err) and every case prints them.

Bounds: forward outputs 2e-5, input gradients 5e-5, gamma / beta gradients 2e-5 (the single-kernel bounds of the suite);
running statistics 2e-6 per element.  The offset cases add the one term fp32 storage of the mean implies, 2^-23 |mean| / std
(_mean_term), computed from the data of the case.

A ReLU / LeakyReLU / max-pool mask is a discontinuity: where the float64 pre-activation lies within MASK_BAND of the switch
point (or a 2x2 window's two largest values are that close) the fp32 kernel may legitimately take the other side, and one such
element costs ~3e-4 of a 8M-element gradient's norm.  Those elements (a fraction of ~1e-4, asserted below MASK_FRACTION) are left
out of the elementwise gradient comparisons; forward outputs are compared everywhere.  batch_norm_lrelu's gamma / beta gradients
are sums over every pixel of a channel, so there the reference takes the kernel's own branch inside the band instead (the sign of
its output).  A float64 pre-activation below 1e-9 is the rounding residue of an exactly constant plane, whose normalised value
is exactly 0 in fp32: the reference snaps it to 0, where the ReLU masks it on both sides.

Which kernel a row reaches follows from the dispatch in norm.hip: al16 (16-byte aligned pointers) and C % 4 == 0 pick the
float4 kernels, walk_ok(C / 4) (C / 4 a power of two <= 256) the pipelined reduction k_plane_reduce4p and the division-free
walks *4w; plane_splits / plane_splits_p give the reduction splits per image, walk_blocks the walk's workgroups per image (a
thread walks more than one 4 R-pixel step, R = 256 / (C / 4), only when N * H * W * C > 8M).
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

FWD_TOL = 2e-5          # forward outputs
GRAD_TOL = 5e-5         # input gradients
PARAM_TOL = 2e-5        # gamma / beta gradients
STAT_TOL = 2e-6         # running mean / var, per element
MASK_BAND = 1e-4        # |float64 pre-activation| (in units of the normalised value) below which the mask may flip in fp32
MASK_FRACTION = 1e-3    # at most this share of the elements may fall in that band
CONST_RESIDUE = 1e-9    # |float64 normalised value| below this: an exactly constant plane (exactly 0 in fp32)


def _ops():
    from hipops import ops
    return ops


def _seed(case):
    return zlib.crc32(repr(case).encode())


def _gpu(t, grad=False):
    """fp32 channels_last copy on the GPU of a CPU tensor."""
    g = t.float().to(DEV)
    if g.dim() == 4:
        g = g.contiguous(memory_format=CL)
    return g.requires_grad_(True) if grad else g


def _ref(t):
    """float64 CPU leaf holding exactly the values the GPU sees."""
    return t.detach().float().cpu().double().requires_grad_(True)


def _check(tag, what, got, ref, tol, keep=None):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if keep is not None:
        got, ref = got * keep, ref * keep
    print("  %-48s %-12s rel %.2e  (bound %.2e)" % (tag, what, rel_err(got, ref), tol))
    assert_close(got, ref, tol, "%s: %s" % (tag, what))


def _band(z):
    """1 where the float64 pre-activation z is clear of the switch point at 0, else 0 (see MASK_BAND).  An exact zero (a constant
    plane) stays: both sides compute it exactly and mask it."""
    z = z.detach()
    keep = ((z.abs() >= MASK_BAND) | (z.abs() < CONST_RESIDUE)).double()
    assert float(1.0 - keep.mean()) <= MASK_FRACTION, "%.2e of the pre-activations within %.0e of zero" % (1.0 - float(keep.mean()), MASK_BAND)
    return keep


def _mean_term(x64):
    """2^-23 * max over planes of |mean| / std: the error fp32 storage of the plane mean adds to a normalised value."""
    m = x64.detach().mean(dim=(2, 3))
    s = x64.detach().std(dim=(2, 3), unbiased=False)
    return 2.0 ** -23 * float((m.abs() / s.clamp_min(1e-30)).max())


def _planes(g, N, C, H, W, kind):
    """Test data: per-(image, channel) planes with their own scale and offset.
    kind 'offset': planes 100 standard deviations off zero (E[x^2] - mean^2 cancels in fp32);
    'edge': channel 0 exactly constant, channel 1 exactly zero - both have var = 0 and rstd = 1 / sqrt(eps).  The constant 1.15
    has an fp32 square 4.5e-8 above its exact square: E[x^2] - mean^2 from fp32 squares would leave that as the variance, 0.45 %
    of eps; 'small': std ~0.05, so that eps matters."""
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    if kind == "offset":
        sign = torch.where(torch.rand(N, C, 1, 1, generator=g) < 0.5, -1.0, 1.0).double()
        return x * 0.02 + 2.0 * sign
    if kind == "small":
        return x * 0.05 + 0.1
    scale = 0.5 + 1.5 * torch.rand(N, C, 1, 1, generator=g, dtype=torch.float64)
    shift = torch.rand(N, C, 1, 1, generator=g, dtype=torch.float64) * 2 - 1
    x = x * scale + shift
    if kind == "edge":
        x[:, 0] = 1.15
        x[:, 1] = 0.0
    return x


# --------------------------------------------------------------------------------------------------
# instance_norm
# --------------------------------------------------------------------------------------------------
IN_CASES = [
    # (N, C, H, W, data, eps)
    (4, 32, 256, 256, "randn", 1e-5),     # FStats4 / FInBwd4 in k_plane_reduce4p at 64 splits (plane_splits_p), k_inorm_apply4w / k_inorm_bwd_apply4w with 512 workgroups per image, one walk step per thread
    (8, 32, 256, 256, "randn", 1e-5),     # the same walks with two 4 R-pixel steps per thread (walk_blocks 256 < 512 steps per image)
    (32, 16, 64, 64, "randn", 1e-5),      # large N: k_plane_reduce4p at 2 splits, 16 walk workgroups per image (C4 = 4, R = 64)
    (3, 32, 97, 83, "randn", 1e-5),       # ragged: 7 reduction splits of 1151 pixels (the last one short), 63 walk workgroups, the last step partial
    (2, 48, 128, 128, "randn", 1e-5),     # C4 = 12 (not a power of two): k_plane_reduce4 at 64 splits, flat-index k_inorm_apply4 / k_inorm_bwd_apply4
    (2, 160, 128, 128, "randn", 1e-5),    # C4 = 40: the same float4 kernels without walks, 40 lanes per pixel
    (3, 5, 97, 83, "randn", 1e-5),        # C = 5: generic k_plane_reduce (31 splits of 260 pixels, the last 251), k_inorm_apply / k_inorm_bwd_apply
    (2, 258, 12, 12, "randn", 1e-5),      # C = 258 > 256: k_plane_reduce's channel loop (two passes of 256 lanes), one split
    (2, 32, 128, 128, "offset", 1e-5),    # walk forms, planes 100 std off zero: the statistics must not cancel in fp32
    (3, 5, 97, 83, "offset", 1e-5),       # generic kernels, planes 100 std off zero
    (2, 8, 64, 64, "edge", 1e-5),         # constant and zero channels (var = 0, rstd = 1 / sqrt(eps)): k_plane_reduce4p, C4 = 2 walks
    (2, 12, 32, 32, "edge", 1e-5),        # the same through k_plane_reduce4 and the flat float4 kernels (C4 = 3)
    (2, 16, 64, 64, "small", 1e-3),       # eps = 1e-3 against variances ~2.5e-3
]


def _in_case_id(c):
    return "%dx%dx%dx%d-%s-eps%g" % c


def _in_ref(x64, relu, eps):
    y = F.instance_norm(x64, eps=eps)
    if not relu:
        return y, y
    return torch.relu(y * (y.detach().abs() >= CONST_RESIDUE)), y


@pytest.mark.parametrize("relu", [False, True], ids=["norm", "norm_relu"])
@pytest.mark.parametrize("case", IN_CASES, ids=_in_case_id)
def test_instance_norm_vs_float64(case, relu):
    ops = _ops()
    N, C, H, W, kind, eps = case
    g = torch.Generator().manual_seed(_seed(case))
    x = _planes(g, N, C, H, W, kind)
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    x64 = _ref(x)
    y64, z64 = _in_ref(x64, relu, eps)
    (y64 * r).sum().backward()
    dx = _gpu(x, grad=True)
    y = ops.instance_norm(dx, relu=relu, eps=eps)
    (y * _gpu(r)).sum().backward()
    torch.cuda.synchronize()
    extra = _mean_term(x64) if kind == "offset" else 0.0
    keep = _band(z64) if relu else None
    tag = "instance_norm %s relu=%d" % (_in_case_id(case), relu)
    if extra:
        print("  %-48s mean term %.2e" % (tag, extra))
    assert torch.isfinite(y).all() and torch.isfinite(dx.grad).all()
    _check(tag, "y", y, y64, FWD_TOL + extra)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL + extra, keep)


def test_instance_norm_misaligned_input():
    """A channels_last view at storage offset 1 passes nhwc() uncopied; its pointer fails al16, so the forward and backward take
    the generic kernels (k_plane_reduce, k_inorm_apply, k_inorm_bwd_apply) although C % 4 == 0.  They agree with float64 and with
    the aligned run (float4 walks) to 1e-6."""
    ops = _ops()
    N, C, H, W = 2, 32, 64, 64
    g = torch.Generator().manual_seed(5)
    x = _planes(g, N, C, H, W, "randn")
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    for relu in (False, True):
        x64 = _ref(x)
        y64, z64 = _in_ref(x64, relu, 1e-5)
        (y64 * r).sum().backward()
        buf = torch.empty(N * H * W * C + 1, device=DEV)
        buf[1:].copy_(x.float().permute(0, 2, 3, 1).reshape(-1).to(DEV))
        xm = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2).detach().requires_grad_(True)
        assert xm.is_contiguous(memory_format=CL) and xm.data_ptr() % 16 == 4
        assert ops.nhwc(xm).data_ptr() == xm.data_ptr()
        xa = _gpu(x, grad=True)
        rr = _gpu(r)
        ym = ops.instance_norm(xm, relu=relu)
        ya = ops.instance_norm(xa, relu=relu)
        (ym * rr).sum().backward()
        (ya * rr).sum().backward()
        torch.cuda.synchronize()
        tag = "instance_norm misaligned relu=%d" % relu
        keep = _band(z64) if relu else None
        _check(tag, "y", ym, y64, FWD_TOL)
        _check(tag, "dx", xm.grad, x64.grad, GRAD_TOL, keep)
        _check(tag, "y vs aligned", ym, ya, 1e-6)
        _check(tag, "dx vs aligned", xm.grad, xa.grad, 1e-6)


@pytest.mark.parametrize("relu", [False, True], ids=["norm", "norm_relu"])
def test_instance_norm_from_conv_partials(relu):
    """instance_norm(y, part=...) with the (sum, M2) partials of the producing convolution's epilogue at 256 x 256
    (k_plane_finalize<TileMoments>, then the walks), against float64 of the same y - not against the HIP reduction."""
    ops = _ops()
    torch.manual_seed(7)
    N, Cin, C, S = 4, 32, 32, 256
    u = torch.randn(N, Cin, S, S, device=DEV).contiguous(memory_format=CL)
    w = (torch.randn(C, Cin, 3, 3, device=DEV) * 0.1).contiguous(memory_format=CL)
    b = torch.randn(C, device=DEV)
    with torch.no_grad():
        y_raw, part = ops.conv2d(u, w, b, want_stats=True)
    assert part is not None
    r = torch.randn(N, C, S, S, dtype=torch.float64)
    x64 = _ref(y_raw)
    y64, z64 = _in_ref(x64, relu, 1e-5)
    (y64 * r).sum().backward()
    dx = y_raw.detach().clone(memory_format=CL).requires_grad_(True)
    y = ops.instance_norm(dx, relu=relu, part=part)
    (y * _gpu(r)).sum().backward()
    torch.cuda.synchronize()
    tag = "instance_norm conv partials relu=%d" % relu
    _check(tag, "y", y, y64, FWD_TOL)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL, _band(z64) if relu else None)


def test_instance_norm_backward_sums_from_the_consumer_conv():
    """InstanceNorm + ReLU feeding ONE 3x3 convolution (conv2d(..., norm_input=True)): the convolution's input-gradient launch
    leaves the norm's backward sums and the norm's backward finalises them (k_plane_finalize<RegionSums>) - against float64 of
    conv(relu(IN(x)))."""
    ops = _ops()
    g = torch.Generator().manual_seed(9)
    N, C, S = 2, 32, 64
    x = _planes(g, N, C, S, S, "randn")
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * 0.1
    r = torch.randn(N, C, S, S, generator=g, dtype=torch.float64)
    x64, w64 = _ref(x), w.float().double()
    z64 = F.instance_norm(x64, eps=1e-5)
    y64 = F.conv2d(torch.relu(z64), w64, padding=1)
    (y64 * r).sum().backward()
    dx = _gpu(x, grad=True)
    dw = _gpu(w)
    n0 = ops.in_bwd_fused_calls
    y = ops.conv2d(ops.instance_norm(dx, relu=True), dw, None, norm_input=True)
    (y * _gpu(r)).sum().backward()
    torch.cuda.synchronize()
    assert ops.in_bwd_fused_calls == n0 + 1, "the fused backward route was not taken"
    tag = "instance_norm -> conv (norm_input)"
    _check(tag, "y", y, y64, FWD_TOL)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL, _band(z64))


# --------------------------------------------------------------------------------------------------
# instance_norm_cat (the ASPP tail)
# --------------------------------------------------------------------------------------------------
CAT_CASES = [
    # (N, H, W, channels per input, parts from the producing convolutions)
    (2, 128, 128, (32, 32, 32, 32, 32), False),   # five slices of a 160-channel output at offsets 0, 32, ...: walks with strides ycs4 = gcs4 = 40
    (2, 128, 128, (32, 32, 32, 32, 32), True),    # the same with every input's statistics from its convolution (k_plane_finalize<TileMoments>)
    (2, 40, 40, (16, 5, 32), False),              # total 53 channels, offsets 0, 16, 21: the stride (and offset 21) defeat float4, C = 5 generic throughout
    (2, 40, 40, (8, 4, 36), False),               # offsets 0, 8, 12 keep float4: C4 = 2, 1 walks and C4 = 9 flat k_inorm_apply4 / k_inorm_bwd_apply4 on a 12-float4 stride
]


@pytest.mark.parametrize("case", CAT_CASES, ids=lambda c: "%dx%dx%d-%s-parts%d" % (c[0], c[1], c[2], "-".join(map(str, c[3])), c[4]))
def test_instance_norm_cat_vs_float64(case):
    ops = _ops()
    N, H, W, chans, with_parts = case
    g = torch.Generator().manual_seed(_seed(case))
    if with_parts:
        xs, parts = [], []
        for k, C in enumerate(chans):
            u = _gpu(torch.randn(N, 16, H, W, generator=g))
            w = _gpu(torch.randn(C, 16, 3, 3, generator=g) * 0.2)
            with torch.no_grad():
                y_raw, part = ops.conv2d(u, w, _gpu(torch.randn(C, generator=g)), want_stats=True)
            assert part is not None
            xs.append(y_raw.detach().cpu().double())
            parts.append(part)
    else:
        xs, parts = [_planes(g, N, C, H, W, "randn") for C in chans], None
    r = torch.randn(N, sum(chans), H, W, generator=g, dtype=torch.float64)
    x64 = [_ref(x) for x in xs]
    z64 = [F.instance_norm(x, eps=1e-5) for x in x64]
    y64 = torch.cat([torch.relu(z) for z in z64], 1)
    (y64 * r).sum().backward()
    dxs = [_gpu(x, grad=True) for x in xs]
    y = ops.instance_norm_cat(dxs, relu=True, eps=1e-5, parts=parts)
    (y * _gpu(r)).sum().backward()
    torch.cuda.synchronize()
    tag = "instance_norm_cat %s parts=%d" % ("+".join(map(str, chans)), with_parts)
    _check(tag, "y", y, y64, FWD_TOL)
    for k in range(len(xs)):
        _check(tag, "dx[%d]" % k, dxs[k].grad, x64[k].grad, GRAD_TOL, _band(z64[k]))


# --------------------------------------------------------------------------------------------------
# add_norm, res_tail_norm
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["norm", "norm_relu"])
@pytest.mark.parametrize("with_part", [False, True], ids=["stats", "parts"])
def test_add_norm_vs_float64(with_part, relu):
    """a + relu?(IN(x)) in one walk (k_inorm_add4w) at 256 x 256, statistics by k_plane_reduce4p or from the conv's partials;
    x's gradient by vqw_inorm_bwd."""
    ops = _ops()
    torch.manual_seed(13)
    N, C, S = 2, 32, 256
    g = torch.Generator().manual_seed(13)
    a = _planes(g, N, C, S, S, "randn")
    if with_part:
        with torch.no_grad():
            y_raw, part = ops.conv2d(_gpu(torch.randn(N, 32, S, S, generator=g)), _gpu(torch.randn(C, 32, 3, 3, generator=g) * 0.1),
                                     _gpu(torch.randn(C, generator=g)), want_stats=True)
        assert part is not None
        x = y_raw.cpu().double()
    else:
        x, part = _planes(g, N, C, S, S, "randn"), None
    r = torch.randn(N, C, S, S, generator=g, dtype=torch.float64)
    a64, x64 = _ref(a), _ref(x)
    z64 = F.instance_norm(x64, eps=1e-5)
    y64 = a64 + (torch.relu(z64) if relu else z64)
    (y64 * r).sum().backward()
    da, dx = _gpu(a, grad=True), _gpu(x, grad=True)
    assert ops.add_norm_supported(da, dx)
    y = ops.add_norm(da, dx, part=part, relu=relu, eps=1e-5)
    (y * _gpu(r)).sum().backward()
    torch.cuda.synchronize()
    tag = "add_norm parts=%d relu=%d" % (with_part, relu)
    _check(tag, "y", y, y64, FWD_TOL)
    _check(tag, "da", da.grad, a64.grad, GRAD_TOL)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL, _band(z64) if relu else None)


def _window_keep(out64):
    """1 on the 2x2 windows whose two largest float64 values are at least MASK_BAND apart (the max-pool's routing is settled)."""
    N, C, H, W = out64.shape
    win = out64.detach().reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    top = win.topk(2, dim=-1).values
    ok = (((top[..., 0] - top[..., 1]) >= MASK_BAND) | (top[..., 0] <= 0)).double()     # (an all-zero window routes nothing)
    return ok.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


RES_TAIL_CASES = [
    # (N, C, H, W, statistics of x2 / xid from: "stats" own reduction, "parts" conv partials of both, "part2" of x2 only)
    (2, 32, 256, 256, "stats"),   # vqw_inorm_stats twice (k_plane_reduce4p), fused backward k_res_tail_bwd_pair_reduce4 + two-job k_plane_finalize<SplitSums> + k_inorm_bwd_pair_apply4w
    (2, 32, 256, 256, "parts"),   # both norms' statistics in one launch (two-job k_plane_finalize<TileMoments>)
    (2, 32, 256, 256, "part2"),   # x2 from partials (k_plane_finalize<TileMoments>), xid by its own reduction
    (2, 48, 64, 64, "stats"),     # C4 = 12: flat k_inorm_bwd_pair_apply4
]


@pytest.mark.parametrize("fused_bwd", [True, False], ids=["bwd_fused", "bwd_pair"])
@pytest.mark.parametrize("case", RES_TAIL_CASES, ids=lambda c: "%dx%dx%dx%d-%s" % c)
def test_res_tail_norm_vs_float64(case, fused_bwd, monkeypatch):
    """out = relu(relu(IN(x2)) + IN(xid)), pooled = maxpool2(out): both outputs and both input gradients.  fused_bwd=False takes
    vqw_res_tail_bwd, then vqw_inorm_bwd_pair (k_inorm_bwd_pair_reduce4)."""
    ops = _ops()
    monkeypatch.setattr(ops, "RES_TAIL_BWD_FUSED", fused_bwd)
    N, C, H, W, src = case
    g = torch.Generator().manual_seed(_seed(case))
    part2 = partid = None
    if src == "stats":
        x2, xid = _planes(g, N, C, H, W, "randn"), _planes(g, N, C, H, W, "randn")
    else:
        raws = []
        for _ in range(2):
            with torch.no_grad():
                raws.append(ops.conv2d(_gpu(torch.randn(N, 32, H, W, generator=g)), _gpu(torch.randn(C, 32, 3, 3, generator=g) * 0.1),
                                       _gpu(torch.randn(C, generator=g)), want_stats=True))
            assert raws[-1][1] is not None
        x2, xid = raws[0][0].cpu().double(), raws[1][0].cpu().double()
        part2 = raws[0][1]
        partid = raws[1][1] if src == "parts" else None
    rp = torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64)
    ro = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    x264, xid64 = _ref(x2), _ref(xid)
    za = F.instance_norm(x264, eps=1e-5)
    s64 = torch.relu(za) + F.instance_norm(xid64, eps=1e-5)
    out64 = torch.relu(s64)
    pooled64 = F.max_pool2d(out64, 2)
    ((pooled64 * rp).sum() + (out64 * ro).sum()).backward()
    keep = _band(za) * _band(s64) * _window_keep(out64)
    d2, did = _gpu(x2, grad=True), _gpu(xid, grad=True)
    pooled, out = ops.res_tail_norm(d2, did, eps=1e-5, part2=part2, partid=partid)
    ((pooled * _gpu(rp)).sum() + (out * _gpu(ro)).sum()).backward()
    torch.cuda.synchronize()
    tag = "res_tail_norm %dx%dx%dx%d %s fused_bwd=%d" % (N, C, H, W, src, fused_bwd)
    _check(tag, "pooled", pooled, pooled64, FWD_TOL)
    _check(tag, "out", out, out64, FWD_TOL)
    _check(tag, "dx2", d2.grad, x264.grad, GRAD_TOL, keep)
    _check(tag, "dxid", did.grad, xid64.grad, GRAD_TOL, keep)


# --------------------------------------------------------------------------------------------------
# spade_norm (StyledDenorm): BatchNorm2d(affine=False)(x) * (1 + gamma) + beta, ReLU, + residual
# --------------------------------------------------------------------------------------------------
SPADE_CASES = [
    # (N, C, H, W, [gamma|beta] fused, residual: None / "plain" / "norm" / "norm_part", relu, x from a conv with partials)
    (4, 32, 256, 256, True, None, True, False),           # FSpadeBwd4 in k_plane_reduce4p, k_spade_fwd4w<RES 0>, k_spade_bwd_apply4w; k_bn_finalize
    (4, 32, 256, 256, False, "plain", False, True),       # k_spade_fwd4w<RES 1>; statistics from the producing conv (k_channel_finalize<TileMoments, BN>)
    (4, 32, 256, 256, False, "norm_part", True, False),   # shortcut norm inside the kernel: k_spade_fwd4w<RES 2> with k_plane_finalize<TileMoments>
    (4, 32, 256, 256, True, "norm", False, True),         # RES 2 with the shortcut's statistics by vqw_inorm_stats (k_plane_reduce4p)
    (2, 32, 48, 64, False, "norm_part", True, False),     # H * W = 3072 not a power of two: residual_norm falls back to instance_norm(part) + RES 1
    (4, 48, 64, 64, False, "plain", True, True),          # C4 = 12: k_plane_reduce4, flat k_spade_fwd4 (with residual), k_spade_bwd_apply4
    (4, 48, 64, 64, True, "norm", False, False),          # C4 = 12 with residual_norm: fallback (not walk_ok)
    (2, 6, 40, 40, False, "plain", True, False),          # C = 6: generic k_plane_reduce, k_spade_fwd, k_spade_bwd_apply; residual by ops.add
    (2, 6, 40, 40, True, "norm", False, False),           # C = 6 with a 12-channel [gamma | beta] map, residual_norm fallback
]


def _conv_raw(ops, g, N, C, H, W):
    with torch.no_grad():
        y, part = ops.conv2d(_gpu(torch.randn(N, 16, H, W, generator=g)), _gpu(torch.randn(C, 16, 3, 3, generator=g) * 0.2),
                             _gpu(torch.randn(C, generator=g)), want_stats=True)
    return y, part


def _spade_id(c):
    return "%dx%dx%dx%d-%s-res_%s-relu%d-xpart%d" % (c[0], c[1], c[2], c[3], "fused" if c[4] else "sep", c[5], c[6], c[7])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", SPADE_CASES, ids=_spade_id)
def test_spade_norm_vs_float64(case, training):
    ops = _ops()
    N, C, H, W, fused, res, relu, xpart = case
    g = torch.Generator().manual_seed(_seed(case))
    momentum, eps = 0.1, 1e-5
    # inputs of the two calls (running statistics are checked after both)
    xs, parts = [], []
    for _ in range(2):
        if xpart:
            y_raw, part = _conv_raw(ops, g, N, C, H, W)
            assert part is not None
            xs.append(y_raw.cpu().double())
            parts.append(part)
        else:
            xs.append(_planes(g, N, C, H, W, "randn"))
            parts.append(None)
    gm = torch.randn(N, 2 * C if fused else C, H, W, generator=g, dtype=torch.float64) * 0.5
    bt = None if fused else torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 0.5
    rpart = None
    if res == "norm_part":
        r_raw, rpart = _conv_raw(ops, g, N, C, H, W)
        assert rpart is not None
        rs = r_raw.cpu().double()
    elif res is not None:
        rs = _planes(g, N, C, H, W, "randn")
    rrelu = res in ("norm", "norm_part") and relu
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    rm0 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).float()
    rv0 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float()

    # float64 reference
    rm64, rv64 = rm0.double(), rv0.double()
    x64, gm64 = _ref(xs[0]), _ref(gm)
    bt64 = _ref(bt) if bt is not None else None
    res64 = _ref(rs) if res is not None else None
    gam, bet = (gm64[:, :C], gm64[:, C:]) if fused else (gm64, bt64)
    s64 = F.batch_norm(x64, rm64, rv64, training=training, momentum=momentum, eps=eps) * (1 + gam) + bet
    y64 = torch.relu(s64) if relu else s64
    if res in ("norm", "norm_part"):
        zr = F.instance_norm(res64, eps=eps)
        y64 = y64 + (torch.relu(zr) if rrelu else zr)
    elif res == "plain":
        y64 = y64 + res64
    (y64 * r).sum().backward()
    if training:
        F.batch_norm(xs[1], rm64, rv64, training=True, momentum=momentum, eps=eps)

    # HIP
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.full((), 5, dtype=torch.long, device=DEV)
    dx, dgm = _gpu(xs[0], grad=True), _gpu(gm, grad=True)
    dbt = _gpu(bt, grad=True) if bt is not None else None
    dres = _gpu(rs, grad=True) if res is not None else None
    rnorm = (rpart, rrelu, eps) if res in ("norm", "norm_part") else None
    y = ops.spade_norm(dx, dgm, dbt, rm, rv, training, momentum, eps, relu=relu, num_batches_tracked=nbt, residual=dres,
                       part=parts[0], residual_norm=rnorm)
    (y * _gpu(r)).sum().backward()
    if training:
        with torch.no_grad():
            ops.spade_norm(_gpu(xs[1]), _gpu(gm), _gpu(bt) if bt is not None else None, rm, rv, True, momentum, eps, relu=relu,
                           num_batches_tracked=nbt, part=parts[1])
    torch.cuda.synchronize()
    ops.flush_counters()

    tag = "spade_norm %s %s" % (_spade_id(case), "train" if training else "eval")
    keep = _band(s64) if relu else None
    _check(tag, "y", y, y64, FWD_TOL)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL, keep)
    _check(tag, "dgamma", dgm.grad, gm64.grad, PARAM_TOL, keep if not fused else
           (torch.cat([keep, keep], 1) if keep is not None else None))
    if bt is not None:
        _check(tag, "dbeta", dbt.grad, bt64.grad, PARAM_TOL, keep)
    if res is not None:
        _check(tag, "dresidual", dres.grad, res64.grad, GRAD_TOL, _band(zr) if rrelu else None)
    _check_running(tag, rm, rv, rm64, rv64, rm0, rv0, training)
    assert int(nbt) == (7 if training else 5), "num_batches_tracked %d after %s" % (int(nbt), "two training calls" if training else "eval")


def _check_running(tag, rm, rv, rm64, rv64, rm0, rv0, training):
    if not training:      # untouched, bit for bit
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), "%s: running stats changed in eval" % tag
        return
    for name, got, ref in (("running_mean", rm, rm64), ("running_var", rv, rv64)):
        d = ((got.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max()      # relative, absolute below 1
        print("  %-48s %-12s max %.2e  (bound %.2e)" % (tag, name, float(d), STAT_TOL))
        assert float(d) <= STAT_TOL, "%s: %s max elementwise error %.3e" % (tag, name, float(d))


# --------------------------------------------------------------------------------------------------
# batch_norm_lrelu (the discriminator): LeakyReLU(BatchNorm2d(affine)(x))
# --------------------------------------------------------------------------------------------------
BN_CASES = [
    # (N, C, H, W, slope, data)
    (8, 128, 31, 31, 0.2, "randn"),   # statistics by k_plane_reduce4p (C4 = 32), k_bn_affine_fwd, backward sums by generic k_plane_reduce
    (8, 256, 30, 30, 0.2, "randn"),   # C4 = 64
    (8, 512, 15, 15, 0.2, "randn"),   # C = 512 > 256: k_plane_reduce's channel loop in the backward sums; C4 = 128 in the pipelined statistics
    (8, 64, 30, 30, 1.0, "randn"),    # slope 1: plain BatchNorm
    (8, 3, 31, 31, 0.2, "randn"),     # C = 3: generic k_plane_reduce for the statistics too
    (4, 8, 16, 16, 0.2, "edge"),      # a constant and a zero channel (var = 0): k_bn_finalize's variance and the unbiased running var
]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%dx%dx%dx%d-slope%g-%s" % c)
def test_batch_norm_lrelu_vs_float64(case, training):
    ops = _ops()
    N, C, H, W, slope, kind = case
    g = torch.Generator().manual_seed(_seed(case))
    momentum, eps = 0.1, 1e-5
    xs = [_planes(g, N, C, H, W, kind) for _ in range(2)]
    sign = torch.tensor([(-1.0) ** c for c in range(C)], dtype=torch.float64)
    gamma = (0.2 + torch.randn(C, generator=g, dtype=torch.float64).abs()) * sign     # every other entry negative
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    rm0 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).float()
    rv0 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float()
    assert (gamma < 0).any() and (gamma > 0).any()

    rm64, rv64 = rm0.double(), rv0.double()
    x64, ga64, be64 = _ref(xs[0]), _ref(gamma), _ref(beta)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.full((), 5, dtype=torch.long, device=DEV)
    dx, dga, dbe = _gpu(xs[0], grad=True), _gpu(gamma, grad=True), _gpu(beta, grad=True)
    y = ops.batch_norm_lrelu(dx, dga, dbe, rm, rv, training, momentum, eps, slope=slope, num_batches_tracked=nbt)
    (y * _gpu(r)).sum().backward()

    z64 = F.batch_norm(x64, rm64, rv64, weight=ga64, bias=be64, training=training, momentum=momentum, eps=eps)
    pos = z64.detach() > 0
    amb = z64.detach().abs() < MASK_BAND
    assert float(amb.double().mean()) <= MASK_FRACTION
    pos = torch.where(amb, y.detach().cpu() > 0, pos)        # inside the band: the kernel's own branch
    y64 = z64 * torch.where(pos, 1.0, slope).double()        # = F.leaky_relu(z64, slope) outside the band
    assert rel_err(y64, F.leaky_relu(z64, slope)) < 1e-6
    (y64 * r).sum().backward()
    if training:
        F.batch_norm(xs[1], rm64, rv64, weight=gamma, bias=beta, training=True, momentum=momentum, eps=eps)
    if training:
        with torch.no_grad():
            ops.batch_norm_lrelu(_gpu(xs[1]), _gpu(gamma), _gpu(beta), rm, rv, True, momentum, eps, slope=slope, num_batches_tracked=nbt)
    torch.cuda.synchronize()
    ops.flush_counters()

    tag = "batch_norm_lrelu %dx%dx%dx%d slope=%g %s" % (N, C, H, W, slope, "train" if training else "eval")
    _check(tag, "y", y, F.leaky_relu(z64, slope), FWD_TOL)
    _check(tag, "dx", dx.grad, x64.grad, GRAD_TOL)
    _check(tag, "dgamma", dga.grad, ga64.grad, PARAM_TOL)
    _check(tag, "dbeta", dbe.grad, be64.grad, PARAM_TOL)
    _check_running(tag, rm, rv, rm64, rv64, rm0, rv0, training)
    assert int(nbt) == (7 if training else 5), "num_batches_tracked %d after %s" % (int(nbt), "two training calls" if training else "eval")
