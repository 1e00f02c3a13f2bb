"""k_conv_wino64 with the weight (U) chunks loaded straight into LDS, against a float64 convolution.

The kernel's U loader issues one direct global -> LDS load per slot: the wave's 1 KB piece of a U buffer is lane-linear, the swap
of a row's two float4 halves (couts 8..15 of an N block) sits in the per-lane SOURCE address, the prologue loads chunk 0 and every
item loads the chunk of the next one into the other buffer.  What can go wrong is an address (cout tile base, slot and chunk
strides, the half swap), a missing wait or barrier between the load and the B-fragment reads, and the aliasing of U buffer 1 with
the region epilogue's exchange area.  The cases are the smallest shapes that reach each of those, all through the C ABI, all
with N = 2:

  Cin = 16 ......... two chunks: the prologue's chunk 0 and exactly one in-loop load per region
  Cin = 48 ......... six chunks
  Cout = 128 ....... two cout tiles: co_base != 0 in the source address, the half swap on a tile that is not the first
  24 x 64 .......... six regions per image on the 64-cout form
  16 x 16 .......... the 16-wide region geometry
  32 -> 32 ......... the four-wave 32-cout form at 16 x 32 (with statistics) and 20 x 32 (ragged last region row, without)
  520 x 32, 16 -> 128 ... 65 regions per image and 128 runs of the 130 regions on a 256-CU device: runs of two regions, one of
                      which crosses the image boundary (the smaller shapes run one region per workgroup there)
  every epilogue once at 16 -> 64, 16 x 32: plain (bias + ReLU), masked, accumulating, norm-sums, two tensors (pooled and
  not), and the dilation-2 entry on 32 x 32 phase images (32 -> 32 at 64 x 64).

Bound: the project's single-kernel bound, |got - ref|_2 <= 2e-5 |ref|_2 against F.conv2d in float64 on the float32 inputs.
Derived outputs: the accumulating form adds one fp32 rounding of (preset + result), 2^-23 |preset + result|_2; a sum of n outputs
is held to 2e-5 of the sum of their magnitudes; M2 = sum (y - mean)^2 is quadratic in y, so an error of eps in y is 2 eps in M2:
4e-5.  Every test prints what it measured ("UDMA <case> | <tensor> <error>"; run with -s).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
EPS32 = 2.0 ** -23


def _L():
    from hipops import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(N, H, W, Cin, Cout, dil=1, seed=0):
    """Inputs (float32, NHWC / OHWI, on the CPU) and the float64 convolution without bias, NHWC."""
    g = torch.Generator().manual_seed(1000 * Cin + Cout + H + seed)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * (1.0 / (3.0 * Cin ** 0.5))
    b = torch.randn(Cout, generator=g)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=dil, dilation=dil).permute(0, 2, 3, 1).contiguous()
    return x, w, b, y


def _u(w, Cin, Cout):
    lib, L = _L()
    wd = w.to(DEV).contiguous()
    ws = torch.empty(L.vqw_conv3x3_wino_ws_bytes(Cin, Cout), dtype=torch.uint8, device=DEV)
    lib.check(L.vqw_conv3x3_wino_prepare(_p(wd), _p(ws), ws.numel(), Cin, Cout, _st()), "prepare")
    return ws


def _report(case, what, got, want, scale=None, tol=TOL, extra=0.0):
    got = got.detach().double().cpu().reshape(-1)
    want = want.double().reshape(-1)
    assert got.numel() == want.numel(), "%s %s: %d vs %d elements" % (case, what, got.numel(), want.numel())
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite values" % (case, what)
    sn = float((want if scale is None else scale.double().reshape(-1)).norm())
    d = float((got - want).norm())
    print("UDMA %s | %s %.3e" % (case, what, d / (sn + 1e-30)))
    assert d <= tol * sn + extra, "%s, %s: |diff| %.3e > %.3e (%.3e relative)" % (case, what, d, tol * sn + extra, d / (sn + 1e-30))


def _plain(N, H, W, Cin, Cout, bias, relu):
    lib, L = _L()
    assert L.vqw_conv3x3_wino_supported(Cin, Cout, N, H, W) == 1 and L.vqw_conv3x3_wino_masked_supported(Cin, Cout, N, H, W) == 1, \
        "the shape must be served by k_conv_wino64"
    x, w, b, yref = _case(N, H, W, Cin, Cout)
    u = _u(w, Cin, Cout)
    y = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    xd, bd = x.to(DEV), (b.to(DEV) if bias else None)
    lib.check(L.vqw_conv3x3_wino_fwd(_p(xd), _p(u), _p(bd), _p(y), N, H, W, Cin, Cout, int(relu), _st()), "wino_fwd")
    torch.cuda.synchronize()
    ref = yref + b.double() if bias else yref
    return y, (ref.clamp_min(0) if relu else ref)


# (name, N, H, W, Cin, Cout, bias, relu)
SHAPES = [
    ("cin16 16->64 @8x32", 2, 8, 32, 16, 64, False, False),
    ("cin48 48->64 @8x32", 2, 8, 32, 48, 64, True, False),
    ("cout128 16->128 @8x32", 2, 8, 32, 16, 128, False, False),
    ("six-regions 16->64 @24x64", 2, 24, 64, 16, 64, False, False),
    ("rw16 32->64 @16x16", 2, 16, 16, 32, 64, True, True),
    ("four-wave ragged 32->32 @20x32", 2, 20, 32, 32, 32, False, False),
    ("runs-of-two 16->128 @520x32", 2, 520, 32, 16, 128, False, False),
]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0].split()[0] for c in SHAPES])
def test_wino64_direct_u_shapes(case):
    name, N, H, W, Cin, Cout, bias, relu = case
    y, ref = _plain(N, H, W, Cin, Cout, bias, relu)
    _report(name, "y", y, ref)


def _region_stats(y, TR, RW):
    """(sum, M2 about the region mean, sum of magnitudes) per (image, region, channel), regions ordered (column, row)."""
    N, H, W, C = y.shape
    r = y.reshape(N, H // TR, TR, W // RW, RW, C).permute(0, 3, 1, 2, 4, 5).reshape(N, (W // RW) * (H // TR), TR * RW, C)
    s = r.sum(2)
    m2 = ((r - r.mean(2, keepdim=True)) ** 2).sum(2)
    return s, m2, r.abs().sum(2)


def test_wino64_direct_u_four_wave_with_statistics():
    """32 -> 32 at 16 x 32: two regions of 8 x 32 pixels per image on the four-wave form, bias, statistics partials."""
    lib, L = _L()
    N, H, W, Cin, Cout = 2, 16, 32, 32, 32
    x, w, b, yref = _case(N, H, W, Cin, Cout)
    parts = L.vqw_conv3x3_wino_fwd_stats_parts(Cin, Cout, N, H, W)
    assert parts == 2
    u = _u(w, Cin, Cout)
    y = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    part = torch.full((N, parts, Cout, 2), float("nan"), device=DEV)
    xd, bd = x.to(DEV), b.to(DEV)
    lib.check(L.vqw_conv3x3_wino_fwd_stats(_p(xd), _p(u), _p(bd), _p(y), _p(part), N, H, W, Cin, Cout, _st()), "wino_fwd_stats")
    torch.cuda.synchronize()
    ref = yref + b.double()
    _report("four-wave 32->32 @16x32", "y", y, ref)
    s, m2, sa = _region_stats(ref, 8, 32)
    _report("four-wave 32->32 @16x32", "region sums", part[..., 0], s, scale=sa)
    _report("four-wave 32->32 @16x32", "region M2", part[..., 1], m2, tol=2 * TOL)


EPI = (2, 16, 32, 16, 64)       # N, H, W, Cin, Cout of the epilogue variants: two regions of 8 x 32 pixels per image


def test_wino64_direct_u_epilogue_plain_bias_relu():
    y, ref = _plain(*EPI, True, True)
    _report("epi plain", "y", y, ref)


def test_wino64_direct_u_epilogue_masked():
    lib, L = _L()
    N, H, W, Cin, Cout = EPI
    x, w, _, yref = _case(*EPI)
    mask = torch.randn(N, H, W, Cout, generator=torch.Generator().manual_seed(5)).clamp_min(0)     # a ReLU's output: half zeros
    y = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    xd, u, md = x.to(DEV), _u(w, Cin, Cout), mask.to(DEV)
    lib.check(L.vqw_conv3x3_wino_fwd_masked(_p(xd), _p(u), _p(md), _p(y), N, H, W, Cin, Cout, _st()), "masked")
    torch.cuda.synchronize()
    _report("epi masked", "y", y, torch.where(mask.double() > 0, yref, torch.zeros_like(yref)))


def test_wino64_direct_u_epilogue_accumulating():
    lib, L = _L()
    N, H, W, Cin, Cout = EPI
    x, w, _, yref = _case(*EPI)
    y0 = torch.randn(N, H, W, Cout, generator=torch.Generator().manual_seed(6)) * float(yref.std())
    y = y0.to(DEV).clone()
    xd, u = x.to(DEV), _u(w, Cin, Cout)
    lib.check(L.vqw_conv3x3_wino_fwd_acc(_p(xd), _p(u), _p(y), N, H, W, Cin, Cout, _st()), "acc")
    torch.cuda.synchronize()
    want = y0.double() + yref
    _report("epi acc", "y", y, want, scale=yref, extra=EPS32 * float(want.norm()))


def test_wino64_direct_u_epilogue_norm_sums():
    lib, L = _L()
    N, H, W, Cin, Cout = EPI
    x, w, _, yref = _case(*EPI)
    parts = L.vqw_conv3x3_wino_fwd_inbwd_parts(Cin, Cout, N, H, W)
    assert parts == 2
    g = torch.Generator().manual_seed(7)
    nx = torch.randn(N, H, W, Cout, generator=g) * 1.5 + 0.3
    mr = torch.stack([nx.mean((1, 2)), 1.0 / (nx.var((1, 2), unbiased=False) + 1e-5).sqrt()], -1).contiguous()     # [N][Cout][2]
    y = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    part = torch.full((N, parts, Cout, 2), float("nan"), device=DEV)
    xd, u, nxd, mrd = x.to(DEV), _u(w, Cin, Cout), nx.to(DEV), mr.to(DEV)
    lib.check(L.vqw_conv3x3_wino_fwd_inbwd(_p(xd), _p(u), _p(nxd), _p(mrd), 1, _p(y), _p(part), N, H, W, Cin, Cout, _st()), "inbwd")
    torch.cuda.synchronize()
    _report("epi inbwd", "y", y, yref)
    xh = (nx.double() - mr[:, None, None, :, 0].double()) * mr[:, None, None, :, 1].double()
    gm = torch.where(xh > 0, yref, torch.zeros_like(yref))
    s1, _, a1 = _region_stats(gm, 8, 32)
    s2, _, a2 = _region_stats(gm * xh, 8, 32)
    _report("epi inbwd", "sum gm", part[..., 0], s1, scale=a1)
    _report("epi inbwd", "sum gm xhat", part[..., 1], s2, scale=a2)


@pytest.mark.parametrize("pool0", [0, 1], ids=["full", "pooled"])
def test_wino64_direct_u_epilogue_two_tensors(pool0):
    lib, L = _L()
    N, H, W, Cin, Cout = EPI
    split = 32
    assert L.vqw_conv3x3_wino_split_supported(Cin, Cout, split, pool0, N, H, W) == 1
    x, w, b, yref = _case(*EPI)
    bias, relu = (None, 0) if pool0 else (b, 1)
    ya = torch.full((N, H >> pool0, W >> pool0, split), float("nan"), device=DEV)
    yb = torch.full((N, H, W, Cout - split), float("nan"), device=DEV)
    xd, u, bd = x.to(DEV), _u(w, Cin, Cout), (bias.to(DEV) if bias is not None else None)
    lib.check(L.vqw_conv3x3_wino_fwd_split(_p(xd), _p(u), _p(bd), _p(ya), _p(yb), N, H, W, Cin, Cout, split, pool0, relu, _st()), "split")
    torch.cuda.synchronize()
    ref = (yref + b.double()).clamp_min(0) if relu else yref
    ra, rb = ref[..., :split], ref[..., split:]
    if pool0:
        scale = ra.abs().reshape(N, H // 2, 2, W // 2, 2, split).sum((2, 4))
        ra = ra.reshape(N, H // 2, 2, W // 2, 2, split).sum((2, 4))
        _report("epi split pooled", "y0", ya, ra, scale=scale)
    else:
        _report("epi split", "y0", ya, ra)
    _report("epi split" + (" pooled" if pool0 else ""), "y1", yb, rb)


def test_wino64_direct_u_dilation2_entry():
    """32 -> 32 at 64 x 64, dilation 2: the four-wave form on four 32 x 32 phase images per image."""
    lib, L = _L()
    N, H, W, Cin, Cout = 2, 64, 64, 32, 32
    assert L.vqw_conv3x3_wino_dil2_supported(Cin, Cout, N, H, W) == 1
    x, w, b, yref = _case(N, H, W, Cin, Cout, dil=2)
    y = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    xd, u, bd = x.to(DEV), _u(w, Cin, Cout), b.to(DEV)
    lib.check(L.vqw_conv3x3_wino_dil2_fwd(_p(xd), _p(u), _p(bd), _p(y), None, 0, N, H, W, Cin, Cout, 0, _st()), "dil2")
    torch.cuda.synchronize()
    _report("dil2 32->32 @64x64", "y", y, yref + b.double())
