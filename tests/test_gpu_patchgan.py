"""The PatchGAN path of the second training step against float64 on every dispatch route: the strided convolutions of
csrc/gan.hip with the conv_k4s2_* / conv_k4s1_* entry points of csrc/conv_mfma.hip behind them, vqw_leaky_relu_bwd, the hinge /
generator losses, the ActNorm operator (vqw_actnorm_stats, vqw_actnorm_prepare, vqw_actnorm_loc_grad and the eval form of vqw_bn_affine_*), and the
default-width NLayerDiscriminator(1, 1, 64, 3) once.  Run with `pytest -m gpu tests/test_gpu_patchgan.py -s` on an MI355X; -s
shows the measured error of every comparison.  The module imports without a GPU: tests/test_patchgan_cases_host.py checks the
case table (routes, geometry, mask bands, planted values) on the CPU.

Every case draws fp32 inputs from a seeded generator on the CPU, runs the HIP path through hipops.ops (the C ABI directly only
for the misaligned-pointer rows, which ops cannot reach: it allocates its own outputs) and evaluates plain ATen in float64 on
the same fp32 values cast to double: F.conv2d(..., stride, padding), F.leaky_relu, relu, mean.  Reference gradients come from
float64 autograd against a fixed random cotangent.  Errors are relative L2 (helpers.rel_err); every comparison prints its own.

Routes.  `routes(case)` restates the host predicates of gan.hip / conv_mfma.hip; each row names what it is there for and the
host test holds the names to the predicates and the predicates to the library's size queries:
  Ho = (H + 2 pad - ks) / stride + 1, Po = N Ho Wo
  mfma  = ks == 4, pad == 1, Cin % 4 == Cout % 4 == 0, Cin >= 8, Cout >= 8 and (stride 1: H >= 4 and W >= 4; stride 2: H, W even)
  forward ........ slope == 1 and mfma: conv_k4s2_fwd (stride 2) or conv_k4s1_grid + crop (stride 1, "grid"); else ks == 4,
                   Cin == 1, Cout % 4 == 0, Cout <= 1024: k_sconv_fwd_c1 (Cout * 64 bytes of dynamic LDS); else ks == 4, Cout == 1,
                   Cin % 4 == 0: k_sconv_fwd_o1 (a wave per pixel, lanes 4 channels each, `c += 256` trips); else k_sconv_fwd
                   (float4 when Cin % 4 == 0 and x, w are 16-byte aligned, else scalar)
  input gradient . mfma: conv_k4s2_dgrad or pad + conv_k4s1_grid (whatever the slope: the mask is applied in front by
                   vqw_leaky_relu_bwd); else the c1 / o1 / generic kernels by the same conditions
  weight gradient  mfma and (stride 1 or (W / 2) % 16 == 0): conv_k4s1_wgrad_grid with the tile pair (wg_tile(Cout), wg_tile(Cin)),
                   wg_tile(c) = 32 / 64 / 128 for c <= 32 / <= 64 / above, or conv_k4s2_wgrad; else Cin == 1, ks == 4, Cout <= 256 and
                   256 % Cout == 0: k_sconv_wgrad_c1 at min(max(Po / 1024, 1), 1024) pixel splits; else k_sconv_wgrad at
                   min(max(Po / 512, 1), 256) splits with cl = 256 / 64 / 16 / 4 / 1 lanes over Cin (the first tier <= Cin), the
                   last channel trip ragged when Cin % cl != 0; a split holds ceil(Po / splits) pixels, the last one fewer
  stream_grid caps a launch at 2048 * 256 threads and grid-strides the rest ("wraps"): k_sconv_fwd_o1 above 8192 output pixels,
  k_sconv_dgrad_o1 above 524288 * 4 input elements, k_sconv_fwd_c1 above 524288 * 4 outputs, k_sconv_dgrad_c1 above 524288 input
  pixels, k_hinge_bwd / k_leaky_bwd above 524288 elements.
What the size queries tell: vqw_sconv_fwd_ws_bytes > 0 is the stride-1 grid form of an mfma shape (it does not see the slope: at
slope != 1 the forward still takes a direct kernel); vqw_sconv_dgrad_ws_bytes > 0 is either MFMA form; vqw_sconv_wgrad_ws_bytes
minus the bias rows equals splits * Cout * ks^2 * Cin floats for k_sconv_wgrad and splits * Cout * 16 for k_sconv_wgrad_c1.  They
cannot tell c1 / o1 / generic apart in the forward and the input gradient, nor the tile pair or the lane tier: those rows rest
on the predicates above and on their result.

LeakyReLU rows (slope 0.2).  The mask is a discontinuity: where the float64 pre-activation z lies within MASK_BAND standard
deviations of 0 the fp32 kernel may take the other side.  At most MASK_FRACTION of a row's outputs may lie there (asserted; the
host test checks it for the seeds in use).  The forward output is compared everywhere.  dw and db are sums over pixels and dx
over the taps and output channels that touch an input element, so none of them can leave single outputs out: inside the band
the reference takes the kernel's own branch (the sign of its output), as batch_norm_lrelu's does in test_gpu_norms.py.
vqw_leaky_relu_bwd on its own is elementwise and compared exactly on the y it is given.

Bounds.  Convolution rows: 2e-5 relative L2 for y, dx, dw, db, the single-kernel bound of test_conv2d / test_sconv2d.  Hinge /
generator losses 1e-6 relative (test_gan_losses_golden's), their gradients 1e-6 of each element.  ActNorm: forward, written
loc / scale 2e-5, input gradient 5e-5, parameter gradients 2e-5 (test_gpu_norms.py's), plus 2^-23 |mean| / std for the channel
far from zero on the quantities that hold x + loc.  The default-width module: 1e-4 forward, 1e-3 gradients, 1e-5 state
(_run_block's).  The long reductions (512 -> 1: 8192 products per output; 256 -> 512: 4096; the 2 x 66 x 66 weight gradient:
8450 pixels per entry) stay a factor ten inside 2e-5: no row takes the wider bound of twice torch's own fp32 error.  For
comparison, torch's fp32 CPU convolution on the rows of this table is at most 2.4e-6 from the same float64 reference (the
9 x 256 x 256 weight gradient), 1.5e-6 on 512 -> 1 and 1.1e-6 on 256 -> 512.

Measured on an MI355X (largest error per group; bound in brackets):
  convolution rows .......... y 1.4e-6, dx 1.4e-6, dw 4.2e-7, db 4.2e-7 [2e-5]; at most 1.2e-4 of a slope row's outputs in the band [1e-3]
  misaligned pointers ....... y 2.1e-7, dx 8.2e-8, dw 1.5e-7, db 7.5e-8 [2e-5]
  hinge / generator loss .... loss 4.2e-8 [1e-6], gradient elements 4.8e-9 [1e-6]; vqw_leaky_relu_bwd elements 7.1e-8 [1e-6]
  act_norm_lrelu ............ y 7.4e-8 [2e-5], dx 5.4e-8 [5e-5], dloc 7.0e-8, dscale 6.9e-8 [2e-5], written loc 3.5e-8, scale 4.7e-8 [2e-5]
    channel 1e3 std off zero  y 1.2e-5 [2e-5 + 1.2e-4], scale 4.0e-8 [2e-5]; constant channel: scale 1e6 exactly
  default-width module ...... out 2.1e-6 [1e-4], input gradient 1.8e-6, parameter gradients 2.5e-6 [1e-3], state 3.7e-7 [1e-5]
  The Cout = 1024 launch of k_sconv_fwd_c1 / k_sconv_dgrad_c1 (64 KiB of dynamic LDS) is accepted as it is.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

KERNEL_TOL = 2e-5       # y, dx, dw, db of one convolution
LOSS_TOL = 1e-6         # hinge / generator loss, and each element of their gradients
FWD_TOL = 2e-5          # ActNorm forward, written loc / scale
GRAD_TOL = 5e-5         # ActNorm input gradient
PARAM_TOL = 2e-5        # ActNorm loc / scale gradients
MASK_BAND = 1e-4        # |float64 pre-activation| / its standard deviation below which the mask may flip in fp32
MASK_FRACTION = 1e-3    # at most this share of a row's outputs may fall in that band
GRID_THREADS = 2048 * 256


def _ops():
    from hipops import ops
    return ops


def _seed(case):
    return zlib.crc32(repr(case).encode())


def _check(tag, what, got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    print("  %-58s %-8s rel %.2e  (bound %.1e)" % (tag, what, rel_err(got, ref), tol))
    assert_close(got, ref, tol, "%s: %s" % (tag, what))


# --------------------------------------------------------------------------------------------------
# a. the strided convolution: one case table, routes restated from the host predicates
# --------------------------------------------------------------------------------------------------
def out_dim(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


def legal(case):
    """check_sconv of gan.hip."""
    N, H, W, Cin, Cout, ks, stride, pad = case[:8]
    return (N > 0 and H > 0 and W > 0 and Cin > 0 and Cout > 0 and 1 <= ks <= 7 and stride in (1, 2) and 0 <= pad < ks
            and H + 2 * pad >= ks and W + 2 * pad >= ks)


def wg_tile(c):
    return 128 if c > 64 else (64 if c > 32 else 32)


def routes(case):
    """The kernels a row reaches and the launch facts that decide what they do (see the header)."""
    N, H, W, Cin, Cout, ks, stride, pad, _, slope = case[:10]
    Ho, Wo = out_dim(H, ks, stride, pad), out_dim(W, ks, stride, pad)
    Po = N * Ho * Wo
    mfma = (ks == 4 and pad == 1 and Cin % 4 == 0 and Cout % 4 == 0 and Cin >= 8 and Cout >= 8
            and ((H >= 4 and W >= 4) if stride == 1 else (H % 2 == 0 and W % 2 == 0)))
    c1 = ks == 4 and Cin == 1 and Cout % 4 == 0 and Cout <= 1024
    o1 = ks == 4 and Cout == 1 and Cin % 4 == 0
    direct = "c1" if c1 else ("o1" if o1 else "generic")
    form = "mfma_s%d" % stride
    r = dict(Ho=Ho, Wo=Wo, Po=Po, mfma=mfma, fwd=form if (mfma and slope == 1.0) else direct, dgrad=form if mfma else direct)
    r["fwd_wrap"] = {"c1": Po * Cout // 4, "o1": Po * 64, "generic": Po * Cout}.get(r["fwd"], 0) > GRID_THREADS
    r["dgrad_wrap"] = {"c1": N * H * W, "o1": N * H * W * Cin // 4, "generic": N * H * W * Cin}.get(r["dgrad"], 0) > GRID_THREADS
    if mfma and (stride == 1 or (W // 2) % 16 == 0):
        r.update(wgrad=form, tiles=(wg_tile(Cout), wg_tile(Cin)) if stride == 1 else None)
    elif Cin == 1 and ks == 4 and Cout <= 256 and 256 % Cout == 0:
        ns = min(max(Po // 1024, 1), 1024)
        r.update(wgrad="c1", splits=ns, ws_floats=ns * Cout * 16)
    else:
        ns = min(max(Po // 512, 1), 256)
        r.update(wgrad="generic", splits=ns, ws_floats=ns * Cout * ks * ks * Cin,
                 cl=256 if Cin >= 256 else (64 if Cin >= 64 else (16 if Cin >= 16 else (4 if Cin >= 4 else 1))))
    if "splits" in r:
        r["ragged_split"] = r["splits"] > 1 and -(-Po // r["splits"]) * r["splits"] > Po
    return r


def _tile(m, n):
    return lambda c, r: r["wgrad"] == "mfma_s1" and r["tiles"] == (m, n)


def _wg(cl, ragged):
    return lambda c, r: r["wgrad"] == "generic" and r["cl"] == cl and (c[3] % cl != 0) == ragged


# every route of the list this file was written against: name -> what must hold for a row that claims it
ROUTES = {
    # Cout = 1
    "o1_two_trips": lambda c, r: r["fwd"] == "o1" and c[3] == 512,
    "o1_ragged_trip": lambda c, r: r["fwd"] == "o1" and c[3] > 256 and c[3] % 256 != 0,
    "o1_fwd_wrap": lambda c, r: r["fwd"] == "o1" and r["fwd_wrap"],
    "o1_dgrad": lambda c, r: r["dgrad"] == "o1",
    "o1_dgrad_wrap": lambda c, r: r["dgrad"] == "o1" and r["dgrad_wrap"],
    # Cin = 1
    "c1_cout64": lambda c, r: r["fwd"] == r["dgrad"] == r["wgrad"] == "c1" and c[4] == 64,
    "c1_cout1024": lambda c, r: r["fwd"] == r["dgrad"] == "c1" and c[4] == 1024,
    "c1_cout512_wgrad_generic": lambda c, r: r["fwd"] == "c1" and c[4] == 512 and r["wgrad"] == "generic" and r["cl"] == 1,
    "c1_cout48_wgrad_generic": lambda c, r: r["fwd"] == "c1" and c[4] == 48 and r["wgrad"] == "generic" and r["cl"] == 1,
    "c1_wgrad_splits": lambda c, r: r["wgrad"] == "c1" and r["splits"] > 1,
    "c1_wgrad_ragged_split": lambda c, r: r["wgrad"] == "c1" and r["ragged_split"],
    "c1_fwd_wrap": lambda c, r: r["fwd"] == "c1" and r["fwd_wrap"],
    "c1_dgrad_wrap": lambda c, r: r["dgrad"] == "c1" and r["dgrad_wrap"],
    "c1_stride1": lambda c, r: r["fwd"] == r["dgrad"] == "c1" and c[6] == 1,
    # generic weight gradient
    "wg_cl64": _wg(64, False), "wg_cl256": _wg(256, False),
    "wg_cl4_ragged": _wg(4, True), "wg_cl16_ragged": _wg(16, True), "wg_cl64_ragged": _wg(64, True), "wg_cl256_ragged": _wg(256, True),
    "wg_splits": lambda c, r: r["wgrad"] == "generic" and r["splits"] > 1,
    "wg_ragged_split": lambda c, r: r["wgrad"] == "generic" and r["ragged_split"],
    # stride-1 MFMA grid form
    "s1_tile_32x32": _tile(32, 32), "s1_tile_32x64": _tile(32, 64), "s1_tile_64x32": _tile(64, 32), "s1_tile_64x64": _tile(64, 64),
    "s1_tile_32x128": _tile(32, 128), "s1_tile_128x32": _tile(128, 32), "s1_tile_64x128": _tile(64, 128),
    "s1_tile_128x64": _tile(128, 64), "s1_tile_128x128": _tile(128, 128),
    "s1_256_512": lambda c, r: r["fwd"] == r["dgrad"] == r["wgrad"] == "mfma_s1" and c[3:5] == (256, 512),
    "s1_unfilled_36": lambda c, r: r["wgrad"] == "mfma_s1" and 36 in c[3:5],
    "s1_unfilled_68": lambda c, r: r["wgrad"] == "mfma_s1" and 68 in c[3:5],
    "s1_unfilled_100": lambda c, r: r["wgrad"] == "mfma_s1" and 100 in c[3:5],
    "s1_h4_mfma": lambda c, r: r["fwd"] == "mfma_s1" and min(c[1], c[2]) == 4 and c[3] >= 256,
    "s1_h3_direct_wide": lambda c, r: c[5:8] == (4, 1, 1) and c[1] == 3 and c[3] >= 256 and not r["mfma"],
    # stride-2 MFMA form
    "s2_single_row": lambda c, r: r["fwd"] == r["dgrad"] == r["wgrad"] == "mfma_s2" and c[1] == 2,
    "s2_h_ne_w": lambda c, r: r["fwd"] == r["dgrad"] == r["wgrad"] == "mfma_s2" and c[1] != c[2],
    "s2_wgrad_fallback_wide": lambda c, r: r["fwd"] == "mfma_s2" and r["wgrad"] == "generic" and r["cl"] == 64 and c[2] // 2 == 8,
    "s2_odd_generic_wide": lambda c, r: c[3:8] == (64, 128, 4, 2, 1) and r["fwd"] == r["dgrad"] == r["wgrad"] == "generic",
    # generic kernels, other kernel sizes and paddings
    "ks1": lambda c, r: c[5] == 1, "ks2": lambda c, r: c[5] == 2, "ks5": lambda c, r: c[5] == 5, "ks6": lambda c, r: c[5] == 6,
    "ks7": lambda c, r: c[5] == 7,
    "pad0": lambda c, r: c[7] == 0 and c[5] > 1,
    "pad_max": lambda c, r: c[7] == c[5] - 1 and c[5] > 2,
    "one_pixel": lambda c, r: c[1] + 2 * c[7] == c[5] and c[2] + 2 * c[7] == c[5] and r["Ho"] == r["Wo"] == 1,
    # LeakyReLU epilogue
    "slope": lambda c, r: c[9] == 0.2,
    "slope_mfma_bwd": lambda c, r: c[9] == 0.2 and r["mfma"] and r["fwd"] == "generic" and r["dgrad"].startswith("mfma"),
}

ROUTE_CASES = [
    # (N, H, W, Cin, Cout, ks, stride, pad, bias, slope, routes claimed)    forward / input gradient / weight gradient
    # ---- Cout = 1 (512 -> 1 is the discriminator's last layer)
    (2, 9, 9, 512, 1, 4, 1, 1, True, 1.0, "o1_two_trips o1_dgrad wg_cl256"),           # k_sconv_fwd_o1, two full trips of the lane loop / k_sconv_dgrad_o1 / k_sconv_wgrad cl 256, two channel trips, one split
    (2, 3, 3, 512, 1, 4, 1, 1, True, 1.0, "o1_two_trips s1_h3_direct_wide"),           # the same at the 3 x 3 map a 32 x 32 input leaves it: every output pixel sees padding
    (1, 5, 6, 260, 1, 4, 1, 1, False, 1.0, "o1_ragged_trip o1_dgrad wg_cl256_ragged"), # o1, second trip on lane 0 only / o1 / cl 256, second trip 4 channels
    (2, 66, 66, 8, 1, 4, 1, 1, True, 0.2, "o1_fwd_wrap slope wg_splits wg_ragged_split"),   # o1 over 8450 pixels: wraps, 2 of 64 lanes / o1 / cl 4, 16 splits of 529 pixels, the last 515
    (2, 66, 66, 256, 1, 4, 1, 1, False, 1.0, "o1_fwd_wrap o1_dgrad_wrap wg_cl256 wg_splits"),   # o1 wraps, one full trip / o1 over 557568 float4: wraps / cl 256, 16 splits
    # ---- Cin = 1 (1 -> 64 is the first layer)
    (2, 8, 8, 1, 64, 4, 2, 1, True, 0.2, "c1_cout64 slope"),                           # k_sconv_fwd_c1 / k_sconv_dgrad_c1 / k_sconv_wgrad_c1 64 cout lanes x 4 pixel lanes, one split
    (1, 6, 5, 1, 1024, 4, 2, 1, False, 1.0, "c1_cout1024"),                            # c1 at 64 KiB of dynamic LDS / c1 at 64 KiB / k_sconv_wgrad cl 1 (Cout > 256)
    (2, 8, 8, 1, 512, 4, 2, 1, True, 1.0, "c1_cout512_wgrad_generic"),                 # c1 / c1 / k_sconv_wgrad cl 1
    (2, 9, 7, 1, 48, 4, 2, 1, True, 0.2, "c1_cout48_wgrad_generic slope"),             # c1 / c1 / k_sconv_wgrad cl 1 (256 % 48 != 0); odd map
    (3, 62, 50, 1, 16, 4, 2, 1, True, 1.0, "c1_wgrad_splits c1_wgrad_ragged_split"),   # c1 / c1 / wgrad_c1 16 x 16 lanes, 2 splits of 1163 pixels, the last 1162
    (9, 128, 128, 1, 64, 4, 2, 1, False, 0.2, "c1_fwd_wrap c1_wgrad_splits slope"),    # c1 over 589824 float4: wraps / c1 / wgrad_c1 36 splits of 1024
    (9, 256, 256, 1, 4, 4, 2, 1, False, 1.0, "c1_dgrad_wrap c1_wgrad_splits"),         # c1 / c1 over 589824 input pixels: wraps / wgrad_c1 4 x 64 lanes, 144 splits
    (1, 7, 9, 1, 8, 4, 1, 1, True, 1.0, "c1_stride1"),                                 # the c1 kernels at stride 1
    # ---- k_sconv_wgrad's lane tiers with a ragged last channel trip (Cout % 4 != 0 or Cin % 4 != 0 keeps these off the MFMA forms)
    (1, 6, 6, 6, 5, 4, 2, 1, True, 1.0, "wg_cl4_ragged"),                              # k_sconv_fwd scalar / k_sconv_dgrad / cl 4: trips of 4 + 2
    (1, 7, 6, 20, 3, 4, 1, 1, False, 1.0, "wg_cl16_ragged"),                           # k_sconv_fwd float4 / k_sconv_dgrad / cl 16: 16 + 4
    (1, 6, 6, 96, 2, 4, 2, 1, True, 1.0, "wg_cl64_ragged"),                            # generic / generic / cl 64: 64 + 32
    (1, 5, 5, 300, 2, 4, 1, 1, False, 1.0, "wg_cl256_ragged"),                         # generic / generic / cl 256: 256 + 44
    # ---- stride 1 on the MFMA grid: the nine (wg_tile(Cout), wg_tile(Cin)) pairs of conv_k4s1_wgrad_grid; forward and input
    #      gradient are conv_k4s1_grid (forward: + crop; input gradient: pad + flipped weights, channel roles swapped).  The
    #      queries tell the grid form (all three > 0), not the pair.
    (2, 6, 6, 16, 24, 4, 1, 1, True, 1.0, "s1_tile_32x32"),
    (1, 7, 7, 36, 32, 4, 1, 1, False, 1.0, "s1_tile_32x64 s1_unfilled_36"),
    (1, 6, 7, 32, 36, 4, 1, 1, True, 1.0, "s1_tile_64x32 s1_unfilled_36"),
    (1, 8, 8, 64, 64, 4, 1, 1, False, 1.0, "s1_tile_64x64"),
    (1, 7, 6, 68, 16, 4, 1, 1, True, 1.0, "s1_tile_32x128 s1_unfilled_68"),
    (1, 6, 6, 16, 68, 4, 1, 1, False, 1.0, "s1_tile_128x32 s1_unfilled_68"),
    (1, 9, 9, 100, 36, 4, 1, 1, True, 1.0, "s1_tile_64x128 s1_unfilled_100 s1_unfilled_36"),
    (1, 6, 8, 36, 100, 4, 1, 1, False, 1.0, "s1_tile_128x64 s1_unfilled_100"),
    (1, 8, 8, 256, 512, 4, 1, 1, False, 1.0, "s1_tile_128x128 s1_256_512"),            # the discriminator's 256 -> 512 layer
    (2, 4, 4, 256, 512, 4, 1, 1, False, 1.0, "s1_h4_mfma s1_tile_128x128"),            # H = 4: still the grid form, 3 x 3 output
    (2, 3, 3, 256, 512, 4, 1, 1, False, 1.0, "s1_h3_direct_wide wg_cl256"),            # H = 3: k_sconv_fwd float4 / k_sconv_dgrad / k_sconv_wgrad cl 256
    (1, 8, 8, 16, 32, 4, 1, 1, True, 0.2, "slope slope_mfma_bwd"),                     # slope: k_sconv_fwd float4 (fwd_ws_bytes > 0 all the same) / grid form / grid form
    # ---- stride 2 on the MFMA kernels
    (2, 2, 32, 16, 16, 4, 2, 1, True, 1.0, "s2_single_row s2_h_ne_w"),                 # conv_k4s2_fwd, one output row / conv_k4s2_dgrad / conv_k4s2_wgrad (low-res width 16)
    (1, 6, 32, 8, 40, 4, 2, 1, False, 1.0, "s2_h_ne_w"),                               # three output rows of 16
    (1, 16, 16, 64, 128, 4, 2, 1, False, 1.0, "s2_wgrad_fallback_wide wg_cl64"),       # MFMA / MFMA / low-res width 8: k_sconv_wgrad cl 64
    (1, 9, 7, 64, 128, 4, 2, 1, True, 1.0, "s2_odd_generic_wide wg_cl64"),             # odd H, W: k_sconv_fwd float4 / k_sconv_dgrad / k_sconv_wgrad cl 64
    (1, 8, 8, 16, 32, 4, 2, 1, False, 0.2, "slope slope_mfma_bwd"),                    # slope: k_sconv_fwd / conv_k4s2_dgrad / k_sconv_wgrad cl 16 (low-res width 4)
    # ---- the generic kernels at the other kernel sizes and paddings check_sconv admits: k_sconv_fwd (scalar; float4 where
    #      Cin = 4) / k_sconv_dgrad / k_sconv_wgrad at cl 1 (Cin < 4) or cl 4, one split.  No size query tells them apart.
    (2, 5, 6, 3, 4, 1, 1, 0, True, 1.0, "ks1"),
    (1, 7, 8, 2, 3, 1, 2, 0, False, 0.2, "ks1 slope"),
    (1, 9, 8, 3, 2, 2, 2, 1, True, 1.0, "ks2"),
    (2, 8, 9, 4, 3, 5, 2, 4, True, 0.2, "ks5 pad_max slope"),
    (1, 6, 7, 5, 3, 6, 1, 3, False, 1.0, "ks6"),
    (1, 10, 9, 2, 5, 7, 1, 6, False, 1.0, "ks7 pad_max"),
    (1, 11, 12, 3, 2, 7, 2, 0, True, 1.0, "ks7 pad0"),
    (3, 2, 2, 5, 4, 4, 1, 1, True, 1.0, "one_pixel"),                                  # H + 2 pad == ks: one output pixel per image
    (2, 3, 3, 4, 6, 7, 2, 2, False, 1.0, "one_pixel ks7"),
    (2, 3, 3, 3, 2, 3, 1, 0, True, 1.0, "one_pixel pad0"),
]


def case_id(c):
    return "%dx%dx%d-%dto%d-k%ds%dp%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], "lrelu" if c[9] != 1.0 else "lin") + ("-b" if c[8] else "")


def sconv_inputs(case):
    """fp32 x, w, b, cotangent r of a row, from its own seed."""
    N, H, W, Cin, Cout, ks, stride, pad, bias, _ = case[:10]
    g = torch.Generator().manual_seed(_seed(case[:10]))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) * (2.0 / (Cin * ks * ks)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.5 if bias else None
    r = torch.randn(N, Cout, out_dim(H, ks, stride, pad), out_dim(W, ks, stride, pad), generator=g)
    return x, w, b, r


def pre_activation(case):
    """float64 convolution output of a row in front of the LeakyReLU, and the leaves it was made from."""
    x, w, b, _ = sconv_inputs(case)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    return F.conv2d(x64, w64, b64, stride=case[6], padding=case[7]), (x64, w64, b64)


def band(z64):
    """Outputs whose float64 pre-activation is within MASK_BAND standard deviations of the switch point."""
    z = z64.detach()
    return z.abs() < MASK_BAND * float(z.std()) if z.numel() > 1 else z.abs() < MASK_BAND


def sconv_reference(case, y_sign=None):
    """-> (y, dx, dw, db, share of the outputs inside the band) in float64.  y_sign: the kernel's own y > 0, taken inside the
    band of a slope row for the gradients (the forward reference is F.leaky_relu everywhere)."""
    slope = case[9]
    z, (x64, w64, b64) = pre_activation(case)
    r = sconv_inputs(case)[3].double()
    share = 0.0
    if slope == 1.0:
        y = yg = z
    else:
        y = F.leaky_relu(z, slope)
        amb = band(z)
        share = float(amb.double().mean())
        pos = z.detach() > 0
        if y_sign is not None:
            pos = torch.where(amb, y_sign, pos)
        yg = z * torch.where(pos, 1.0, slope).double()
    (yg * r).sum().backward()
    return y.detach(), x64.grad, w64.grad, (b64.grad if b64 is not None else None), share


def size_query_facts(L, case):
    """What the public size queries say about a row against routes(): called by the GPU test and, on a CPU-only machine, by
    tests/test_patchgan_cases_host.py (the queries are host code)."""
    N, H, W, Cin, Cout, ks, stride, pad = case[:8]
    r = routes(case)
    assert (L.vqw_sconv_fwd_ws_bytes(N, H, W, Cin, Cout, ks, stride, pad) > 0) == (r["mfma"] and stride == 1), "forward grid form"
    assert (L.vqw_sconv_dgrad_ws_bytes(N, H, W, Cin, Cout, ks, stride, pad) > 0) == r["dgrad"].startswith("mfma"), "input gradient form"
    bias_rows = L.vqw_sconv_wgrad_ws_bytes(1, 1, 1, 1, 1, 1, 1, 0) // 4 - 1         # a 1 x 1 x 1 layer: one split of one float
    fl = L.vqw_sconv_wgrad_ws_bytes(Cin, Cout, ks, N, H, W, stride, pad) // 4 - bias_rows * Cout
    if r["wgrad"] in ("c1", "generic"):
        assert fl == r["ws_floats"], "weight gradient: %d floats of partials, %s at %d splits has %d" % (fl, r["wgrad"], r["splits"], r["ws_floats"])
    else:
        assert fl > 0


def _run_sconv(case):
    ops = _ops()
    N, H, W, Cin, Cout, ks, stride, pad, bias, slope = case[:10]
    x, w, b, r = sconv_inputs(case)
    dx = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    dw = w.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    db = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.sconv2d(dx, dw, db, stride=stride, padding=pad, slope=slope)
    (y * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    yref, gx, gw, gb, share = sconv_reference(case, (y.detach() > 0).cpu() if slope != 1.0 else None)
    tag = case_id(case)
    assert tuple(y.shape) == tuple(yref.shape)
    assert torch.isfinite(y).all() and torch.isfinite(dx.grad).all() and torch.isfinite(dw.grad).all()
    if slope != 1.0:
        print("  %-58s %.1e of the outputs within %.0e std of the switch point (cap %.0e)" % (tag, share, MASK_BAND, MASK_FRACTION))
        assert share <= MASK_FRACTION
    _check(tag, "y", y, yref, KERNEL_TOL)
    _check(tag, "dx", dx.grad, gx, KERNEL_TOL)
    _check(tag, "dw", dw.grad, gw, KERNEL_TOL)
    if bias:
        _check(tag, "db", db.grad, gb, KERNEL_TOL)


def _claims(prefixes):
    return [c for c in ROUTE_CASES if any(t.startswith(prefixes) for t in c[10].split())]


ENDS = _claims(("o1", "c1"))
MFMA_S1 = [c for c in _claims(("s1",)) if c not in ENDS]
OTHER = [c for c in ROUTE_CASES if c not in ENDS and c not in MFMA_S1]
assert len(ENDS) + len(MFMA_S1) + len(OTHER) == len(ROUTE_CASES) == len(set(ROUTE_CASES))


def _lib():
    from hipops import _lib as B
    return B.load()


@pytest.mark.parametrize("case", ENDS, ids=case_id)
def test_sconv_one_channel_ends_vs_float64(case):
    """Cin = 1 and Cout = 1: the c1 / o1 kernels, their LDS sizes, lane trips, pixel splits and grid wraps."""
    size_query_facts(_lib(), case)
    _run_sconv(case)


@pytest.mark.parametrize("case", MFMA_S1, ids=case_id)
def test_sconv_stride1_grid_vs_float64(case):
    """conv_k4s1_grid / conv_k4s1_wgrad_grid: every weight-gradient tile pair, unfilled tiles, the H = 4 / H = 3 boundary."""
    size_query_facts(_lib(), case)
    _run_sconv(case)


@pytest.mark.parametrize("case", OTHER, ids=case_id)
def test_sconv_stride2_and_generic_vs_float64(case):
    """The stride-2 MFMA form and its fall-backs, k_sconv_wgrad's lane tiers, the generic kernels at ks 1..7 and pad 0..ks-1."""
    size_query_facts(_lib(), case)
    _run_sconv(case)


# ---- misaligned pointers through the C ABI: every array one float off a 16-byte boundary sends the c1 / o1 shapes to the
#      generic kernels, and k_sconv_fwd's float4 branch (Cin % 4 == 0) to its scalar one.  (The MFMA entry points are not
#      reached: these shapes are not MFMA shapes.)
MISALIGNED_CASES = [
    (2, 9, 9, 8, 1, 4, 1, 1, True, 1.0),      # Cout = 1 shape: k_sconv_fwd scalar although Cin % 4 == 0 / k_sconv_dgrad / k_sconv_wgrad
    (2, 8, 8, 1, 8, 4, 2, 1, True, 0.2),      # Cin = 1 shape: k_sconv_fwd / k_sconv_dgrad / k_sconv_wgrad_c1 (scalar loads only)
    (1, 6, 6, 4, 6, 4, 2, 1, False, 1.0),     # generic shape with Cin % 4 == 0
]


def _off1(flat):
    """A copy of a flat fp32 tensor on the GPU whose first element is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(flat.numel() + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(flat)
    out = buf[1:]
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("case", MISALIGNED_CASES, ids=case_id)
def test_sconv_misaligned_pointers_vs_float64(case):
    from hipops import _lib as B
    L = B.load()
    N, H, W, Cin, Cout, ks, stride, pad, bias, slope = case
    assert not routes(case)["mfma"]
    Ho, Wo = out_dim(H, ks, stride, pad), out_dim(W, ks, stride, pad)
    x, w, b, r = sconv_inputs(case)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().reshape(-1)      # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    geo = (N, H, W, Cin, Cout, ks, stride, pad)
    xd, wd, rd = _off1(nhwc(x)), _off1(nhwc(w)), _off1(nhwc(r))
    bd = _off1(b) if bias else None
    y, gm = _off1(torch.zeros(N * Ho * Wo * Cout)), _off1(torch.zeros(N * Ho * Wo * Cout))
    gx, gw = _off1(torch.zeros(x.numel())), _off1(torch.zeros(w.numel()))
    gb = _off1(torch.zeros(Cout)) if bias else None
    ws = torch.empty(max(L.vqw_sconv_fwd_ws_bytes(*geo), L.vqw_sconv_dgrad_ws_bytes(*geo),
                         L.vqw_sconv_wgrad_ws_bytes(Cin, Cout, ks, N, H, W, stride, pad), 16), dtype=torch.uint8, device=DEV)
    B.check(L.vqw_sconv_fwd(p(xd), p(wd), p(bd), p(y), p(ws), ws.numel(), *geo, slope, st), "vqw_sconv_fwd")
    gy = rd
    if slope != 1.0:
        B.check(L.vqw_leaky_relu_bwd(p(y), p(rd), p(gm), slope, y.numel(), st), "vqw_leaky_relu_bwd")
        gy = gm
    B.check(L.vqw_sconv_dgrad(p(gy), p(wd), p(gx), p(ws), ws.numel(), *geo, st), "vqw_sconv_dgrad")
    B.check(L.vqw_sconv_wgrad(p(xd), p(gy), p(gw), p(gb), p(ws), ws.numel(), *geo, 0, st), "vqw_sconv_wgrad")
    torch.cuda.synchronize()
    back = lambda flat, n, c, h, w_: flat.view(n, h, w_, c).permute(0, 3, 1, 2)      # noqa: E731
    y4 = back(y, N, Cout, Ho, Wo)
    yref, rgx, rgw, rgb, share = sconv_reference(case, (y4 > 0).cpu() if slope != 1.0 else None)
    assert share <= MASK_FRACTION
    tag = "misaligned " + case_id(case)
    _check(tag, "y", y4, yref, KERNEL_TOL)
    _check(tag, "dx", back(gx, N, Cin, H, W), rgx, KERNEL_TOL)
    _check(tag, "dw", back(gw, Cout, Cin, ks, ks), rgw, KERNEL_TOL)
    if bias:
        _check(tag, "db", gb, rgb, KERNEL_TOL)


# --------------------------------------------------------------------------------------------------
# c. hinge_real, hinge_fake, neg_mean; vqw_leaky_relu_bwd on its own
# --------------------------------------------------------------------------------------------------
# n -> a 4-D shape with that many elements (30752 = the default discriminator's output for a batch of 32 at 256 x 256; 524291 =
# 524288 + 3 = 29 * 101 * 179: one element-wise launch of stream_grid and three elements of a second trip)
HINGE_SHAPES = {1: (1, 1, 1, 1), 1023: (1, 3, 11, 31), 1025: (1, 5, 5, 41), 30752: (2, 16, 31, 31), 524291: (1, 29, 101, 179)}
KINKS = (1.0, -1.0, 0.0)        # exactly representable: 1 - x, 1 + x are exact and the kernel's subgradient there is relu's, 0


def hinge_input(n, variant=0):
    """fp32 logits of HINGE_SHAPES[n] with the kink values planted at the front, the middle and the end (n = 1: KINKS[variant])."""
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(HINGE_SHAPES[n], generator=g) * 1.5 + 0.2
    flat = x.view(-1)
    if n == 1:
        flat[0] = KINKS[variant]
    else:
        for k, v in enumerate(KINKS):
            flat[k] = v
            flat[n // 2 + k] = v
            flat[n - 1 - k] = v
    return x


HINGE_REFS = {
    "hinge_real": lambda x: F.relu(1.0 - x).mean(),
    "hinge_fake": lambda x: F.relu(1.0 + x).mean(),
    "neg_mean": lambda x: -x.mean(),
}


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("fn", sorted(HINGE_REFS))
@pytest.mark.parametrize("n", sorted(HINGE_SHAPES))
def test_hinge_losses_vs_float64(n, fn, layout):
    ops = _ops()
    upstream = 2.5
    for variant in range(3 if n == 1 else 1):
        x = hinge_input(n, variant)
        x64 = x.double().requires_grad_(True)
        l64 = HINGE_REFS[fn](x64)
        (upstream * l64).backward()
        xd = x.to(DEV)
        if layout == "channels_last":
            xd = xd.contiguous(memory_format=CL)
        xd.requires_grad_(True)
        loss = getattr(ops, fn)(xd)
        (upstream * loss).backward()
        torch.cuda.synchronize()
        got, ref = xd.grad.double().cpu(), x64.grad
        el = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()) if float(ref.abs().max()) > 0 else float(got.abs().max())
        got_l, ref_l = float(loss.detach()), float(l64.detach())
        lerr = abs(got_l - ref_l) / abs(ref_l) if ref_l != 0 else abs(got_l)
        print("  %-10s n=%-7d %-13s loss rel %.2e, gradient worst element rel %.2e  (bound %.0e)" % (fn, n, layout, lerr, el, LOSS_TOL))
        assert xd.grad.shape == x.shape and xd.grad.stride() == xd.stride()
        assert lerr <= LOSS_TOL
        assert bool(((got - ref).abs() <= LOSS_TOL * ref.abs()).all()), "gradient: an element is more than 1e-6 off (zeros must be exact)"
        if fn != "neg_mean":       # the planted kinks take the zero subgradient
            kink = x.view(-1) == (1.0 if fn == "hinge_real" else -1.0)
            assert bool(kink.any()) or n == 1
            assert float(xd.grad.cpu().reshape(-1)[kink.reshape(-1)].abs().sum()) == 0.0


@pytest.mark.parametrize("n", sorted(HINGE_SHAPES))
def test_leaky_relu_bwd_vs_float64(n):
    """vqw_leaky_relu_bwd(y, gy) = gy where y > 0, slope * gy elsewhere (y = 0 included, as F.leaky_relu's gradient has it)."""
    ops = _ops()
    slope = 0.2
    y = hinge_input(n, 2)                       # planted +1, -1 and exact zeros
    g = torch.Generator().manual_seed(2000 + n)
    gy = torch.randn(y.shape, generator=g)
    y64 = y.double().requires_grad_(True)
    (F.leaky_relu(y64, slope) * gy.double()).sum().backward()
    yd, gyd = y.to(DEV), gy.to(DEV)
    gx = torch.empty_like(yd)
    ops._L().vqw_leaky_relu_bwd(yd, gyd, gx, slope, n)
    torch.cuda.synchronize()
    got, ref = gx.double().cpu(), y64.grad
    el = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    print("  leaky_relu_bwd n=%-7d worst element rel %.2e  (bound %.0e)" % (n, el, LOSS_TOL))
    assert bool((y.view(-1) == 0).any()) or n == 1
    assert bool(((got - ref).abs() <= LOSS_TOL * ref.abs()).all())


# --------------------------------------------------------------------------------------------------
# d. ops.act_norm_lrelu
# --------------------------------------------------------------------------------------------------
def actnorm_input(C, kind):
    """(2, C, 9, 7) fp32: channels with their own scale and offset.  'far': channel 1 has mean / std = 1e3.
    'const': channel 1 is exactly 1.15 (its fp32 square is 4.5e-8 above the exact one; the variance must still come out 0)."""
    g = torch.Generator().manual_seed(300 + C)
    x = torch.randn(2, C, 9, 7, generator=g)
    x = x * (0.5 + 1.5 * torch.rand(1, C, 1, 1, generator=g)) + (torch.rand(1, C, 1, 1, generator=g) * 2 - 1)
    if kind == "far":
        x[:, 1] = torch.randn(2, 9, 7, generator=g) * 0.01 + 10.0
    elif kind == "const":
        x[:, 1] = 1.15
    return x


def _mean_term(x64):
    """2^-23 * max over channels of |mean| / std: the error fp32 storage of loc = -mean adds to scale * (x + loc)."""
    m = x64.detach().mean(dim=(0, 2, 3))
    s = x64.detach().std(dim=(0, 2, 3), unbiased=False)
    live = s > 0
    return 2.0 ** -23 * float((m.abs()[live] / s[live]).max())


def actnorm_setup(case):
    """-> fp32 x, cotangent r, the loc / scale the operator is handed, and the float64 leaves x, loc, scale of the reference (at
    initialisation loc = -mean, scale = 1 / (unbiased std + 1e-6) of x itself)."""
    C, slope, init, kind = case
    x = actnorm_input(C, kind)
    g = torch.Generator().manual_seed(400 + C)
    r = torch.randn(x.shape, generator=g)
    x64 = x.double().requires_grad_(True)
    if init:
        flat = x64.detach().transpose(0, 1).reshape(C, -1)
        loc64 = (-flat.mean(1)).view(1, C, 1, 1)
        scale64 = (1.0 / (flat.std(1, unbiased=True) + 1e-6)).view(1, C, 1, 1)
        loc0, scale0 = torch.zeros(1, C, 1, 1), torch.ones(1, C, 1, 1)
    else:
        loc0 = torch.randn(1, C, 1, 1, generator=g) * 0.5
        scale0 = (0.5 + torch.rand(1, C, 1, 1, generator=g)) * torch.where(torch.arange(C).view(1, C, 1, 1) % 2 == 0, 1.0, -1.0)
        loc64, scale64 = loc0.double(), scale0.double()
    return x, r, loc0, scale0, x64, loc64.requires_grad_(True), scale64.requires_grad_(True)


def actnorm_band(case, z64):
    """Elements whose float64 pre-activation scale * (x + loc) is within MASK_BAND of the switch point."""
    amb = z64.detach().abs() < MASK_BAND
    if case[3] == "const":
        amb[:, 1] = False          # scale * 0: exactly 0 in fp32, 1e6 * the rounding of the mean in float64; masked on both sides
    return amb


ACTNORM_CASES = [(C, slope, init, kind) for C in (3, 4, 64, 260) for slope in (0.2, 1.0) for init in (True, False)
                 for kind in ("randn",)] + [(4, 0.2, True, "far"), (260, 1.0, True, "far"), (3, 0.2, True, "const"), (64, 1.0, True, "const")]


@pytest.mark.parametrize("params_grad", [True, False], ids=["train_params", "frozen_params"])
@pytest.mark.parametrize("case", ACTNORM_CASES, ids=lambda c: "C%d-slope%g-%s-%s" % (c[0], c[1], "init" if c[2] else "given", c[3]))
def test_act_norm_lrelu_vs_float64(case, params_grad):
    """y = leaky_relu(scale * (x + loc)); with the `initialized` flag loc = -mean, scale = 1 / (unbiased std + 1e-6) per channel
    are written first and the flag raised.  C = 260 reaches the second workgroup of k_actnorm_prepare / k_actnorm_loc_grad and
    the fifth, four channels wide, of k_actnorm_stats; frozen_params is the generator pass (no parameter gradient, the reduce
    launch is skipped).  'far' and 'const' are what the initialisation's own statistics pass is there for: with the fp32 squares
    of vqw_bn_partial_stats the far channel's scale was 1.9e-4 (C = 4) and 7.7e-4 (C = 260) off, the constant channel's 4.7e3."""
    ops = _ops()
    C, slope, init, kind = case
    x, r, loc0, scale0, x64, loc64, scale64 = actnorm_setup(case)

    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    loc, scale = loc0.to(DEV).requires_grad_(params_grad), scale0.to(DEV).requires_grad_(params_grad)
    flag = torch.zeros((), dtype=torch.uint8, device=DEV)
    y = ops.act_norm_lrelu(xd, loc, scale, flag if init else None, slope=slope)
    (y * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()

    z64 = scale64 * (x64 + loc64)
    amb = actnorm_band(case, z64)
    assert float(amb.double().mean()) <= MASK_FRACTION
    pos = torch.where(amb, y.detach().cpu() > 0, z64.detach() > 0)
    (z64 * torch.where(pos, 1.0, slope).double() * r.double()).sum().backward()
    yref = F.leaky_relu(z64, slope)

    extra = _mean_term(x64) if kind == "far" else 0.0
    tag = "act_norm_lrelu C=%d slope=%g %s %s %s" % (C, slope, "init" if init else "given", kind, "params" if params_grad else "frozen")
    if extra:
        print("  %-58s mean term %.2e" % (tag, extra))
    assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all()
    _check(tag, "y", y, yref, FWD_TOL + extra)
    _check(tag, "dx", xd.grad, x64.grad, GRAD_TOL)
    if params_grad:
        assert loc.grad.shape == scale.grad.shape == (1, C, 1, 1)
        _check(tag, "dloc", loc.grad, loc64.grad, PARAM_TOL)
        _check(tag, "dscale", scale.grad, scale64.grad, PARAM_TOL + extra)
    else:
        assert loc.grad is None and scale.grad is None
    if init:
        assert int(flag) == 1, "the initialized flag was not raised"
        _check(tag, "loc", loc, loc64, FWD_TOL)
        _check(tag, "scale", scale, scale64, FWD_TOL)
        if kind == "const":
            assert abs(float(scale.detach().view(-1)[1]) - 1e6) <= 1.0, "constant channel: scale %r, not 1 / 1e-6" % float(scale.detach().view(-1)[1])
    else:
        assert int(flag) == 0
        assert torch.equal(loc.detach().cpu(), loc0) and torch.equal(scale.detach().cpu(), scale0), "given loc / scale were written"


# --------------------------------------------------------------------------------------------------
# e. the default-width module once
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalization", ["batchnorm", "actnorm"])
def test_default_width_discriminator_vs_float64(normalization):
    """NLayerDiscriminator(1, 1, 64, 3) in train mode at 2 x 1 x 64 x 64: 1 -> 64 s2 (c1), 64 -> 128 s2 and 128 -> 256 s2 (MFMA,
    the second with the direct weight gradient: low-res width 8), 256 -> 512 s1 at 8 x 8 (grid form), 512 -> 1 s1 (o1), against
    the float64 restatement from the same state dict, at _run_block's bounds."""
    from networks import NLayerDiscriminator
    from oracle import gan_ref
    import gan_norm_ref
    torch.manual_seed(17)
    dis = NLayerDiscriminator(1, 1, n_filters=64, n_layers=3, normalization=normalization)
    state = {k: v.detach().clone().double() if v.is_floating_point() else v.detach().clone() for k, v in dis.state_dict().items()}
    names = [k for k, _ in dis.named_parameters()]
    for k in names:
        state[k].requires_grad_(True)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, 1, 64, 64, generator=g)
    x64 = x.double().requires_grad_(True)
    if normalization == "batchnorm":
        out64 = gan_ref.discriminator_forward(state, x64, True, 3)
    else:
        out64 = gan_norm_ref.discriminator_ref(x64, state, 3, True)
    r = torch.randn(out64.shape, generator=g)
    (out64 * r.double()).sum().backward()

    dis.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    out = dis(xd)
    (out * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _ops().flush_counters()
    tag = "NLayerDiscriminator(1, 1, 64, 3) %s" % normalization

    def report(what, got, ref, tol, atol=0.0):
        print("  %-44s %-28s rel %.2e  (bound %.0e)" % (tag, what, rel_err(got, ref), tol))
        assert_close(got, ref, tol, "%s %s" % (tag, what), atol=atol)
    assert tuple(out.shape) == tuple(out64.shape) == (2, 1, 6, 6)
    report("out", out, out64, 1e-4)
    report("gin", xd.grad, x64.grad, 1e-3, atol=1e-6)
    for k, p in dis.named_parameters():
        assert p.grad is not None, k
        report("gP." + k, p.grad, state[k].grad, 1e-3, atol=2e-5)
    n_state = 0
    for k, v in dis.state_dict().items():
        if k in names and not k.endswith(("loc", "scale")):
            continue                                 # parameters no forward writes
        if v.is_floating_point():
            report("after." + k, v, state[k], 1e-5)
        else:
            assert int(v) == int(state[k]) == 1, k        # num_batches_tracked / initialized
        n_state += 1
    assert n_state == 9          # three norm layers: running_mean, running_var, num_batches_tracked or loc, scale, initialized
