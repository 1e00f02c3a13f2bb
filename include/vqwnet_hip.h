/*
 * vqwnet_hip.h — C ABI of libvqwnet_hip.so: the MI355X (gfx950) kernels behind the
 * VQ-W-Net training hot path of Kaz-K/medical-image-editing.
 *
 * The reference has no FFI of its own: every operator below replaces a stock
 * ATen call made from the reference's torch.nn modules (citations are to
 * /root/reference/src).  The drop-in boundary is therefore this library, bound
 * with ctypes from the Python host code in medical-image-editing_amd/hipops,
 * which re-implements the reference's nn.Module classes on top of it.
 *
 * Conventions
 *   - All tensor arguments are DEVICE pointers to dense fp32 in NHWC order
 *     (PyTorch `channels_last`), ids are int64/int32 as stated.
 *   - Conv weights are OHWI: w[co][ky][kx][ci] (PyTorch OIHW storage in
 *     channels_last memory format), i.e. the same bytes a
 *     `weight.contiguous(memory_format=torch.channels_last)` holds.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *     only enqueue work; no call synchronises, allocates or frees device memory
 *     (safe for hipGraph capture).  Scratch comes in through `ws` arguments whose
 *     size the matching *_ws_bytes() query returns.
 *   - Return value: 0 = ok, <0 = error (argument / launch); the message is
 *     available from vqw_last_error() (thread-local).  The Python binding turns a
 *     non-zero status into RuntimeError, mirroring the reference's assert /
 *     torch error behaviour.
 */
#ifndef VQWNET_HIP_H
#define VQWNET_HIP_H
#include <stddef.h>
#include <stdint.h>

/* vqw_abi_version() returns it; the Python binding reads it from here and refuses a library built from another version */
#define VQW_ABI_VERSION 9

#ifdef __cplusplus
extern "C" {
#endif

const char* vqw_last_error(void);
int vqw_abi_version(void);
/* 0 = auto (MFMA kernels when shapes allow), 1 = force the generic VALU kernels, 2 = MFMA kernels but
 * never the LDS-resident halo-tile forward (A/B timing, tests), 3 = auto but never a Winograd-form kernel (every plain
 * 3x3 layer in direct form: the reference for "the training forward's codebook indices do not depend on the Winograd
 * kernels").  Returns the previous mode. */
int vqw_set_conv_backend(int mode);
/* Measurement aid (bench.py roofline): HIP events recorded on the launch stream around every convolution kernel
 * family - and around the HBM-bound normalisation / element-wise entry points - between begin and end.  end() synchronises
 * on those events and fills out[6][4] = {launches, total ms, total FLOPs, total algorithmic bytes} for {MFMA fwd/dgrad, MFMA
 * wgrad, generic fwd, generic wgrad, Winograd-form fwd/dgrad/wgrad, HBM-bound norm / element-wise (bytes = tensor passes as
 * launched)}; FLOPs are the ones the kernels execute (collapsed up-sampled and Winograd-form layers: 4/9 of the direct
 * form's).  (ABI 6: the sixth family.  ABI 7: vqw_conv3x3_wino_fwd_masked, vqw_conv3x3_wino_fwd_acc, vqw_conv3x3_up2_dgrad_acc,
 * vqw_conv3x3_wino_fwd_inbwd, vqw_inorm_bwd_parts.)
 * Not meant for graph capture; off by default.                                                              */
int vqw_profile_begin(void);
int vqw_profile_end(double* out);
/* Which families record events (bit f = family f; default all).  bench.py keeps the ~390 norm / element-wise launches of a
 * step out of its TIMED region (two event records each would cost the step 2 %) and times them in the serialised pass.
 * Returns the previous mask. */
int vqw_profile_families(unsigned mask);

/* ---- convolution: replaces F.conv2d fwd/bwd behind nn.Conv2d in
 *      networks/blocks.py:5-6,25,45,48,75,79,80,102,108,112,117; networks/aspp.py:19-24;
 *      networks/unet_decoder.py:105.
 * The input is the *virtual* channel-concat [src0 (C0 ch, optionally nearest x2
 * up-sampled from H/2 x W/2), src1 (C1 ch, may be NULL/0)] so that
 * nn.Upsample + torch.cat (blocks.py:12,16-17,106,123) are never materialised.
 * ksize in {1,3}; stride 1; padding = dil*(ksize/2) ("same").                      */
int vqw_conv2d_fwd(const float* src0, int C0, int up0, const float* src1, int C1,
                   const float* w_ohwi, const float* bias, float* y,
                   int N, int H, int W, int Cout, int ksize, int dil, int relu, void* stream);
/* dgrad weights: wt[ci][2-ky][2-kx][co] = w[co][ky][kx][ci]; then
 * dX = vqw_conv2d_fwd(dY, Cout, 0, NULL, 0, wt, NULL, dX, N,H,W, Cin, ksize, dil, 0).
 * relu=1 fuses nn.ReLU into the epilogue (blocks.py:75-77 mlp_shared).             */
int vqw_pack_dgrad_weights(const float* w_ohwi, float* wt, int Cout, int Cin, int ksize, void* stream);
/* conv -> InstanceNorm (blocks.py:45-49): the convolution's epilogue also leaves the norm's statistics as per-tile
 * partials part[N][parts][Cout][2] = (sum, M2 = sum (x - tile mean)^2) of one equal-sized tile each (fp32, merged pairwise
 * inside the tile; the norm combines tiles in double: no fp32 value ever holds a sum of squares), so
 * the norm skips its reduction pass (vqw_inorm_fwd_parts).  ..._stats_parts() returns `parts` for a shape, 0 when
 * the shape is not served (the halo-tile and the implicit-GEMM kernel are; then use vqw_conv2d_fwd + vqw_inorm_fwd).
 * No ReLU epilogue.                                                                                              */
int vqw_conv2d_fwd_stats_parts(int C0, int C1, int up0, int N, int H, int W, int Cout, int ksize, int dil);
int vqw_conv2d_fwd_stats(const float* src0, int C0, int up0, const float* src1, int C1,
                         const float* w_ohwi, const float* bias, float* y, float* part,
                         int N, int H, int W, int Cout, int ksize, int dil, void* stream);
/* y += conv(src0) ('same' conv, no bias): the input gradient of one of several convolutions of the same tensor summed in
 * place (aspp.py:44-47: five branches of one input; autograd would add their gradients pairwise, three passes each).
 * Served for the shapes of the row-chain kernel (dilated 3x3, 32 channels, rows <= 256 pixels) and (ABI 8) for 1x1 layers on
 * the implicit-GEMM kernel, whose epilogue then adds to y: query ..._supported. */
int vqw_conv2d_fwd_acc_supported(int C0, int N, int H, int W, int Cout, int ksize, int dil);
int vqw_conv2d_fwd_acc(const float* src0, int C0, const float* w_ohwi, float* y, int N, int H, int W, int Cout, int ksize,
                       int dil, void* stream);
size_t vqw_conv2d_wgrad_ws_bytes(int C0, int C1, int N, int H, int W, int Cout, int ksize);
/* dW[co][ky][kx][ci] (OHWI) and, if dbias != NULL, dbias[co] = sum_p dY.
 * accumulate=1 adds into dw / dbias (a layer used by both views of a step: one gradient buffer, no extra pass). */
int vqw_conv2d_wgrad(const float* src0, int C0, int up0, const float* src1, int C1,
                     const float* dy, float* dw_ohwi, float* dbias, void* ws, size_t ws_bytes,
                     int N, int H, int W, int Cout, int ksize, int dil, int accumulate, void* stream);
/* 3x3 conv over a nearest x2 up-sampled single source (StyledResUpBlock conv / conv1, blocks.py:106,117,123-126),
 * collapsed onto the low-resolution grid: four 2x2 convs forward, one 4x4 stride-2 gather for the input gradient —
 * 4/9 of the FLOPs of the direct form and no full-resolution gradient intermediate.  x_low is [N,h,w,Cin], y and dy
 * are [N,2h,2w,Cout].  prepare() writes the tap-summed weights for both directions into ws (valid while w is unchanged). */
int vqw_conv3x3_up2_supported(int Cin, int Cout, int N, int h, int w);
size_t vqw_conv3x3_up2_ws_bytes(int Cin, int Cout);
int vqw_conv3x3_up2_prepare(const float* w_ohwi, void* ws, size_t ws_bytes, int Cin, int Cout, void* stream);
int vqw_conv3x3_up2_fwd(const float* x_low, const void* ws, const float* bias, float* y, int N, int h, int w, int Cin,
                        int Cout, int relu, void* stream);
/* forward that also leaves the following norm's statistics partials (see vqw_conv2d_fwd_stats); parts = 0: not served */
int vqw_conv3x3_up2_fwd_stats_parts(int Cin, int Cout, int N, int h, int w);
int vqw_conv3x3_up2_fwd_stats(const float* x_low, const void* ws, const float* bias, float* y, float* part, int N, int h, int w,
                              int Cin, int Cout, void* stream);
/* (ABI 8) TWO 32-cout layers of the same up-sampled input - StyledResUpBlock's shortcut `conv` and `conv1`, blocks.py:100-112 - as ONE
 * 64-cout launch of the nine-product kernel.  ws = vqw_conv3x3_up2_prepare() of the concatenated weights [w_a | w_b] (Cout = 64),
 * bias_cat = [b_a | b_b] or NULL; y_a / y_b (N, 2h, 2w, 32) and their InstanceNorm / BatchNorm statistics partials part_a / part_b
 * ([N][parts][32][2], parts = the value ..._supported returns; 0 = not served) come out as separate tensors. */
int vqw_conv3x3_up2_fwd_pair_supported(int Cin, int Cout_each, int N, int h, int w);
int vqw_conv3x3_up2_fwd_pair(const float* x_low, const void* ws, const float* bias_cat, float* y_a, float* y_b, float* part_a,
                             float* part_b, int N, int h, int w, int Cin, int Cout_each, void* stream);
int vqw_conv3x3_up2_dgrad(const float* dy, const void* ws, float* dx_low, int N, int h, int w, int Cin, int Cout,
                          void* stream);
/* ABI 7.  dx_low += the same input gradient: the second of the two up-sampled convolutions that read one tensor (a
 * StyledResUpBlock's `conv` and `conv1`, blocks.py:100-112) adds to the first one's result in its epilogue. */
int vqw_conv3x3_up2_dgrad_acc_supported(int Cin, int Cout, int N, int h, int w);
int vqw_conv3x3_up2_dgrad_acc(const float* dy, const void* ws, float* dx_low, int N, int h, int w, int Cin, int Cout,
                              void* stream);
/* weight (and bias) gradient of the same layer on the low-resolution grid (needs w % 16 == 0) */
int vqw_conv3x3_up2_wgrad_supported(int Cin, int Cout, int N, int h, int w);
size_t vqw_conv3x3_up2_wgrad_ws_bytes(int Cin, int Cout, int N, int h, int w);
int vqw_conv3x3_up2_wgrad(const float* x_low, const float* dy, float* dw_ohwi, float* dbias, void* ws, size_t ws_bytes,
                          int N, int h, int w, int Cin, int Cout, int accumulate, void* stream);
/* Plain 3x3 stride-1 convolution (every F.conv2d(x, w, padding=1) of blocks.py / unet_*.py on >= 16 input and >= 32
 * output channels) in Winograd F(2x2, 3x3) form: 4/9 of the direct form's matrix work, same fp32 arithmetic type; the
 * result differs from the direct form by a few ulps of the accumulated magnitude (a different product / summation order).
 * prepare() writes U = G w G^T [16][Cout][Cin] into ws (valid while w is unchanged).  The input gradient is the same
 * call on dy with the U of the packed dgrad weights (vqw_pack_dgrad_weights), roles of Cin / Cout swapped.
 * ..._fwd_stats: also leaves the following norm's statistics partials (see vqw_conv2d_fwd_stats); parts = 0: not served. */
int vqw_conv3x3_wino_supported(int Cin, int Cout, int N, int H, int W);
size_t vqw_conv3x3_wino_ws_bytes(int Cin, int Cout);
int vqw_conv3x3_wino_prepare(const float* w_ohwi, void* ws, size_t ws_bytes, int Cin, int Cout, void* stream);
/* The same for a layer's INPUT-GRADIENT convolution, straight from the layer's own weight (ABI 8): w_ohwi = the layer's
 * [Cin][3][3][Cout] tensor (its couts are this convolution's Cin input channels); equals vqw_pack_dgrad_weights followed by
 * vqw_conv3x3_wino_prepare(.., Cin, Cout), bit for bit, without the packed copy. */
int vqw_conv3x3_wino_prepare_dgrad(const float* w_ohwi, void* ws, size_t ws_bytes, int Cin, int Cout, void* stream);
int vqw_conv3x3_wino_fwd(const float* x, const void* ws, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                         int relu, void* stream);
/* ABI 7.  The same convolution with its outputs zeroed where mask <= 0 (mask shaped like y, no bias): the input gradient of
 * a layer whose forward read the output of a fused ReLU (StyledDenorm's mlp_shared -> mlp_gamma | mlp_beta, blocks.py:63-66,
 * 85-87) delivered in front of that ReLU - mask = the ReLU's output, i.e. the layer's own saved input - so that the
 * separate mask pass (vqw_relu_bwd) is not needed.  Served where the 64-cout kernel is (..._masked_supported). */
int vqw_conv3x3_wino_masked_supported(int Cin, int Cout, int N, int H, int W);
int vqw_conv3x3_wino_fwd_masked(const float* x, const void* ws, const float* mask, float* y, int N, int H, int W, int Cin,
                                int Cout, void* stream);
/* y += conv(x) (no bias): a later member of a gradient group - several convolutions of one input tensor (ResBlock's 3x3 and
 * 1x1 branches, blocks.py:14-36; the two mlp_shared convolutions of a StyledResUpBlock's StyledDenorms on one style input,
 * blocks.py:100-134) - adds its input gradient to the shared buffer in its epilogue instead of leaving the sum to a separate
 * add pass.  Served where ..._masked_supported says so. */
int vqw_conv3x3_wino_fwd_acc(const float* x, const void* ws, float* y, int N, int H, int W, int Cin, int Cout, void* stream);
/* A 3x3 layer of dilation 2 (the pyramid's first branch, aspp.py:27-30) in Winograd form (ABI 8): the plain kernel on the four
 * phase images of x and y; ws = vqw_conv3x3_wino_prepare of the layer (forward) or vqw_conv3x3_wino_prepare_dgrad (input
 * gradient: x = dY, Cin / Cout swapped).  part (optional, forward with relu == 0): the following norm's statistics partials
 * [N][parts][Cout][2], parts = ..._dil2_stats_parts; accumulate: y += result (no bias, no ReLU).  The weight gradient of such a
 * layer takes the same route inside vqw_conv2d_wgrad.  Served where ..._dil2_supported says so (H even, W a multiple of 64). */
int vqw_conv3x3_wino_dil2_supported(int Cin, int Cout, int N, int H, int W);
int vqw_conv3x3_wino_dil2_stats_parts(int Cin, int Cout, int N, int H, int W);
int vqw_conv3x3_wino_dil2_fwd(const float* x, const void* ws, const float* bias, float* y, float* part, int accumulate,
                              int N, int H, int W, int Cin, int Cout, int relu, void* stream);
/* One launch, two output tensors (ABI 8): couts [0, split) -> y0 [N,H,W,split] - or, with pool0, summed over each 2 x 2 output
 * tile into y0 [N,H/2,W/2,split] - and couts [split, Cout) -> y1 [N,H,W,Cout-split].  Two uses: (i) the input gradient of a 3x3
 * layer over [nearest-up2x(a) | b] (UpBlock, blocks.py:9-18 with unet_encoder.py's torch.cat): x = dY, ws = the transformed
 * input-gradient weights, Cout = Ca + Cb, split = Ca, pool0 = 1: the gradients of a and b leave the epilogue, replacing two
 * vqw_input_grad_gather passes over the concatenated gradient; (ii) two layers of one input on concatenated weights (the two
 * mlp_shared convolutions of a StyledResUpBlock's StyledDenorms, blocks.py:72-75, 100-134): pool0 = 0, bias / relu as in
 * vqw_conv3x3_wino_fwd.  split % 16 == 0; served where ..._split_supported says so. */
int vqw_conv3x3_wino_split_supported(int Cin, int Cout, int split, int pool0, int N, int H, int W);
int vqw_conv3x3_wino_fwd_split(const float* x, const void* ws, const float* bias, float* y0, float* y1, int N, int H, int W,
                               int Cin, int Cout, int split, int pool0, int relu, void* stream);
/* The same for a layer widened to the kernel's cout tile (ABI 8): ws = the transformed weights of Cout couts of which only
 * split + c1 are real (zero weights behind them), y1 has c1 channels, the padding couts are not stored.  The input gradient of the
 * 48-channel two-source layer at the encoder's full-resolution level (unet_encoder.py's last UpBlock) runs as a 64-cout launch. */
int vqw_conv3x3_wino_split_padded_supported(int Cin, int Cout, int split, int c1, int pool0, int N, int H, int W);
int vqw_conv3x3_wino_fwd_split_padded(const float* x, const void* ws, const float* bias, float* y0, float* y1, int N, int H, int W,
                                      int Cin, int Cout, int split, int c1, int pool0, int relu, void* stream);
/* The input gradient of a layer whose forward read the output of an InstanceNorm (+ReLU) (DoubleConv: conv -> norm -> ReLU ->
 * conv, blocks.py:39-61): y = the gradient as usual, and part[N][parts][Cout][2] = that norm's backward sums per region,
 * (sum gm, sum gm * xhat) with xhat = (norm_x - mean) * rstd and gm = the gradient where the norm's ReLU passed - what
 * vqw_inorm_bwd otherwise reduces in a pass of its own over norm_x and the gradient (vqw_inorm_bwd_parts takes them from here).
 * norm_x: the norm's raw input, shaped like y; norm_mean_rstd: its (mean, rstd) per (image, channel).  parts = 0: not served. */
int vqw_conv3x3_wino_fwd_inbwd_parts(int Cin, int Cout, int N, int H, int W);
int vqw_conv3x3_wino_fwd_inbwd(const float* x, const void* ws, const float* norm_x, const float* norm_mean_rstd, int norm_relu,
                               float* y, float* part, int N, int H, int W, int Cin, int Cout, void* stream);
int vqw_conv3x3_wino_fwd_stats_parts(int Cin, int Cout, int N, int H, int W);
int vqw_conv3x3_wino_fwd_stats(const float* x, const void* ws, const float* bias, float* y, float* part, int N, int H, int W,
                               int Cin, int Cout, void* stream);
/* Gradient of the virtual input: g_full is [N,H,W,Ctot]; takes channels
 * [c_off, c_off+C).  up=1: dst[N,H/2,W/2,C] = 2x2 block sums; up=0: plain slice copy.
 * accumulate=1 adds into dst.                                                      */
int vqw_input_grad_gather(const float* g_full, int Ctot, int c_off, int C, int up,
                          float* dst, int accumulate, int N, int H, int W, void* stream);

/* ---- InstanceNorm2d(affine=False) [+ReLU]: blocks.py:26,46-47,49-50,118-119; aspp.py:25-28 */
size_t vqw_plane_ws_bytes(int N, int C, int HW);
/* y / gy may be a channel slice [c_off, c_off+C) of a wider NHWC tensor with `cstride` channels
 * (cstride == C, c_off == 0 for a plain tensor): the ASPP concat (aspp.py:47) is written in place. */
int vqw_inorm_fwd(const float* x, float* y, int y_cstride, int y_coff, float* mean_rstd /*[N][C][2]*/,
                  void* ws, size_t ws_bytes, int N, int HW, int C, float eps, int relu, void* stream);
/* the same with the statistics taken from the producing convolution's partials (vqw_conv2d_fwd_stats) */
int vqw_inorm_fwd_parts(const float* x, float* y, int y_cstride, int y_coff, float* mean_rstd, const float* part,
                        int nparts, int N, int HW, int C, float eps, int relu, void* stream);
/* statistics only: mean_rstd[N][C][2] by reduction over x, or from a convolution's partials */
int vqw_inorm_stats(const float* x, float* mean_rstd, void* ws, size_t ws_bytes, int N, int HW, int C, float eps, void* stream);
int vqw_inorm_stats_parts(const float* part, int nparts, float* mean_rstd, int N, int HW, int C, float eps, void* stream);
/* Two norms of one shape in one launch (ABI 8; a ResBlock's main and 1x1 branches, blocks.py:21-36). */
int vqw_inorm_stats_parts2(const float* part_a, int nparts_a, float* mean_rstd_a, const float* part_b, int nparts_b,
                           float* mean_rstd_b, int N, int HW, int C, float eps, void* stream);
/* y = a + InstanceNorm(+ReLU)(x) from x's statistics mean_rstd [N][C][2] (ABI 8): the residual add behind a block that ends in
 * that norm (the decoder's tail `x + conv_last(x)`, unet_decoder.py:169-171); the normalised tensor is never written.  The
 * backward is vqw_inorm_bwd on the gradient of y (and the gradient of `a` is that gradient).  C / 4 a power of two <= 256. */
int vqw_inorm_add_supported(int C);
int vqw_inorm_add_fwd(const float* x, const float* mean_rstd, const float* a, float* y, int N, int HW, int C, int relu, void* stream);
int vqw_inorm_bwd(const float* x, const float* mean_rstd, const float* gy, int gy_cstride, int gy_coff,
                  float* gx, void* ws, size_t ws_bytes, int N, int HW, int C, int relu, void* stream);
/* ABI 7.  The same with the two sums taken from part[N][nparts][C][2] = (sum gm, sum gm * xhat) per region, left by the
 * consumer convolution's input-gradient launch (vqw_conv3x3_wino_fwd_inbwd); means_ws: N * C * 2 floats of scratch. */
int vqw_inorm_bwd_parts(const float* x, const float* mean_rstd, const float* gy, const float* part, int nparts, float* means_ws,
                        float* gx, int N, int HW, int C, int relu, void* stream);
/* backward of two InstanceNorms fed with the SAME gradient (the two branches in front of a ResBlock tail; a: norm + ReLU,
 * b: norm): the common gradient is read once per pass.  ws: 2 x vqw_plane_ws_bytes(N, C, HW).  C % 4 == 0.          */
int vqw_inorm_bwd_pair(const float* xa, const float* mra, const float* xb, const float* mrb, const float* gy,
                       float* gxa, float* gxb, void* ws, size_t ws_bytes, int N, int HW, int C, void* stream);
/* vqw_res_tail_bwd followed by vqw_inorm_bwd_pair as one entry point (ABI 8; a ResBlock's tail, blocks.py:29-36): the first
 * kernel forms g = [out > 0] (g_out + the pooled gradient routed to each window's first maximum), stores it in `g` (a workspace
 * tensor shaped like out) and adds it to both norms' backward sums in the same pass; the apply pass reads g once.  g_pooled or
 * g_out may be NULL.  ws as for vqw_inorm_bwd_pair. */
int vqw_res_tail_bwd_pair(const float* out, const float* g_pooled, const float* g_out, const float* xa, const float* mra,
                          const float* xb, const float* mrb, float* g, float* gxa, float* gxb, void* ws, size_t ws_bytes,
                          int N, int H, int W, int C, void* stream);

/* ---- StyledDenorm = BatchNorm2d(affine=False)(x)*(1+gamma)+beta [+ReLU]: blocks.py:82-90,126-132.
 * training=1: batch statistics, running stats updated in place (momentum, unbiased var);
 * training=0: running stats.  stats_io: training fwd receives per-channel
 * [sum, sumsq] partial totals via (sum_out) for cross-rank reduction: see vqw_bn_* below.  */
int vqw_bn_partial_stats(const float* x, double* sums /*[C][2]*/, void* ws, size_t ws_bytes,
                         int N, int HW, int C, void* stream);
/* sums[C][2] from the per-tile partials part[rows = N * parts][C][2] of the producing convolution (vqw_conv2d_fwd_stats):
 * each partial is (sum, M2 = sum (x - tile mean)^2) of one tile of `tile_count` = N*HW / rows pixels */
int vqw_bn_stats_from_parts(const float* part, double* sums /*[C][2]*/, int rows, int C, double tile_count, void* stream);
int vqw_bn_finalize(const double* sums /*[C][2]*/, double count, float* mean_rstd /*[C][2]*/,
                    float* running_mean, float* running_var, float momentum, float eps,
                    int C, void* stream);
/* vqw_bn_stats_from_parts + vqw_bn_finalize in one launch (ABI 8): for a BatchNorm without a collective between its sums and its
 * statistics (one rank, or SyncBN off).  `sums` [C][2] doubles is written as vqw_bn_stats_from_parts writes it. */
int vqw_bn_finalize_parts(const float* part, int rows, double tile_count, double* sums, double count, float* mean_rstd,
                          float* running_mean, float* running_var, float momentum, float eps, int C, void* stream);
int vqw_bn_eval_stats(const float* running_mean, const float* running_var, float* mean_rstd,
                      float eps, int C, void* stream);
/* gamma / beta (and dgamma / dbeta) are addressed as ptr[pixel * gb_stride + c]: gb_stride = C for two dense
 * maps, 2C when mlp_gamma and mlp_beta were evaluated as one conv with concatenated output channels
 * (gamma = gb, beta = gb + C). */
int vqw_spade_fwd(const float* x, const float* mean_rstd /*[C][2]*/, const float* gamma,
                  const float* beta, int gb_stride, float* y, long P, int C, int relu, void* stream);
/* the same with the block's residual added after the activation: y = act(...) + res (blocks.py:134, `shortcut + main`) */
int vqw_spade_fwd_res(const float* x, const float* mean_rstd, const float* gamma, const float* beta, int gb_stride,
                      const float* res, float* y, long P, int C, int relu, void* stream);
/* The same with the residual given RAW together with its InstanceNorm statistics (ABI 8): y = act(spade(x)) +
 * InstanceNorm(+ReLU)(res_raw), res_mean_rstd [N][C][2] - the shortcut branch of a StyledResUpBlock (blocks.py:113-116, 134)
 * normalised while it is read, its normalised tensor never written.  HW a power of two, C / 4 a power of two <= 256. */
int vqw_spade_fwd_res_norm_supported(long HW, int C);
int vqw_spade_fwd_res_norm(const float* x, const float* mean_rstd, const float* gamma, const float* beta, int gb_stride,
                           const float* res_raw, const float* res_mean_rstd, int res_relu, float* y, int N, long HW, int C,
                           int relu, void* stream);
/* backward, phase 1: dgamma, dbeta and per-channel sums [sum dxhat, sum dxhat*xhat] */
int vqw_spade_bwd_reduce(const float* x, const float* mean_rstd, const float* gamma, const float* beta,
                         const float* gy, float* dgamma, float* dbeta, int gb_stride,
                         double* sums /*[C][2]*/, void* ws, size_t ws_bytes, int N, int HW, int C,
                         int relu, void* stream);
/* phase 2: dx (training: sums/count terms; training=0: dx = dxhat*rstd) */
int vqw_spade_bwd_apply(const float* x, const float* mean_rstd, const float* gamma, const float* beta,
                        int gb_stride, const float* gy, const double* sums, double count, float* gx,
                        long P, int C, int relu, int training, void* stream);

/* ---- element-wise / pooling: blocks.py:29-30,34-36 (add, ReLU, MaxPool2d(2)), 134; unet_decoder.py:107,159-163 */
int vqw_add(const float* a, const float* b, float* y, long n, int relu, void* stream);
int vqw_relu_bwd(const float* y, const float* gy, float* gx, long n, void* stream);
int vqw_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int vqw_maxpool2_bwd(const float* x, const float* gy, const float* g_skip /*nullable*/, float* gx,
                     int N, int H, int W, int C, void* stream);
/* ResBlock tail (blocks.py:29-36: out = ReLU(a + b); pooled = MaxPool2d(2)(out)), forward and backward in one pass each:
 * gx = [out > 0] * (g_out + g_pooled routed to each 2x2 window's arg-max) = d/da = d/db.  Either gradient may be
 * NULL (that output unused).  H, W even, C % 4 == 0, 16-byte aligned tensors.                                  */
int vqw_res_tail_fwd(const float* a, const float* b, float* out, float* pooled, int N, int H, int W, int C, void* stream);
/* the tail reading the RAW outputs of the block's two conv branches and their InstanceNorm statistics (mean, rstd per
 * (n, c)): a = ReLU(IN(x2)), b = IN(xid), out = ReLU(a + b) — the two normalisation apply passes disappear.       */
int vqw_res_tail_norm_fwd(const float* x2, const float* mr2, const float* xid, const float* mrid, float* out, float* pooled,
                          int N, int H, int W, int C, void* stream);
int vqw_res_tail_bwd(const float* out, const float* g_pooled /*nullable*/, const float* g_out /*nullable*/, float* gx,
                     int N, int H, int W, int C, void* stream);
int vqw_tanh_fwd(const float* x, float* y, long n, void* stream);
int vqw_tanh_bwd(const float* y, const float* gy, float* gx, long n, void* stream);
int vqw_affine(const float* x, float* y, float scale, float shift, long n, void* stream); /* utils norm/denorm */
int vqw_mse_fwd(const float* a, const float* b, float* loss, void* ws, size_t ws_bytes, long n, void* stream);
int vqw_mse_bwd(const float* a, const float* b, const float* gloss, float* ga, long n, void* stream);
size_t vqw_reduce_ws_bytes(long n);
int vqw_weighted_sum(const float* const* terms_dev /*device array of ptrs*/, const float* weights_dev,
                     int n_terms, float* out, void* stream);
/* the same with HOST arrays of (device) term pointers and weights, passed to the kernel by value: 1..16 terms, no
 * host-to-device copy */
int vqw_weighted_sum_host(const float* const* terms /*host array of device ptrs*/, const float* weights /*host*/,
                          int n_terms, float* out, void* stream);

/* ---- vector quantisation: networks/vq/vq_module.py:45-62,159-211; grad_approximation.py:7-29 */
size_t vqw_vq_ws_bytes(long Npix, int D, int K);
/* which search / statistics route (D, K) takes: 0 = codebook in LDS + matrix-core statistics, 1 = codebook in LDS +
 * sorted statistics, 2 = fused MFMA score GEMM / arg-max + sorted statistics, 3 = generic scalar + sorted statistics */
int vqw_vq_plan(int D, int K);
/* x [Npix][D] (NHWC rows), embed [K][D].  Outputs: ids int64 [Npix], q [Npix][D],
 * commit = mean((x-q)^2); when stats != NULL also counts[K] and embed_sum[D][K]
 * (layout of the reference's embed_avg) as double in `stats` = [K + D*K].
 * ids are written as code + id_base (unet_encoder.py:116 adds 1).                   */
int vqw_vq_fwd(const float* x, const float* embed, int64_t* ids, int id_base, float* q, float* commit,
               double* stats, void* ws, size_t ws_bytes, long Npix, int D, int K, void* stream);
/* EMA + Laplace-smoothed normalisation (vq_module.py:195-200), in place on the buffers.
 * sum_scale multiplies embed_sum before the EMA (1/world_size in the reference's quirk mode). */
int vqw_vq_ema_update(const double* stats, float* embed, float* cluster_size, float* embed_avg,
                      float momentum, float eps, float sum_scale, int D, int K, void* stream);
/* The same with the weight of the new statistics given: vqw_vq_ema_update uses 1.f - momentum formed in float32; the reference's
 * add_(update, alpha=1 - momentum) rounds the double once, which is what a caller passes here to follow it to the last bit
 * of that weight (9.5e-7 apart at momentum 0.99). */
int vqw_vq_ema_update_w(const double* stats, float* embed, float* cluster_size, float* embed_avg, float momentum,
                        float new_weight, float eps, float sum_scale, int D, int K, void* stream);
/* One Lloyd iteration of the k-means codebook initialisation (unet_encoder.py:66-91): centres[k] <- mean of its members
 * from the statistics vqw_vq_fwd leaves (codes without members keep their centre).  shift[0] = sum_k |delta_k|_2,
 * shift[1] = number of empty codes.  ws: 16 K bytes. */
int vqw_kmeans_update(const double* stats, float* centres, double* shift, void* ws, size_t ws_bytes, int D, int K,
                      void* stream);
int vqw_vq_lookup(const int64_t* ids, const float* embed, const uint8_t* mask /*nullable*/,
                  const float* scale_dev /*nullable, 1 float*/, float* out, long Npix, int D, int K,
                  void* stream);
/* gx = g_q (straight-through) + g_commit * 2 (x - q) / numel */
int vqw_vq_bwd(const float* x, const float* q, const float* g_q, const float* g_commit,
               float* gx, long numel, void* stream);
/* mask count -> scale = numel / count (run_recon.py:191-192) */
int vqw_mask_scale(const int64_t* label_map, uint8_t* mask, int64_t* ids0, float* scale_dev,
                   long n, void* stream);

/* ---- losses: functions/embed_loss.py:22-88, functions/onehot.py:11-20 */
size_t vqw_cross_ws_bytes(int B, int K, long HW);
/* labels int32 [B][HW] in [0,K] (0 = out of frame); embed [B][HW][D]; codebook [K][D] (= vq.embed).
 * loss = mean over present (b,k) of sum_p |e-c_k|^2 / (cnt+1e-6); coef[B][K] saved for backward.
 * Both forward entry points (this one and the dense one) accept K <= 5120 and reject anything larger in their argument check:
 * the partial sums live in 32 K bytes of LDS per workgroup (160 KiB at most; the opt-in above 64 KiB is taken here). */
int vqw_cross_loss_fwd(const float* embed, const int32_t* labels, const float* codebook_kd,
                       float* loss, float* coef, void* ws, size_t ws_bytes,
                       int B, long HW, int D, int K, void* stream);
int vqw_cross_loss_bwd(const float* embed, const int32_t* labels, const float* codebook_kd,
                       const float* coef, const float* gloss, float* gembed,
                       int B, long HW, int D, int K, void* stream);
/* general (soft / one-hot float r[B][K][HW] NCHW as the reference passes it) */
int vqw_cross_loss_dense_fwd(const float* embed, const float* r_nchw, const float* codebook_kd,
                             float* loss, float* coef, void* ws, size_t ws_bytes,
                             int B, long HW, int D, int K, void* stream);
int vqw_cross_loss_dense_bwd(const float* embed, const float* r_nchw, const float* codebook_kd,
                             const float* coef, const float* gloss, float* gembed,
                             int B, long HW, int D, int K, void* stream);
/* l_dist / l_reg of embed_loss.py:68-88 (no gradient: the codebook is a buffer); ws: 16 K bytes */
int vqw_codebook_losses(const float* codebook_kd, float margin, float* l_dist, float* l_reg,
                        void* ws, size_t ws_bytes, int D, int K, void* stream);
int vqw_onehot(const int32_t* labels, float* out_nchw, int B, long HW, int n_classes, void* stream);
int vqw_flip_labels(const int64_t* ids, int32_t* out, int border, int B, int H, int W, void* stream);

/* ---- optional paths
 * PixelShuffle(2) in NHWC (blocks.py:100-104): (H, W, C) are the high-resolution output dims; inverse=1 is the backward. */
int vqw_pixel_shuffle2(const float* src, float* dst, int N, int H, int W, int C, int inverse, void* stream);
/* DropBlock (dropblock.py:47-94): keep = 1 - dilate(seed), scale = numel/sum(keep); apply is also its own backward. */
int vqw_dropblock_mask(const float* seed, float* keep, float* scale_dev, int N, int H, int W, int block_size, void* stream);
int vqw_dropblock_apply(const float* x, const float* keep, const float* scale_dev, float* y, long P, int C, void* stream);
/* SoftDice + Focal (functions/seg_loss.py:15-62) on NCHW logits / one-hot targets, C <= 64: loss_out = {dice, focal}. */
size_t vqw_seg_ws_bytes(int C);
int vqw_seg_losses_fwd(const float* logits_nchw, const float* target_nchw, float* loss_out, double* sums, void* ws,
                       size_t ws_bytes, int B, long HW, int C, int ignore_index, float smooth, float gamma, float eps,
                       void* stream);
int vqw_seg_losses_bwd(const float* logits_nchw, const float* target_nchw, const double* sums, const float* g_dice,
                       const float* g_focal, float* glogits, int B, long HW, int C, int ignore_index, float smooth,
                       float gamma, float eps, void* stream);

/* ---- two-view augmentation + id-map warps (networks/random_transform.py:10-112; used at
 * single_window_trainer.py:75-76, 91-96).  The reference builds these from kornia 0.5.1, which is not available
 * offline: the arithmetic is the one oracle/augment_ref.py states (parity unpinned).  Matrices are per-sample 3x3,
 * row-major, mapping a DESTINATION pixel (x, y, 1) to the SOURCE pixel; pixel centres sit on integer coordinates.
 * warp_image: bilinear, zero padding, (B, C, H, W) planes.  warp_labels: nearest (round half to even), 0 = out of frame.
 * photometric params per sample {brightness add, contrast multiplier, posterize bits (8 = off), noise std}: clamp(x+b),
 * clamp(x*c), posterize, + std * noise (noise may be NULL).  gauss_blur: separable, reflect border, apply[b] on/off. */
int vqw_warp_image(const float* src, const float* minv /*[B][9]*/, float* dst, int B, int C, int H, int W, void* stream);
int vqw_warp_labels(const void* ids, int ids_are_int64, const float* minv /*[B][9]*/, int32_t* out, int B, int H, int W,
                    void* stream);
int vqw_photometric(const float* x, const float* params /*[B][4]*/, const float* noise, float* y, int B, long per_sample,
                    void* stream);
int vqw_gauss_blur(const float* x, const float* taps /*[K]*/, const unsigned char* apply /*[B] or NULL*/, float* tmp, float* y,
                   int B, int C, int H, int W, int K, void* stream);

/* ---- second training step: PatchGAN discriminator + GAN losses (networks/discriminator.py:18-87,
 * functions/gan_loss.py:6-10, trainers/single_window_trainer.py:434-488).  NHWC activations, OHWI weights
 * [Cout][k][k][Cin]; output size floor((H + 2 pad - k) / stride) + 1; stride 1 or 2; H, W are INPUT dims.
 * sconv_fwd applies LeakyReLU(slope) in the epilogue (slope = 1: none). */
size_t vqw_sconv_fwd_ws_bytes(int N, int H, int W, int Cin, int Cout, int ks, int stride, int pad);
int vqw_sconv_fwd(const float* x, const float* w_ohwi, const float* bias, float* y, void* ws, size_t ws_bytes, int N, int H,
                  int W, int Cin, int Cout, int ks, int stride, int pad, float slope, void* stream);
size_t vqw_sconv_dgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int ks, int stride, int pad);
int vqw_sconv_dgrad(const float* gy, const float* w_ohwi, float* gx, void* ws, size_t ws_bytes, int N, int H, int W, int Cin,
                    int Cout, int ks, int stride, int pad, void* stream);
size_t vqw_sconv_wgrad_ws_bytes(int Cin, int Cout, int ks, int N, int H, int W, int stride, int pad);
int vqw_sconv_wgrad(const float* x, const float* gy, float* dw_ohwi, float* dbias, void* ws, size_t ws_bytes, int N, int H,
                    int W, int Cin, int Cout, int ks, int stride, int pad, int accumulate, void* stream);
int vqw_leaky_relu_bwd(const float* y, const float* gy, float* gx, float slope, long n, void* stream);
/* 3x3 stride-2 convolution behind a zero pad of one pixel at the bottom and right only (the VQGAN `Downsample`, vqgan.py:40-58:
 * F.pad(x, (0, 1, 0, 1)) then Conv2d(C, C, 3, 2, 0)): y[n][yo][xo][co] = bias + sum w[co][ky][kx][ci] x[n][2 yo + ky][2 xo + kx][ci].
 * x [N][H][W][Cin], y / gy [N][H/2][W/2][Cout], OHWI weights; H, W (the INPUT dims) even, Cin and Cout multiples of 32, every
 * tensor below 4 GiB: anything else is refused.  Exact-fp32 matrix cores, nine taps on each pass: the input gradient multiplies
 * 4 / 2 / 2 / 1 taps by output parity.  The weight gradient sums its split partials in a fixed order (no atomics); dbias may be
 * NULL; accumulate: dw_ohwi (and dbias) += the result. */
int vqw_conv3s2_fwd(const float* x, const float* w_ohwi, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                    void* stream);
size_t vqw_conv3s2_dgrad_ws_bytes(int Cin, int Cout);
int vqw_conv3s2_dgrad(const float* gy, const float* w_ohwi, float* gx, void* ws, size_t ws_bytes, int N, int H, int W, int Cin,
                      int Cout, void* stream);
size_t vqw_conv3s2_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout);
int vqw_conv3s2_wgrad(const float* x, const float* gy, float* dw_ohwi, float* dbias, void* ws, size_t ws_bytes, int N, int H,
                      int W, int Cin, int Cout, int accumulate, void* stream);
/* BatchNorm2d(affine) + LeakyReLU: y = lrelu(((x - mean) * rstd) * gamma + beta); statistics through
 * vqw_bn_partial_stats / vqw_bn_finalize.  bwd_reduce: sums[C][2] = {sum g', sum g' * xhat} (dbeta, dgamma);
 * bwd_apply: dx, and dgamma / dbeta (may be NULL) written or accumulated. */
int vqw_bn_affine_fwd(const float* x, const float* mean_rstd, const float* gamma, const float* beta, float* y, long P, int C,
                      float slope, void* stream);
int vqw_bn_affine_bwd_reduce(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* gy,
                             double* sums, void* ws, size_t ws_bytes, int N, int HW, int C, float slope, void* stream);
int vqw_bn_affine_bwd_apply(const float* x, const float* mean_rstd, const float* gamma, const float* beta, const float* gy,
                            const double* sums, double count, float* gx, float* dgamma, float* dbeta, long P, int C,
                            float slope, int training, int accumulate, void* stream);
/* mode 0: mean(relu(1 - x)), 1: mean(relu(1 + x)) (hinge_d_loss halves), 2: -mean(x) (generator loss) */
int vqw_hinge_fwd(const float* x, long n, int mode, float* loss, void* stream);
int vqw_hinge_bwd(const float* x, long n, int mode, const float* gloss, float* gx, void* stream);

/* ---- ActNorm and spectral normalisation of the discriminator (networks/actnorm.py:23-70, utils/__init__.py:54-64 =
 * torch.nn.utils.spectral_norm defaults: one power iteration, eps 1e-12, dim 0).
 * ActNorm runs on the vqw_bn_affine_* kernels with mean = -loc, rstd = 1, gamma = scale, beta = 0: vqw_actnorm_prepare writes
 * mean_rstd_beta = [C][2] {-loc, 1} followed by [C] zeros; with `sums` ([C][2] doubles of vqw_actnorm_stats over `count`
 * pixels, the first training forward) it first sets loc = -mean, scale = 1 / (unbiased std + 1e-6) and initialized[0] = 1.
 * vqw_actnorm_stats: sums[c] = {sum x, sum x^2} over the P pixels of an NHWC tensor with every square and addition in double
 * (ActNorm divides by the std itself: the fp32 squares of vqw_bn_partial_stats are not exact enough for it).
 * vqw_actnorm_loc_grad: dloc = scale * dbeta. */
int vqw_actnorm_stats(const float* x, double* sums /*[C][2]*/, long P, int C, void* stream);
int vqw_actnorm_prepare(const double* sums /*[C][2] or NULL*/, double count, float* loc, float* scale,
                        unsigned char* initialized /*[1] or NULL*/, float* mean_rstd_beta /*[3C]*/, int C, void* stream);
int vqw_actnorm_loc_grad(const float* dbeta, const float* scale, float* dloc, int C, void* stream);
/* All spectrally normalised weights of one forward in three launches (two in eval mode).  layers_dev: n_layers records of 16
 * int64 {W, u, v, out, save, t, s, rows, K, Cin, blk1, blk2, blk3, sv, 0, 0}: W / out [rows][K] in OHWI memory order
 * (K = k*k*Cin), u [rows] and v [K] the module buffers (v in torch's logical (Cin, k, k) order), save [rows + K + 1] receives this
 * forward's u, v (memory order) and sigma for its backward, t [K] and s [rows] scratch.  blkP = first workgroup of the layer in
 * phase P: phase 1 has ceil(K / 64) workgroups per layer, phase 2 `rows`, phase 3 ceil(rows * K / 4096); blocksP their totals.
 * training: v <- normalize(W^T u), u <- normalize(W v) in place first; eval: the stored u, v.  out = W / (u^T W v).
 * sv (0 = none): one float that receives sigma in training - BigGAN's SN (networks/biggan/layers.py:25-94: buffers u0, sv0, no
 * stored v) is this training arithmetic with `v` a scratch array; its eval forward iterates too, on a copy of u0.
 * vqw_spectral_norm_bwd: records of 8 int64 {G, weight, save, gW, part, rows, K, blk}: gW = (G - <G, weight> u v^T) / sigma with
 * part [ceil(rows * K / 4096)] doubles of scratch per layer, blk = first workgroup, `blocks` their total; two launches. */
int vqw_spectral_norm_fwd(const void* layers_dev, int n_layers, int blocks1, int blocks2, int blocks3, int training, float eps,
                          void* stream);
int vqw_spectral_norm_bwd(const void* grads_dev, int n_layers, int blocks, void* stream);

/* ---- U-Net discriminator (networks/unet_discriminator.py:386-627, BigGAN blocks networks/biggan/layers.py:416-506) and its
 *      second training step (trainers/single_window_trainer.py:264-432).  Added functions only; the ABI stays 9.
 * Down-block tail: out [N,H/2,W/2,C] = avgpool2(a) (+ s_low), relu_out = relu(out).  s_low and either output may be NULL.
 * Backward: g = g_out + g_relu * [relu_out > 0] (either gradient NULL), g_full = g / 4 at the four positions of each window
 * (d/da), g_low = g (d/ds_low); either may be NULL.  H, W even. */
int vqw_unet_dtail_fwd(const float* a, const float* s_low, float* out, float* relu_out, int N, int H, int W, int C, void* stream);
int vqw_unet_dtail_bwd(const float* relu_out, const float* g_out, const float* g_relu, float* g_full, float* g_low, int N, int H,
                       int W, int C, void* stream);
/* Up-block tail: out [N,H,W,C] = h + up2x(s_low [N,H/2,W/2,C]); cat [N,H,W,C+Cr] = [relu(out) | relu(res [N,H,W,Cr])] (channel
 * concat; Cr = 0: no residual): the rectified concat input of the next up block.  out or cat may be NULL.  Backward:
 * g = g_out + g_cat[.., :C] * [cat[.., :C] > 0]; g_h = g, g_s_low = the sum of g over each 2x2 window, g_res = g_cat[.., C:] *
 * [cat[.., C:] > 0] (NULL: not wanted). */
int vqw_unet_utail_fwd(const float* h, const float* s_low, const float* res, float* out, float* cat, int N, int H, int W, int C,
                       int Cr, void* stream);
int vqw_unet_utail_bwd(const float* cat, const float* g_out, const float* g_cat, float* g_h, float* g_s_low, float* g_res, int N,
                       int H, int W, int C, int Cr, void* stream);
/* Bottleneck head: y[n] = bias + sum_c w[c] * sum_p relu(h[n, p, c]), h [N][HW][C]; backward g_h = gy[n] w[c] [h > 0],
 * g_w[c] = sum_n gy[n] sum_p relu(h), g_bias = sum_n gy[n] (each may be NULL). */
int vqw_unet_head_fwd(const float* h, const float* w, const float* bias, float* y, int N, int HW, int C, void* stream);
int vqw_unet_head_bwd(const float* h, const float* w, const float* gy, float* g_h, float* g_w, float* g_bias, int N, int HW, int C,
                      void* stream);
/* CutMix (utils/__init__.py:208-218 with mask = 1 outside the rectangle [y0, y1) x [x0, x1), 0 inside; flip: 1 - mask):
 * out = image where the mask is 1, recon where it is 0.  [N,H,W,C]. */
int vqw_cutmix_select(const float* image, const float* recon, float* out, int N, int H, int W, int C, int y0, int y1, int x0, int x1,
                      int flip, void* stream);
/* The discriminator half's three losses in one pass over the maps [B,H,W] and bottlenecks [B], the mask given by the rectangle:
 *   l_dis = hinge_d_loss(r_map, f_map) + hinge_d_loss(r_bottle, f_bottle)          (gan_loss.py:6-10)
 *   l_cutmix = mean(relu(1 + c_bottle)) + mean(relu(1 - (2 mask - 1) c_map))
 *   l_consistency = mean((c_map - (mask r_map + (1 - mask) f_map))^2)
 * Backward: all six gradients from dL/d(l_dis, l_cutmix, l_consistency) (device scalars; NULL = 0). */
size_t vqw_unet_dis_losses_ws_bytes(long n);
int vqw_unet_dis_losses_fwd(const float* r_map, const float* f_map, const float* c_map, const float* r_bottle, const float* f_bottle,
                            const float* c_bottle, float* l_dis, float* l_cutmix, float* l_consistency, void* ws, size_t ws_bytes,
                            int B, int H, int W, int y0, int y1, int x0, int x1, int flip, void* stream);
int vqw_unet_dis_losses_bwd(const float* r_map, const float* f_map, const float* c_map, const float* r_bottle, const float* f_bottle,
                            const float* c_bottle, const float* g_dis, const float* g_cutmix, const float* g_consistency,
                            float* g_r_map, float* g_f_map, float* g_c_map, float* g_r_bottle, float* g_f_bottle, float* g_c_bottle,
                            int B, int H, int W, int y0, int y1, int x0, int x1, int flip, void* stream);

/* ---- multi-window reconstruction loss (trainers/multi_window_trainer.py:93-109, base.py:290-314):
 * mean((w(a) - w(b))^2) with w(x) = clamp(alpha * x + beta, lo, hi); gradient w.r.t. a (zero where clamped). */
int vqw_window_mse_fwd(const float* a, const float* b, float* loss, void* ws, size_t ws_bytes, long n, float alpha,
                       float beta, float lo, float hi, void* stream);
int vqw_window_mse_bwd(const float* a, const float* b, const float* gloss, float* ga, long n, float alpha, float beta,
                       float lo, float hi, void* stream);

/* ---- window stack (trainers/multi_window_trainer.py:226-227): 1 <= nwin <= 3 re-windowed copies of x[n] from one read,
 * o_w = clamp(alpha_w * x + beta_w, lo_w, hi_w) (one fma, one clamp) with win = the [nwin][4] DEVICE table of
 * (alpha, beta, lo, hi) rows; a NULL o_w is skipped.  Backward: gx = sum over w, in window order, of
 * g_w * (alpha_w where lo_w < alpha_w * x + beta_w < hi_w, else 0) (the vqw_window_mse_bwd convention); a NULL g_w
 * contributes nothing and with all of them NULL gx is zero.  Pointers past nwin are ignored. */
int vqw_window_stack_fwd(const float* x, const float* win, float* o0, float* o1, float* o2, int nwin, long n, void* stream);
int vqw_window_stack_bwd(const float* x, const float* win, const float* g0, const float* g1, const float* g2, float* gx, int nwin,
                         long n, void* stream);

/* ---- focal frequency loss (ABI 9; the focal-frequency-loss package v0.3.0 as FFL(loss_weight, alpha) in
 *      trainers/base.py:277-278, single_window_trainer.py:117-136, 286-309, 453-466, multi_window_trainer.py:100-126).
 * pred, target: [N,H,W,C] cut into patch_factor^2 patches of h x w = H/pf x W/pf; per plane (n, patch, c)
 * D = fft2(win(pred) - win(target), ortho), loss = loss_weight * mean(w |D|^2) with w = |D|^alpha (log(. + 1) with
 * log_matrix) over its max per plane (over everything with batch_matrix), NaN -> 0.  win(x) = clamp(win_alpha * x +
 * win_beta, win_lo, win_hi) when `windowed`, else the identity.  tw_h / tw_w: the twiddle tables of sides h and w
 * ([n][2], vqw_freq_twiddles; built once per side and device).  The forward leaves D and the folded maxima in `ws`: the
 * backward reads them from the same buffer (and uses the rest as scratch).  gpred = dL/dpred, gtarget = dL/dtarget
 * (either may be NULL; zero where the window clamps). */
size_t vqw_freq_loss_ws_bytes(int N, int C, int H, int W, int patch_factor);
int vqw_freq_twiddles(float* tw, int n, void* stream);
int vqw_freq_loss_fwd(const float* pred, const float* target, const float* tw_h, const float* tw_w, float* loss, void* ws,
                      size_t ws_bytes, int N, int C, int H, int W, int patch_factor, float alpha, int log_matrix,
                      int batch_matrix, float loss_weight, int windowed, float win_alpha, float win_beta, float win_lo,
                      float win_hi, void* stream);
int vqw_freq_loss_bwd(const float* pred, const float* target, const float* tw_h, const float* tw_w, const float* gloss,
                      float* gpred, float* gtarget, void* ws, size_t ws_bytes, int N, int C, int H, int W, int patch_factor,
                      float alpha, int log_matrix, float loss_weight, int windowed, float win_alpha, float win_beta,
                      float win_lo, float win_hi, void* stream);

/* ---- test-mode evaluation metrics (the reference's _test_step, single_window_trainer.py:781-827: torchmetrics 0.6.2
 *      MeanSquaredError / StructuralSimilarityIndexMeasure / PeakSignalNoiseRatio with data_range=None, and
 *      scipy.stats.entropy(bincount(ids, minlength=K+1)[1:], base=2)).  Added functions only; the ABI stays 9.
 * pred, target: N*C planes of H x W, dense (C = 1: NCHW and NHWC coincide).  ksize: the SSIM window (odd, <= 15; 0 skips
 * the SSIM pass); data_range > 0 replaces both the SSIM range max(range p, range t) and the zero-seeded PSNR range
 * max(max t, 0) - min(min t, 0).  ids: n_ids codes (either may be NULL: pred/target = NULL computes the entropy alone,
 * ids = NULL the image metrics alone).  out[16] (double): mse, ssim, psnr, SSIM range, PSNR range, SSE, min t, max t,
 * entropy (bits, over bins 1..K), the number of ids outside [0, K], the number of ids; NaN for what was not computed.
 * counts (optional): [K + 1] int64 counts of ids 0..K.  At most four launches, no host synchronisation. */
size_t vqw_recon_metrics_ws_bytes(int N, int C, int H, int W, int K);
int vqw_recon_metrics(const float* pred, const float* target, const int64_t* ids, double* out, int64_t* counts, void* ws,
                      size_t ws_bytes, int N, int C, int H, int W, long n_ids, int K, int ksize, float sigma, float k1,
                      float k2, float data_range, void* stream);
int vqw_code_entropy(const int64_t* ids, double* out, int64_t* counts, void* ws, size_t ws_bytes, long n, int K, void* stream);

/* ---- VGG perceptual loss (the reference's VGGLoss(conv_index='22') = vgg19.features[:8], functions/perceptual_loss.py,
 *      trainers/base.py:271-275, single_window_trainer.py:124-137, 458-467, multi_window_trainer.py:54, 101-119).
 *      Added functions only; the ABI stays 9.
 * One batch of 2M = 2 * nwin * N images: the sr half [nwin][N] first, then the hr half [nwin][N].  The stem, conv1_2 (direct
 * form: vqw_conv2d_fwd), the max-pool (vqw_maxpool2_fwd) and conv2_1 run on the whole batch; conv2_2 runs once on the
 * difference of the two halves (its output is taken before its ReLU, so the bias cancels); the backward is the existing
 * input-gradient convolutions on the sr half and the stem's input gradient below.
 * sr, hr: [N,H,W,Cin], Cin = 1 (w = the stem weight summed over its 3 input channels, [64][3][3][1]) or 3 (w = the stem
 * weight [64][3][3][3]).  win: NULL (no window, nwin = 1) or [nwin][4] device floats (alpha, beta, lo, hi) of
 * x -> clamp(alpha x + beta, lo, hi) per window (alpha 1, beta 0, lo -inf, hi inf: none).  a1: [2M,H,W,64] = relu(stem).
 * ..._supported: 0 when a shape is not served (Cin not 1 or 3, H or W below 2). */
int vqw_percep_supported(int N, int Cin, int H, int W);
int vqw_percep_stem_fwd(const float* sr, const float* hr, const float* w, const float* bias, const float* win, float* a1,
                        int N, int nwin, int Cin, int H, int W, void* stream);
/* d[i] = a2[i] - a2[n + i], i < n (the sr half minus the hr half; n % 4 == 0) */
int vqw_percep_diff(const float* a2, float* d, long n, void* stream);
/* loss[w] = sum over y[w * per_window .. (w + 1) * per_window) of y^2 / per_window, w < nwin: a fixed-order fold */
size_t vqw_percep_loss_ws_bytes(int nwin);
int vqw_percep_loss_fwd(const float* y, float* loss, void* ws, size_t ws_bytes, int nwin, long per_window, void* stream);
/* gsr = sum_w 2 g_w / numel * win_w'(sr) * conv3x3^T(dz1[w], w): the stem's input gradient.  dz1: [nwin * N,H,W,64], the
 * gradient in front of the stem's ReLU (sr half); g0 .. g2: the incoming gradient of each window's loss (device scalars;
 * unused ones may be NULL); numel = N * 128 * (H/2) * (W/2).  win' = alpha where alpha sr + beta lies strictly inside
 * (lo, hi), else 0 (the vqw_window_mse_bwd convention). */
int vqw_percep_stem_bwd(const float* sr, const float* w, const float* win, const float* g0, const float* g1, const float* g2,
                        const float* dz1, float* gsr, int N, int nwin, int Cin, int H, int W, long numel, void* stream);

/* ---- LPIPS perceptual loss, lpips.LPIPS(net='alex') v0.1 with its defaults (the reference's LPIPSLoss,
 *      functions/lpips_loss.py, trainers/base.py:271-275).  Added functions only; the ABI stays 9.
 * One batch of 2M = 2 * nwin * N images as for the VGG loss: the sr half [nwin][N] first, then the hr half.  Front end:
 * scaling layer + conv 11x11/4 pad 2 (3 -> 64) + ReLU [tap 0]; max-pool 3/2; conv 5x5 pad 2 (64 -> 192) + ReLU [tap 1];
 * max-pool 3/2; three 3x3 layers (192 -> 384 -> 256 -> 256, each + ReLU) [taps 2..4] on the stock 3x3 entry points.  All
 * tensors NHWC fp32; every sum has one fixed order (bit-deterministic; equal neighbourhoods give bit-equal outputs).
 * ..._supported: 0 when a shape is not served (Cin not 1 or 3, H or W below 31: the second pool needs a 3-wide map).
 * stem: wp = [planes][121][64] weights (tap = ky * 11 + kx).  Cin = 3: the three input channels' weights, and
 * sc = shift[3], scale[3] of the scaling layer (x - shift) / scale, applied on load with zero padding after it.  Cin = 1
 * (expand() feeds one value to all three): planes (wA, wB) = (sum_c w_c / scale_c, -sum_c w_c shift_c / scale_c), wB
 * counting for in-bounds taps only, and cint[64] = wB summed over the 121 taps in tap order in fp32 (what the kernel's own
 * sum gives where every tap is in bounds).  win: as in vqw_percep_stem_fwd.  f1: [2M,Ho,Wo,64], Ho = (H - 7) / 4 + 1. */
int vqw_lpips_supported(int N, int Cin, int H, int W);
int vqw_lpips_stem_fwd(const float* sr, const float* hr, const float* wp, const float* cint, const float* sc, const float* bias,
                       const float* win, float* f1, int N, int nwin, int Cin, int H, int W, void* stream);
/* gsr = sum_w g_w * win_w'(sr) / scale * conv11x11/4^T(dz1[w], wp): the stem's input gradient.  dz1: [nwin * N,Ho,Wo,64], the
 * gradient in front of the stem's ReLU (sr half) for a unit loss gradient; g0 .. g2: the incoming gradient of each window's
 * loss (device scalars; unused ones may be NULL).  win' as in vqw_percep_stem_bwd. */
int vqw_lpips_stem_bwd(const float* sr, const float* wp, const float* sc, const float* win, const float* g0, const float* g1,
                       const float* g2, const float* dz1, float* gsr, int N, int nwin, int Cin, int H, int W, void* stream);
/* MaxPool2d(3, stride 2), floor mode: y [N,(H-3)/2+1,(W-3)/2+1,C], C % 4 == 0.  Backward as a gather: gx = [x > 0] * the
 * gradients of the windows whose first row-major maximum (ATen's rule) the pixel is (x = the ReLU output that was pooled). */
int vqw_lpips_pool_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int vqw_lpips_pool_bwd(const float* x, const float* gy, float* gx, int N, int H, int W, int C, void* stream);
/* 5x5 padding-2 convolution (+ bias, ReLU with relu = 1) on the implicit-GEMM matrix-core kernel; w_ohwi [Cout][5][5][Cin].
 * The input gradient is the same call on dY with vqw_pack_dgrad_weights(.., 5) weights, Cin / Cout swapped. */
int vqw_lpips_conv5_supported(int Cin, int Cout, int N, int H, int W);
int vqw_lpips_conv5_fwd(const float* x, const float* w_ohwi, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                        int relu, void* stream);
/* Tap distance.  f: [2M,HW,C] (C in 64, 192, 384, 256), lw: [C] lin weights.  Per pixel a = f / (|f| + 1e-10), b likewise
 * from the hr half, d = sum_c lw_c (a_c - b_c)^2; ..._dist_fwd leaves tap `tap`'s double partials per image in ws, and
 * ..._loss_fold (after all five taps) loss[w] = sum_tap sum_n mean_pixels d / N, hw0 .. hw4 = the taps' pixel counts.
 * ..._dist_bwd: gout = [f > 0] * (gin + d(mean d_tap / N)/df) for a unit loss gradient on the sr half [M,HW,C]; the distance
 * term is zero at a pixel whose features are all zero; gin: the gradient from the deeper tap, NULL at the last, may be gout. */
size_t vqw_lpips_ws_bytes(int N, int nwin);
int vqw_lpips_dist_fwd(const float* f, const float* lw, void* ws, size_t ws_bytes, int tap, int N, int nwin, int HW, int C,
                       void* stream);
int vqw_lpips_loss_fold(const void* ws, size_t ws_bytes, float* loss, int N, int nwin, int hw0, int hw1, int hw2, int hw3,
                        int hw4, void* stream);
int vqw_lpips_dist_bwd(const float* f, const float* lw, const float* gin, float* gout, int N, int nwin, int HW, int C,
                       void* stream);

/* ---- 8-bit export (the validation mosaic, the inference export and test-mode pictures: what the reference's to_image /
 *      save_image do on the host, single_window_trainer.py:563-638, 716-779).  Added functions only; the ABI stays 9.
 * The kernels read every input element once (vqw_export_grey_auto: twice), take B * H * W < 2^31 and B <= 65535, and flip rows
 * top to bottom with flip = 1.
 * vqw_export_grey: x [B][H][W] float (a (B,1,H,W) tensor in either memory format), win [nwin][6] device floats
 * (alpha, beta, lo, hi, vmin, vmax - vmin), nwin <= 8; out [nwin][B][H][W] bytes,
 *   u8 = min(255, floor(256 * clamp((clamp(alpha * x + beta, lo, hi) - vmin) / (vmax - vmin), 0, 1)))
 * with one float32 rounding per operation (no fused multiply-add).  alpha 1, beta 0, lo -inf, hi inf: no window.
 * vqw_export_labels: ids [B][H][W] in [0, K], K <= 65535.  index_out (nullable): [B][H][W] uint8 when K <= 255, else uint16;
 * rgb (nullable): [B][H][W][3] bytes = palette[id], palette [K + 1][3] bytes (held in LDS up to 4096 entries); counts
 * (nullable): [B][K + 1] int32, exact integer atomics; err [1]: set to 1 when an id lies outside [0, K] (it exports as 0 and is
 * not counted), else 0.  counts and err are cleared by the call. */
int vqw_export_grey(const float* x, const float* win, uint8_t* out, int nwin, int B, int H, int W, int flip, void* stream);
int vqw_export_labels(const int64_t* ids, const uint8_t* palette, void* index_out, uint8_t* rgb, int32_t* counts, int32_t* err,
                      int B, int H, int W, int K, int flip, void* stream);
/* vqw_export_grey_auto: every image through its own range (what matplotlib's imshow does with vmin = vmax = None: the
 * discriminator maps of the VQGAN trainer's validation picture).  x [B][H][W] float, out [B][H][W] bytes,
 *   u8 = min(255, floor(256 * clamp((x - vmin_b) / (vmax_b - vmin_b), 0, 1)))
 * with vmin_b / vmax_b the minimum / maximum over the FINITE values of image b, one float32 rounding per operation.  A
 * non-finite value exports as 0, and so does every pixel of a constant image and of an image without a finite value.
 * range (nullable): [B][2] = (vmin_b, vmax_b); (+inf, -inf) for an image without a finite value.  Two passes: per-workgroup
 * partial minima / maxima into ws (vqw_export_auto_ws_bytes(B) bytes), then each workgroup of the export pass folds its image's
 * partials: x is read twice, out written once, no floating-point atomics.  Same limits and flip as vqw_export_grey. */
size_t vqw_export_auto_ws_bytes(int B);
int vqw_export_grey_auto(const float* x, uint8_t* out, float* range, float* ws, size_t ws_bytes, int B, int H, int W, int flip,
                         void* stream);

/* ---- preprocessing: NIfTI volumes -> per-slice datasets (the reference's src/preprocess/preprocess_crc.py,
 *      make_crc_testing_dataset.py, preprocess_brats.py).  Added functions only; the ABI stays 9.
 * vol: the volume as stored, [Z][Y][X] with x fastest (NIfTI's Fortran order), dtype = 0 uint8, 1 int16, 2 uint16, 3 int32,
 * 4 float32, 5 float64.  A voxel's value is double(stored), then * slope + inter in double when scaled != 0 (nibabel's
 * get_fdata).  Every operation rounds once (the file is compiled without contraction) and sums run in a fixed order.
 * vqw_volume_stats: stats [5] doubles = min, max, then over the voxels whose float32(value) > 0: count, mean and population
 * standard deviation of the float32 values, summed in double (two passes for the deviation; per-workgroup partials, then one
 * fold: no floating-point atomics, the same bits every run).  ws: vqw_volume_stats_ws_bytes() bytes.
 * vqw_volume_to_slices: out [Z][S][S] float = PIL's F-mode bilinear Image.resize((S, S)) of every oriented, normalised
 * slice.  norm 0: float32(v); 1: float32(((v - min) / (max - min)) * 255) in double; 2: (float32(v) - float32(mean)) /
 * float32(std) in float32, with min, max, mean, std read from stats (device; nullable for norm 0).  orient 0: the slice
 * v[x, y] as it is (rows along x); 1: np.rot90(slice[::-1]); 2: np.rot90(slice, k=3) (both: Y rows, X columns).  kh [S][ksh]
 * doubles and bh [S][2] ints (first tap, tap count) are the horizontal pass's normalised coefficients, kv / bv [S][ksv] the
 * vertical pass's; ksh = 0 / ksv = 0: that pass keeps its size (PIL skips it).  The horizontal pass is rounded to float32
 * into tmp [Z][rows][S] (nullable when ksv = 0), then the vertical pass; both accumulate in double in index order.
 * vqw_label_slices: out [Z][S][S] int32 = the oriented slice at rows ytab [S], columns xtab [S] (PIL's NEAREST); relabel 1
 * writes label 4 as 3 and sets err [1] to 1 when any voxel of the volume already is 3, else err = 0. */
long vqw_volume_stats_ws_bytes(void);
int vqw_volume_stats(const void* vol, double* stats, double* ws, int dtype, long n, double slope, double inter, int scaled,
                     void* stream);
int vqw_volume_to_slices(const void* vol, const double* stats, const double* kh, const int* bh, const double* kv,
                         const int* bv, float* tmp, float* out, int dtype, int X, int Y, int Z, int S, int ksh, int ksv,
                         int norm, int orient, double slope, double inter, int scaled, void* stream);
int vqw_label_slices(const int32_t* vol, const int* xtab, const int* ytab, int32_t* out, int32_t* err, int X, int Y, int Z,
                     int S, int orient, int relabel, void* stream);

/* ---- VQGAN decoder blocks (networks/vqgan.py:10-19 Normalize / nonlinearity, :125-180 AttnBlock).  Added functions only; the
 *      ABI stays 9.
 * GroupNorm(32 groups, affine) with or without swish: y = act(gamma_c (x - mean_{n,g}) rstd_{n,g} + beta_c), act = identity or
 * u sigmoid(u); x, y [N][HW][C], C a multiple of 32 (anything else is rejected, as torch rejects it), at most 1024.  The
 * statistics are double sums folded in a fixed order (per-thread, workgroup rows, splits): the same bits every run, and no fp32
 * E[x^2] - mean^2.  mean, rstd [N][32] are what the backward needs besides x: it recomputes gamma xhat + beta.
 * vqw_groupnorm_splits: workgroups per image of the reduction passes; 1 = the plane is reduced and finalised by one workgroup
 * (H W C <= 16384), else it is split and a finalise pass folds the partials.  ws: vqw_groupnorm_ws_bytes() bytes.
 * Backward: a reduce pass (per image and channel sum g', sum g' xhat with g' = gy act'(gamma xhat + beta); from them
 * dgamma_c, dbeta_c and per group sum gamma g', sum gamma g' xhat), then the apply pass
 * gx = rstd (gamma g' - mean_g(gamma g') - xhat mean_g(gamma g' xhat)).  dgamma, dbeta [C] are overwritten. */
int vqw_groupnorm_splits(int HW, int C);
size_t vqw_groupnorm_ws_bytes(int N, int HW, int C);
int vqw_groupnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, void* ws,
                      size_t ws_bytes, int N, int HW, int C, float eps, int swish, void* stream);
int vqw_groupnorm_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                      const float* gy, float* gx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int N, int HW,
                      int C, int swish, void* stream);
/* swish on its own, y = x sigmoid(x) (vqgan.py:10-12 `nonlinearity`), and its gradient gx = gy swish'(x): n elements */
int vqw_swish_fwd(const float* x, float* y, long n, void* stream);
int vqw_swish_bwd(const float* x, const float* gy, float* gx, long n, void* stream);
/* Single-head self-attention over a feature map: o = softmax(scale q k^T) v per batch element; q, k, v, o [B][N][C] (N = H W of
 * an NHWC map), C a multiple of 32 up to 512 or a multiple of 64 up to 1024; lse [B][N] = the row log-sum-exp of scale q k^T.  Both matrix products run on the
 * exact-fp32 matrix cores; the softmax is online (running row maximum), the N x N scores never reach memory.
 * Backward: d_ws [B][N] receives D_i = sum_c go o; P = exp(scale S - lse) is recomputed; one pass over query tiles writes
 * gq = scale (P o (go v^T - D)) k, one pass over key tiles gk = scale (P o (go v^T - D))^T q and gv = P^T go.  No atomics.
 * Above 512 channels every pass runs as two halves of the value / output columns, each recomputing its score tiles. */
int vqw_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int C, float scale,
                      void* stream);
int vqw_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                      float* d_ws, float* gq, float* gk, float* gv, int B, int N, int C, float scale, void* stream);

/* ---- minGPT blocks (networks/mingpt.py:34-119 CausalSelfAttention / Block).  Added functions only; the ABI stays 9.
 * LayerNorm(C, eps, affine) over the rows of x [rows][C]: y = gamma (x - mean_r) rstd_r + beta, biased variance from the centred
 * values of the row, which is read once and held in registers.  C a multiple of 4 with 4 <= C <= 4096; anything else is refused
 * by the argument check.  mean, rstd [rows] are what the backward needs besides x.  Backward: gx = rstd (gamma gy - mean_c(gamma
 * gy) - xhat mean_c(gamma gy xhat)); dgamma = sum_r gy xhat and dbeta = sum_r gy are per-workgroup partials (32 rows each) in ws
 * (vqw_layernorm_ws_bytes() bytes) that a second kernel folds in index order: no atomics, the same bits every run.  dgamma,
 * dbeta [C] are overwritten. */
size_t vqw_layernorm_ws_bytes(long rows, int C);
int vqw_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C,
                      float eps, void* stream);
int vqw_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* gy, float* gx,
                      float* dgamma, float* dbeta, void* ws, size_t ws_bytes, long rows, int C, void* stream);
/* nn.GELU() in its exact form, y = 0.5 x (1 + erf(x / sqrt 2)), and its gradient gx = gy (Phi(x) + x phi(x)): n >= 1 elements,
 * in fp32 with the device erff / expf */
int vqw_gelu_fwd(const float* x, float* y, long n, void* stream);
int vqw_gelu_bwd(const float* x, const float* gy, float* gx, long n, void* stream);
/* Multi-head attention with a causal mask and an unmasked prefix: q, o [B][Tq][E], k, v [B][Tk][E], E = n_head hs, head h in the
 * columns [h hs, (h + 1) hs) of a row of E floats (the layout three nn.Linear projections leave: no transpose pass);
 * lse [B][n_head][Tq] = the row log-sum-exp of the visible scale q k^T.  hs a multiple of 32 with 32 <= hs <= 128, 1 <= Tq, Tk
 * <= 65536, B n_head <= 65535, tensors 16-byte aligned; anything else is refused with a message that names the constraint.
 * causal = 1 needs Tq == Tk = T and 0 <= n_unmasked <= T: query i sees key j iff j <= (i < n_unmasked ? n_unmasked - 1 : i),
 * i.e. tril with mask[:n_unmasked, :n_unmasked] = 1.  causal = 0 (n_unmasked = 0): no mask, Tq != Tk allowed, forward only (the
 * layer_past route).  Key steps wholly above a query tile's limit are not walked.  Backward (Tq == Tk): d_ws [B][n_head][T]
 * receives D_i = sum_c go o over the head; P = exp(scale S - lse) is recomputed; gq per query tile, gk and gv per key tile.  No
 * atomics; the same bits every run. */
int vqw_causal_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Tq, int Tk,
                             int n_head, int hs, float scale, int causal, int n_unmasked, void* stream);
int vqw_causal_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                             float* d_ws, float* gq, float* gk, float* gv, int B, int Tq, int Tk, int n_head, int hs, float scale,
                             int causal, int n_unmasked, void* stream);

/* ---- dropout of the GPT prior (networks/mingpt.py:83, :88, :104, :189).  Added functions only; the ABI stays 9.
 * Counter-based: whether an element is kept is a pure integer function of (seed, call, site, element index) - csrc/dropout.h
 * holds it, tests/dropout_ref.py restates it - generated in registers where it is used and never stored; a kept element is
 * multiplied by float32(1 / (1 - p)), keep iff the element's 32-bit draw >= round(p 2^32).  0 <= p < 1, anything else is refused.
 * The element index of these sites is the linear index into the dense tensor.  n >= 1, tensors 16-byte aligned.
 * vqw_dropout: y = drop(x); its backward is the same call on the gradient.  vqw_add_dropout: y = a + drop(b) in one pass; the
 * gradient of a is gy, that of b is vqw_dropout(gy) under the same key.  y may be x (or a, or b). */
int vqw_dropout(const float* x, float* y, long n, float p, long seed, long call, int site, void* stream);
int vqw_add_dropout(const float* a, const float* b, float* y, long n, float p, long seed, long call, int site, void* stream);
/* The keep masks themselves as bytes (1 = kept), through the same device function: out [n] of an element-wise site, out
 * [B][n_head][Tq][Tk] of an attention site (element (b n_head + h, i, j)).  For tests and for looking at a mask: nothing on the
 * training path calls them. */
int vqw_dropout_mask(unsigned char* out, long n, float p, long seed, long call, int site, void* stream);
int vqw_attention_dropout_mask(unsigned char* out, int B, int n_head, int Tq, int Tk, float p, long seed, long call, int site,
                               void* stream);
/* vqw_causal_attention_fwd / _bwd with dropout on the probabilities (mingpt.py:83): o = (softmax(.) o M) v with M = keep / (1 - p)
 * of element (b n_head + h, i, j), the mask regenerated in the forward and in both backward kernels from the logical position.
 * Same contract and argument checks as the functions above; in addition Tq == Tk is needed with causal = 0 too (the layer_past
 * route is inference only) and 0 <= p < 1.  lse is that of the undropped probabilities: the same bits as without dropout.
 * Backward: D = sum_c go o as before; gv = (P o M)^T go, dS = scale P o (M o (go v^T) - D). */
int vqw_causal_attention_drop_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Tq, int Tk,
                                  int n_head, int hs, float scale, int causal, int n_unmasked, float p, long seed, long call, int site,
                                  void* stream);
int vqw_causal_attention_drop_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                  float* d_ws, float* gq, float* gk, float* gv, int B, int Tq, int Tk, int n_head, int hs, float scale,
                                  int causal, int n_unmasked, float p, long seed, long call, int site, void* stream);

/* ---- the GPT code prior around the blocks (networks/mingpt.py:122-224 GPT).  Added functions only; the ABI stays 9.  fp32, dense,
 * no float atomics: every sum has a fixed order, the same bits every run.
 * Embedding: x[b][t] = (t < Te ? prefix[b][t] : tok[idx[b][t - Te]]) + pos[t0 + t], T = Te + Ti.  idx [B][Ti] (torch.long),
 * tok [V][E], pos [block_size][E], prefix [B][Te][E] or null with Te = 0 (the reference's `embeddings=`), x [B][T][E]; t0 is
 * the position offset (past_length on the cached route).  E a multiple of 4 with 4 <= E <= 4096, V >= 1, Ti >= 0, B >= 1,
 * T >= 1, t0 + T <= block_size, tensors 16-byte aligned; anything else is refused with a message that names the constraint.
 * An index outside [0, V) reads nothing: its row of x is NaN and the backward skips it.  Backward, from gx [B][T][E], both
 * overwritten: gpos[t0 + t] = sum_b gx[b][t] with b ascending, 0 in the rows of pos outside [t0, t0 + T); gtok[v] = the sum of
 * gx[b][Te + t] over the (b, t) with idx[b][t] == v in ascending (b, t) order (a wave owns a row and walks the B Ti indices),
 * exactly 0 for a row no token uses.  The prefix's gradient is gx[:, :Te]: no kernel. */
int vqw_embed_fwd(const long* idx, const float* tok, const float* pos, const float* prefix, float* x, int B, int Ti, int Te, int E,
                  int V, int block_size, int t0, void* stream);
int vqw_embed_bwd(const long* idx, const float* gx, float* gtok, float* gpos, int B, int Ti, int Te, int E, int V, int block_size,
                  int t0, void* stream);
/* Cross-entropy over the last axis of z [rows][V] against target [rows] (torch.long): lse_r = log sum_c exp(z_rc) with the row
 * maximum subtracted first, loss_r = lse_r - z[r][target_r]; loss, lse [rows].  mean [1] (may be null; then ws is not needed)
 * receives the mean of loss: per-workgroup partial sums (32 rows each) in double in ws (vqw_xent_ws_bytes() bytes, 8-byte
 * aligned), folded in index order in double and rounded once.  1 <= V <= 65536, rows >= 1; up to V = 1024 a row is read once
 * into registers, above it is walked with an online maximum and sum.  A target outside [0, V) reads nothing: loss_r and the
 * row of gz are NaN.  Backward: gz[r][c] = (exp(z_rc - lse_r) - [c == target_r]) w_r with w_r = gw[0] / rows (mean = 1: gw is
 * the device scalar d loss, read by the kernel) or gw[r] (mean = 0: gw [rows], reduction 'none'). */
size_t vqw_xent_ws_bytes(long rows);
int vqw_xent_fwd(const float* z, const long* target, float* loss, float* lse, float* mean, void* ws, size_t ws_bytes, long rows, int V,
                 void* stream);
int vqw_xent_bwd(const float* z, const long* target, const float* lse, const float* gw, float* gz, long rows, int V, int mean,
                 void* stream);
/* Top-k sampling, one token per row of logits [B][V] (taming-transformers' top_k_logits, softmax, inverse CDF): s = z /
 * temperature; thr = the top_k-th largest s (top_k = 0 or >= V: no filter); every entry >= thr is kept, ties at the threshold
 * included; p_c = exp(s_c - max) over the kept entries; out[b] = the first kept index, in index order, whose running sum of p
 * exceeds u[b] total, or the last kept index if rounding leaves none - never an index outside the kept set.  u [B] are uniforms
 * in [0, 1) from the caller: the kernel has no random numbers of its own, a seed reproduces a sample bit for bit.  out [B]
 * (torch.long).  1 <= V <= 65536, B >= 1, temperature > 0, top_k >= 0.  A NaN logit makes the result unspecified (some index
 * in [0, V)). */
int vqw_sample_topk(const float* logits, const float* u, long* out, int B, int V, float temperature, int top_k, void* stream);
/* Sample or force, with top-k, top-p and the log-probability (GPT.generate_masked's step), one row of logits [B][V] per workgroup.
 * Filter: s = z / temperature; K1 = vqw_sample_topk's kept set (every entry >= the top_k-th largest, ties included; top_k = 0 or
 * >= V keeps all); the nucleus is taken over K1: with p_c = exp(s_c - max) / sum_{K1}, entry c stays iff the mass of the entries
 * of K1 STRICTLY GREATER than it is <= top_p (top_k_top_p_filtering's rule; tied entries share one fate, so no sort order
 * enters; the largest entry always stays).  The masses are 2^-40 fixed point in 64-bit integers (p <= 1, V <= 2^16: the sums
 * fit; integer addition has no order): the threshold is exact for the fp32 values of p up to V 2^-41 of the total.  top_p >= 1:
 * no nucleus filter, and no code for it runs.  Draw: vqw_sample_topk's inverse CDF in index order over the kept set from u[b];
 * no random numbers of the kernel's own; never an index outside the kept set.  forced [B] (torch.long; may be null): forced[b]
 * in [0, V) gives out[b] = forced[b] and u[b] is not read; forced[b] < 0 draws; forced[b] >= V draws as well and sets logp[b]
 * to NaN.  logp [B] (may be null): z[out] - logsumexp(z) under the model's own distribution - temperature 1, unfiltered,
 * whatever the filter was: fp32 terms exp(z - max), summed in double in a fixed order, rounded once (vqw_xent_fwd's rule).
 * No float atomics; the same bits every run.  With forced = null and top_p >= 1, out has the bits of vqw_sample_topk on the same
 * inputs.  1 <= V <= 65536, B >= 1, temperature > 0, top_k >= 0, top_p > 0; logits, u and out must not be null. */
int vqw_sample_filtered(const float* logits, const float* u, const long* forced, long* out, float* logp, int B, int V,
                        float temperature, int top_k, float top_p, void* stream);
/* Classifier-free guidance inside the same sampler (GPT.generate_masked's guided step).  Added function only; the ABI stays 9.
 * logits [2B][V]: the rows [0, B) are the conditional rows z_c, the rows [B, 2B) the unconditional rows z_u of the same samples.
 * The mixed logit z[c] = fmaf(scale, z_c[c] - z_u[c], z_u[c]) - one fp32 subtraction, one fused multiply-add, the same bits in
 * every pass of the kernel - takes the place of vqw_sample_filtered's row: temperature, top-k, top-p, forced and the draw apply to
 * it word for word, with u, forced [B].  No [B][V] intermediate is written; each pass reads both rows.  out [2B]: out[b] = out[B + b]
 * = the token, so the decode step of the next position takes out as its idx for both halves.  logp [B] (may be null): the token's
 * log-probability under the CONDITIONAL row - temperature 1, unfiltered: what vqw_sample_filtered returns for z_c with that token
 * forced; logp_u [B] (may be null): the same under z_u.  forced[b] >= V sets both to NaN.  scale must be finite and >= 0 (0: z_u,
 * 1: z_c up to the rounding of the mix); otherwise vqw_sample_filtered's constraints. */
int vqw_sample_guided(const float* logits, const float* u, const long* forced, long* out, float* logp, float* logp_u, int B, int V,
                      float scale, float temperature, int top_k, float top_p, void* stream);
/* The composite of an edit: out[b][y][x][c] = cellmask[b][y / fy][x / fx] ? edit[b][y][x][c] : image[b][y][x][c] on NHWC
 * tensors [N][H][W][C]; cellmask [N][h][w] bytes (non-zero: the edit), fy = H / h, fx = W / w; H % h == 0 and W % w == 0.  One
 * streaming kernel, 16-byte accesses when a cell's row (fx C floats) is a multiple of 4 floats and the tensors are 16-byte
 * aligned, else one float per thread.  N H W C < 2^31.  No gradient. */
int vqw_paste_cells(const float* image, const float* edit, const uint8_t* cellmask, float* out, int N, int H, int W, int C, int h,
                    int w, void* stream);

/* ---- cached generation for the GPT code prior (networks/gpt.py GPT.prefill / decode_step / generate).  Added functions only; the
 * ABI stays 9.  fp32 in, fp32 out, fp32 accumulation, no float atomics: every sum has a fixed order, the same bits every run.
 * Forward only.
 * Skinny fused linear: y[m][y_col + n] = act(sum_k LN?(x[m])[k] w[n][k] + bias[n]) (+ residual[m][n]) for x [M][K] (M: the batch of
 * a decode step), w [N][K] as nn.Linear stores it, y with the row stride ldy >= y_col + N (elements outside the N columns and M
 * rows are not touched).  Optional, each chosen by a non-null pointer or flag: the LayerNorm of the input row with ln_gamma,
 * ln_beta [K] and eps (both or neither; K <= 4096; biased variance from the centred values, vqw_layernorm_fwd's formulas); bias
 * [N]; gelu != 0: the exact erf GELU, vqw_gelu_fwd's formula; residual [M][N], dense - y may be the residual itself (then ldy ==
 * N, y_col == 0), never x.  K a multiple of 4 with 4 <= K <= 16384, N >= 1, 1 <= M <= 524280; x, w, ln_gamma, ln_beta 16-byte
 * aligned.  A wave owns an output column and reads its weight row once for the rows of a group of 8: up to M = 8 every weight
 * element is read once per launch. */
int vqw_dec_linear(const float* x, const float* w, const float* bias, const float* ln_gamma, const float* ln_beta, const float* residual,
                   float* y, int M, int K, int N, long ldy, long y_col, int gelu, float eps, void* stream);
/* Decode attention: o[b] = softmax(scale q[b] k[b][:Tk]^T) v[b][:Tk] per head for ONE query row per batch row, q, o [B][E], k, v
 * [B][capacity][E] (a plane of the cache below), E = n_head hs, head h in the columns [h hs, (h + 1) hs).  No mask (the layer_past
 * route, as vqw_causal_attention_fwd with causal = 0).  Rows at or beyond Tk are never read.  hs a multiple of 32 with 32 <= hs <=
 * 128, B n_head <= 65535 (vqw_causal_attention_fwd's limits), 1 <= Tk <= capacity <= 65536, tensors 16-byte aligned.  One
 * workgroup per (b, head); measured up to Tk = 256. */
int vqw_dec_attention(const float* q, const float* k, const float* v, float* o, int B, int Tk, int capacity, int n_head, int hs,
                      float scale, void* stream);
/* One decode step of the GPT: ONE host call per token, 2 + 5 n_layer launches, no allocation, synchronisation or host read.
 * idx [B] (torch.long, on the device): the token of each row at position t; tok [V][E], pos [block_size][E]: the model's embedding
 * tables.  kv: the cache, [n_layer][2][B][capacity][E] (k-plane, v-plane per layer; the heads side by side in the last axis - the
 * (B, T, E) layout vqw_causal_attention_fwd takes); its rows [0, t) hold the past, row t is written, the attention runs over the
 * rows [0, t].  logits [B][V].  ws: vqw_gpt_decode_ws_bytes(B, E, V) bytes (the x, q, att [B][E] and h [B][4E] buffers).
 * packed: vqw_gpt_decode_pack_floats(n_layer, E, V) floats, the model's weights in one buffer with the fixed layout
 *     per layer l (12 E E + 13 E floats):  ln1.weight [E] | ln1.bias [E] | W_q | W_k | W_v as one [3E][E] | b_q | b_k | b_v [3E] |
 *                                          W_proj [E][E] | b_proj [E] | ln2.weight [E] | ln2.bias [E] | W_fc1 [4E][E] | b_fc1 [4E] |
 *                                          W_fc2 [E][4E] | b_fc2 [E]
 *     then:                                ln_f.weight [E] | ln_f.bias [E] | W_head [V][E]
 * filled by plain copies of the parameters.  Refused before any device work, with a message that names the constraint: a null
 * pointer, E no multiple of 4 or outside [4, 4096], E not divisible by n_head, a head size outside vqw_dec_attention's limits,
 * t < 0, t >= capacity, t >= block_size, a short workspace, pointers not 16-byte aligned.  The two size queries return 0 for a
 * non-positive argument. */
long vqw_gpt_decode_pack_floats(int n_layer, int E, int V);
size_t vqw_gpt_decode_ws_bytes(int B, int E, int V);
int vqw_gpt_decode_step(const float* packed, const float* tok, const float* pos, const long* idx, float* kv, float* logits, void* ws,
                        size_t ws_bytes, int B, int t, int capacity, int n_layer, int n_head, int E, int V, int block_size, float eps,
                        void* stream);

/* ---- deferred split-K folds of the weight gradients (ABI 8).  Every conv weight-gradient entry point ends in one or two
 * short fold launches (dW and dbias slabs -> the gradient).  With vqw_fold_defer(1) those folds are only recorded - the
 * caller must then keep the `ws` buffers of the weight-gradient calls alive - and vqw_fold_flush_host() folds everything
 * recorded so far in ONE launch on `stream` (which must be ordered after the recorded calls' streams).  Two recorded folds
 * into the same output (overwrite, then accumulate: the two views of a training step) are summed in recording order; a
 * third one is an error (flush first).  table_host: pinned host buffer, table_dev: device buffer, both of at least
 * vqw_fold_table_bytes() bytes, both untouched by the caller until the launch has run.  Process-wide state (backward nodes
 * and end-of-pass callbacks run on different host threads).  Replaces nothing upstream: plumbing behind F.conv2d's weight
 * gradient (see the convolution section). */
int vqw_fold_defer(int on);              /* returns the previous setting */
int vqw_fold_pending(void);              /* number of recorded, unflushed fold records */
size_t vqw_fold_table_bytes(void);
int vqw_fold_discard(void);              /* drop the recorded folds (after an aborted backward pass); returns how many */
int vqw_fold_flush_host(void* table_host, void* table_dev, size_t table_bytes, void* stream);

/* ---- optimiser: torch.optim.Adam as built in trainers/base.py:165-175 */
int vqw_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                  void* stream);
/* the same update for many tensors in one launch: chunks_dev points to n_chunks device records
 * {float* p; const float* g; float* m; float* v; int64_t n} (40 bytes each), one workgroup per record */
int vqw_adam_multi(const void* chunks_dev, int n_chunks, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float bias_corr1, float bias_corr2, void* stream);

/* ---- training the GPT code prior (trainers/prior.py; minGPT's and taming-transformers' recipe).  Added functions only; the ABI
 * stays 9.  fp32 in, fp32 out, no float atomics: every sum has a fixed order, the same bits every run.  No host synchronisation.
 * Global gradient norm: the L2 norm over the g tensors of vqw_adam_multi's chunk table (p, m, v are not touched).  Stage one, a
 * workgroup per record, leaves the sum of g g of its chunk, in double, in ws (vqw_grad_norm_ws_bytes(n_chunks) bytes, 8-byte
 * aligned; 0 for n_chunks < 1); stage two, one workgroup, folds the partials in index order in double and writes norm_out[0] =
 * (float)sqrt(sum) and norm_out[1] = the clip coefficient min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s
 * formula in fp32; max_norm <= 0: the coefficient is 1.  A NaN norm gives a NaN coefficient and an infinite norm the coefficient
 * 0 (then 0 inf = NaN in the update), both as torch's clamp leaves them: a non-finite gradient poisons the step, nothing hides it. */
size_t vqw_grad_norm_ws_bytes(int n_chunks);
int vqw_grad_norm_multi(const void* chunks_dev, int n_chunks, float max_norm, void* ws, size_t ws_bytes, float* norm_out, void* stream);
/* torch.optim.AdamW (decoupled decay): p *= 1 - lr wd; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2; p -= (lr / bias_corr1)
 * m / (sqrt(v) / sqrt(bias_corr2) + eps), with g' = clip[0] g.  clip: a device scalar - norm_out + 1 of vqw_grad_norm_multi - or
 * null, which means 1.  The gradient tensors are NOT rewritten: after a clipped step p.grad still holds the unclipped values,
 * unlike torch's in-place clip_grad_norm_.  Argument order, chunk table and walk as vqw_adam_multi / vqw_adam_step; the scalars
 * are doubles: 1 - lr wd, 1 - beta, lr / bias_corr1 and sqrt(bias_corr2) are formed in double and rounded once, as torch forms
 * them before its fp32 tensor operations (an fp32 beta2 = 0.95 would leave 1 - beta2 2.4e-7 off in every element). */
int vqw_adamw_multi(const void* chunks_dev, int n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay,
                    double bias_corr1, double bias_corr2, const float* clip, void* stream);
int vqw_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, double bias_corr1, double bias_corr2, const float* clip, void* stream);
/* The transformer's input from a batch of code sequences ids [B][T] (torch.long): inp[b][0] = sos, inp[b][t] = corrupted[b][t - 1]
 * with corrupted[b][t] = ids[b][t] if u_keep[b][t] < pkeep, else min(V - 1, (long)floorf(u_rand[b][t] V)) - taming-transformers'
 * pkeep corruption behind a start token; the target stays ids.  u_keep, u_rand [B][T] are uniforms in [0, 1) from the caller: the
 * kernel has no random numbers of its own (vqw_sample_topk's rule).  pkeep >= 1 reads neither, both may be null.  An ids entry
 * outside [0, V) is passed through unchanged (vqw_embed_fwd defines what follows).  B, T, V >= 1. */
int vqw_prior_tokens(const long* ids, const float* u_keep, const float* u_rand, long* inp, int B, int T, int V, long sos, float pkeep,
                     void* stream);

/* ---- conditioning the code prior on label maps (csrc/cond.hip; networks.LabelCondition, trainers.ConditionalPriorTrainer;
 * taming-transformers' recipe: one conditioning token per latent cell).  Added functions only; the ABI stays 9.  Integer counts, no
 * float atomics: the same bits every run.  Every refusal arrives with a message before any launch.
 * Cell labels: label [B][H][W] of elem_bytes = 1 (unsigned, torch.uint8), 4 or 8 (signed) byte integers, fy = H / h, fx = W / w
 * with H % h == 0 and W % w == 0.  tokens[b][cy][cx] (torch.long) = the label in [0, n_labels) that most pixels of the cell carry;
 * a tie goes to the smallest label; a pixel outside [0, n_labels) counts for nothing; a cell with no counted pixel gets -1.
 * purity [B][h][w] (may be null) = float(the winner's count) / float(fy fx), one fp32 division; 0 for the -1 cell.  A workgroup
 * takes one row of cells of one image (fewer cells where n_labels counters per cell would exceed 32 KB of LDS or the grid would be
 * small), reads the image rows in 16-byte units at aligned addresses and counts with integer LDS atomics.  1 <= n_labels <= 256,
 * B and h <= 65535, fy fx <= 2^24, label aligned to its element size.
 * Cells changed: out[b][cy][cx] (bytes) = 1 iff any pixel of the cell differs between a and b, two maps of one shape and element
 * size; the same walk, 16-byte units where the two pointers agree modulo 16.
 * Table lookup: out[r] = table[idx[r]] for idx [rows] (torch.long), table [L][E], out [rows][E]; an index outside [0, L) writes a
 * NaN row.  E a multiple of 4 with 4 <= E <= 4096, table and out 16-byte aligned.  Its gradient is vqw_embed_bwd's gtok. */
int vqw_cell_labels(const void* label, long* tokens, float* purity, int B, int H, int W, int h, int w, int n_labels, int elem_bytes,
                    void* stream);
int vqw_cells_changed(const void* a, const void* b, uint8_t* out, int B, int H, int W, int h, int w, int elem_bytes, void* stream);
int vqw_embed_lookup(const long* idx, const float* table, float* out, long rows, int E, int L, void* stream);
/* The lookup with the condition dropped per SAMPLE (the training side of classifier-free guidance).  Added function only; the ABI
 * stays 9.  Sample b = r / rows_per_sample is dropped iff the draw of csrc/dropout.h for element b under (seed, call) and the site
 * COND_DROP_SITE (-1: outside the sites GPT.seed_dropout numbers from 0) is below round(p 2^32); every row of a dropped sample reads
 * table[null_index].  eff [rows] (torch.long) receives the index actually read: the gradient is vqw_embed_bwd's gtok over eff.  No
 * mask tensor, no host read, the same bits every run; at p = 0 out has vqw_embed_lookup's bits.  rows a multiple of
 * rows_per_sample >= 1, 0 <= null_index < L, 0 <= p < 1, otherwise vqw_embed_lookup's constraints. */
int vqw_embed_lookup_drop(const long* idx, const float* table, float* out, long* eff, long rows, int rows_per_sample, int E, int L,
                          long null_index, float p, long seed, long call, void* stream);
/* The conditioned embedding of the masked prior (networks.MaskedGPT.forward_conditioned): the label token of latent cell t is ADDED
 * to the embedding of position t.  Added function only; the ABI stays 9.
 *   x[b][t][:] = fp32(fp32(tok[idx[b][t]] + pos[t]) + ctab[e]),   e = cidx[b][t], or null_index when sample b is dropped
 * - two fp32 additions in this order: the bits of vqw_embed_fwd's output plus vqw_embed_lookup_drop's, added in fp32.  idx, cidx
 * [B][T] (torch.long), tok [V][E], pos [block_size][E], ctab [L][E], x [B][T][E]; eff [B][T] (torch.long, may be null) receives e.
 * The drop is vqw_embed_lookup_drop's, decided by the same function: the draw of csrc/dropout.h for element b under (seed, call)
 * and COND_DROP_SITE against round(p 2^32); p = 0 reads neither seed nor call and drops nobody.  An idx outside [0, V) or an e
 * outside [0, L) (vqw_cell_labels' -1) writes a NaN row.  One streaming pass, a wave per row, 16-byte accesses, no intermediate of
 * the size of x, no float atomics.  The gradients are vqw_embed_bwd's: gtok and gpos over idx with Te = 0, gctab the gtok walk
 * over eff.  E a multiple of 4 with 4 <= E <= 4096, T <= block_size, tok, pos, ctab and x 16-byte aligned, 0 <= p < 1, and
 * 0 <= null_index < L when p > 0. */
int vqw_embed_cond_fwd(const long* idx, const float* tok, const float* pos, const long* cidx, const float* ctab, float* x, long* eff,
                       int B, int T, int E, int V, int L, int block_size, long null_index, float p, long seed, long call, void* stream);

/* ---- anomaly detection with the code prior (trainers/prior.py PriorTrainer.detect, trainers/fit.py Fit.detect; the reference has
 * nothing like it).  Added functions only; the ABI stays 9.  fp32 in, no float atomics, the same bits every run; every refusal below
 * arrives with a message before any launch.
 * The map of a restoration: map = G(r o U(m)) on NHWC a, b [N][H][W][C] -> map [N][H][W].  r[y][x] = (sum_c |a - b|) / C, c
 * ascending.  m = float(cellmask != 0), cellmask [N][h][w] bytes with H = fy h, W = fx w for integers fy, fx; U is bilinear
 * up-sampling with half-pixel centres and clamped edges, the values of F.interpolate(mode='bilinear', align_corners=False): source
 * coordinate max(0, (y + 0.5) h / H - 0.5), its floor and the next cell (clamped to h - 1), weights from the fraction.  cellmask
 * null: m is all ones, U is skipped and h, w are not read.  G is the separable filter of the K = 2 R + 1 taps [K] (the caller's
 * normalised Gaussian; device, fp32) with clamped (replicate) borders, rows first, then columns, each sum over the taps in
 * ascending order from 0; K = 1 with the tap 1 is no blur.  ONE kernel: a workgroup owns a 32 x 64 tile, computes r o U(m) for the
 * tile and its halo of R pixels into LDS, runs both passes there and writes the tile - a and b are read once (plus the halo), the
 * map is written once, nothing else touches memory.  Refused: K even, K < 1 or K > 33 (R <= 16 is the halo the tile geometry
 * holds: sigma <= 5.33 under K = 2 ceil(3 sigma) + 1); H or W no multiple of h, w; an empty tensor (N, H, W or C < 1); N > 65535;
 * a, b, taps or map null or not 16-byte aligned. */
int vqw_anomaly_map(const float* a, const float* b, const uint8_t* cellmask, const float* taps, float* map, int N, int H, int W, int C,
                    int h, int w, int K, void* stream);
/* The histogram of scores [n] by an order-preserving key, ACCUMULATED into hist [2][65536] (torch.long; hist[0]: the negatives,
 * labels[i] == 0, hist[1]: the positives): the key of a finite score s >= 0 is bits(s) >> 15 - 8 exponent and 8 mantissa bits,
 * monotone non-decreasing in s, relative resolution 2^-8; -0 counts as 0.  A NaN, an infinity or a negative score is not binned and
 * adds 1 to err[0] (torch.long, accumulated too).  labels [n] bytes.  Integer atomics: the counts are exact and do not depend on the
 * order.  A workgroup keeps 32-bit counters for a window of 24 exponents x 256 keys per label in LDS - the window ends one exponent
 * above the largest key of the workgroup's first chunk - and for key 0 (the exact zeros of untouched pixels), and adds the non-zero
 * ones to hist once; any other key outside the window goes to hist at once; before any add a wave merges the lanes that share
 * the key of its first lane into one add per label, so a constant map costs two adds per wave-instruction.  16 bytes of scores and 4 of labels per load when scores is 16-byte and
 * labels 4-byte aligned, else one score per load.  Refused: a null pointer, n < 1 (an empty tensor), n > 2^40, scores not 4-byte
 * or hist, err not 8-byte aligned. */
int vqw_score_histogram(const float* scores, const uint8_t* labels, long* hist, long* err, long n, void* stream);
/* The detection scores of a histogram, out [8] doubles on the device, one launch, one workgroup.  With P_b = hist[1][b], N_b =
 * hist[0][b], P = sum P_b, N = sum N_b, TP_b = sum_{b' >= b} P_b', FP_b = sum_{b' >= b} N_b' (64-bit integer scans over the bins
 * in descending order):
 *   out[0] auroc          = sum_b P_b (N_{<b} + N_b / 2) / (P N)                      (Mann-Whitney; ties inside a bin count half)
 *   out[1] ap             = sum_{b non-empty} (P_b / P) TP_b / (TP_b + FP_b)           (one threshold per distinct key)
 *   out[2] best_dice      = max over the non-empty bins of 2 TP_b / (TP_b + FP_b + P)  (= 2 TP / (2 TP + FP + FN))
 *   out[3] best_threshold = the float whose bits are b << 15 for the bin of best_dice; a tie goes to the highest bin (the Dice
 *                           values are compared exactly, as fractions)
 *   out[4] P, out[5] N, out[6] 1 if err is null or err[0] == 0 else 0, out[7] 0.
 * Every term is formed in double from the exact integers (no integer product) and summed in a fixed order.  With P = 0 or N = 0
 * out[0..3] are NaN: that is the definition, not an error.  Refused: hist or out null, a pointer not 8-byte aligned. */
int vqw_detection_scores(const long* hist, const long* err, double* out, void* stream);

/* ---- lesion-wise detection scores: connected components of score maps (csrc/components.hip; ops.label_components,
 * ops.component_areas, ops.lesion_match, functions/lesion_scores.py LesionScores, trainers/fit.py Fit.detect; the reference has
 * nothing like it).  Added functions only; the ABI stays 9.  Integer atomics only (minima, counts, same-value stores), the same bits
 * every run; no allocation and no host read inside a call; every refusal below arrives with a message before any launch.
 * Labelling: images [N][H][W], foreground = mask byte != 0 (mask given, scores null) or score >= threshold (scores fp32 given,
 * mask null; a NaN score is background, a NaN threshold is refused).  Two foreground pixels of ONE image are joined when they are
 * neighbours - connectivity 4: W, E, N, S; 8: the diagonals too - never across images.  labels [N][H][W] int32: background 0, the
 * components of image n numbered 1..counts[n] in raster order of each component's first pixel, the one with the smallest y W + x
 * (scipy.ndimage.label's numbering: the result is canonical).  counts [N] int32.
 * Plan, six launches, no workgroup ever waits for another (no flag, no spin, no cooperative launch: kernel boundaries order the
 * passes): (1) a workgroup labels a 32 x 64 tile in LDS - row runs by pointer jumping, then a union-find with atomicMin links to
 * the row above - and writes each pixel's provisional label, the GLOBAL index n H W + y W + x of its tile-local root, into the
 * workspace; (2) the foreground pixels of a tile's top row and left column union with their neighbours in the adjacent tiles (N,
 * else NW and NE; W, else NW and SW) in that array by the lock-free minimum rule: find both roots, atomicMin the larger root's slot
 * with the smaller, go on from the value the atomic returned if the slot was no longer a root - parents are read with relaxed
 * agent-scope atomic loads and the decision to stop is taken only on the atomic's return value; the root of a finished component is
 * its smallest pixel index whatever the order of the merges; (3) every pixel walks to its root, roots are counted per chunk of
 * 1024 pixels; (4) one workgroup per image scans the chunk counts; (5) roots take their numbers; (6) every pixel takes its
 * root's number.  Every walk descends through strictly decreasing indices, so it ends; each also counts its steps against a bound
 * (twice the pixel count of the launch: two walkers; four tile sizes inside a tile) and past it stops and ORs a bit into err [1] int32 (accumulated, the
 * caller clears it once): 1 tile pass, 2 seam pass, 4 flatten pass, 8 vqw_component_areas met a label outside [0, cap].  err != 0
 * means the result is not to be used.  ws: vqw_label_components_ws_ints(N, H, W) int32 (0 for arguments out of range).
 * Refused: N, H or W < 1 (an empty tensor); N H W >= 2^31 (32-bit indices); connectivity not 4 or 8; both or neither of mask and
 * scores; a null labels, counts, err or ws; scores, labels, counts, err or ws not 4-byte aligned; a workspace that is too small.
 * Areas: areas [N][cap] int32, cleared by the call; areas[n][l - 1] = the pixels of image n with label l >= 1.  cap is the most
 * components an H x W image can hold - ceil(H / 2) ceil(W / 2) under connectivity 8, ceil(H W / 2) under 4 - a function of the
 * shape alone, so nothing is read back to size it; a label outside [0, cap] is not counted and sets err bit 8.  One streaming
 * pass; the lanes of a wave that share the label of its first active lane are merged into one add by a ballot.
 * Matching: acc [8] (torch.long), ADDED to: [0] slices = N; [1] gt_lesions = sum gt_counts; [2] gt_detected: ground-truth
 * components that share at least one pixel with a KEPT predicted component - one whose area is >= min_size (equal is kept);
 * [3] pred_components: the kept ones; [4] pred_false: kept components that share no pixel with any ground-truth pixel; [5] inter:
 * pixels both kept-predicted and ground truth; [6] pred_pixels: pixels of kept components; [7] gt_pixels.  pred_areas [N][pcap] as
 * above; a label above its image's count (or cap) is background.  One streaming pass sets the hit flags (same-value byte stores
 * into ws, cleared by the call) and adds the three pixel counts once per wave, then one workgroup per image folds flags, the kept
 * test and the counts into acc.  ws: vqw_lesion_match_ws_bytes(N, pcap, gcap) bytes.  Refused: an empty tensor; N H W >= 2^31;
 * min_size < 1; pcap or gcap < 1; a null pointer; int32 tensors not 4-byte or acc not 8-byte aligned; a workspace that is too
 * small.  (Label maps of different shapes are refused by ops.lesion_match: the C call takes one shape.) */
long vqw_label_components_ws_ints(int N, int H, int W);
int vqw_label_components(const uint8_t* mask, const float* scores, float threshold, int* labels, int* counts, int* err, int* ws,
                         long ws_ints, int N, int H, int W, int connectivity, void* stream);
int vqw_component_areas(const int* labels, int* areas, int* err, int N, int H, int W, int cap, void* stream);
long vqw_lesion_match_ws_bytes(int N, int pcap, int gcap);
int vqw_lesion_match(const int* pred_labels, const int* pred_counts, const int* pred_areas, const int* gt_labels, const int* gt_counts,
                     long* acc, uint8_t* ws, long ws_bytes, int N, int H, int W, int pcap, int gcap, int min_size, void* stream);

/* ---- the bidirectional masked code prior (csrc/masked_prior.hip; networks.MaskedGPT, trainers.MaskedPriorTrainer; MaskGIT's
 * recipe: fill in masked codes, decode in a few parallel passes).  Added functions only; the ABI stays 9.  Integer LDS atomics only,
 * no float atomics: the same bits every run.  One workgroup per sample; 1 <= B <= 65535, 1 <= T <= 65536, T a multiple of nothing.
 * Every refusal arrives with a message that names the constraint, before any launch.
 * The select: out[b][t] (bytes) = 1 for exactly min(max(n[b], 0), count_b) of the count_b eligible entries of row b - those with
 * the smallest (key, position) - and 0 elsewhere.  keys [B][T] fp32, compared as unsigned integers under the order-preserving map
 * of their bits (-0 < +0, the infinities order as numbers, a NaN with a clear sign bit lies above +inf); eligible [B][T] bytes,
 * null: every entry; n [B] int32.  The n-th smallest key is found by a byte-wise radix walk on an LDS histogram; entries EQUAL to it
 * are taken in ascending position (a workgroup prefix count), so ties do not depend on scheduling. */
int vqw_select_lowest(const float* keys, const uint8_t* eligible, const int* n, uint8_t* out, int B, int T, void* stream);
/* The corruption of a training step, from ids [B][T] (torch.long): sample b masks n[b] = clamp(ceil(r_b T), 1, T) positions (the
 * product and the ceil in double), r_b = cos(pi/2 u_b) with u_b = draw / 2^32, the draw of csrc/dropout.h for element b under
 * (seed, call) and the site MASK_RATIO_SITE = -2 (MaskGIT's cosine schedule); 0 < ratio <= 1 replaces r_b for every sample,
 * ratio = 0 means the schedule.  The masked set: the n[b] positions with the smallest (draw of element b T + t under
 * MASK_KEY_SITE = -3, t) - the select above over integer keys: exactly n[b], no Bernoulli draw.  inp [B][T] (torch.long) =
 * mask_token where masked, else ids; masked [B][T] bytes; n [B] int32.  No mask tensor from the host, no host read: the output is
 * a function of (seed, call) alone.  mask_token >= 0; ids and inp 8-byte, n 4-byte aligned. */
int vqw_mask_tokens(const long* ids, long* inp, uint8_t* masked, int* n, int B, int T, long mask_token, double ratio, long seed,
                    long call, void* stream);
/* One iteration of parallel decoding, one launch.  tokens [B][T] (torch.long), logp [B][T]: vqw_sample_filtered's output over all
 * B T rows, the known positions forced; masked [B][T] bytes; m0 [B] int32: the positions masked when decoding began.  Per sample,
 * with cur the masked count now: n_keep = gamma <= 0 ? 0 : max(0, min(cur - 1, floor(gamma m0))), the product in double - every
 * iteration fixes at least one code, gamma = 0 fixes all.  The confidence of a masked position is logp + tau g with g =
 * -logf(-logf(clamp(u, 2^-24, 1 - 2^-24))), u [B][T] the caller's uniforms; tau = 0: logp itself, bit for bit, and u is not read
 * (it may be null).  The n_keep masked positions of lowest (confidence, position) stay masked - the select above.  ids_out [B][T] =
 * mask_token where still masked, else tokens; masked_out [B][T]; fixed_logp [B][T], in / out: written with logp only where a
 * position turns from masked to fixed, untouched elsewhere; conf [B][T] (may be null): the confidence of the masked positions,
 * +inf at the others.  A position that was not masked keeps its token and is never masked.  gamma and tau finite, tau >= 0,
 * mask_token >= 0; masked_out and ids_out must not be masked and tokens themselves. */
int vqw_unmask_step(const long* tokens, const float* logp, const uint8_t* masked, const float* u, const int* m0, long* ids_out,
                    uint8_t* masked_out, float* fixed_logp, float* conf, int B, int T, double gamma, float tau, long mask_token,
                    void* stream);

/* ---- the pseudo-likelihood map of the masked code prior (csrc/pseudo_nll.hip; networks.MaskedGPT.pseudo_nll,
 * trainers.MaskedPriorTrainer.pseudo_nll / detect_pseudo).  Added functions only; the ABI stays 9.  Forward only, no gradient, no
 * atomics: the same bits every run.  Every refusal arrives with a message that names the constraint, before any launch.
 * The lattice: a latent grid h x w (T = h w <= 65536, raster order) and a stride 1 <= sy <= h, 1 <= sx <= w; position t = y w + x
 * belongs to group g(t) = (y mod sy) sx + (x mod sx) of S = sy sx groups, which partition the grid.  Pass s masks group s; the
 * passes of a sample run side by side as batch rows, in chunks [s0, s0 + ns) with 0 <= s0, ns >= 1, s0 + ns <= S: chunk row
 * r = b ns + (s - s0).  B ns T <= 2^31 - 4.
 * vqw_lattice_inputs: ids [B][T], inp [B ns][T] (torch.long, 8-byte aligned, distinct).  inp[b ns + (s - s0)][t] = mask_token where
 * g(t) = s, ids[b][t] elsewhere.  One streaming pass with 8-byte accesses, no mask tensor from the host.  mask_token >= 0.
 * vqw_lattice_gather_ln: x [B ns][T][E], the trunk's output in front of ln_f; y [B][T][E].  For every (b, t) with s0 <= g(t) <
 * s0 + ns: y[b][t][:] = LayerNorm(x[b ns + g(t) - s0][t][:]) under gamma, beta [E] and eps; every other row of y is left untouched,
 * so successive chunks fill one y.  One wave per output row, the group computed once per row; the row's body is
 * vqw_layernorm_fwd's (csrc/ln_row.h), so y has the bits of vqw_layernorm_fwd on the gathered row.  No statistics are written.  E a
 * multiple of 4 with 4 <= E <= 4096; x, gamma, beta and y 16-byte aligned; y must not be x. */
int vqw_lattice_inputs(const long* ids, long* inp, int B, int h, int w, int sy, int sx, int s0, int ns, long mask_token, void* stream);
int vqw_lattice_gather_ln(const float* x, const float* gamma, const float* beta, float* y, int B, int h, int w, int E, int sy, int sx,
                          int s0, int ns, float eps, void* stream);

/* ---- scores of the prior's samples (csrc/sample_scores.hip; functions/sample_scores.py, PriorTrainer.score, Fit.score; the
 * reference has nothing like it).  Added functions only; the ABI stays 9.  Feature rows x [N][D], fp32, dense, 1 <= D <= 2048, any
 * N >= 1 up to 2^30; a row is used as y = fp32(x - shift), one fp32 subtraction per element while staging, shift [D] or null (0):
 * the caller's centring, which keeps the Gram form below from cancelling on features far from the origin.  No float atomics; the
 * same bits every run.  Every refusal arrives with a message that names the constraint, before any launch: D or k out of range,
 * N < k + 1, a null or misaligned pointer (4 bytes for fp32 / int32, 8 for doubles), N or M above 2^30, a short workspace.
 * Moments: sum [D] += sum_n y and outer [D][D] += sum_n y y^T, both double and ACCUMULATED (the caller clears them once), the
 * products in double (exact for fp32 factors), plain double FMAs.  The rows are split over workgroups and each split is walked in
 * row order; the splits are folded in index order; both triangles of outer are written from one folded value, so it stays exactly
 * symmetric.  ws: vqw_feature_moments_ws_bytes(N, D) bytes, 8-byte aligned (0 for an argument out of range).
 * Distances: d2(q, a) = max(0, |q|^2 + |a|^2 - 2 q.a) in fp32, the products on the exact-fp32 matrix cores, the squared norms
 * through the same instruction in the same column order, so bit-identical rows have d2 exactly 0.  Centre tiles of 64 rows stream
 * through LDS against a query tile of 64 rows; the row reduction runs in registers; the N x M distances are never written and the
 * workspace holds the squared norms alone ((N + M) floats: vqw_knn_radius_ws_bytes(N), vqw_ball_counts_ws_bytes(M, N)).
 * vqw_knn_radius: r2 [N], r2[i] = the k-th smallest d2(i, j) over j != i - self is excluded by index, not by value; 1 <= k <= 8,
 * N >= k + 1.
 * vqw_ball_counts: queries q [M][D], centres a [N][D], r2 [N].  cnt_q [M] (int32) = the number of i with d2(q, a_i) <= r2[i]
 * (inclusive); hit_a [N] (int32) = the number of queries inside ball i, cleared by the call and counted with integer atomics
 * (counts have no order).  A NaN r2[i] contains nobody. */
size_t vqw_feature_moments_ws_bytes(long N, int D);
int vqw_feature_moments(const float* x, const float* shift, double* sum, double* outer, void* ws, size_t ws_bytes, long N, int D,
                        void* stream);
size_t vqw_knn_radius_ws_bytes(long N);
int vqw_knn_radius(const float* a, const float* shift, float* r2, void* ws, size_t ws_bytes, long N, int D, int k, void* stream);
size_t vqw_ball_counts_ws_bytes(long M, long N);
int vqw_ball_counts(const float* q, const float* a, const float* r2, const float* shift, int32_t* cnt_q, int32_t* hit_a, void* ws,
                    size_t ws_bytes, long M, long N, int D, void* stream);

/* ---- the seamless composite of an edit (csrc/blend.hip; ops.blend_cells, PriorTrainer.edit with blend="pyramid"; the reference has
 * nothing like it).  Added functions only; the ABI stays 9.  Burt-Adelson multi-band blending on NHWC fp32 pictures [N][H][W][C]
 * under the cell mask [N][h][w] bytes (non-zero: the edit; H = fy h, W = fx w).  Per image and channel, separable, clamped
 * (replicated) borders, w = [1, 4, 6, 4, 1] / 16:
 *   REDUCE(x)[i][j] = sum_m sum_n w[m] w[n] x[clamp(2i+m)][clamp(2j+n)], m, n = -2..2: (H, W) -> (H/2, W/2)
 *   EXPAND(x) to (2H, 2W), along each axis in turn: [2k] = (x[k-1] + 6 x[k] + x[k+1]) / 8, [2k+1] = (x[k] + x[k+1]) / 2, clamped
 *   M_0 = the mask at pixels (0 / 1), M_{l+1} = REDUCE(M_l); G_0 = d, G_{l+1} = REDUCE(G_l), d = edit - image, or edit - recon
 *   when recon is not null (the difference of two decodes: the first stage's own error cancels where the codes did not change)
 *   R_L = M_L G_L; R_l = M_l (G_l - EXPAND(G_{l+1})) + EXPAND(R_{l+1}) for l = L-1 .. 0; out = image + R_0,  L = levels.
 * Order: every filter runs its row pass (along x) first, then its column pass, taps ascending, accumulated from the left -
 * ((w0 x0 + w1 x1) + w2 x2) ... with the fp32 taps 0.0625, 0.25, 0.375; EXPAND is ((a + 6 b) + c) 0.125 and (b + c) 0.5; the band is
 * m (g - eg) + er; one fp32 rounding per operation, no fused multiply-add, no float atomics: the same bits every run.  Where the
 * mask pyramid is 0 under every tap, R_0 is exactly 0 and out has the bits of image.
 * Plan: `levels` reduce launches (the C planes of G and the plane of M of a level through one LDS tile with a 2-pixel halo) and
 * `levels` collapse launches (EXPAND of G and of R, the product with M and the sum fused over one LDS tile; R_L is formed while the
 * top collapse stages).  Level 0 is never stored: image and edit (or edit and recon) are read by the first reduce and again by the
 * last collapse, out is written once.  workspace: vqw_blend_cells_workspace(N, H, W, C, levels) floats - the planes of G_l, M_l for
 * l = 1..L and of R_l for l = 1..L-1; the query returns 0 for arguments out of range.
 * Refused, with a message before any launch: a null pointer (recon alone may be null); N, H, W or C < 1; levels outside [1, 12];
 * 2^levels not dividing H or W; H % h or W % w non-zero; a workspace that is too small; N > 65535 or C > 65534;
 * N H W (C + 1) >= 2^31; image, edit, recon, out or workspace not 16-byte aligned.  out must not be an input. */
long vqw_blend_cells_workspace(int N, int H, int W, int C, int levels);
int vqw_blend_cells(const float* image, const float* edit, const float* recon, const uint8_t* cellmask, float* out, float* workspace,
                    long workspace_floats, int N, int H, int W, int C, int h, int w, int levels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
