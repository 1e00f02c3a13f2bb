// LPIPS perceptual loss, lpips.LPIPS(net='alex') version 0.1 with its defaults (linear layers on, spatial=False, eval mode):
// the reference's LPIPSLoss (functions/lpips_loss.py, trainers/base.py:271-275).  The operator (hipops.ops.lpips_loss) runs
// one batch of 2M = 2 * nwin * N images like the VGG loss: the sr (recon) half first, then the hr (clear) half, each ordered
// (window, image).  The kernels here are the parts the stock convolutions do not cover:
//
//   stem forward      F1 = relu(conv11x11/4(scale(win(x))) + b), 1 or 3 input channels -> 64.  A block stages the 71 x 71
//                     input patch of a 16 x 16 output tile in LDS (split by x mod 4, so the 16 lanes of an output row read
//                     consecutive words) and computes 16 of the 64 channels; the weights are block-uniform (scalar loads).
//                     The window map is applied on load, then the scaling layer (x - shift) / scale, zero padding after both.
//                     With C = 1 the three input-channel weights fold into one, wA = sum_c w_c / scale_c, and the shifts into
//                     a per-tap constant wB = -sum_c w_c shift_c / scale_c that counts for in-bounds taps only: a second
//                     "plane" of 0 / 1 flags, summed on its own in tap order, which for a tile whose patch lies inside the
//                     image is the constant the caller passes (the same sum in the same order: bit-equal).
//   max-pool 3x3 / 2  forward; backward as a gather (each input pixel visits the <= 4 windows that hold it, recomputes each
//                     window's first maximum in row-major order - ATen's rule - and sums what it wins), with the ReLU mask
//                     of the layer in front applied to the values in hand
//   5x5 pad-2 conv    forward (+ bias, ReLU) and input gradient on the fp32 matrix cores: conv_mfma.hip's implicit-GEMM kernel
//                     with a 25-entry tap table
//   tap distance      per pixel a = f / (|f| + eps), b likewise from the hr half, d = sum_c w_c (a_c - b_c)^2; per (image,
//                     tap) double partials folded in one fixed order; the backward adds the gradient arriving from the deeper
//                     tap and applies the tap's ReLU mask in the same pass
//   stem input grad   64 -> Cin transposed stride-4 gather, times the scaling and window derivatives and each window's
//                     incoming loss gradient, summed over windows
//
// Every accumulation runs in one fixed order per output element, independent of its position: equal input neighbourhoods
// give bit-equal outputs, so plateaus of the input stay exact ties for the two max-pools.  No float atomics.
#include "common.h"
#include "conv_common.h"
#include "prof.h"
#include "../../include/vqwnet_hip.h"

#define LP_C1 64        // stem channels
#define LP_K 11         // stem kernel
#define LP_TAPS 121
#define LP_TILE 16      // stem output tile edge
#define LP_PATCH 71     // (LP_TILE - 1) * 4 + LP_K
#define LP_RS 20        // row stride of a phase plane: 4 rows apart = 80 words = 16 banks, the 4 rows of a wave never collide
#define LP_NB 16        // distance partials per (image, tap)
#define LP_EPS 1e-10f

__device__ __forceinline__ float lp_win(float x, const float* win) {
    return fminf(fmaxf(win[0] * x + win[1], win[2]), win[3]);
}

static inline int lp_out11(int n) { return (n + 4 - LP_K) / 4 + 1; }
static inline int lp_out3(int n) { return (n - 3) / 2 + 1; }

extern "C" int vqw_lpips_supported(int N, int Cin, int H, int W) {
    if (N < 1 || (Cin != 1 && Cin != 3) || H < 31 || W < 31) return 0;
    return (long)N * H * W <= (1L << 31) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// stem forward.  grid (tiles, 2M, 4): tile of 16 x 16 outputs, image, group of 16 output channels.
// wp: [planes][121][64]; planes = (wA, wB) for CIN 1, the raw w_c for CIN 3.  sc: shift[3], scale[3] (CIN 3).
template <int CIN>
__global__ __launch_bounds__(256) void k_lpips_stem_fwd(const float* __restrict__ sr, const float* __restrict__ hr,
                                                        const float* __restrict__ wp, const float* __restrict__ cint,
                                                        const float* __restrict__ sc, const float* __restrict__ bias,
                                                        const float* __restrict__ win, float* __restrict__ f1, int N, int nwin,
                                                        int H, int W, int Ho, int Wo, int tiles_x) {
    __shared__ float s[4 * LP_PATCH * LP_RS];
    constexpr int NP = CIN == 1 ? 2 : 3;
    const int tid = threadIdx.x, ox = tid & 15, oy = tid >> 4;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int g = blockIdx.z;
    const long b = blockIdx.y, M = (long)nwin * N;
    const int half = (int)(b / M);
    const long m = b - half * M;
    const int wi = (int)(m / N);
    const long n = m - (long)wi * N;
    const float* src = (half ? hr : sr) + n * H * W * CIN;
    float wv[4] = {1.f, 0.f, 0.f, 0.f};
    if (win) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = win[4 * wi + k];
    }
    const int iy0 = ty * (4 * LP_TILE) - 2, ix0 = tx * (4 * LP_TILE) - 2;
    const bool interior = iy0 >= 0 && iy0 + LP_PATCH <= H && ix0 >= 0 && ix0 + LP_PATCH <= W;      // block-uniform
    float acc[16], cc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = cc[j] = 0.f;

    auto stage = [&](int pl) {
        for (int e = tid; e < LP_PATCH * LP_PATCH; e += 256) {
            const int r = e / LP_PATCH, col = e - r * LP_PATCH;
            const int iy = iy0 + r, ix = ix0 + col;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                if (CIN == 1 && pl == 1) {
                    v = 1.f;
                } else {
                    v = src[((long)iy * W + ix) * CIN + (CIN == 1 ? 0 : pl)];
                    if (win) v = lp_win(v, wv);
                    if (CIN == 3) v = (v - sc[pl]) / sc[3 + pl];
                }
            }
            s[((col & 3) * LP_PATCH + r) * LP_RS + (col >> 2)] = v;
        }
    };
    auto run = [&](float (&d)[16], const float* __restrict__ wpl) {
        for (int ky = 0; ky < LP_K; ++ky) {
            const float* srow = s + (4 * oy + ky) * LP_RS + ox;
#pragma unroll
            for (int kx = 0; kx < LP_K; ++kx) {
                const float v = srow[(kx & 3) * LP_PATCH * LP_RS + (kx >> 2)];
                const float* wt = wpl + (ky * LP_K + kx) * LP_C1;
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = fmaf(wt[j], v, d[j]);
            }
        }
    };

    for (int pl = 0; pl < NP; ++pl) {
        if (CIN == 1 && pl == 1 && interior) {
#pragma unroll
            for (int j = 0; j < 16; ++j) cc[j] = cint[16 * g + j];
            break;
        }
        if (pl) __syncthreads();
        stage(pl);
        __syncthreads();
        const float* wpl = wp + (long)pl * LP_TAPS * LP_C1 + 16 * g;
        if (CIN == 1 && pl == 1)
            run(cc, wpl);
        else
            run(acc, wpl);
    }
    const int oyg = ty * LP_TILE + oy, oxg = tx * LP_TILE + ox;
    if (oyg < Ho && oxg < Wo) {
        float* o = f1 + (((long)b * Ho + oyg) * Wo + oxg) * LP_C1 + 16 * g;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            float4_t v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf((acc[4 * j4 + j] + cc[4 * j4 + j]) + bias[16 * g + 4 * j4 + j], 0.f);
            *(float4_t*)(o + 4 * j4) = v;
        }
    }
}

extern "C" int vqw_lpips_stem_fwd(const float* sr, const float* hr, const float* wp, const float* cint, const float* sc,
                                  const float* bias, const float* win, float* f1, int N, int nwin, int Cin, int H, int W,
                                  void* stream) {
    VQW_CHECK(sr && hr && wp && bias && f1, "vqw_lpips_stem_fwd: bad arguments");
    VQW_CHECK(vqw_lpips_supported(N, Cin, H, W), "vqw_lpips_stem_fwd: unsupported shape N=%d Cin=%d H=%d W=%d", N, Cin, H, W);
    VQW_CHECK(Cin == 1 ? cint != nullptr : sc != nullptr, "vqw_lpips_stem_fwd: Cin=1 needs cint, Cin=3 needs sc");
    VQW_CHECK(nwin >= 1 && nwin <= 3 && (win || nwin == 1), "vqw_lpips_stem_fwd: nwin=%d needs a window table (1..3)", nwin);
    const int Ho = lp_out11(H), Wo = lp_out11(W);
    const long B = 2L * nwin * N;
    VQW_CHECK(B <= 65535, "vqw_lpips_stem_fwd: batch too large (%ld images)", B);
    const int tx = ceil_div(Wo, LP_TILE), ty = ceil_div(Ho, LP_TILE);
    const double P = (double)B * Ho * Wo;
    ProfScope ps(2, 2.0 * P * LP_C1 * LP_TAPS * (Cin == 1 ? 2 : 3), (hipStream_t)stream, 4.0 * (B * (double)H * W * Cin + P * LP_C1));
    const dim3 grid(tx * ty, (unsigned)B, 4);
    if (Cin == 1)
        k_lpips_stem_fwd<1><<<grid, 256, 0, (hipStream_t)stream>>>(sr, hr, wp, cint, sc, bias, win, f1, N, nwin, H, W, Ho, Wo, tx);
    else
        k_lpips_stem_fwd<3><<<grid, 256, 0, (hipStream_t)stream>>>(sr, hr, wp, cint, sc, bias, win, f1, N, nwin, H, W, Ho, Wo, tx);
    VQW_LAUNCH_CHECK("vqw_lpips_stem_fwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// stem input gradient.  Thread = one input pixel x 4 of the 64 gradient channels, all windows; the 16 lanes of a pixel are
// combined by a fixed butterfly.  Input pixel (y, x) meets output (oy, ox) at tap (y + 2 - 4 oy, x + 2 - 4 ox): <= 3 x 3.
template <int CIN>
__global__ __launch_bounds__(256) void k_lpips_stem_bwd(const float* __restrict__ sr, const float* __restrict__ wp,
                                                        const float* __restrict__ sc, const float* __restrict__ win,
                                                        const float* __restrict__ g0, const float* __restrict__ g1,
                                                        const float* __restrict__ g2, const float* __restrict__ dz1,
                                                        float* __restrict__ gsr, int N, int nwin, int H, int W, int Ho, int Wo) {
    const int q = threadIdx.x & 15;
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = p < (long)N * HW;          // whole 16-lane groups: every lane takes part in the shuffles
    const long n = live ? p / HW : 0;
    const int r = live ? (int)(p - n * HW) : 0, y = r / W, x = r - y * W;
    const int oy_lo = max(0, (y - 8 + 3) >> 2), oy_hi = min(Ho - 1, (y + 2) >> 2);
    const int ox_lo = max(0, (x - 8 + 3) >> 2), ox_hi = min(Wo - 1, (x + 2) >> 2);
    float g[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) g[ci] = 0.f;
    for (int wi = 0; wi < nwin; ++wi) {
        const float* gl = wi == 0 ? g0 : wi == 1 ? g1 : g2;
        const float s = gl[0];
        const float* dz = dz1 + ((long)wi * N + n) * Ho * Wo * LP_C1 + 4 * q;
        float acc[CIN];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
        if (live) {
            for (int oy = oy_lo; oy <= oy_hi; ++oy)
                for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                    const int t = (y + 2 - 4 * oy) * LP_K + (x + 2 - 4 * ox);
                    const float4_t v = *(const float4_t*)(dz + ((long)oy * Wo + ox) * LP_C1);
#pragma unroll
                    for (int ci = 0; ci < CIN; ++ci) {
                        const float4_t wv = *(const float4_t*)(wp + ((long)ci * LP_TAPS + t) * LP_C1 + 4 * q);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[ci] = fmaf(wv[j], v[j], acc[ci]);
                    }
                }
        }
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[ci] += __shfl_xor(acc[ci], o, 64);
            float f = s;
            if (win && live) {
                const float* wv = win + 4 * wi;
                const float z = wv[0] * sr[p * CIN + ci] + wv[1];
                f = (z > wv[2] && z < wv[3]) ? s * wv[0] : 0.f;
            }
            if (CIN == 3) f = f / sc[3 + ci];
            g[ci] = fmaf(acc[ci], f, g[ci]);
        }
    }
    if (live && q == 0) {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) gsr[p * CIN + ci] = g[ci];
    }
}

extern "C" int vqw_lpips_stem_bwd(const float* sr, const float* wp, const float* sc, const float* win, const float* g0,
                                  const float* g1, const float* g2, const float* dz1, float* gsr, int N, int nwin, int Cin, int H,
                                  int W, void* stream) {
    VQW_CHECK(sr && wp && g0 && dz1 && gsr, "vqw_lpips_stem_bwd: bad arguments");
    VQW_CHECK(vqw_lpips_supported(N, Cin, H, W), "vqw_lpips_stem_bwd: unsupported shape N=%d Cin=%d H=%d W=%d", N, Cin, H, W);
    VQW_CHECK(Cin == 1 || sc, "vqw_lpips_stem_bwd: Cin=3 needs sc");
    VQW_CHECK(nwin >= 1 && nwin <= 3 && (win || nwin == 1) && (nwin < 2 || g1) && (nwin < 3 || g2),
              "vqw_lpips_stem_bwd: nwin=%d needs a window table and one loss gradient per window", nwin);
    const long P = (long)N * H * W;
    const int Ho = lp_out11(H), Wo = lp_out11(W);
    ProfScope ps(2, 2.0 * nwin * N * (double)Ho * Wo * LP_C1 * LP_TAPS * Cin, (hipStream_t)stream,
                 4.0 * (nwin * N * (double)Ho * Wo * LP_C1 + 2.0 * P * Cin));
    const long blocks = (P + 15) / 16;
    VQW_CHECK(blocks < (1L << 31), "vqw_lpips_stem_bwd: batch too large");
    if (Cin == 1)
        k_lpips_stem_bwd<1><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, wp, sc, win, g0, g1, g2, dz1, gsr, N, nwin, H, W, Ho, Wo);
    else
        k_lpips_stem_bwd<3><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, wp, sc, win, g0, g1, g2, dz1, gsr, N, nwin, H, W, Ho, Wo);
    VQW_LAUNCH_CHECK("vqw_lpips_stem_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, stride 2), floor mode.  Thread = one pixel x 4 channels.
__global__ __launch_bounds__(256) void k_lpips_pool_fwd(const float4_t* __restrict__ x, float4_t* __restrict__ y, int N, int H, int W,
                                                        int Ho, int Wo, int C4) {
    const long total = (long)N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % Wo);
        p /= Wo;
        const int ho = (int)(p % Ho);
        const long n = p / Ho;
        const float4_t* b = x + ((n * H + 2 * ho) * W + 2 * wo) * C4 + c;
        float4_t m = b[0];
#pragma unroll
        for (int t = 1; t < 9; ++t) {
            const float4_t v = b[((long)(t / 3) * W + t % 3) * C4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
        }
        y[i] = m;
    }
}

extern "C" int vqw_lpips_pool_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    VQW_PROF_HBM(stream, 1.25, (double)N * H * W * C);
    VQW_CHECK(x && y && N > 0 && C > 0 && C % 4 == 0 && H >= 3 && W >= 3, "vqw_lpips_pool_fwd: bad arguments (N=%d H=%d W=%d C=%d)", N, H, W, C);
    const int Ho = lp_out3(H), Wo = lp_out3(W);
    const long total = (long)N * Ho * Wo * (C / 4);
    k_lpips_pool_fwd<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>((const float4_t*)x, (float4_t*)y, N, H, W, Ho, Wo, C / 4);
    VQW_LAUNCH_CHECK("vqw_lpips_pool_fwd");
    return VQW_OK;
}

// gx[y, x] = [x > 0] * sum over the windows (oy, ox) holding (y, x) whose first row-major maximum is (y, x) of gy[oy, ox]
__global__ __launch_bounds__(256) void k_lpips_pool_bwd(const float4_t* __restrict__ x, const float4_t* __restrict__ gy,
                                                        float4_t* __restrict__ gx, int N, int H, int W, int Ho, int Wo, int C4) {
    const long total = (long)N * H * W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long p = i / C4;
        const int w = (int)(p % W);
        p /= W;
        const int h = (int)(p % H);
        const long n = p / H;
        const float4_t me = x[i];
        float4_t g = {0.f, 0.f, 0.f, 0.f};
        const int oy_lo = h >= 2 ? (h - 1) >> 1 : 0, oy_hi = min(Ho - 1, h >> 1);
        const int ox_lo = w >= 2 ? (w - 1) >> 1 : 0, ox_hi = min(Wo - 1, w >> 1);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const float4_t* b = x + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c;
                const int mine = (h - 2 * oy) * 3 + (w - 2 * ox);
                float4_t m = b[0];
                int am[4] = {0, 0, 0, 0};
#pragma unroll
                for (int t = 1; t < 9; ++t) {
                    const float4_t v = b[((long)(t / 3) * W + t % 3) * C4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (v[j] > m[j]) { m[j] = v[j]; am[j] = t; }
                }
                const float4_t gv = gy[((n * Ho + oy) * Wo + ox) * C4 + c];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (am[j] == mine) g[j] += gv[j];
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = me[j] > 0.f ? g[j] : 0.f;
        gx[i] = g;
    }
}

extern "C" int vqw_lpips_pool_bwd(const float* x, const float* gy, float* gx, int N, int H, int W, int C, void* stream) {
    VQW_PROF_HBM(stream, 2.25, (double)N * H * W * C);
    VQW_CHECK(x && gy && gx && N > 0 && C > 0 && C % 4 == 0 && H >= 3 && W >= 3, "vqw_lpips_pool_bwd: bad arguments (N=%d H=%d W=%d C=%d)", N, H, W, C);
    const long total = (long)N * H * W * (C / 4);
    k_lpips_pool_bwd<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>((const float4_t*)x, (const float4_t*)gy, (float4_t*)gx, N, H, W,
                                                                              lp_out3(H), lp_out3(W), C / 4);
    VQW_LAUNCH_CHECK("vqw_lpips_pool_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// 5x5 padding-2 convolution on the implicit-GEMM matrix-core kernel (forward; the input gradient is the same call on the
// gradient with vqw_pack_dgrad_weights(.., 5) weights, Cin / Cout swapped)
extern "C" int vqw_lpips_conv5_supported(int Cin, int Cout, int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || Cin < 8 || Cout < 8 || Cin % 4 || Cout % 4) return 0;
    return (long)N * H * W * (long)(Cin > Cout ? Cin : Cout) * 4 <= 0xFFFFFFE0L ? 1 : 0;
}

extern "C" int vqw_lpips_conv5_fwd(const float* x, const float* w_ohwi, const float* bias, float* y, int N, int H, int W, int Cin,
                                   int Cout, int relu, void* stream) {
    VQW_CHECK(x && w_ohwi && y && (relu == 0 || relu == 1), "vqw_lpips_conv5_fwd: bad arguments");
    VQW_CHECK(vqw_lpips_conv5_supported(Cin, Cout, N, H, W), "vqw_lpips_conv5_fwd: unsupported shape N=%d H=%d W=%d Cin=%d Cout=%d", N, H, W,
              Cin, Cout);
    const double px = (double)N * H * W;
    ProfScope ps(0, 2.0 * px * Cout * 25.0 * Cin, (hipStream_t)stream, 4.0 * (px * Cin + px * Cout + 25.0 * Cin * Cout));
    return conv_k5_grid(x, w_ohwi, bias, y, N, H, W, Cin, Cout, relu, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// tap distance.  A group of 16 lanes owns a pixel: lane q holds channels 4q + 64k .. + 3, k < C / 64, of both halves.
template <int C64>
__device__ __forceinline__ void lp_load(const float* __restrict__ f, float4_t (&v)[C64], int q) {
#pragma unroll
    for (int k = 0; k < C64; ++k) v[k] = *(const float4_t*)(f + 64 * k + 4 * q);
}
__device__ __forceinline__ float lp_sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int C64>
__device__ __forceinline__ float lp_sumsq(const float4_t (&v)[C64]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < C64; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(v[k][j], v[k][j], s);
    return lp_sum16(s);
}

// grid (LP_NB, M): block k of image m strides over the image's pixels in a fixed pattern; part[m][k]
template <int C64>
__global__ __launch_bounds__(256) void k_lpips_dist_fwd(const float* __restrict__ f, const float* __restrict__ lw,
                                                        double* __restrict__ part, long M, int HW) {
    __shared__ double sm[4];
    constexpr int C = 64 * C64;
    const int q = threadIdx.x & 15, pg = threadIdx.x >> 4;
    const long m = blockIdx.y;
    float4_t w[C64];
    lp_load<C64>(lw, w, q);
    double acc = 0.0;
    const int iters = (HW + LP_NB * 16 - 1) / (LP_NB * 16);
    for (int it = 0; it < iters; ++it) {
        const int p = (it * LP_NB + blockIdx.x) * 16 + pg;
        const bool live = p < HW;
        float4_t a[C64], b[C64];
        const long off = (long)(live ? p : 0) * C;
        lp_load<C64>(f + m * HW * C + off, a, q);
        lp_load<C64>(f + (M + m) * HW * C + off, b, q);
        const float ia = 1.f / (sqrtf(lp_sumsq<C64>(a)) + LP_EPS), ib = 1.f / (sqrtf(lp_sumsq<C64>(b)) + LP_EPS);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < C64; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = a[k][j] * ia - b[k][j] * ib;
                d = fmaf(w[k][j] * e, e, d);
            }
        d = lp_sum16(d);
        if (live && q == 0) acc += (double)d;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[m * LP_NB + blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

extern "C" size_t vqw_lpips_ws_bytes(int N, int nwin) {
    return (size_t)5 * (nwin > 0 ? nwin : 1) * (N > 0 ? N : 1) * LP_NB * sizeof(double);
}

static bool lp_dist_c_ok(int C) { return C == 64 || C == 192 || C == 256 || C == 384; }

extern "C" int vqw_lpips_dist_fwd(const float* f, const float* lw, void* ws, size_t ws_bytes, int tap, int N, int nwin, int HW, int C,
                                  void* stream) {
    VQW_CHECK(f && lw && ws && tap >= 0 && tap < 5 && N >= 1 && nwin >= 1 && nwin <= 3 && HW >= 1, "vqw_lpips_dist_fwd: bad arguments");
    VQW_CHECK(lp_dist_c_ok(C), "vqw_lpips_dist_fwd: C=%d is not a tap width of the AlexNet front end (64, 192, 384, 256)", C);
    VQW_CHECK(ws_bytes >= vqw_lpips_ws_bytes(N, nwin), "vqw_lpips_dist_fwd: workspace too small");
    const long M = (long)nwin * N;
    VQW_CHECK(M <= 65535, "vqw_lpips_dist_fwd: batch too large");
    VQW_PROF_HBM(stream, 2, (double)M * HW * C);
    double* part = (double*)ws + (long)tap * M * LP_NB;
    const dim3 grid(LP_NB, (unsigned)M);
    hipStream_t st = (hipStream_t)stream;
    switch (C / 64) {
        case 1: k_lpips_dist_fwd<1><<<grid, 256, 0, st>>>(f, lw, part, M, HW); break;
        case 3: k_lpips_dist_fwd<3><<<grid, 256, 0, st>>>(f, lw, part, M, HW); break;
        case 4: k_lpips_dist_fwd<4><<<grid, 256, 0, st>>>(f, lw, part, M, HW); break;
        default: k_lpips_dist_fwd<6><<<grid, 256, 0, st>>>(f, lw, part, M, HW); break;
    }
    VQW_LAUNCH_CHECK("vqw_lpips_dist_fwd");
    return VQW_OK;
}

struct LpScales { double s[5]; };

// loss[w] = sum_tap sum_n sum_k part[tap][w * N + n][k] / (HW_tap * N): one block per window, a fixed-order fold
__global__ __launch_bounds__(256) void k_lpips_fold(const double* __restrict__ part, int N, long M, LpScales sc, float* __restrict__ loss) {
    __shared__ double sm[4];
    const int per = N * LP_NB;
    double acc = 0.0;
    for (int tap = 0; tap < 5; ++tap) {
        const double* pw = part + ((long)tap * M + (long)blockIdx.x * N) * LP_NB;
        double a = 0.0;
        for (int i = threadIdx.x; i < per; i += blockDim.x) a += pw[i];
        acc += a * sc.s[tap];
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)((sm[0] + sm[1]) + (sm[2] + sm[3]));
}

extern "C" int vqw_lpips_loss_fold(const void* ws, size_t ws_bytes, float* loss, int N, int nwin, int hw0, int hw1, int hw2, int hw3,
                                   int hw4, void* stream) {
    VQW_CHECK(ws && loss && N >= 1 && nwin >= 1 && nwin <= 3 && hw0 > 0 && hw1 > 0 && hw2 > 0 && hw3 > 0 && hw4 > 0,
              "vqw_lpips_loss_fold: bad arguments");
    VQW_CHECK(ws_bytes >= vqw_lpips_ws_bytes(N, nwin), "vqw_lpips_loss_fold: workspace too small");
    const int hw[5] = {hw0, hw1, hw2, hw3, hw4};
    LpScales sc;
    for (int t = 0; t < 5; ++t) sc.s[t] = 1.0 / ((double)hw[t] * N);
    k_lpips_fold<<<nwin, 256, 0, (hipStream_t)stream>>>((const double*)ws, N, (long)nwin * N, sc, loss);
    VQW_LAUNCH_CHECK("vqw_lpips_loss_fold");
    return VQW_OK;
}

// gout = [f > 0] * (gin + scale * (2 / n0) * (w delta - a S / r)), r = |f|, n0 = r + eps, a = f / n0, delta = a - b,
// S = sum_k w_k delta_k f_k; the distance term is zero where r = 0.  gin may be NULL (the deepest tap) or gout itself.
template <int C64>
__global__ __launch_bounds__(256) void k_lpips_dist_bwd(const float* __restrict__ f, const float* __restrict__ lw, const float* gin,
                                                        float* gout, long M, int HW, float scale) {
    constexpr int C = 64 * C64;
    const int q = threadIdx.x & 15;
    const long P = M * HW;
    float4_t w[C64];
    lp_load<C64>(lw, w, q);
    const long groups = (long)gridDim.x * 16;
    const long iters = (P + groups - 1) / groups;
    for (long it = 0; it < iters; ++it) {
        const long p = (it * gridDim.x + blockIdx.x) * 16 + (threadIdx.x >> 4);
        const bool live = p < P;
        const long off = (live ? p : 0) * C;
        float4_t a[C64], b[C64];
        lp_load<C64>(f + off, a, q);
        lp_load<C64>(f + P * C + off, b, q);
        const float r = sqrtf(lp_sumsq<C64>(a));
        const float ia = 1.f / (r + LP_EPS), ib = 1.f / (sqrtf(lp_sumsq<C64>(b)) + LP_EPS);
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < C64; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                b[k][j] = w[k][j] * (a[k][j] * ia - b[k][j] * ib);       // w delta
                S = fmaf(b[k][j], a[k][j], S);
            }
        S = lp_sum16(S);
        const float coef = r > 0.f ? S / r * ia : 0.f, s2 = r > 0.f ? 2.f * scale * ia : 0.f;
        if (live) {
#pragma unroll
            for (int k = 0; k < C64; ++k) {
                float4_t gi = {0.f, 0.f, 0.f, 0.f};
                if (gin) gi = *(const float4_t*)(gin + off + 64 * k + 4 * q);
                float4_t o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = a[k][j] > 0.f ? fmaf(s2, b[k][j] - a[k][j] * coef, gi[j]) : 0.f;
                *(float4_t*)(gout + off + 64 * k + 4 * q) = o;
            }
        }
    }
}

extern "C" int vqw_lpips_dist_bwd(const float* f, const float* lw, const float* gin, float* gout, int N, int nwin, int HW, int C,
                                  void* stream) {
    VQW_CHECK(f && lw && gout && N >= 1 && nwin >= 1 && nwin <= 3 && HW >= 1, "vqw_lpips_dist_bwd: bad arguments");
    VQW_CHECK(lp_dist_c_ok(C), "vqw_lpips_dist_bwd: C=%d is not a tap width of the AlexNet front end (64, 192, 384, 256)", C);
    const long M = (long)nwin * N;
    VQW_PROF_HBM(stream, gin ? 4 : 3, (double)M * HW * C);
    const float scale = (float)(1.0 / ((double)HW * N));
    const int grid = stream_grid(M * HW * 16, 256);
    hipStream_t st = (hipStream_t)stream;
    switch (C / 64) {
        case 1: k_lpips_dist_bwd<1><<<grid, 256, 0, st>>>(f, lw, gin, gout, M, HW, scale); break;
        case 3: k_lpips_dist_bwd<3><<<grid, 256, 0, st>>>(f, lw, gin, gout, M, HW, scale); break;
        case 4: k_lpips_dist_bwd<4><<<grid, 256, 0, st>>>(f, lw, gin, gout, M, HW, scale); break;
        default: k_lpips_dist_bwd<6><<<grid, 256, 0, st>>>(f, lw, gin, gout, M, HW, scale); break;
    }
    VQW_LAUNCH_CHECK("vqw_lpips_dist_bwd");
    return VQW_OK;
}
