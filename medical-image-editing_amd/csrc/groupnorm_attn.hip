// GroupNorm(32 groups, affine)(+swish) and single-head self-attention over a feature map: the two kernel families of the
// VQGAN decoder blocks (networks/vqgan.py: Normalize / nonlinearity :10-19, AttnBlock :125-180).  NHWC fp32.
//
// GroupNorm.  A thread owns one float4 column (four channels) of the tensor and walks pixels, so gamma, beta and the
// statistics of its channels are loaded once.  Every reduction is two-stage and deterministic: per-thread double sums, a
// fixed fold over the workgroup's rows in LDS to per-channel sums, then per-(image, split, channel) double partials that a
// finalise pass folds in a fixed order (norm.hip's scheme; a channel's splits are dealt to several threads).  Groups are folded
// from channel sums, so any channel count that is a multiple of 32 works - a group of 3 channels (C = 96) does not have to be a
// float4 multiple.  A plane of at most GN_ONE_WG_ELEMS elements per image takes one workgroup that finalises in its own tail; a
// larger one is split.
//
// Attention.  o = softmax(scale q k^T) v per batch element, q, k, v [B][N][C].  All five matrix products (q k^T and p v
// forward; recomputed q k^T, dO v^T, dS k, dS^T q and p^T dO backward) are one of two forms on the exact-fp32 32x32x2 MFMA:
//   attn_gemm_nt: T[32][64] = A[32 rows][C] . B[64 rows][C]^T   (operands staged in LDS in chunks of <= 128 channels)
//   attn_gemm_pv: acc[32][C] += P[32][64] (LDS) . B[64 rows][C]  (each wave owns the 32-column blocks w, w + 4, ...)
// A workgroup owns 32 "tile rows" (queries forward and for dQ; keys for dK / dV, where the transposed score tile is computed
// directly as k q^T - no transposed LDS reads) and walks the other axis in tiles of 64.  The N x N matrix never leaves LDS.
// No atomics anywhere: every output element is written by one thread, sums run in a fixed order.
#include <type_traits>
#include "common.h"
#include "mfma_util.h"
#include "../../include/vqwnet_hip.h"

__device__ __forceinline__ int imin_d(int a, int b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------------- GroupNorm
#define GN_GROUPS 32
#define GN_ONE_WG_ELEMS 16384      // H*W*C per image up to which one workgroup per image reduces the whole plane
#define GN_MAX_SPLITS 256
#define GN_MAX_C 1024              // one float4 column per thread of a 256-thread workgroup

static inline int gn_splits(int HW, int C) {
    const long elems = (long)HW * C;
    if (elems <= GN_ONE_WG_ELEMS) return 1;
    return imin(GN_MAX_SPLITS, ceil_div(elems, GN_ONE_WG_ELEMS));
}
extern "C" int vqw_groupnorm_splits(int HW, int C) { return (HW < 1 || C < 1) ? 0 : gn_splits(HW, C); }
// partials [N][splits][C][2] doubles, the per-(image, channel) totals [N][C][2] doubles, then the backward's group means
// [N][32][2] floats
static inline size_t gn_part_bytes(int N, int HW, int C) { return (size_t)N * gn_splits(HW, C) * C * 2 * sizeof(double); }
static inline size_t gn_tot_bytes(int N, int C) { return (size_t)N * C * 2 * sizeof(double); }
extern "C" size_t vqw_groupnorm_ws_bytes(int N, int HW, int C) {
    if (N < 1 || HW < 1 || C < 1) return 0;
    return gn_part_bytes(N, HW, C) + gn_tot_bytes(N, C) + (size_t)N * GN_GROUPS * 2 * sizeof(float);
}

// The per-element formulas, each written once.
__device__ __forceinline__ float gn_sigmoid(float u) { return 1.f / (1.f + expf(-u)); }
// u = gamma * xhat + beta (the pre-activation, recomputed in the backward); xh = xhat
__device__ __forceinline__ float gn_pre(float x, float mean, float rstd, float gamma, float beta, float& xh) {
    xh = (x - mean) * rstd;
    return fmaf(gamma, xh, beta);
}
template <int SWISH>
__device__ __forceinline__ float gn_act(float u) { return SWISH ? u * gn_sigmoid(u) : u; }
// g' = g * swish'(u), swish'(u) = s (1 + u (1 - s)), s = sigmoid(u)
template <int SWISH>
__device__ __forceinline__ float gn_gprime(float g, float u) {
    if (!SWISH) return g;
    const float s = gn_sigmoid(u);
    return g * (s * fmaf(u, 1.f - s, 1.f));
}
// dx = rstd * (gamma g' - mean_group(gamma g') - xhat * mean_group(gamma g' xhat))
__device__ __forceinline__ float gn_bwd_out(float gp, float gamma, float xh, float rstd, float e1, float e2) {
    return rstd * (gamma * gp - e1 - xh * e2);
}
// (sum, sum of squares) over m values -> (mean, rstd); in double: no fp32 quantity holds E[x^2] - mean^2
__device__ __forceinline__ void gn_stats_finalize(double s, double ss, double m, float eps, float& mean, float& rstd) {
    const double mu = s / m;
    double var = ss / m - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// How a 256-thread workgroup lies on a [pixels][C] slab: `cols` = C / 4 float4 columns, `rows` = 256 / cols pixel rows.
struct GnWalk {
    int col, row, rows;
    bool active;
    __device__ GnWalk(int C) {
        const int cols = C >> 2;
        rows = 256 / cols;
        col = threadIdx.x % cols;
        row = threadIdx.x / cols;
        active = row < rows;
    }
};

// A thread's walk over its pixels p, p + step, ... < end with GN_UNROLL loads in flight: body(integral_constant<U>, p) handles
// the U pixels p, p + step, ..., loading all of them before it uses any (one 16-byte load per iteration does not fill HBM).
// The pixels are still visited in order, so a sum accumulated by the body keeps one fixed order.
#define GN_UNROLL 4
// the loads above this point are issued before any instruction below it (the scheduler would otherwise sink each load to
// its use to save registers, and serialise them again)
__device__ __forceinline__ void gn_loads_issued() { __builtin_amdgcn_sched_barrier(0); }
// the same for a batch of float4 loads whose uses are separated by stores: every value passes through one empty asm statement,
// so all of the batch's loads are issued before its first use
template <int U>
__device__ __forceinline__ void gn_pin(float4_t (&v)[U]) {
    if constexpr (U == GN_UNROLL) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}
static_assert(GN_UNROLL == 4, "gn_pin names four values");
template <class Body>
__device__ __forceinline__ void gn_walk_pixels(int p, int step, int end, Body body) {
    for (; p + (GN_UNROLL - 1) * step < end; p += GN_UNROLL * step) body(std::integral_constant<int, GN_UNROLL>(), p);
    for (; p < end; p += step) body(std::integral_constant<int, 1>(), p);
}

// per-channel constants of a thread's four channels
struct GnChan {
    float mean[4], rstd[4], gamma[4], beta[4];
    __device__ void load(const float* mean_n, const float* rstd_n, const float* gm, const float* bt, int c0, int cg) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = (c0 + i) / cg;
            mean[i] = mean_n[g]; rstd[i] = rstd_n[g]; gamma[i] = gm[c0 + i]; beta[i] = bt[c0 + i];
        }
    }
};
__device__ __forceinline__ void gn_unpack(const float4& v, float* o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void gn_unpack(const float4_t& v, float* o) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }

// Reduction functors: load(idx) fetches a pixel's float4 column, terms(in, a, b) adds the two summands of its four channels.
struct FGnStats {
    const float* x;
    static constexpr bool kKeepChannels = false;       // the one-workgroup tier needs no partials
    float* mean; float* rstd; float eps;
    __device__ void setup(int, int, int) {}
    struct In { float4 x; };
    __device__ In load(long idx) const { return In{*(const float4*)(x + idx)}; }
    __device__ void terms(const In& in, double* a, double* b) const {
        float v[4];
        gn_unpack(in.x, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double d = (double)v[i]; a[i] += d; b[i] = fma(d, d, b[i]); }
    }
    // chan: this image's per-channel sums [C][2]
    __device__ void finalize(int n, int g, const double* chan, int cg, double m) const {
        double s = 0.0, ss = 0.0;
        for (int c = g * cg; c < (g + 1) * cg; ++c) { s += chan[2 * c]; ss += chan[2 * c + 1]; }
        gn_stats_finalize(s, ss, m, eps, mean[n * GN_GROUPS + g], rstd[n * GN_GROUPS + g]);
    }
};
template <int SWISH>
struct FGnBwd {
    const float* x; const float* gy; const float* mean; const float* rstd; const float* gamma; const float* beta;
    float* gmeans;                                      // [N][32][2]: mean over the group of gamma g', of gamma g' xhat
    static constexpr bool kKeepChannels = true;        // dgamma / dbeta fold the per-(image, channel) sums
    GnChan ch;
    __device__ void setup(int n, int c0, int cg) { ch.load(mean + n * GN_GROUPS, rstd + n * GN_GROUPS, gamma, beta, c0, cg); }
    struct In { float4 x, g; };
    __device__ In load(long idx) const { return In{*(const float4*)(x + idx), *(const float4*)(gy + idx)}; }
    __device__ void terms(const In& in, double* a, double* b) const {
        float v[4], g[4];
        gn_unpack(in.x, v);
        gn_unpack(in.g, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float xh;
            const float u = gn_pre(v[i], ch.mean[i], ch.rstd[i], ch.gamma[i], ch.beta[i], xh);
            const float gp = gn_gprime<SWISH>(g[i], u);
            a[i] += (double)gp;
            b[i] += (double)(gp * xh);
        }
    }
    __device__ void finalize(int n, int g, const double* chan, int cg, double m) const {
        double s1 = 0.0, s2 = 0.0;
        for (int c = g * cg; c < (g + 1) * cg; ++c) { s1 += (double)gamma[c] * chan[2 * c]; s2 += (double)gamma[c] * chan[2 * c + 1]; }
        gmeans[(n * GN_GROUPS + g) * 2] = (float)(s1 / m);
        gmeans[(n * GN_GROUPS + g) * 2 + 1] = (float)(s2 / m);
    }
};

// grid (splits, N).  Workgroup (s, n) reduces the pixels [s * chunk, (s + 1) * chunk) of image n to per-channel sums.
// LDS: red [rows][C][2] doubles (rows * C <= 1024) and chan [C][2] doubles.
template <class F, bool ONE_WG>
__global__ void __launch_bounds__(256) k_gn_reduce(F f, double* __restrict__ part, double* __restrict__ tot, int HW, int C, int cg, int chunk) {
    __shared__ double red[2048];
    __shared__ double chan[2 * GN_MAX_C];
    const int n = blockIdx.y, s = blockIdx.x, splits = gridDim.x;
    const GnWalk w(C);
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    if (w.active) {
        f.setup(n, w.col * 4, cg);
        const int p1 = imin_d(HW, (s + 1) * chunk);
        const long base = (long)n * HW * C + w.col * 4;
        const int rows = w.rows;
        gn_walk_pixels(s * chunk + w.row, rows, p1, [&](auto uc, int p) {
            constexpr int U = decltype(uc)::value;
            typename F::In in[U];
#pragma unroll
            for (int u = 0; u < U; ++u) in[u] = f.load(base + (long)(p + u * rows) * C);
            gn_loads_issued();
#pragma unroll
            for (int u = 0; u < U; ++u) f.terms(in[u], a, b);
        });
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            red[(w.row * C + w.col * 4 + i) * 2] = a[i];
            red[(w.row * C + w.col * 4 + i) * 2 + 1] = b[i];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double sa = 0.0, sb = 0.0;
        for (int r = 0; r < w.rows; ++r) { sa += red[(r * C + c) * 2]; sb += red[(r * C + c) * 2 + 1]; }
        if (ONE_WG) { chan[2 * c] = sa; chan[2 * c + 1] = sb; }
        if (!ONE_WG || F::kKeepChannels) {
            double* o = ONE_WG ? tot + ((long)n * C + c) * 2 : part + (((long)n * splits + s) * C + c) * 2;
            o[0] = sa; o[1] = sb;
        }
    }
    if (ONE_WG) {
        __syncthreads();
        if (threadIdx.x < GN_GROUPS) f.finalize(n, threadIdx.x, chan, cg, (double)HW * cg);
    }
}

// grid N: the split partials of image n folded in a fixed order, then the groups.  A channel's splits are dealt to L = 256 / C
// threads (lane l adds the splits l, l + L, ... in index order; the lanes are then added in lane order), so the fold is not one
// thread's chain of `splits` dependent loads; C > 256 takes 256 channels per round with L = 1.
template <class F>
__global__ void __launch_bounds__(256) k_gn_finalize(F f, const double* __restrict__ part, double* __restrict__ tot, int HW, int C, int cg,
                                                     int splits) {
    __shared__ double chan[2 * GN_MAX_C];
    __shared__ double lanes[512];
    const int n = blockIdx.x;
    const int L = C <= 256 ? 256 / C : 1;
    for (int c0 = 0; c0 < C; c0 += 256) {
        const int cw = imin_d(256, C - c0), c = threadIdx.x % cw, l = threadIdx.x / cw;
        if (l < L) {
            double sa = 0.0, sb = 0.0;
            for (int s = l; s < splits; s += L) {
                const double* o = part + (((long)n * splits + s) * C + c0 + c) * 2;
                sa += o[0]; sb += o[1];
            }
            lanes[(l * cw + c) * 2] = sa; lanes[(l * cw + c) * 2 + 1] = sb;
        }
        __syncthreads();
        if (threadIdx.x < cw) {
            double sa = 0.0, sb = 0.0;
            for (int k = 0; k < L; ++k) { sa += lanes[(k * cw + c) * 2]; sb += lanes[(k * cw + c) * 2 + 1]; }
            chan[2 * (c0 + c)] = sa; chan[2 * (c0 + c) + 1] = sb;
            if (F::kKeepChannels) { tot[((long)n * C + c0 + c) * 2] = sa; tot[((long)n * C + c0 + c) * 2 + 1] = sb; }
        }
        __syncthreads();
    }
    if (threadIdx.x < GN_GROUPS) f.finalize(n, threadIdx.x, chan, cg, (double)HW * cg);
}

// dbeta_c = sum g', dgamma_c = sum g' xhat over the images, in index order, from the per-(image, channel) totals
__global__ void k_gn_dparam(const double* __restrict__ tot, float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sa = 0.0, sb = 0.0;
    for (int n = 0; n < N; ++n) { sa += tot[((long)n * C + c) * 2]; sb += tot[((long)n * C + c) * 2 + 1]; }
    dbeta[c] = (float)sa;
    dgamma[c] = (float)sb;
}

// grid (blocks per image, N): y = act(gamma xhat + beta)
template <int SWISH>
__global__ void __launch_bounds__(256) k_gn_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                  int HW, int C, int cg) {
    const int n = blockIdx.y;
    const GnWalk w(C);
    if (!w.active) return;
    GnChan ch;
    ch.load(mean + n * GN_GROUPS, rstd + n * GN_GROUPS, gamma, beta, w.col * 4, cg);
    const long base = (long)n * HW * C + w.col * 4;
    const int step = gridDim.x * w.rows;
    gn_walk_pixels(blockIdx.x * w.rows + w.row, step, HW, [&](auto uc, int p) {
        constexpr int U = decltype(uc)::value;
        float4_t in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) in[u] = *(const float4_t*)(x + base + (long)(p + u * step) * C);
        gn_pin(in);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float v[4], o[4];
            gn_unpack(in[u], v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float xh;
                o[i] = gn_act<SWISH>(gn_pre(v[i], ch.mean[i], ch.rstd[i], ch.gamma[i], ch.beta[i], xh));
            }
            *(float4*)(y + base + (long)(p + u * step) * C) = make_float4(o[0], o[1], o[2], o[3]);
        }
    });
}

template <int SWISH>
__global__ void __launch_bounds__(256) k_gn_bwd_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ gy, const float* __restrict__ gmeans, float* __restrict__ gx,
                                                      int HW, int C, int cg) {
    const int n = blockIdx.y;
    const GnWalk w(C);
    if (!w.active) return;
    GnChan ch;
    ch.load(mean + n * GN_GROUPS, rstd + n * GN_GROUPS, gamma, beta, w.col * 4, cg);
    float e1[4], e2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int g = (w.col * 4 + i) / cg;
        e1[i] = gmeans[(n * GN_GROUPS + g) * 2];
        e2[i] = gmeans[(n * GN_GROUPS + g) * 2 + 1];
    }
    const long base = (long)n * HW * C + w.col * 4;
    const int step = gridDim.x * w.rows;
    gn_walk_pixels(blockIdx.x * w.rows + w.row, step, HW, [&](auto uc, int p) {
        constexpr int U = decltype(uc)::value;
        float4_t in[U], gin[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            in[u] = *(const float4_t*)(x + base + (long)(p + u * step) * C);
            gin[u] = *(const float4_t*)(gy + base + (long)(p + u * step) * C);
        }
        gn_pin(in);
        gn_pin(gin);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float v[4], g[4], o[4];
            gn_unpack(in[u], v);
            gn_unpack(gin[u], g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float xh;
                const float pre = gn_pre(v[i], ch.mean[i], ch.rstd[i], ch.gamma[i], ch.beta[i], xh);
                o[i] = gn_bwd_out(gn_gprime<SWISH>(g[i], pre), ch.gamma[i], xh, ch.rstd[i], e1[i], e2[i]);
            }
            *(float4*)(gx + base + (long)(p + u * step) * C) = make_float4(o[0], o[1], o[2], o[3]);
        }
    });
}

static inline bool gn_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the tier choice, written once: one workgroup per image that finalises in its tail, or split + finalise pass
template <class F>
static void gn_launch_reduce(F f, double* part, double* tot, int N, int HW, int C, hipStream_t st) {
    const int splits = gn_splits(HW, C), cg = C / GN_GROUPS;
    if (splits == 1) {
        hipLaunchKernelGGL((k_gn_reduce<F, true>), dim3(1, N), dim3(256), 0, st, f, part, tot, HW, C, cg, HW);
    } else {
        hipLaunchKernelGGL((k_gn_reduce<F, false>), dim3(splits, N), dim3(256), 0, st, f, part, tot, HW, C, cg, ceil_div(HW, splits));
        hipLaunchKernelGGL((k_gn_finalize<F>), dim3(N), dim3(256), 0, st, f, part, tot, HW, C, cg, splits);
    }
}
static inline dim3 gn_apply_grid(int N, int HW, int C) {
    const int rows = 256 / (C / 4);
    return dim3(imax(1, imin(ceil_div(HW, rows), ceil_div(4096, N))), N);
}

static int gn_check(const char* name, int N, int HW, int C, size_t ws_bytes) {
    VQW_CHECK(N >= 1 && N <= 65535 && HW >= 1 && C >= GN_GROUPS, "%s: bad shape N=%d HW=%d C=%d", name, N, HW, C);
    VQW_CHECK(C % GN_GROUPS == 0, "%s: num_channels (%d) must be divisible by num_groups (32)", name, C);
    VQW_CHECK(C <= GN_MAX_C, "%s: C=%d exceeds %d", name, C, GN_MAX_C);
    VQW_CHECK((long)N * HW * C < (1L << 40), "%s: tensor too large", name);
    VQW_CHECK(ws_bytes >= vqw_groupnorm_ws_bytes(N, HW, C), "%s: workspace of %zu bytes, %zu needed", name, ws_bytes,
              vqw_groupnorm_ws_bytes(N, HW, C));
    return VQW_OK;
}

extern "C" int vqw_groupnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, void* ws,
                                 size_t ws_bytes, int N, int HW, int C, float eps, int swish, void* stream) {
    VQW_CHECK(x && gamma && beta && y && mean && rstd && ws, "vqw_groupnorm_fwd: null pointer");
    if (int rc = gn_check("vqw_groupnorm_fwd", N, HW, C, ws_bytes)) return rc;
    VQW_CHECK(gn_al16(x) && gn_al16(y) && gn_al16(ws), "vqw_groupnorm_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    FGnStats f{x, mean, rstd, eps};
    gn_launch_reduce(f, (double*)ws, (double*)((char*)ws + gn_part_bytes(N, HW, C)), N, HW, C, st);
    const int cg = C / GN_GROUPS;
    if (swish) hipLaunchKernelGGL((k_gn_apply<1>), gn_apply_grid(N, HW, C), dim3(256), 0, st, x, mean, rstd, gamma, beta, y, HW, C, cg);
    else hipLaunchKernelGGL((k_gn_apply<0>), gn_apply_grid(N, HW, C), dim3(256), 0, st, x, mean, rstd, gamma, beta, y, HW, C, cg);
    VQW_LAUNCH_CHECK("vqw_groupnorm_fwd");
    return VQW_OK;
}

extern "C" int vqw_groupnorm_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                 const float* gy, float* gx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int N, int HW,
                                 int C, int swish, void* stream) {
    VQW_CHECK(x && gamma && beta && mean && rstd && gy && gx && dgamma && dbeta && ws, "vqw_groupnorm_bwd: null pointer");
    if (int rc = gn_check("vqw_groupnorm_bwd", N, HW, C, ws_bytes)) return rc;
    VQW_CHECK(gn_al16(x) && gn_al16(gy) && gn_al16(gx) && gn_al16(ws), "vqw_groupnorm_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    double* tot = (double*)((char*)ws + gn_part_bytes(N, HW, C));
    float* gmeans = (float*)((char*)tot + gn_tot_bytes(N, C));
    const int cg = C / GN_GROUPS;
    if (swish) {
        FGnBwd<1> f{x, gy, mean, rstd, gamma, beta, gmeans};
        gn_launch_reduce(f, part, tot, N, HW, C, st);
    } else {
        FGnBwd<0> f{x, gy, mean, rstd, gamma, beta, gmeans};
        gn_launch_reduce(f, part, tot, N, HW, C, st);
    }
    hipLaunchKernelGGL(k_gn_dparam, dim3(ceil_div(C, 64)), dim3(64), 0, st, tot, dgamma, dbeta, N, C);
    if (swish) hipLaunchKernelGGL((k_gn_bwd_apply<1>), gn_apply_grid(N, HW, C), dim3(256), 0, st, x, mean, rstd, gamma, beta, gy, gmeans, gx, HW, C, cg);
    else hipLaunchKernelGGL((k_gn_bwd_apply<0>), gn_apply_grid(N, HW, C), dim3(256), 0, st, x, mean, rstd, gamma, beta, gy, gmeans, gx, HW, C, cg);
    VQW_LAUNCH_CHECK("vqw_groupnorm_bwd");
    return VQW_OK;
}

// swish on its own (vqgan.py:10-12 `nonlinearity`), through the same two formulas
__global__ void k_swish_fwd(const float* __restrict__ x, float* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = gn_act<1>(x[i]);
}
__global__ void k_swish_bwd(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) gx[i] = gn_gprime<1>(gy[i], x[i]);
}
extern "C" int vqw_swish_fwd(const float* x, float* y, long n, void* stream) {
    VQW_CHECK(x && y && n > 0, "vqw_swish_fwd: bad arguments");
    hipLaunchKernelGGL(k_swish_fwd, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    VQW_LAUNCH_CHECK("vqw_swish_fwd");
    return VQW_OK;
}
extern "C" int vqw_swish_bwd(const float* x, const float* gy, float* gx, long n, void* stream) {
    VQW_CHECK(x && gy && gx && n > 0, "vqw_swish_bwd: bad arguments");
    hipLaunchKernelGGL(k_swish_bwd, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, x, gy, gx, n);
    VQW_LAUNCH_CHECK("vqw_swish_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- attention
#define AT_BM 32           // tile rows a workgroup owns
#define AT_BN 64           // tile columns per step of the walk
#define AT_KC 128          // channels per staged chunk
#define AT_LD (AT_KC + 4)  // LDS row stride of a staged chunk: ds_read_b128 of 32 consecutive rows conflict-free
#define AT_LDS (AT_BN + 4) // LDS row stride of a score tile
#define AT_MAX_C 512        // widest value / output column window one workgroup keeps in registers
#define AT_MAX_C2 1024      // two such windows: the grid's z dimension

// LDS carve-up (floats).  A: staged 32-row operand chunk; B: staged 64-row operand chunk; T0 / T1: two score tiles as two
// half-sums each; P0 / P1: the element-wise stage's results (the A operand of attn_gemm_pv); row vectors.
#define AT_OFF_A 0
#define AT_OFF_B (AT_OFF_A + AT_BM * AT_LD)
#define AT_OFF_T0 (AT_OFF_B + AT_BN * AT_LD)
#define AT_OFF_T1 (AT_OFF_T0 + 2 * AT_BM * AT_LDS)
#define AT_OFF_P0 (AT_OFF_T1 + 2 * AT_BM * AT_LDS)
#define AT_OFF_P1 (AT_OFF_P0 + AT_BM * AT_LDS)
#define AT_OFF_V (AT_OFF_P1 + AT_BM * AT_LDS)         // 4 x 64 floats of row / column vectors
#define AT_LDS_FLOATS (AT_OFF_V + 4 * AT_BN)
#define AT_LDS_BYTES (AT_LDS_FLOATS * 4)

// rows [row0, row0 + R) x channels [c0, c0 + wt) of src [n_rows][C] -> dst [R][AT_LD]; rows at or past n_rows are zeros
__device__ __forceinline__ void attn_stage(float* dst, const float* __restrict__ src, int row0, int n_rows, int R, int c0, int wt, int C) {
    const int w4 = wt >> 2;
    for (int i = threadIdx.x; i < R * w4; i += 256) {
        const int r = i / w4, c4 = i - r * w4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < n_rows) v = *(const float4*)(src + (long)(row0 + r) * C + c0 + c4 * 4);
        *(float4*)(dst + r * AT_LD + c4 * 4) = v;
    }
}

// T[32][64] = A[a0 .. a0+32) . B[b0 .. b0+64)^T over all C channels, left in LDS as two half-sums T[0], T[1] ([32][AT_LDS]
// each; the consumer adds them): wave w takes the 32 columns (w & 1) and half (w >> 1) of every chunk's channels.
// Lane l feeds row / column l % 32; its four consecutive channels 8 s + 4 (l / 32) + {0..3} go to four MFMAs.
// FOLD (the kernels above 512 channels): every chunk's sum is added to a second accumulator, so that no chain of dependent roundings is longer than
// at 128 channels (a single chain over 1024 channels left lse twice as far from float64 as torch's fp32 bmm is).
template <bool FOLD>
__device__ __forceinline__ void attn_gemm_nt(float* lds, float* T, const float* __restrict__ A, int a0, int na, const float* __restrict__ B,
                                             int b0, int nb, int C) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kb = wv & 1, hf = wv >> 1;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc = {0}, tot = {0};
    for (int c0 = 0; c0 < C; c0 += AT_KC) {
        const int wt = imin_d(AT_KC, C - c0);
        __syncthreads();                      // the previous users of the staging buffers are done
        attn_stage(lds + AT_OFF_A, A, a0, na, AT_BM, c0, wt, C);
        attn_stage(lds + AT_OFF_B, B, b0, nb, AT_BN, c0, wt, C);
        __syncthreads();
        const int half = wt >> 1;             // a multiple of 16
        const float* pa = lds + AT_OFF_A + lr * AT_LD + hf * half + lh * 4;
        const float* pb = lds + AT_OFF_B + (kb * 32 + lr) * AT_LD + hf * half + lh * 4;
        for (int s = 0; s < half; s += 8) {
            const float4 a = *(const float4*)(pa + s), b = *(const float4*)(pb + s);
            acc = MFMA32(a.x, b.x, acc);
            acc = MFMA32(a.y, b.y, acc);
            acc = MFMA32(a.z, b.z, acc);
            acc = MFMA32(a.w, b.w, acc);
        }
        if constexpr (FOLD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
        }
    }
    if constexpr (FOLD) acc = tot;
    float* t = T + hf * (AT_BM * AT_LDS) + kb * 32 + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[((r & 3) + 8 * (r >> 2) + 4 * lh) * AT_LDS] = acc[r];
    __syncthreads();
}

// The value / output side works on a window of Cw = C / gridDim.z columns starting at column blockIdx.z Cw of rows of C floats
// (one window = the whole row up to 512 channels, two halves above): the callers offset the pointers by attn_col0.
__device__ __forceinline__ int attn_col0(int C) { return (int)blockIdx.z * (C / (int)gridDim.z); }

// acc[t] (the 32 x 32 block of columns 128 t + 32 w of wave w) += P[32][64] . B[b0 .. b0+64)[window of row stride C]
template <int CT>
__device__ __forceinline__ void attn_gemm_pv(float* lds, const float* P, const float* __restrict__ B, int b0, int nb, int C, f32x16 (&acc)[CT]) {
    const int Cw = C / (int)gridDim.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int c0 = t * AT_KC, wt = imin_d(AT_KC, Cw - c0);
        __syncthreads();
        attn_stage(lds + AT_OFF_B, B, b0, nb, AT_BN, c0, wt, C);
        __syncthreads();
        if (wv * 32 < wt) {
            const float* pa = P + lr * AT_LDS + lh * 4;
            const float* pb = lds + AT_OFF_B + (lh * 4) * AT_LD + wv * 32 + lr;
#pragma unroll
            for (int s = 0; s < AT_BN; s += 8) {
                const float4 a = *(const float4*)(pa + s);
                acc[t] = MFMA32(a.x, pb[(s + 0) * AT_LD], acc[t]);
                acc[t] = MFMA32(a.y, pb[(s + 1) * AT_LD], acc[t]);
                acc[t] = MFMA32(a.z, pb[(s + 2) * AT_LD], acc[t]);
                acc[t] = MFMA32(a.w, pb[(s + 3) * AT_LD], acc[t]);
            }
        }
    }
}

// out[row0 + row][128 t + 32 w + lane % 32] = acc * f(row) for the valid rows (columns of the window, rows of C floats)
template <int CT, class RowScale>
__device__ __forceinline__ void attn_store(float* __restrict__ out, int row0, int n_rows, int C, const f32x16 (&acc)[CT], RowScale rs) {
    const int Cw = C / (int)gridDim.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int c = t * AT_KC + wv * 32;
        if (c < Cw) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row0 + row < n_rows) out[(long)(row0 + row) * C + c + lr] = acc[t][r] * rs(row);
            }
        }
    }
}

// element-wise stage: thread -> row tid / 8, columns tid % 8 + 8 e (e = 0..7): the eight threads of a row are neighbours
#define AT_EW_ROW (threadIdx.x >> 3)
#define AT_EW_COL(e) ((threadIdx.x & 7) + 8 * (e))
__device__ __forceinline__ float attn_row8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
    return v;
}
__device__ __forceinline__ float attn_row8_sum(float v) {       // fixed butterfly: the same bits in all eight lanes, every run
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    return v;
}

// grid (ceil(N / 32), B, column windows).  Online softmax: running row maximum m and sum l live in the row's eight threads.
template <int CT, bool WIDE>
__global__ void __launch_bounds__(256) k_attn_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                  float* __restrict__ o, float* __restrict__ lse, int N, int C, float scale) {
    extern __shared__ __align__(16) float lds[];
    const long boff = (long)blockIdx.y * N * C;
    q += boff; k += boff; v += boff + attn_col0(C); o += boff + attn_col0(C);
    const int i0 = blockIdx.x * AT_BM;
    float* T = lds + AT_OFF_T0;
    float* P = lds + AT_OFF_P0;
    float* alpha = lds + AT_OFF_V;          // [32] this step's rescale of the accumulated rows
    f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = (f32x16){0};
    float m = -INFINITY, l = 0.f;
    const int row = AT_EW_ROW;
    for (int j0 = 0; j0 < N; j0 += AT_BN) {
        attn_gemm_nt<WIDE>(lds, T, q, i0, N, k, j0, N, C);
        float s[8], mt = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = AT_EW_COL(e);
            s[e] = (j0 + col < N) ? scale * (T[row * AT_LDS + col] + T[AT_BM * AT_LDS + row * AT_LDS + col]) : -INFINITY;
            mt = fmaxf(mt, s[e]);
        }
        const float mn = fmaxf(m, attn_row8_max(mt));       // finite: every tile holds at least one key
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = expf(s[e] - mn);
            P[row * AT_LDS + AT_EW_COL(e)] = p;
            ps += p;
        }
        const float a = expf(m - mn);
        l = fmaf(l, a, attn_row8_sum(ps));
        m = mn;
        if ((threadIdx.x & 7) == 0) alpha[row] = a;
        __syncthreads();
        {
            const int lh = (threadIdx.x & 63) >> 5;
            float ar[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ar[r] = alpha[(r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] *= ar[r];
        }
        attn_gemm_pv<CT>(lds, P, v, j0, N, C, acc);
    }
    __syncthreads();
    float* rinv = lds + AT_OFF_V + AT_BN;
    if ((threadIdx.x & 7) == 0) {
        rinv[row] = 1.f / l;
        if (i0 + row < N && blockIdx.z == 0) lse[(long)blockIdx.y * N + i0 + row] = m + logf(l);
    }
    __syncthreads();
    attn_store<CT>(o, i0, N, C, acc, [&](int r) { return rinv[r]; });
}

// D[b][i] = sum_c dO O: one wave per row, fixed butterfly
__global__ void __launch_bounds__(256) k_attn_rowdot(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, long rows, int C) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 x = *(const float4*)(a + r * C + c), y = *(const float4*)(b + r * C + c);
        s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    s = wave_sum_f(s);
    if (lane == 0) d[r] = s;
}

// The backward's element-wise stage on the two tiles T0 = (q k^T or k q^T) and T1 = (dO v^T or v dO^T): P = exp(scale S - lse),
// dS = scale P (dP - D), with lse / D indexed by the QUERY: the tile row (ROWS_ARE_QUERIES) or the tile column.  Entries whose
// row or column lies past N are zero.  vec: lse at [0, 64), D at [64, 128) of the tile's query range.
template <bool ROWS_ARE_QUERIES>
__device__ __forceinline__ void attn_bwd_stage(float* lds, const float* vec, int r0, int c0, int N, float scale, bool want_p) {
    const float* T0 = lds + AT_OFF_T0;
    const float* T1 = lds + AT_OFF_T1;
    float* P = lds + AT_OFF_P0;
    float* dS = lds + AT_OFF_P1;
    const int row = AT_EW_ROW;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int col = AT_EW_COL(e), qi = ROWS_ARE_QUERIES ? row : col;
        const bool ok = (r0 + row < N) && (c0 + col < N);
        const float sc = scale * (T0[row * AT_LDS + col] + T0[AT_BM * AT_LDS + row * AT_LDS + col]);
        const float dp = T1[row * AT_LDS + col] + T1[AT_BM * AT_LDS + row * AT_LDS + col];
        const float p = ok ? expf(sc - vec[qi]) : 0.f;
        if (want_p) P[row * AT_LDS + col] = p;
        dS[row * AT_LDS + col] = scale * p * (dp - vec[AT_BN + qi]);
    }
    __syncthreads();
}

// grid (ceil(N / 32), B): dQ = scale (P o (dO v^T - D)) k for a tile of 32 queries, walking the keys
template <int CT, bool WIDE>
__global__ void __launch_bounds__(256) k_attn_dq(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                 const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                                 float* __restrict__ gq, int N, int C, float scale) {
    extern __shared__ __align__(16) float lds[];
    const long boff = (long)blockIdx.y * N * C;
    q += boff; k += boff; v += boff; go += boff; gq += boff + attn_col0(C);
    lse += (long)blockIdx.y * N; D += (long)blockIdx.y * N;
    const int i0 = blockIdx.x * AT_BM;
    float* vec = lds + AT_OFF_V;
    if (threadIdx.x < AT_BM) {
        const bool ok = i0 + threadIdx.x < N;
        vec[threadIdx.x] = ok ? lse[i0 + threadIdx.x] : 0.f;
        vec[AT_BN + threadIdx.x] = ok ? D[i0 + threadIdx.x] : 0.f;
    }
    f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = (f32x16){0};
    for (int j0 = 0; j0 < N; j0 += AT_BN) {
        attn_gemm_nt<WIDE>(lds, lds + AT_OFF_T0, q, i0, N, k, j0, N, C);
        attn_gemm_nt<WIDE>(lds, lds + AT_OFF_T1, go, i0, N, v, j0, N, C);
        attn_bwd_stage<true>(lds, vec, i0, j0, N, scale, false);
        attn_gemm_pv<CT>(lds, lds + AT_OFF_P1, k + attn_col0(C), j0, N, C, acc);
    }
    attn_store<CT>(gq, i0, N, C, acc, [](int) { return 1.f; });
}

// grid (ceil(N / 32), B): dK = scale (P o (dO v^T - D))^T q and dV = P^T dO for a tile of 32 keys, walking the queries
template <int CT, bool WIDE>
__global__ void __launch_bounds__(256) k_attn_dkdv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                   const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                                   float* __restrict__ gk, float* __restrict__ gv, int N, int C, float scale) {
    extern __shared__ __align__(16) float lds[];
    const long boff = (long)blockIdx.y * N * C;
    q += boff; k += boff; v += boff; go += boff; gk += boff + attn_col0(C); gv += boff + attn_col0(C);
    lse += (long)blockIdx.y * N; D += (long)blockIdx.y * N;
    const int j0 = blockIdx.x * AT_BM;
    float* vec = lds + AT_OFF_V;
    f32x16 ak[CT], av[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) { ak[t] = (f32x16){0}; av[t] = (f32x16){0}; }
    for (int i0 = 0; i0 < N; i0 += AT_BN) {
        __syncthreads();                      // the previous step's readers of vec are done
        if (threadIdx.x < AT_BN) {
            const bool ok = i0 + threadIdx.x < N;
            vec[threadIdx.x] = ok ? lse[i0 + threadIdx.x] : 0.f;
            vec[AT_BN + threadIdx.x] = ok ? D[i0 + threadIdx.x] : 0.f;
        }
        attn_gemm_nt<WIDE>(lds, lds + AT_OFF_T0, k, j0, N, q, i0, N, C);
        attn_gemm_nt<WIDE>(lds, lds + AT_OFF_T1, v, j0, N, go, i0, N, C);
        attn_bwd_stage<false>(lds, vec, j0, i0, N, scale, true);
        attn_gemm_pv<CT>(lds, lds + AT_OFF_P0, go + attn_col0(C), i0, N, C, av);
        attn_gemm_pv<CT>(lds, lds + AT_OFF_P1, q + attn_col0(C), i0, N, C, ak);
    }
    attn_store<CT>(gk, j0, N, C, ak, [](int) { return 1.f; });
    attn_store<CT>(gv, j0, N, C, av, [](int) { return 1.f; });
}

static int attn_check(const char* name, int B, int N, int C) {
    VQW_CHECK(B >= 1 && B <= 65535 && N >= 1 && N <= (1 << 20), "%s: bad shape B=%d N=%d", name, B, N);
    VQW_CHECK(C >= 32 && ((C % 32 == 0 && C <= AT_MAX_C) || (C % 64 == 0 && C <= AT_MAX_C2)),
              "%s: C=%d must be a multiple of 32 up to %d or a multiple of 64 up to %d", name, C, AT_MAX_C, AT_MAX_C2);
    return VQW_OK;
}
// column windows of the value / output side (the grid's z dimension), and the 128-channel blocks of one window
static inline int attn_windows(int C) { return C > AT_MAX_C ? 2 : 1; }
static inline int attn_ct(int C) { return ceil_div(C / attn_windows(C), AT_KC); }

template <int CT, bool WIDE = false>
static int attn_fwd_launch(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int C, float scale, hipStream_t st) {
    if (int rc = lds_opt_in<k_attn_fwd<CT, WIDE>>(AT_LDS_BYTES, "vqw_attention_fwd")) return rc;
    hipLaunchKernelGGL((k_attn_fwd<CT, WIDE>), dim3(ceil_div(N, AT_BM), B, attn_windows(C)), dim3(256), AT_LDS_BYTES, st, q, k, v, o, lse, N, C, scale);
    return VQW_OK;
}
template <int CT, bool WIDE = false>
static int attn_bwd_launch(const float* q, const float* k, const float* v, const float* go, const float* lse, const float* D, float* gq,
                           float* gk, float* gv, int B, int N, int C, float scale, hipStream_t st) {
    if (int rc = lds_opt_in<k_attn_dq<CT, WIDE>>(AT_LDS_BYTES, "vqw_attention_bwd")) return rc;
    if (int rc = lds_opt_in<k_attn_dkdv<CT, WIDE>>(AT_LDS_BYTES, "vqw_attention_bwd")) return rc;
    const dim3 grid(ceil_div(N, AT_BM), B, attn_windows(C));
    hipLaunchKernelGGL((k_attn_dq<CT, WIDE>), grid, dim3(256), AT_LDS_BYTES, st, q, k, v, go, lse, D, gq, N, C, scale);
    hipLaunchKernelGGL((k_attn_dkdv<CT, WIDE>), grid, dim3(256), AT_LDS_BYTES, st, q, k, v, go, lse, D, gk, gv, N, C, scale);
    return VQW_OK;
}

extern "C" int vqw_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int C, float scale,
                                 void* stream) {
    VQW_CHECK(q && k && v && o && lse, "vqw_attention_fwd: null pointer");
    if (int rc = attn_check("vqw_attention_fwd", B, N, C)) return rc;
    VQW_CHECK(gn_al16(q) && gn_al16(k) && gn_al16(v), "vqw_attention_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (attn_windows(C) == 2) {          // 576 ... 1024 channels: windows of 288 ... 512, three or four 128-channel blocks
        rc = attn_ct(C) == 3 ? attn_fwd_launch<3, true>(q, k, v, o, lse, B, N, C, scale, st) : attn_fwd_launch<4, true>(q, k, v, o, lse, B, N, C, scale, st);
    } else switch (attn_ct(C)) {
        case 1: rc = attn_fwd_launch<1>(q, k, v, o, lse, B, N, C, scale, st); break;
        case 2: rc = attn_fwd_launch<2>(q, k, v, o, lse, B, N, C, scale, st); break;
        case 3: rc = attn_fwd_launch<3>(q, k, v, o, lse, B, N, C, scale, st); break;
        default: rc = attn_fwd_launch<4>(q, k, v, o, lse, B, N, C, scale, st); break;
    }
    if (rc) return rc;
    VQW_LAUNCH_CHECK("vqw_attention_fwd");
    return VQW_OK;
}

extern "C" int vqw_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                 float* d_ws, float* gq, float* gk, float* gv, int B, int N, int C, float scale, void* stream) {
    VQW_CHECK(q && k && v && o && lse && go && d_ws && gq && gk && gv, "vqw_attention_bwd: null pointer");
    if (int rc = attn_check("vqw_attention_bwd", B, N, C)) return rc;
    VQW_CHECK(gn_al16(q) && gn_al16(k) && gn_al16(v) && gn_al16(o) && gn_al16(go), "vqw_attention_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * N;
    hipLaunchKernelGGL(k_attn_rowdot, dim3(ceil_div(rows, 4)), dim3(256), 0, st, go, o, d_ws, rows, C);
    int rc;
    if (attn_windows(C) == 2) {
        rc = attn_ct(C) == 3 ? attn_bwd_launch<3, true>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st)
                             : attn_bwd_launch<4, true>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st);
    } else switch (attn_ct(C)) {
        case 1: rc = attn_bwd_launch<1>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st); break;
        case 2: rc = attn_bwd_launch<2>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st); break;
        case 3: rc = attn_bwd_launch<3>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st); break;
        default: rc = attn_bwd_launch<4>(q, k, v, go, lse, d_ws, gq, gk, gv, B, N, C, scale, st); break;
    }
    if (rc) return rc;
    VQW_LAUNCH_CHECK("vqw_attention_bwd");
    return VQW_OK;
}
