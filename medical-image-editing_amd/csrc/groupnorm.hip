// GroupNorm(32 groups, affine)(+swish) and swish on its own: the normalisation of the VQGAN blocks (networks/vqgan.py:
// Normalize / nonlinearity :10-19).  NHWC fp32.  The blocks' self-attention is in attention.hip.
//
// GroupNorm.  A thread owns one float4 column (four channels) of the tensor and walks pixels, so gamma, beta and the
// statistics of its channels are loaded once.  Every reduction is two-stage and deterministic: per-thread double sums, a
// fixed fold over the workgroup's rows in LDS to per-channel sums, then per-(image, split, channel) double partials that a
// finalise pass folds in a fixed order (norm.hip's scheme; a channel's splits are dealt to several threads).  Groups are folded
// from channel sums, so any channel count that is a multiple of 32 works - a group of 3 channels (C = 96) does not have to be a
// float4 multiple.  A plane of at most GN_ONE_WG_ELEMS elements per image takes one workgroup that finalises in its own tail; a
// larger one is split.
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
    VQW_CHECK(al16(x) && al16(y) && al16(ws), "vqw_groupnorm_fwd: tensors must be 16-byte aligned");
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
    VQW_CHECK(al16(x) && al16(gy) && al16(gx) && al16(ws), "vqw_groupnorm_bwd: tensors must be 16-byte aligned");
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
