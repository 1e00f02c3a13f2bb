// The three kernel families of the minGPT blocks (networks/mingpt.py: Block :93-119, CausalSelfAttention :34-90): LayerNorm over
// the last axis, the exact (erf) GELU, and multi-head attention with a causal mask and an unmasked prefix.  fp32.
//
// LayerNorm.  One wave owns a row of [rows][C]: lane l holds the float4 columns l, l + 64, ... in registers, the row is read
// once.  mean = sum / C plus the mean of the residuals, then the variance from the centred values (never E[x^2] - mean^2,
// mfma_util.h:65-67); every sum is one fixed butterfly.  Backward: a workgroup owns LN_WG_ROWS consecutive rows, wave w the rows
// w, w + 4, ... of them; dgamma / dbeta are summed per lane over the wave's rows, the four waves are folded in wave order in LDS,
// the workgroup's partial goes to the workspace and a second kernel folds the partials in index order (in double).  No atomics.
//
// GELU.  0.5 x (1 + erf(x / sqrt 2)) and its gradient Phi(x) + x phi(x) with the device erff / expf in fp32.
//
// Attention.  q [B][Tq][E], k, v [B][Tk][E], E = n_head hs, head h in the columns [h hs, (h + 1) hs): the layout the three
// projections leave; the row stride is E.  The tile structure is groupnorm_attn.hip's (32 tile rows per workgroup, steps of 64
// on the other axis, 32x32x2 fp32 MFMA, a score tile as two half-sums in LDS) with hs <= 128 as a single staged chunk.  Query i
// sees key j iff j <= limit(i), limit(i) = (i < n_unmasked ? n_unmasked - 1 : i) under the causal mask and Tk - 1 without:
// steps that lie wholly above a tile's largest limit are not walked, the others are masked element by element.  In the P V
// products the four waves split the hs / 32 column blocks and, where those are fewer than four, the 64 keys of a step; the
// per-wave partial accumulators are linear in everything the walk does to them and are added once, in wave order, at the end.
#include "common.h"
#include "mfma_util.h"
#include "../../include/vqwnet_hip.h"

__device__ __forceinline__ int mg_min(int a, int b) { return a < b ? a : b; }
static inline bool mg_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------- LayerNorm
#define LN_MIN_C 4
#define LN_MAX_C 4096
#define LN_SMALL_C 1024     // up to here a lane holds 4 float4 columns of a row, above 16
#define LN_WG_ROWS 32       // rows per workgroup of the backward: one dgamma / dbeta partial each

extern "C" size_t vqw_layernorm_ws_bytes(long rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return (size_t)ceil_div(rows, LN_WG_ROWS) * 2 * C * sizeof(float);
}

__device__ __forceinline__ float4 ln_ld(const float* p, int c4, int C4) {
    return c4 < C4 ? *(const float4*)(p + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float ln_sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// grid ceil(rows / 4): wave w of workgroup g normalises row 4 g + w
template <int NV>
__global__ void __launch_bounds__(256) k_ln_fwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, long rows, int C,
                                                float eps) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, C4 = C >> 2;
    const float* xr = x + r * C;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { v[i] = ln_ld(xr, lane + 64 * i, C4); s += ln_sum4(v[i]); }
    // mean = mu0 + delta with delta the mean of x - mu0: on a row that sits far off zero x - mu0 is exact and delta carries what
    // the fp32 sum lost, so the centred values do not inherit the rounding of the mean
    const float mu0 = wave_sum_f(s) / (float)C;
    float s0 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < C4) {
            v[i].x -= mu0; v[i].y -= mu0; v[i].z -= mu0; v[i].w -= mu0;
            s0 += ln_sum4(v[i]);
        }
    }
    const float delta = wave_sum_f(s0) / (float)C, mu = mu0 + delta;
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < C4) {
            v[i].x -= delta; v[i].y -= delta; v[i].z -= delta; v[i].w -= delta;
            m2 = fmaf(v[i].x, v[i].x, m2); m2 = fmaf(v[i].y, v[i].y, m2); m2 = fmaf(v[i].z, v[i].z, m2); m2 = fmaf(v[i].w, v[i].w, m2);
        }
    }
    const float rs = 1.f / sqrtf(wave_sum_f(m2) / (float)C + eps);
    float* yr = y + r * C;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const float4 g = *(const float4*)(gamma + 4 * c4), b = *(const float4*)(beta + 4 * c4);
            *(float4*)(yr + 4 * c4) = make_float4(fmaf(v[i].x * rs, g.x, b.x), fmaf(v[i].y * rs, g.y, b.y), fmaf(v[i].z * rs, g.z, b.z),
                                                  fmaf(v[i].w * rs, g.w, b.w));
        }
    }
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
}

// grid ceil(rows / LN_WG_ROWS).  gx = rstd (gamma g - mean_c(gamma g) - xhat mean_c(gamma g xhat)); part [grid][2][C]: the
// workgroup's sums over its rows of g xhat (dgamma) and g (dbeta)
template <int NV>
__global__ void __launch_bounds__(256) k_ln_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ gy, float* __restrict__ gx,
                                                float* __restrict__ part, long rows, int C) {
    __shared__ float red[2 * LN_MAX_C];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, C4 = C >> 2;
    const long r0 = (long)blockIdx.x * LN_WG_ROWS;
    const long r1 = r0 + LN_WG_ROWS < rows ? r0 + LN_WG_ROWS : rows;
    float4 gm[NV], dg[NV], db[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        gm[i] = ln_ld(gamma, lane + 64 * i, C4);
        dg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        db[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long r = r0 + wv; r < r1; r += 4) {
        const float mu = mean[r], rs = rstd[r];
        float4 xh[NV], g[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {          // columns past C load zeros: g = 0 there, they add nothing
            xh[i] = ln_ld(x + r * C, lane + 64 * i, C4);
            g[i] = ln_ld(gy + r * C, lane + 64 * i, C4);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            xh[i].x = (xh[i].x - mu) * rs; xh[i].y = (xh[i].y - mu) * rs; xh[i].z = (xh[i].z - mu) * rs; xh[i].w = (xh[i].w - mu) * rs;
            const float4 a = make_float4(gm[i].x * g[i].x, gm[i].y * g[i].y, gm[i].z * g[i].z, gm[i].w * g[i].w);
            s1 += ln_sum4(a);
            s2 += (a.x * xh[i].x + a.y * xh[i].y) + (a.z * xh[i].z + a.w * xh[i].w);
            db[i].x += g[i].x; db[i].y += g[i].y; db[i].z += g[i].z; db[i].w += g[i].w;
            dg[i].x = fmaf(g[i].x, xh[i].x, dg[i].x); dg[i].y = fmaf(g[i].y, xh[i].y, dg[i].y);
            dg[i].z = fmaf(g[i].z, xh[i].z, dg[i].z); dg[i].w = fmaf(g[i].w, xh[i].w, dg[i].w);
        }
        const float e1 = wave_sum_f(s1) / (float)C, e2 = wave_sum_f(s2) / (float)C;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c4 = lane + 64 * i;
            if (c4 < C4)
                *(float4*)(gx + r * C + 4 * c4) = make_float4(rs * (gm[i].x * g[i].x - e1 - xh[i].x * e2), rs * (gm[i].y * g[i].y - e1 - xh[i].y * e2),
                                                              rs * (gm[i].z * g[i].z - e1 - xh[i].z * e2), rs * (gm[i].w * g[i].w - e1 - xh[i].w * e2));
        }
    }
    // the four waves' sums, added in wave order
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c4 = lane + 64 * i;
                if (c4 < C4) {
                    float4* pg = (float4*)(red + 4 * c4);
                    float4* pb = (float4*)(red + LN_MAX_C + 4 * c4);
                    if (w == 0) { *pg = dg[i]; *pb = db[i]; }
                    else {
                        const float4 a = *pg, b = *pb;
                        *pg = make_float4(a.x + dg[i].x, a.y + dg[i].y, a.z + dg[i].z, a.w + dg[i].w);
                        *pb = make_float4(b.x + db[i].x, b.y + db[i].y, b.z + db[i].z, b.w + db[i].w);
                    }
                }
            }
        }
        __syncthreads();
    }
    float* o = part + (long)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) { o[c] = red[c]; o[C + c] = red[LN_MAX_C + c]; }
}

// grid ceil(C / 64), 1024 threads: column c's G partials are dealt to LN_FOLD_LANES threads (thread l adds the partials l,
// l + LN_FOLD_LANES, ... in index order), which are then added in that order
#define LN_FOLD_LANES 16
__global__ void __launch_bounds__(64 * LN_FOLD_LANES) k_ln_dparam(const float* __restrict__ part, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int G, int C) {
    __shared__ double lanes[LN_FOLD_LANES * 64 * 2];
    const int cl = threadIdx.x & 63, l = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    double sa = 0.0, sb = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int g = l; g < G; g += LN_FOLD_LANES) { sa += (double)part[(long)g * 2 * C + c]; sb += (double)part[(long)g * 2 * C + C + c]; }
    }
    lanes[(l * 64 + cl) * 2] = sa; lanes[(l * 64 + cl) * 2 + 1] = sb;
    __syncthreads();
    if (l == 0 && c < C) {
        sa = 0.0; sb = 0.0;
        for (int k = 0; k < LN_FOLD_LANES; ++k) { sa += lanes[(k * 64 + cl) * 2]; sb += lanes[(k * 64 + cl) * 2 + 1]; }
        dgamma[c] = (float)sa;
        dbeta[c] = (float)sb;
    }
}

static int ln_check(const char* name, long rows, int C) {
    VQW_CHECK(C % 4 == 0 && C >= LN_MIN_C && C <= LN_MAX_C, "%s: C=%d must be a multiple of 4 with %d <= C <= %d", name, C, LN_MIN_C, LN_MAX_C);
    VQW_CHECK(rows >= 1 && rows <= (1L << 31) - 4, "%s: bad row count %ld", name, rows);
    return VQW_OK;
}

extern "C" int vqw_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C,
                                 float eps, void* stream) {
    if (int rc = ln_check("vqw_layernorm_fwd", rows, C)) return rc;
    VQW_CHECK(x && gamma && beta && y && mean && rstd, "vqw_layernorm_fwd: null pointer");
    VQW_CHECK(mg_al16(x) && mg_al16(gamma) && mg_al16(beta) && mg_al16(y), "vqw_layernorm_fwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(rows, 4));
    if (C <= LN_SMALL_C) hipLaunchKernelGGL((k_ln_fwd<LN_SMALL_C / 256>), grid, dim3(256), 0, st, x, gamma, beta, y, mean, rstd, rows, C, eps);
    else hipLaunchKernelGGL((k_ln_fwd<LN_MAX_C / 256>), grid, dim3(256), 0, st, x, gamma, beta, y, mean, rstd, rows, C, eps);
    VQW_LAUNCH_CHECK("vqw_layernorm_fwd");
    return VQW_OK;
}

extern "C" int vqw_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd, const float* gy, float* gx,
                                 float* dgamma, float* dbeta, void* ws, size_t ws_bytes, long rows, int C, void* stream) {
    if (int rc = ln_check("vqw_layernorm_bwd", rows, C)) return rc;
    VQW_CHECK(x && gamma && mean && rstd && gy && gx && dgamma && dbeta && ws, "vqw_layernorm_bwd: null pointer");
    VQW_CHECK(ws_bytes >= vqw_layernorm_ws_bytes(rows, C), "vqw_layernorm_bwd: workspace of %zu bytes, %zu needed", ws_bytes,
              vqw_layernorm_ws_bytes(rows, C));
    VQW_CHECK(mg_al16(x) && mg_al16(gamma) && mg_al16(gy) && mg_al16(gx) && mg_al16(ws), "vqw_layernorm_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int G = ceil_div(rows, LN_WG_ROWS);
    float* part = (float*)ws;
    if (C <= LN_SMALL_C) hipLaunchKernelGGL((k_ln_bwd<LN_SMALL_C / 256>), dim3(G), dim3(256), 0, st, x, gamma, mean, rstd, gy, gx, part, rows, C);
    else hipLaunchKernelGGL((k_ln_bwd<LN_MAX_C / 256>), dim3(G), dim3(256), 0, st, x, gamma, mean, rstd, gy, gx, part, rows, C);
    hipLaunchKernelGGL(k_ln_dparam, dim3(ceil_div(C, 64)), dim3(64 * LN_FOLD_LANES), 0, st, part, dgamma, dbeta, G, C);
    VQW_LAUNCH_CHECK("vqw_layernorm_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- GELU
// The fp32 form with the device erff / expf: it passes the accuracy gate on every case (within 1.11 of the host's fp32 error) at
// 2.3 times the speed of an evaluation in double, which was measured too.
__device__ __forceinline__ float gelu_y(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_dx(float x, float gy) {
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
    return gy * fmaf(x, pdf, cdf);
}

__global__ void __launch_bounds__(256) k_gelu_fwd(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long n4 = n >> 2, step = (long)gridDim.x * blockDim.x, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = t; i < n4; i += step) {
        const float4 v = *(const float4*)(x + 4 * i);
        *(float4*)(y + 4 * i) = make_float4(gelu_y(v.x), gelu_y(v.y), gelu_y(v.z), gelu_y(v.w));
    }
    if (t < n - 4 * n4) y[4 * n4 + t] = gelu_y(x[4 * n4 + t]);          // the scalar tail of n % 4 elements
}
__global__ void __launch_bounds__(256) k_gelu_bwd(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, long n) {
    const long n4 = n >> 2, step = (long)gridDim.x * blockDim.x, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = t; i < n4; i += step) {
        const float4 v = *(const float4*)(x + 4 * i), g = *(const float4*)(gy + 4 * i);
        *(float4*)(gx + 4 * i) = make_float4(gelu_dx(v.x, g.x), gelu_dx(v.y, g.y), gelu_dx(v.z, g.z), gelu_dx(v.w, g.w));
    }
    if (t < n - 4 * n4) gx[4 * n4 + t] = gelu_dx(x[4 * n4 + t], gy[4 * n4 + t]);
}

extern "C" int vqw_gelu_fwd(const float* x, float* y, long n, void* stream) {
    VQW_CHECK(n >= 1, "vqw_gelu_fwd: n=%ld must be at least 1", n);
    VQW_CHECK(x && y, "vqw_gelu_fwd: null pointer");
    VQW_CHECK(mg_al16(x) && mg_al16(y), "vqw_gelu_fwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_gelu_fwd, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    VQW_LAUNCH_CHECK("vqw_gelu_fwd");
    return VQW_OK;
}
extern "C" int vqw_gelu_bwd(const float* x, const float* gy, float* gx, long n, void* stream) {
    VQW_CHECK(n >= 1, "vqw_gelu_bwd: n=%ld must be at least 1", n);
    VQW_CHECK(x && gy && gx, "vqw_gelu_bwd: null pointer");
    VQW_CHECK(mg_al16(x) && mg_al16(gy) && mg_al16(gx), "vqw_gelu_bwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_gelu_bwd, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, gy, gx, n);
    VQW_LAUNCH_CHECK("vqw_gelu_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- attention
// No contraction from here on: the backward recomputes the forward's scaled score s = scale (T0 + T1) and must get the same bits
// (a single visible key then gives p = exp(s - lse) = 1 exactly); fused into the subtraction that follows, s would not be
// rounded.  The explicit fmaf calls and the MFMAs are not affected.
#pragma clang fp contract(off)
#define CA_BM 32           // tile rows a workgroup owns
#define CA_BN 64           // tile columns per step of the walk
#define CA_MAX_HS 128      // one staged chunk
#define CA_LDS (CA_BN + 4)      // LDS row stride of a score tile
#define CA_MAX_T 65536

// LDS carve-up (floats), groupnorm_attn.hip's with the staging buffers sized by the head: a staged operand row is hs + 4 floats
// (= 4 mod 32 for every hs: ds_read_b128 of 32 consecutive rows conflict-free), so that several workgroups of narrow heads
// share a CU.  A: staged 32-row operand; B: staged 64-row operand; T0 / T1: two score tiles as two half-sums each (T0 at the end
// of a kernel: the four waves' partial accumulators, 4 x 32 x 32); P0 / P1: the element-wise stage's results; V: row vectors.
// The forward uses neither T1 nor P1: they lie last and it does not ask for them.
#define CA_T_FLOATS (2 * CA_BM * CA_LDS)
#define CA_P_FLOATS (CA_BM * CA_LDS)
struct CaLds {
    int ld;
    float *A, *B, *T0, *P0, *V, *T1, *P1;
    __device__ __forceinline__ CaLds(float* base, int hs) : ld(hs + 4) {
        A = base; B = A + CA_BM * ld; T0 = B + CA_BN * ld; P0 = T0 + CA_T_FLOATS; V = P0 + CA_P_FLOATS; T1 = V + 4 * CA_BN; P1 = T1 + CA_T_FLOATS;
    }
};
static inline int ca_lds_bytes(int hs, bool bwd) {
    return ((CA_BM + CA_BN) * (hs + 4) + CA_T_FLOATS + CA_P_FLOATS + 4 * CA_BN + (bwd ? CA_T_FLOATS + CA_P_FLOATS : 0)) * 4;
}
static_assert(4 * CA_BM * 32 <= CA_T_FLOATS, "the partial accumulators fit in T0");

// the mask rule, written once: the last key query i sees
struct CaMask {
    int causal, nu, Tk;
    __device__ __forceinline__ int limit(int i) const { return causal ? mg_min(i < nu ? nu - 1 : i, Tk - 1) : Tk - 1; }
};

// rows [row0, row0 + R) x hs columns of src (row stride ld, already offset to the head) -> dst [R][sld]; rows at or past n_rows
// are zeros
__device__ __forceinline__ void ca_stage(float* dst, int sld, const float* __restrict__ src, int row0, int n_rows, int R, int hs, int ld) {
    const int w4 = hs >> 2;
    for (int i = threadIdx.x; i < R * w4; i += 256) {
        const int r = i / w4, c4 = i - r * w4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < n_rows) v = *(const float4*)(src + (long)(row0 + r) * ld + c4 * 4);
        *(float4*)(dst + r * sld + c4 * 4) = v;
    }
}

// T[32][64] = A[a0 .. a0+32) . B[b0 .. b0+64)^T over the head's hs channels, as two half-sums T[0], T[1]: wave w takes the 32
// columns (w & 1) and the half (w >> 1) of the channels.  stage_a = false: A is still staged from the previous call.
__device__ __forceinline__ void ca_gemm_nt(const CaLds& L, float* T, const float* __restrict__ A, int a0, int na, const float* __restrict__ B, int b0,
                                           int nb, int hs, int ld, bool stage_a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kb = wv & 1, hf = wv >> 1;
    const int lr = lane & 31, lh = lane >> 5;
    __syncthreads();                      // the previous users of the staging buffers and of T are done
    if (stage_a) ca_stage(L.A, L.ld, A, a0, na, CA_BM, hs, ld);
    ca_stage(L.B, L.ld, B, b0, nb, CA_BN, hs, ld);
    __syncthreads();
    const int half = hs >> 1;             // a multiple of 16
    const float* pa = L.A + lr * L.ld + hf * half + lh * 4;
    const float* pb = L.B + (kb * 32 + lr) * L.ld + hf * half + lh * 4;
    f32x16 acc = {0};
    for (int s = 0; s < half; s += 8) {
        const float4 a = *(const float4*)(pa + s), b = *(const float4*)(pb + s);
        acc = MFMA32(a.x, b.x, acc);
        acc = MFMA32(a.y, b.y, acc);
        acc = MFMA32(a.z, b.z, acc);
        acc = MFMA32(a.w, b.w, acc);
    }
    float* t = T + hf * (CA_BM * CA_LDS) + kb * 32 + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[((r & 3) + 8 * (r >> 2) + 4 * lh) * CA_LDS] = acc[r];
    __syncthreads();
}

// acc += P[32][keys of this wave] . B[b0 .. b0+64)[column block of this wave]: with ncb = hs / 32 column blocks and
// ksn = 4 / ncb key splits, wave w takes column block w % ncb and the keys [64 / ksn * (w / ncb), 64 / ksn * (w / ncb + 1))
__device__ __forceinline__ void ca_gemm_pv(const CaLds& L, const float* P, const float* __restrict__ B, int b0, int nb, int hs, int ld, f32x16& acc) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int ncb = hs >> 5, ksn = 4 / ncb, cb = wv % ncb, ks = wv / ncb, kw = CA_BN / ksn;
    __syncthreads();
    ca_stage(L.B, L.ld, B, b0, nb, CA_BN, hs, ld);
    __syncthreads();
    if (ks < ksn) {
        const float* pa = P + lr * CA_LDS + ks * kw + lh * 4;
        const float* pb = L.B + (ks * kw + lh * 4) * L.ld + cb * 32 + lr;
        for (int s = 0; s < kw; s += 8) {
            const float4 a = *(const float4*)(pa + s);
            acc = MFMA32(a.x, pb[(s + 0) * L.ld], acc);
            acc = MFMA32(a.y, pb[(s + 1) * L.ld], acc);
            acc = MFMA32(a.z, pb[(s + 2) * L.ld], acc);
            acc = MFMA32(a.w, pb[(s + 3) * L.ld], acc);
        }
    }
}

// out[row0 + row][c] = f(row) * (sum over the key splits, in split order, of the waves' partial accumulators) for the valid rows
template <class RowScale>
__device__ __forceinline__ void ca_reduce_store(const CaLds& L, const f32x16& acc, float* __restrict__ out, int row0, int n_rows, int hs, int ld,
                                                RowScale rs) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int ncb = hs >> 5, ksn = 4 / ncb;
    float* red = L.T0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wv * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + lr] = acc[r];
    __syncthreads();
    for (int i = threadIdx.x; i < CA_BM * hs; i += 256) {
        const int row = i / hs, c = i - row * hs, cb = c >> 5;
        float s = red[cb * 1024 + row * 32 + (c & 31)];
        for (int ks = 1; ks < ksn; ++ks) s += red[(ks * ncb + cb) * 1024 + row * 32 + (c & 31)];
        if (row0 + row < n_rows) out[(long)(row0 + row) * ld + c] = s * rs(row);
    }
}

// element-wise stage: thread -> row tid / 8, columns tid % 8 + 8 e (e = 0..7): the eight threads of a row are neighbours
#define CA_EW_ROW (threadIdx.x >> 3)
#define CA_EW_COL(e) ((threadIdx.x & 7) + 8 * (e))
__device__ __forceinline__ float ca_row8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
    return v;
}
__device__ __forceinline__ float ca_row8_sum(float v) {
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    return v;
}

// grid (ceil(Tq / 32), B n_head).  Online softmax: the running row maximum m and sum l live in the row's eight threads.  Every
// row - a padding row of the last tile too - sees key 0, so m is finite after the first step; a masked entry is exactly 0.
__global__ void __launch_bounds__(256) k_ca_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                float* __restrict__ o, float* __restrict__ lse, int Tq, int Tk, int nh, int hs, float scale,
                                                CaMask mask) {
    extern __shared__ __align__(16) float lds[];
    const CaLds L(lds, hs);
    const int b = blockIdx.y / nh, h = blockIdx.y - b * nh, E = nh * hs;
    q += (long)b * Tq * E + h * hs; o += (long)b * Tq * E + h * hs;
    k += (long)b * Tk * E + h * hs; v += (long)b * Tk * E + h * hs;
    const int i0 = blockIdx.x * CA_BM;
    float* T = L.T0;
    float* P = L.P0;
    float* alpha = L.V;          // [32] this step's rescale of the accumulated rows
    f32x16 acc = {0};
    float m = -INFINITY, l = 0.f;
    const int row = CA_EW_ROW;
    const int lim = mask.limit(i0 + row);
    const int jmax = mask.limit(mg_min(i0 + CA_BM, Tq) - 1);        // the limit grows with the row: the tile's largest
    for (int j0 = 0; j0 <= jmax; j0 += CA_BN) {
        ca_gemm_nt(L, T, q, i0, Tq, k, j0, Tk, hs, E, j0 == 0);
        float s[8], mt = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = CA_EW_COL(e);
            s[e] = (j0 + col <= lim) ? scale * (T[row * CA_LDS + col] + T[CA_BM * CA_LDS + row * CA_LDS + col]) : -INFINITY;
            mt = fmaxf(mt, s[e]);
        }
        const float mn = fmaxf(m, ca_row8_max(mt));
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = (j0 + CA_EW_COL(e) <= lim) ? expf(s[e] - mn) : 0.f;
            P[row * CA_LDS + CA_EW_COL(e)] = p;
            ps += p;
        }
        const float a = expf(m - mn);
        l = fmaf(l, a, ca_row8_sum(ps));
        m = mn;
        if ((threadIdx.x & 7) == 0) alpha[row] = a;
        __syncthreads();
        {
            const int lh = (threadIdx.x & 63) >> 5;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= alpha[(r & 3) + 8 * (r >> 2) + 4 * lh];
        }
        ca_gemm_pv(L, P, v, j0, Tk, hs, E, acc);
    }
    float* rinv = L.V + CA_BN;
    if ((threadIdx.x & 7) == 0) {
        rinv[row] = 1.f / l;
        if (i0 + row < Tq) lse[(long)blockIdx.y * Tq + i0 + row] = m + logf(l);
    }
    ca_reduce_store(L, acc, o, i0, Tq, hs, E, [&](int r) { return rinv[r]; });
}

// D[b][h][t] = sum over the head's channels of dO O: one wave per (b, t, h), fixed butterfly
__global__ void __launch_bounds__(256) k_ca_rowdot(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, int B, int T,
                                                   int nh, int hs) {
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long)B * T * nh) return;
    const int lane = threadIdx.x & 63, h = (int)(w % nh);
    const long bt = w / nh;
    float s = 0.f;
    if (lane * 4 < hs) {
        const float4 x = *(const float4*)(a + w * hs + lane * 4), y = *(const float4*)(b + w * hs + lane * 4);
        s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    s = wave_sum_f(s);
    if (lane == 0) d[((bt / T) * nh + h) * T + bt % T] = s;
}

// The backward's element-wise stage on T0 = (q k^T or k q^T) and T1 = (dO v^T or v dO^T): P = exp(scale S - lse), dS = scale P (dP - D)
// where the query sees the key, 0 elsewhere.  lse / D are indexed by the QUERY: the tile row (ROWS_ARE_QUERIES) or column.
// vec: lse at [0, 64), D at [64, 128) of the tile's query range.
template <bool ROWS_ARE_QUERIES>
__device__ __forceinline__ void ca_bwd_stage(const CaLds& L, const float* vec, int r0, int c0, int T, float scale, bool want_p, const CaMask& mask) {
    const float* T0 = L.T0;
    const float* T1 = L.T1;
    float* P = L.P0;
    float* dS = L.P1;
    const int row = CA_EW_ROW;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int col = CA_EW_COL(e), qi = ROWS_ARE_QUERIES ? row : col;
        const int iq = ROWS_ARE_QUERIES ? r0 + row : c0 + col, jk = ROWS_ARE_QUERIES ? c0 + col : r0 + row;
        const bool ok = iq < T && jk <= mask.limit(iq);
        const float sc = scale * (T0[row * CA_LDS + col] + T0[CA_BM * CA_LDS + row * CA_LDS + col]);
        const float dp = T1[row * CA_LDS + col] + T1[CA_BM * CA_LDS + row * CA_LDS + col];
        const float p = ok ? expf(sc - vec[qi]) : 0.f;
        if (want_p) P[row * CA_LDS + col] = p;
        dS[row * CA_LDS + col] = ok ? scale * p * (dp - vec[CA_BN + qi]) : 0.f;
    }
    __syncthreads();
}

// grid (ceil(T / 32), B n_head): dQ = scale (P o (dO v^T - D)) k for a tile of 32 queries, over the key steps the forward walked
__global__ void __launch_bounds__(256) k_ca_dq(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                               const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                               float* __restrict__ gq, int T, int nh, int hs, float scale, CaMask mask) {
    extern __shared__ __align__(16) float lds[];
    const CaLds L(lds, hs);
    const int b = blockIdx.y / nh, h = blockIdx.y - b * nh, E = nh * hs;
    const long off = (long)b * T * E + h * hs;
    q += off; k += off; v += off; go += off; gq += off;
    lse += (long)blockIdx.y * T; D += (long)blockIdx.y * T;
    const int i0 = blockIdx.x * CA_BM;
    float* vec = L.V;
    if (threadIdx.x < CA_BM) {
        const bool ok = i0 + threadIdx.x < T;
        vec[threadIdx.x] = ok ? lse[i0 + threadIdx.x] : 0.f;
        vec[CA_BN + threadIdx.x] = ok ? D[i0 + threadIdx.x] : 0.f;
    }
    f32x16 acc = {0};
    const int jmax = mask.limit(mg_min(i0 + CA_BM, T) - 1);
    for (int j0 = 0; j0 <= jmax; j0 += CA_BN) {
        ca_gemm_nt(L, L.T0, q, i0, T, k, j0, T, hs, E, true);
        ca_gemm_nt(L, L.T1, go, i0, T, v, j0, T, hs, E, true);
        ca_bwd_stage<true>(L, vec, i0, j0, T, scale, false, mask);
        ca_gemm_pv(L, L.P1, k, j0, T, hs, E, acc);
    }
    ca_reduce_store(L, acc, gq, i0, T, hs, E, [](int) { return 1.f; });
}

// grid (ceil(T / 32), B n_head): dK = scale (P o (dO v^T - D))^T q and dV = P^T dO for a tile of 32 keys, over the query steps from
// the first one that sees one of its keys: step 0 when its first key lies in the unmasked prefix (or without a mask), else the
// step that holds its first key
__global__ void __launch_bounds__(256) k_ca_dkdv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                 const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                                 float* __restrict__ gk, float* __restrict__ gv, int T, int nh, int hs, float scale, CaMask mask) {
    extern __shared__ __align__(16) float lds[];
    const CaLds L(lds, hs);
    const int b = blockIdx.y / nh, h = blockIdx.y - b * nh, E = nh * hs;
    const long off = (long)b * T * E + h * hs;
    q += off; k += off; v += off; go += off; gk += off; gv += off;
    lse += (long)blockIdx.y * T; D += (long)blockIdx.y * T;
    const int j0 = blockIdx.x * CA_BM;
    float* vec = L.V;
    f32x16 ak = {0}, av = {0};
    const int istart = (!mask.causal || j0 < mask.nu) ? 0 : (j0 / CA_BN) * CA_BN;
    for (int i0 = istart; i0 < T; i0 += CA_BN) {
        __syncthreads();                      // the previous step's readers of vec are done
        if (threadIdx.x < CA_BN) {
            const bool ok = i0 + threadIdx.x < T;
            vec[threadIdx.x] = ok ? lse[i0 + threadIdx.x] : 0.f;
            vec[CA_BN + threadIdx.x] = ok ? D[i0 + threadIdx.x] : 0.f;
        }
        ca_gemm_nt(L, L.T0, k, j0, T, q, i0, T, hs, E, true);
        ca_gemm_nt(L, L.T1, v, j0, T, go, i0, T, hs, E, true);
        ca_bwd_stage<false>(L, vec, j0, i0, T, scale, true, mask);
        ca_gemm_pv(L, L.P0, go, i0, T, hs, E, av);
        ca_gemm_pv(L, L.P1, q, i0, T, hs, E, ak);
    }
    ca_reduce_store(L, ak, gk, j0, T, hs, E, [](int) { return 1.f; });
    ca_reduce_store(L, av, gv, j0, T, hs, E, [](int) { return 1.f; });
}

static int ca_check(const char* name, int B, int Tq, int Tk, int nh, int hs, int causal, int nu) {
    VQW_CHECK(hs % 32 == 0 && hs >= 32 && hs <= CA_MAX_HS, "%s: head size hs=%d must be a multiple of 32 with 32 <= hs <= %d", name, hs, CA_MAX_HS);
    VQW_CHECK(Tq >= 1 && Tq <= CA_MAX_T && Tk >= 1 && Tk <= CA_MAX_T, "%s: Tq=%d, Tk=%d must satisfy 1 <= T <= %d", name, Tq, Tk, CA_MAX_T);
    VQW_CHECK(B >= 1 && nh >= 1 && (long)B * nh <= 65535, "%s: B=%d, n_head=%d must satisfy 1 <= B * n_head <= 65535", name, B, nh);
    VQW_CHECK(!causal || Tq == Tk, "%s: the causal mask needs Tq == Tk (got Tq=%d, Tk=%d)", name, Tq, Tk);
    VQW_CHECK(nu >= 0 && nu <= Tk && (causal || nu == 0), "%s: n_unmasked=%d must satisfy 0 <= n_unmasked <= T=%d (and be 0 without the causal mask)",
              name, nu, Tk);
    return VQW_OK;
}

extern "C" int vqw_causal_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Tq, int Tk, int n_head,
                                        int hs, float scale, int causal, int n_unmasked, void* stream) {
    if (int rc = ca_check("vqw_causal_attention_fwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    VQW_CHECK(q && k && v && o && lse, "vqw_causal_attention_fwd: null pointer");
    VQW_CHECK(mg_al16(q) && mg_al16(k) && mg_al16(v) && mg_al16(o), "vqw_causal_attention_fwd: tensors must be 16-byte aligned");
    if (int rc = lds_opt_in<k_ca_fwd>(ca_lds_bytes(CA_MAX_HS, false), "vqw_causal_attention_fwd")) return rc;
    const CaMask mask{causal ? 1 : 0, n_unmasked, Tk};
    hipLaunchKernelGGL(k_ca_fwd, dim3(ceil_div(Tq, CA_BM), B * n_head), dim3(256), ca_lds_bytes(hs, false), (hipStream_t)stream, q, k, v, o, lse, Tq, Tk,
                       n_head, hs, scale, mask);
    VQW_LAUNCH_CHECK("vqw_causal_attention_fwd");
    return VQW_OK;
}

extern "C" int vqw_causal_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                        float* d_ws, float* gq, float* gk, float* gv, int B, int Tq, int Tk, int n_head, int hs, float scale,
                                        int causal, int n_unmasked, void* stream) {
    if (int rc = ca_check("vqw_causal_attention_bwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    VQW_CHECK(Tq == Tk, "vqw_causal_attention_bwd: the backward needs Tq == Tk (got Tq=%d, Tk=%d): the layer_past route is forward only", Tq, Tk);
    VQW_CHECK(q && k && v && o && lse && go && d_ws && gq && gk && gv, "vqw_causal_attention_bwd: null pointer");
    VQW_CHECK(mg_al16(q) && mg_al16(k) && mg_al16(v) && mg_al16(o) && mg_al16(go) && mg_al16(gq) && mg_al16(gk) && mg_al16(gv),
              "vqw_causal_attention_bwd: tensors must be 16-byte aligned");
    if (int rc = lds_opt_in<k_ca_dq>(ca_lds_bytes(CA_MAX_HS, true), "vqw_causal_attention_bwd")) return rc;
    if (int rc = lds_opt_in<k_ca_dkdv>(ca_lds_bytes(CA_MAX_HS, true), "vqw_causal_attention_bwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int T = Tq;
    const CaMask mask{causal ? 1 : 0, n_unmasked, T};
    hipLaunchKernelGGL(k_ca_rowdot, dim3(ceil_div((long)B * T * n_head, 4)), dim3(256), 0, st, go, o, d_ws, B, T, n_head, hs);
    const dim3 grid(ceil_div(T, CA_BM), B * n_head);
    hipLaunchKernelGGL(k_ca_dq, grid, dim3(256), ca_lds_bytes(hs, true), st, q, k, v, go, lse, d_ws, gq, T, n_head, hs, scale, mask);
    hipLaunchKernelGGL(k_ca_dkdv, grid, dim3(256), ca_lds_bytes(hs, true), st, q, k, v, go, lse, d_ws, gk, gv, T, n_head, hs, scale, mask);
    VQW_LAUNCH_CHECK("vqw_causal_attention_bwd");
    return VQW_OK;
}
