// LayerNorm over the last axis and the exact (erf) GELU of the minGPT blocks (networks/mingpt.py: Block :93-119).  fp32.  The
// blocks' causal multi-head attention is in attention.hip.
//
// LayerNorm.  One wave owns a row of [rows][C]: lane l holds the float4 columns l, l + 64, ... in registers, the row is read
// once (ln_row.h: the row's body, shared with pseudo_nll.hip's gathering LayerNorm).  mean = sum / C plus the mean of the
// residuals, then the variance from the centred values (never E[x^2] - mean^2, mfma_util.h:65-67); every sum is one fixed butterfly.  The steps are gpt_math.h's, shared with the decode step's fused
// LayerNorm.  Backward: a workgroup owns LN_WG_ROWS consecutive rows, wave w the rows
// w, w + 4, ... of them; dgamma / dbeta are summed per lane over the wave's rows, the four waves are folded in wave order in LDS,
// the workgroup's partial goes to the workspace and a second kernel folds the partials in index order (in double).  No atomics.
//
// GELU.  0.5 x (1 + erf(x / sqrt 2)) and its gradient Phi(x) + x phi(x) with the device erff / expf in fp32.
#include "common.h"
#include "gpt_math.h"
#include "ln_row.h"
#include "mfma_util.h"
#include "../../include/vqwnet_hip.h"

// ---------------------------------------------------------------------------------------------------------- LayerNorm
#define LN_MIN_C 4
#define LN_MAX_C 4096
#define LN_SMALL_C 1024     // up to here a lane holds 4 float4 columns of a row, above 16
#define LN_WG_ROWS 32       // rows per workgroup of the backward: one dgamma / dbeta partial each

extern "C" size_t vqw_layernorm_ws_bytes(long rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return (size_t)ceil_div(rows, LN_WG_ROWS) * 2 * C * sizeof(float);
}

// grid ceil(rows / 4): wave w of workgroup g normalises row 4 g + w
template <int NV>
__global__ void __launch_bounds__(256) k_ln_fwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, long rows, int C,
                                                float eps) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    float mu, rs;
    ln_row_fwd<NV>(x + r * C, gamma, beta, y + r * C, lane, C, eps, mu, rs);
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
            s1 += sum4(a);
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
    VQW_CHECK(al16(x) && al16(gamma) && al16(beta) && al16(y), "vqw_layernorm_fwd: tensors must be 16-byte aligned");
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
    VQW_CHECK(al16(x) && al16(gamma) && al16(gy) && al16(gx) && al16(ws), "vqw_layernorm_bwd: tensors must be 16-byte aligned");
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
// gelu_y and gelu_dx: gpt_math.h
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
    VQW_CHECK(al16(x) && al16(y), "vqw_gelu_fwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_gelu_fwd, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    VQW_LAUNCH_CHECK("vqw_gelu_fwd");
    return VQW_OK;
}
extern "C" int vqw_gelu_bwd(const float* x, const float* gy, float* gx, long n, void* stream) {
    VQW_CHECK(n >= 1, "vqw_gelu_bwd: n=%ld must be at least 1", n);
    VQW_CHECK(x && gy && gx, "vqw_gelu_bwd: null pointer");
    VQW_CHECK(al16(x) && al16(gy) && al16(gx), "vqw_gelu_bwd: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_gelu_bwd, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, gy, gx, n);
    VQW_LAUNCH_CHECK("vqw_gelu_bwd");
    return VQW_OK;
}
