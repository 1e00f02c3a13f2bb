// Focal frequency loss (Jiang et al., ICCV 2021; the focal-frequency-loss package v0.3.0 that the reference builds as
// FFL(loss_weight=1.0, alpha=1.0), trainers/base.py:277-278) and its gradient.
//
// For planes (n, patch, c) of h x w pixels:  D = fft2(win(pred) - win(target), norm='ortho'),  f = |D|^alpha (log(f + 1)
// with log_matrix),  w = f / max f (per plane, or over everything with batch_matrix; NaN -> 0),  loss = loss_weight *
// mean(w |D|^2) = loss_weight / M * sum_plane S / F  with S = sum f |D|^2 and F = max f.  The weight is a constant to
// autograd, so dL/dx = 2 loss_weight gL / M * Re(conj(W_h) (w . D) conj(W_w)) per plane.
//
// Every DFT is a dense complex GEMM against the symmetric twiddle matrix W_n[j][k] = exp(-2 pi i jk / n) / sqrt(n), on
// the fp32 MFMA (v_mfma_f32_16x16x4_f32: an exact fp32 fma chain), so one code path covers every size (80, odd sides,
// h != w).  The matrix is never stored: a tile reads the table tw_n[m] = (cos, sin)(2 pi m / n) / sqrt(n) at the integer
// index (j k) mod n; vqw_freq_twiddles evaluates every entry in double and rounds it once.
//
//   row pass       Y = x W_w                 x = win(pred) - win(target) formed on load
//   column pass    D = W_h Y                 epilogue: per-tile (max f, sum f |D|^2)
//   fold           per-plane / global max, loss in a fixed order (no atomics: bit-deterministic)
//   backward       Z = conj(W_h) (c w . D)   weight recomputed on load from D and the folded max
//                  g = Re(Z conj(W_w))       epilogue: the window's slope and clamp mask, -g to the target
#include "mfma_util.h"
#include "../../include/vqwnet_hip.h"

#define FQ_TILE 64           // output tile per workgroup (4 waves x 32 x 32)
#define FQ_KT 16             // k per LDS stage
#define FQ_LD (FQ_TILE + 4)  // LDS row pitch (floats)
#define FQ_MAX_SIDE 4096

enum { FQ_ROW_FWD = 0, FQ_COL_FWD = 1, FQ_COL_BWD = 2, FQ_ROW_BWD = 3 };

struct FqShape {
    int N, C, H, W, pf, h, w, P, tiles_m, tiles_n;
    long M;                  // N * C * H * W
};

static FqShape fq_shape(int N, int C, int H, int W, int pf) {
    FqShape s;
    s.N = N; s.C = C; s.H = H; s.W = W; s.pf = pf;
    s.h = H / pf; s.w = W / pf;
    s.P = N * pf * pf * C;
    s.tiles_m = ceil_div(s.h, FQ_TILE);
    s.tiles_n = ceil_div(s.w, FQ_TILE);
    s.M = (long)N * C * H * W;
    return s;
}

// workspace: Y (the row pass; reused as Z by the backward pass) | D | tile partials [P][tiles][2] double | F [P] float
static size_t fq_off_d(const FqShape& s) { return (size_t)s.M * 2 * sizeof(float); }
static size_t fq_off_part(const FqShape& s) { return fq_off_d(s) * 2; }
static size_t fq_off_f(const FqShape& s) { return fq_off_part(s) + (size_t)s.P * s.tiles_m * s.tiles_n * 2 * sizeof(double); }
static size_t fq_bytes(const FqShape& s) { return fq_off_f(s) + (size_t)s.P * sizeof(float); }

static int fq_check(const char* name, int N, int C, int H, int W, int pf) {
    VQW_CHECK(N > 0 && C > 0 && H > 0 && W > 0 && pf > 0, "%s: bad shape", name);
    VQW_CHECK(H % pf == 0 && W % pf == 0, "%s: H=%d and W=%d must be divisible by patch_factor=%d", name, H, W, pf);
    VQW_CHECK(H / pf <= FQ_MAX_SIDE && W / pf <= FQ_MAX_SIDE, "%s: patch sides above %d", name, FQ_MAX_SIDE);
    VQW_CHECK((long)N * pf * pf * C <= 65535, "%s: more than 65535 planes", name);
    VQW_CHECK((long)N * C * H * W < (1L << 31), "%s: tensor too large", name);
    return VQW_OK;
}

extern "C" size_t vqw_freq_loss_ws_bytes(int N, int C, int H, int W, int patch_factor) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || patch_factor <= 0) return 0;
    return fq_bytes(fq_shape(N, C, H, W, patch_factor));
}

__global__ void k_freq_twiddles(float* __restrict__ tw, int n) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const double a = 6.283185307179586476925286766559 * (double)m / (double)n, s = 1.0 / sqrt((double)n);
    tw[2 * m] = (float)(cos(a) * s);
    tw[2 * m + 1] = (float)(sin(a) * s);
}

extern "C" int vqw_freq_twiddles(float* tw, int n, void* stream) {
    VQW_CHECK(tw && n > 0 && n <= FQ_MAX_SIDE, "vqw_freq_twiddles: bad arguments");
    k_freq_twiddles<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(tw, n);
    VQW_LAUNCH_CHECK("vqw_freq_twiddles");
    return VQW_OK;
}

struct FqArgs {
    const float* pred;
    const float* target;
    const float* tw_h;       // [h][2]
    const float* tw_w;       // [w][2]
    float2* y;               // Y / Z   [P][h][w]
    float2* d;               // D       [P][h][w]
    double* part;            // [P][tiles][2] = (max f, sum f |D|^2)
    const float* fmax;       // [P] folded max (backward)
    const float* gloss;
    float* gpred;
    float* gtarget;
    int C, H, W, pf, h, w, tiles_n;
    float alpha, lw_over_m;
    int log_matrix, windowed;
    float wa, wb, lo, hi;
};

__device__ __forceinline__ float fq_win(float v, const FqArgs& a) {
    return a.windowed ? fminf(fmaxf(a.wa * v + a.wb, a.lo), a.hi) : v;
}

__device__ __forceinline__ float fq_weight_f(float re, float im, const FqArgs& a) {
    const float mag = sqrtf(re * re + im * im);
    float f = a.alpha == 1.f ? mag : powf(mag, a.alpha);
    if (a.log_matrix) f = logf(f + 1.f);
    return f;
}

// pixel offset (NHWC) of element (r, j) of plane p = ((n * pf^2 + patch) * C + c)
__device__ __forceinline__ long fq_pix(int p, int r, int j, const FqArgs& a) {
    const int c = p % a.C, q = p / a.C, patch = q % (a.pf * a.pf), n = q / (a.pf * a.pf);
    const int y = (patch / a.pf) * a.h + r, x = (patch % a.pf) * a.w + j;
    return (((long)n * a.H + y) * a.W + x) * a.C + c;
}

// One 64 x 64 output tile of one plane: O (h x w) = A (h x K) B (K x w) with K = w (row passes) or h (column passes).
template <int MODE>
__global__ void __launch_bounds__(256) k_freq_gemm(FqArgs a) {
    __shared__ float sAr[FQ_KT][FQ_LD], sAi[FQ_KT][FQ_LD], sBr[FQ_KT][FQ_LD], sBi[FQ_KT][FQ_LD];
    __shared__ double sRed[4][2];
    constexpr bool ROW = MODE == FQ_ROW_FWD || MODE == FQ_ROW_BWD;
    constexpr bool A_REAL = MODE == FQ_ROW_FWD;          // x is real
    constexpr bool RE_ONLY = MODE == FQ_ROW_BWD;         // the gradient is the real part
    const int p = blockIdx.y;
    const int tm = blockIdx.x / a.tiles_n, tn = blockIdx.x % a.tiles_n;
    const int m0 = tm * FQ_TILE, n0 = tn * FQ_TILE;
    const int h = a.h, w = a.w, K = ROW ? w : h;
    const float* tw = ROW ? a.tw_w : a.tw_h;             // table of the twiddle operand (side K)
    const float tsign = (MODE == FQ_ROW_FWD || MODE == FQ_COL_FWD) ? -1.f : 1.f;   // forward W, backward conj(W)
    const long pl = (long)p * h * w;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;

    float coef = 0.f, finv_ok = 0.f, fm = 0.f;
    if (MODE == FQ_COL_BWD) {
        coef = (float)(2.0 * (double)a.lw_over_m * (double)a.gloss[0]);
        fm = a.fmax[p];
        finv_ok = fm > 0.f ? 1.f : 0.f;                  // max 0: w = NaN -> 0 everywhere on the plane
    }

    f32x4 accr[2][2], acci[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            accr[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            acci[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }

    for (int k0 = 0; k0 < K; k0 += FQ_KT) {
        // A tile: 64 (m) x 16 (k), stored k-major
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int idx = t + 256 * s, kk = idx & 15, mm = idx >> 4;
            const int m = m0 + mm, k = k0 + kk;
            float vr = 0.f, vi = 0.f;
            if (m < h && k < K) {
                if (MODE == FQ_ROW_FWD) {
                    const long o = fq_pix(p, m, k, a);
                    vr = fq_win(a.pred[o], a) - fq_win(a.target[o], a);
                } else if (MODE == FQ_ROW_BWD) {
                    const float2 z = a.y[pl + (long)m * w + k];
                    vr = z.x; vi = z.y;
                } else {
                    const int e = (int)(((long)m * k) % h);
                    vr = tw[2 * e]; vi = tsign * tw[2 * e + 1];
                }
            }
            sAr[kk][mm] = vr;
            if (!A_REAL) sAi[kk][mm] = vi;
        }
        // B tile: 16 (k) x 64 (n)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int idx = t + 256 * s, nn = idx & 63, kk = idx >> 6;
            const int n = n0 + nn, k = k0 + kk;
            float vr = 0.f, vi = 0.f;
            if (n < w && k < K) {
                if (ROW) {
                    const int e = (int)(((long)k * n) % w);
                    vr = tw[2 * e]; vi = tsign * tw[2 * e + 1];
                } else if (MODE == FQ_COL_FWD) {
                    const float2 v = a.y[pl + (long)k * w + n];
                    vr = v.x; vi = v.y;
                } else {                                 // G = c * w(D) * D
                    const float2 v = a.d[pl + (long)k * w + n];
                    const float f = fq_weight_f(v.x, v.y, a);
                    const float wt = finv_ok > 0.f ? fminf(fmaxf(f / fm, 0.f), 1.f) : 0.f;
                    const float g = coef * (wt == wt ? wt : 0.f);
                    vr = g * v.x; vi = g * v.y;
                }
            }
            sBr[kk][nn] = vr;
            sBi[kk][nn] = vi;
        }
        __syncthreads();
        // the stage's 16 k accumulate in fresh registers and are then added to the running sums: a rounding chain of
        // 16 + K / 16 terms instead of K (at 512 the gradient's error is 2.1e-6 of its max with one chain, the gate 2e-6)
        f32x4 pr[2][2], pi[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pr[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                pi[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int kk = 0; kk < FQ_KT; kk += 4) {
            const int kr = kk + (lane >> 4), c16 = lane & 15;
            float ar[2], ai[2], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ar[i] = sAr[kr][wm + 16 * i + c16];
                ai[i] = A_REAL ? 0.f : sAi[kr][wm + 16 * i + c16];
                br[i] = sBr[kr][wn + 16 * i + c16];
                bi[i] = sBi[kr][wn + 16 * i + c16];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    pr[i][j] = MFMA16(ar[i], br[j], pr[i][j]);
                    if (!A_REAL) pr[i][j] = MFMA16(-ai[i], bi[j], pr[i][j]);
                    if (!RE_ONLY) {
                        pi[i][j] = MFMA16(ar[i], bi[j], pi[i][j]);
                        if (!A_REAL) pi[i][j] = MFMA16(ai[i], br[j], pi[i][j]);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                accr[i][j] += pr[i][j];
                if (!RE_ONLY) acci[i][j] += pi[i][j];
            }
        __syncthreads();
    }

    // epilogue: lane holds rows wm + 16 i + 4 (lane >> 4) + v, column wn + 16 j + (lane & 15)
    float lmax = 0.f;
    double lsum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = m0 + wm + 16 * i + 4 * (lane >> 4) + v, n = n0 + wn + 16 * j + (lane & 15);
                if (m >= h || n >= w) continue;
                const float re = accr[i][j][v], im = acci[i][j][v];
                if (MODE == FQ_ROW_FWD || MODE == FQ_COL_BWD) {
                    a.y[pl + (long)m * w + n] = make_float2(re, im);
                } else if (MODE == FQ_COL_FWD) {
                    a.d[pl + (long)m * w + n] = make_float2(re, im);
                    const float f = fq_weight_f(re, im, a);
                    lmax = fmaxf(lmax, f);
                    lsum += (double)f * ((double)re * re + (double)im * im);
                } else {
                    const long o = fq_pix(p, m, n, a);
                    if (a.gpred) {
                        float g = re;
                        if (a.windowed) {
                            const float z = a.wa * a.pred[o] + a.wb;
                            g = (z > a.lo && z < a.hi) ? g * a.wa : 0.f;
                        }
                        a.gpred[o] = g;
                    }
                    if (a.gtarget) {
                        float g = -re;
                        if (a.windowed) {
                            const float z = a.wa * a.target[o] + a.wb;
                            g = (z > a.lo && z < a.hi) ? g * a.wa : 0.f;
                        }
                        a.gtarget[o] = g;
                    }
                }
            }
    if (MODE == FQ_COL_FWD) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, o, 64));
        lsum = wave_sum_d(lsum);
        if (lane == 0) {
            sRed[wv][0] = (double)lmax;
            sRed[wv][1] = lsum;
        }
        __syncthreads();
        if (t == 0) {
            double* o = a.part + ((long)p * gridDim.x + blockIdx.x) * 2;
            o[0] = fmax(fmax(sRed[0][0], sRed[1][0]), fmax(sRed[2][0], sRed[3][0]));
            o[1] = ((sRed[0][1] + sRed[1][1]) + sRed[2][1]) + sRed[3][1];
        }
    }
}

// per-plane (or global) max and the scalar loss, one workgroup, fixed summation order
__global__ void __launch_bounds__(256) k_freq_fold(const double* __restrict__ part, float* __restrict__ fmax_out,
                                                   float* __restrict__ loss, int P, int tiles, int batch_matrix,
                                                   double lw_over_m) {
    __shared__ double sm[256];
    const int t = threadIdx.x;
    double gmax = 0.0;
    for (int p = t; p < P; p += 256) {
        double f = 0.0;
        for (int i = 0; i < tiles; ++i) f = fmax(f, part[((long)p * tiles + i) * 2]);
        fmax_out[p] = (float)f;                          // a max of fp32 values: exact
        gmax = fmax(gmax, f);
    }
    sm[t] = gmax;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sm[t] = fmax(sm[t], sm[t + s]);
        __syncthreads();
    }
    gmax = sm[0];
    __syncthreads();
    double acc = 0.0;
    for (int p = t; p < P; p += 256) {
        double s = 0.0;
        for (int i = 0; i < tiles; ++i) s += part[((long)p * tiles + i) * 2 + 1];
        const double f = batch_matrix ? gmax : (double)fmax_out[p];
        if (batch_matrix) fmax_out[p] = (float)gmax;
        acc += f > 0.0 ? s / f : 0.0;                    // max 0: every weight NaN -> 0
    }
    sm[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sm[t] += sm[t + s];
        __syncthreads();
    }
    if (t == 0) loss[0] = (float)(sm[0] * lw_over_m);
}

static int fq_args(FqArgs& a, const FqShape& s, const float* pred, const float* target, const float* tw_h,
                   const float* tw_w, void* ws, float alpha, int log_matrix, float loss_weight, int windowed, float wa,
                   float wb, float lo, float hi) {
    a.pred = pred; a.target = target; a.tw_h = tw_h; a.tw_w = tw_w;
    char* b = (char*)ws;
    a.y = (float2*)b;
    a.d = (float2*)(b + fq_off_d(s));
    a.part = (double*)(b + fq_off_part(s));
    a.fmax = (const float*)(b + fq_off_f(s));
    a.gloss = nullptr; a.gpred = nullptr; a.gtarget = nullptr;
    a.C = s.C; a.H = s.H; a.W = s.W; a.pf = s.pf; a.h = s.h; a.w = s.w; a.tiles_n = s.tiles_n;
    a.alpha = alpha;
    a.lw_over_m = (float)((double)loss_weight / (double)s.M);
    a.log_matrix = log_matrix != 0;
    a.windowed = windowed != 0;
    a.wa = wa; a.wb = wb; a.lo = lo; a.hi = hi;
    return VQW_OK;
}

extern "C" int vqw_freq_loss_fwd(const float* pred, const float* target, const float* tw_h, const float* tw_w, float* loss,
                                 void* ws, size_t ws_bytes, int N, int C, int H, int W, int patch_factor, float alpha,
                                 int log_matrix, int batch_matrix, float loss_weight, int windowed, float win_alpha,
                                 float win_beta, float win_lo, float win_hi, void* stream) {
    VQW_CHECK(pred && target && tw_h && tw_w && loss && ws, "vqw_freq_loss_fwd: bad arguments");
    if (fq_check("vqw_freq_loss_fwd", N, C, H, W, patch_factor) != VQW_OK) return VQW_ERR_ARG;
    VQW_CHECK(alpha >= 0.f, "vqw_freq_loss_fwd: alpha must be >= 0 (got %g)", (double)alpha);
    VQW_CHECK(!windowed || win_lo <= win_hi, "vqw_freq_loss_fwd: bad window");
    const FqShape s = fq_shape(N, C, H, W, patch_factor);
    VQW_CHECK(ws_bytes >= fq_bytes(s), "vqw_freq_loss_fwd: workspace too small");
    FqArgs a;
    fq_args(a, s, pred, target, tw_h, tw_w, ws, alpha, log_matrix, loss_weight, windowed, win_alpha, win_beta, win_lo, win_hi);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(s.tiles_m * s.tiles_n, s.P);
    k_freq_gemm<FQ_ROW_FWD><<<grid, 256, 0, st>>>(a);
    k_freq_gemm<FQ_COL_FWD><<<grid, 256, 0, st>>>(a);
    k_freq_fold<<<1, 256, 0, st>>>(a.part, (float*)a.fmax, loss, s.P, s.tiles_m * s.tiles_n, batch_matrix != 0,
                                   (double)loss_weight / (double)s.M);
    VQW_LAUNCH_CHECK("vqw_freq_loss_fwd");
    return VQW_OK;
}

extern "C" int vqw_freq_loss_bwd(const float* pred, const float* target, const float* tw_h, const float* tw_w,
                                 const float* gloss, float* gpred, float* gtarget, void* ws, size_t ws_bytes, int N, int C,
                                 int H, int W, int patch_factor, float alpha, int log_matrix, float loss_weight,
                                 int windowed, float win_alpha, float win_beta, float win_lo, float win_hi, void* stream) {
    VQW_CHECK(pred && target && tw_h && tw_w && gloss && ws && (gpred || gtarget), "vqw_freq_loss_bwd: bad arguments");
    if (fq_check("vqw_freq_loss_bwd", N, C, H, W, patch_factor) != VQW_OK) return VQW_ERR_ARG;
    VQW_CHECK(alpha >= 0.f, "vqw_freq_loss_bwd: alpha must be >= 0 (got %g)", (double)alpha);
    const FqShape s = fq_shape(N, C, H, W, patch_factor);
    VQW_CHECK(ws_bytes >= fq_bytes(s), "vqw_freq_loss_bwd: workspace too small");
    FqArgs a;
    fq_args(a, s, pred, target, tw_h, tw_w, ws, alpha, log_matrix, loss_weight, windowed, win_alpha, win_beta, win_lo, win_hi);
    a.gloss = gloss; a.gpred = gpred; a.gtarget = gtarget;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(s.tiles_m * s.tiles_n, s.P);
    k_freq_gemm<FQ_COL_BWD><<<grid, 256, 0, st>>>(a);
    k_freq_gemm<FQ_ROW_BWD><<<grid, 256, 0, st>>>(a);
    VQW_LAUNCH_CHECK("vqw_freq_loss_bwd");
    return VQW_OK;
}
