// Spectral normalisation of convolution weights (torch.nn.utils.spectral_norm with its defaults: one power iteration,
// eps 1e-12, dim 0) and the ActNorm pieces that the BatchNorm-affine kernels of norm.hip do not already give.
//
// A weight is the matrix W [rows = Cout][K = k*k*Cin] exactly as it lies in memory (OHWI: column m = tap * Cin + ci).  torch
// flattens the logical (Cout, Cin, k, k) tensor, so the buffer `weight_v` is indexed j = ci * taps + tap: only the loads and
// stores of v permute, every product runs in memory order.
//
// All layers of one discriminator forward go through the same launches (a device table of SnLayer records, as vqw_adam_multi
// does for the optimiser), one launch per dependent phase - no grid barrier:
//   1  t = W^T u              workgroup = (layer, 64 columns), 4 row groups per column, doubles        (training only)
//   2  s = W v                workgroup = (layer, row); v = t / max(|t|, eps) recomputed per workgroup (K <= a few thousand
//                             floats out of L2) so that no launch sits between the norm and its use; row 0 stores v
//   3  weight = W / sigma     workgroup = (layer, 4096 elements); u = s / max(|s|, eps) and sigma = u . s recomputed per
//                             workgroup from the <= 512 entries of s; chunk 0 stores u and sigma
// Every sum is a double accumulation in a fixed order (thread-strided partials, wave butterfly, the four wave totals added in
// order): run-to-run bit-identical, no atomics.  Each forward also leaves (u, v in memory order, sigma) in a `save` area of
// its own for its backward:  dL/dW = (G - <G, weight> u v^T) / sigma, two launches for all layers of a backward pass.
#include "common.h"
#include "../../include/vqwnet_hip.h"

namespace {

struct SnLayer {                 // 16 x 8 bytes; the table layout is part of the ABI (hipops/ops.py builds it)
    const float* W;              // [rows][K]
    float* u;                    // [rows]            module buffer weight_u
    float* v;                    // [K] logical order module buffer weight_v
    float* out;                  // [rows][K]         W / sigma
    float* save;                 // u[rows], v[K] in memory order, sigma
    float* t;                    // [K] scratch: W^T u
    float* s;                    // [rows] scratch: W v
    long rows, K, Cin;
    long blk1, blk2, blk3;       // first workgroup of this layer in phases 1, 2, 3
    float* sv;                   // [1] or NULL: receives sigma in training (BigGAN's logging buffer sv0)
    long pad_[2];
};
struct SnGrad {                  // 8 x 8 bytes
    const float* G;              // [rows][K] dL/d weight (OHWI)
    const float* weight;         // [rows][K] the forward's W / sigma
    const float* save;           // that forward's u, v, sigma
    float* gW;                   // [rows][K]
    double* part;                // one partial of <G, weight> per chunk
    long rows, K, blk;
};
constexpr int SN_CHUNK = 4096;   // elements per workgroup of the element-wise phases
constexpr int SN_COLS = 64;      // columns per workgroup of phase 1

// total over the 256 threads of a workgroup, the same bits every run; every thread gets it
__device__ __forceinline__ double block_sum_d(double v, double* sm) {
    v = wave_sum_d(v);
    __syncthreads();                                   // sm may still be read from the previous call
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

template <class T>
__device__ __forceinline__ int layer_of(const T* tab, int n, long b, long T::*first) {
    int l = 0;
    while (l + 1 < n && tab[l + 1].*first <= b) ++l;
    return l;
}

__global__ void __launch_bounds__(256) k_sn_wtu(const SnLayer* __restrict__ tab, int n) {
    __shared__ double sm[4][SN_COLS];
    const SnLayer L = tab[layer_of(tab, n, blockIdx.x, &SnLayer::blk1)];
    const long col = ((long)blockIdx.x - L.blk1) * SN_COLS + (threadIdx.x & 63);
    const int g = threadIdx.x >> 6;
    double a = 0.0;
    if (col < L.K)
        for (long r = g; r < L.rows; r += 4) a += (double)L.W[r * L.K + col] * (double)L.u[r];
    sm[g][threadIdx.x & 63] = a;
    __syncthreads();
    if (g == 0 && col < L.K) L.t[col] = (float)(((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_sn_wv(const SnLayer* __restrict__ tab, int n, int training, float eps) {
    __shared__ double sm[4];
    const SnLayer L = tab[layer_of(tab, n, blockIdx.x, &SnLayer::blk2)];
    const long r = (long)blockIdx.x - L.blk2;
    const long taps = L.K / L.Cin;
    float den = 1.f;
    if (training) {
        double q = 0.0;
        for (long m = threadIdx.x; m < L.K; m += 256) q += (double)L.t[m] * (double)L.t[m];
        den = fmaxf((float)sqrt(block_sum_d(q, sm)), eps);
    }
    float* vs = L.save + L.rows;
    double a = 0.0;
    for (long m = threadIdx.x; m < L.K; m += 256) {
        const long j = (m % L.Cin) * taps + m / L.Cin;
        const float vm = training ? L.t[m] / den : L.v[j];
        a += (double)L.W[r * L.K + m] * (double)vm;
        if (r == 0) {
            vs[m] = vm;
            if (training) L.v[j] = vm;
        }
    }
    a = block_sum_d(a, sm);
    if (threadIdx.x == 0) L.s[r] = (float)a;
}

__global__ void __launch_bounds__(256) k_sn_scale(const SnLayer* __restrict__ tab, int n, int training, float eps) {
    __shared__ double sm[4];
    const SnLayer L = tab[layer_of(tab, n, blockIdx.x, &SnLayer::blk3)];
    const long chunk = (long)blockIdx.x - L.blk3;
    float den = 1.f;
    if (training) {
        double q = 0.0;
        for (long r = threadIdx.x; r < L.rows; r += 256) q += (double)L.s[r] * (double)L.s[r];
        den = fmaxf((float)sqrt(block_sum_d(q, sm)), eps);
    }
    double a = 0.0;
    for (long r = threadIdx.x; r < L.rows; r += 256) {
        const float ur = training ? L.s[r] / den : L.u[r];
        a += (double)ur * (double)L.s[r];
        if (chunk == 0) {
            L.save[r] = ur;
            if (training) L.u[r] = ur;
        }
    }
    const float sigma = (float)block_sum_d(a, sm);
    if (chunk == 0 && threadIdx.x == 0) {
        L.save[L.rows + L.K] = sigma;
        if (training && L.sv) L.sv[0] = sigma;
    }
    const long total = L.rows * L.K, e0 = chunk * SN_CHUNK;
    const long e1 = e0 + SN_CHUNK < total ? e0 + SN_CHUNK : total;
    for (long e = e0 + threadIdx.x; e < e1; e += 256) L.out[e] = L.W[e] / sigma;
}

__global__ void __launch_bounds__(256) k_sn_bwd_dot(const SnGrad* __restrict__ tab, int n) {
    __shared__ double sm[4];
    const SnGrad L = tab[layer_of(tab, n, blockIdx.x, &SnGrad::blk)];
    const long chunk = (long)blockIdx.x - L.blk;
    const long total = L.rows * L.K, e0 = chunk * SN_CHUNK;
    const long e1 = e0 + SN_CHUNK < total ? e0 + SN_CHUNK : total;
    double a = 0.0;
    for (long e = e0 + threadIdx.x; e < e1; e += 256) a += (double)L.G[e] * (double)L.weight[e];
    a = block_sum_d(a, sm);
    if (threadIdx.x == 0) L.part[chunk] = a;
}

__global__ void __launch_bounds__(256) k_sn_bwd_apply(const SnGrad* __restrict__ tab, int n) {
    __shared__ double sm[4];
    const SnGrad L = tab[layer_of(tab, n, blockIdx.x, &SnGrad::blk)];
    const long chunk = (long)blockIdx.x - L.blk;
    const long total = L.rows * L.K, e0 = chunk * SN_CHUNK;
    const long e1 = e0 + SN_CHUNK < total ? e0 + SN_CHUNK : total;
    const long chunks = (total + SN_CHUNK - 1) / SN_CHUNK;
    double a = 0.0;
    for (long c = threadIdx.x; c < chunks; c += 256) a += L.part[c];
    const float dot = (float)block_sum_d(a, sm);
    const float* us = L.save;
    const float* vs = L.save + L.rows;
    const float sigma = L.save[L.rows + L.K];
    for (long e = e0 + threadIdx.x; e < e1; e += 256) L.gW[e] = (L.G[e] - dot * (us[e / L.K] * vs[e % L.K])) / sigma;
}

// ActNorm (networks/actnorm.py:23-70) on the BatchNorm-affine kernels: mean = -loc, rstd = 1, gamma = scale, beta = 0.
// With `sums` (first training forward) the data-dependent initialisation comes first: loc = -mean, scale = 1 / (std + 1e-6),
// std unbiased (torch.std), and the `initialized` flag is raised.
//
// The initialisation takes its sums from k_actnorm_stats, not from the statistics pass of norm.hip: that pass squares in fp32,
// a relative error of 2^-24 per square which E[x^2] - mean^2 multiplies by (mean / std)^2.  BatchNorm divides by sqrt(var + eps)
// and absorbs it; ActNorm divides by std + 1e-6, so a channel 1e3 standard deviations off zero got its scale 2e-4 ... 8e-4 wrong
// from 126 pixels, and an exactly constant channel (x = 1.15: the fp32 square is 4.5e-8 above the exact one) a scale of 4.7e3
// in place of 1 / 1e-6.  Here every square and every addition is a double, in a fixed order: a workgroup owns 64 channels
// (lanes) x 16 pixel lanes and walks the whole batch.  It runs once per layer and training run.  sums[c] = {sum x, sum x^2}, the
// [C][2] layout of vqw_bn_partial_stats, so a process group all-reduces it the same way.
__global__ void __launch_bounds__(1024) k_actnorm_stats(const float* __restrict__ x, double* __restrict__ sums, long P, int C) {
    __shared__ double sa[16][64], sb[16][64];
    const int lc = threadIdx.x & 63, lp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lc;
    double a = 0.0, b = 0.0;
    if (c < C) {
        for (long p = lp; p < P; p += 16) {
            const double v = (double)x[p * C + c];
            a += v;
            b += v * v;
        }
    }
    sa[lp][lc] = a;
    sb[lp][lc] = b;
    __syncthreads();
    if (lp == 0 && c < C) {
        for (int k = 1; k < 16; ++k) {
            a += sa[k][lc];
            b += sb[k][lc];
        }
        sums[2 * c] = a;
        sums[2 * c + 1] = b;
    }
}
// var = E[x^2] - mean^2 from those double sums.  What their rounding leaves of an exactly constant channel (at most one part in
// 2^53 per addition of a thread's chain) must come out 0: a variance within 2^-36 of E[x^2] - chains of 2^17 additions; a
// channel with |mean| / std above 2^18 - is that residue.
__global__ void k_actnorm_prepare(const double* __restrict__ sums, double count, float* __restrict__ loc, float* __restrict__ scale,
                                  unsigned char* __restrict__ initialized, float* __restrict__ mrb, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (sums) {
        const double mean = sums[2 * c] / count, ex2 = sums[2 * c + 1] / count;
        double var = ex2 - mean * mean;
        if (var <= 0x1p-36 * ex2) var = 0.0;
        if (count > 1.0) var *= count / (count - 1.0);
        loc[c] = -(float)mean;
        scale[c] = 1.f / ((float)sqrt(var) + 1e-6f);
        if (c == 0 && initialized) initialized[0] = 1;
    }
    mrb[2 * c] = -loc[c];
    mrb[2 * c + 1] = 1.f;
    mrb[2 * C + c] = 0.f;
}
__global__ void k_actnorm_loc_grad(const float* __restrict__ dbeta, const float* __restrict__ scale, float* __restrict__ dloc, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) dloc[c] = scale[c] * dbeta[c];
}

}  // namespace

extern "C" int vqw_spectral_norm_fwd(const void* layers_dev, int n_layers, int blocks1, int blocks2, int blocks3, int training,
                                     float eps, void* stream) {
    static_assert(sizeof(SnLayer) == 128, "layer table layout is part of the ABI: 7 pointers + 6 int64 + sv + 2 spare");
    VQW_CHECK(layers_dev && n_layers > 0 && n_layers <= 64 && blocks1 > 0 && blocks2 > 0 && blocks3 > 0 && eps > 0.f,
              "vqw_spectral_norm_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const SnLayer* tab = (const SnLayer*)layers_dev;
    if (training) k_sn_wtu<<<blocks1, 256, 0, st>>>(tab, n_layers);
    k_sn_wv<<<blocks2, 256, 0, st>>>(tab, n_layers, training, eps);
    k_sn_scale<<<blocks3, 256, 0, st>>>(tab, n_layers, training, eps);
    VQW_LAUNCH_CHECK("vqw_spectral_norm_fwd");
    return VQW_OK;
}

extern "C" int vqw_spectral_norm_bwd(const void* grads_dev, int n_layers, int blocks, void* stream) {
    static_assert(sizeof(SnGrad) == 64, "gradient table layout is part of the ABI: 5 pointers + 3 int64");
    VQW_CHECK(grads_dev && n_layers > 0 && n_layers <= 64 && blocks > 0, "vqw_spectral_norm_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    k_sn_bwd_dot<<<blocks, 256, 0, st>>>((const SnGrad*)grads_dev, n_layers);
    k_sn_bwd_apply<<<blocks, 256, 0, st>>>((const SnGrad*)grads_dev, n_layers);
    VQW_LAUNCH_CHECK("vqw_spectral_norm_bwd");
    return VQW_OK;
}

extern "C" int vqw_actnorm_stats(const float* x, double* sums, long P, int C, void* stream) {
    VQW_CHECK(x && sums && P > 0 && C > 0, "vqw_actnorm_stats: bad arguments");
    k_actnorm_stats<<<ceil_div(C, 64), 1024, 0, (hipStream_t)stream>>>(x, sums, P, C);
    VQW_LAUNCH_CHECK("vqw_actnorm_stats");
    return VQW_OK;
}

extern "C" int vqw_actnorm_prepare(const double* sums, double count, float* loc, float* scale, unsigned char* initialized,
                                   float* mean_rstd_beta, int C, void* stream) {
    VQW_CHECK(loc && scale && mean_rstd_beta && C > 0 && (!sums || count > 0), "vqw_actnorm_prepare: bad arguments");
    k_actnorm_prepare<<<ceil_div(C, 256), 256, 0, (hipStream_t)stream>>>(sums, count, loc, scale, initialized, mean_rstd_beta, C);
    VQW_LAUNCH_CHECK("vqw_actnorm_prepare");
    return VQW_OK;
}

extern "C" int vqw_actnorm_loc_grad(const float* dbeta, const float* scale, float* dloc, int C, void* stream) {
    VQW_CHECK(dbeta && scale && dloc && C > 0, "vqw_actnorm_loc_grad: bad arguments");
    k_actnorm_loc_grad<<<ceil_div(C, 256), 256, 0, (hipStream_t)stream>>>(dbeta, scale, dloc, C);
    VQW_LAUNCH_CHECK("vqw_actnorm_loc_grad");
    return VQW_OK;
}
