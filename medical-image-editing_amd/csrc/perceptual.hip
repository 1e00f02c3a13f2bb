// VGG perceptual loss (the reference's VGGLoss(conv_index='22'): vgg19.features[:8], trainers/base.py:271-275,
// functions/perceptual_loss.py) around the project's convolution kernels.  The operator (hipops.ops.perceptual_loss)
// runs one batch of 2M = 2 * nwin * N images: the sr (recon) half first, then the hr (clear) half, each ordered
// (window, image).  The kernels here are the parts the stock convolutions do not cover:
//
//   stem forward      A1 = relu(conv3x3(win(x), w1) + b1), 1 or 3 input channels -> 64, both halves in one launch; the
//                     window map win(x) = clamp(alpha x + beta, lo, hi) of image b's window is applied on load, zero
//                     padding after it (the reference windows the image, then pads).  With C = 1 the caller passes w1
//                     summed over its 3 input channels: expand() makes that exact in real arithmetic.
//   difference        D = A2[sr] - A2[hr]: conv2_2 is linear and its output is taken before its ReLU, so the bias cancels
//                     and vgg(sr) - vgg(hr) = conv2_2(D) (one convolution instead of two, no cancellation of two large
//                     fp32 outputs)
//   loss              loss[w] = sum Y^2 / numel over window w's images: per-block double partials, one fixed-order fold
//                     per window (no atomics: bit-deterministic)
//   stem input grad   g_sr = sum over windows of 2 g_w / numel * win'(sr) * conv3x3^T(dZ1, w1) (64 -> Cin), where
//                     win'(x) = alpha inside the clamp (lo < alpha x + beta < hi, the vqw_window_mse_bwd convention), else 0
//
// Every accumulation runs in one fixed order per output element, independent of its position: equal input neighbourhoods
// give bit-equal outputs, so plateaus of the windowed input stay exact ties for the max-pool behind conv1_2.
#include "common.h"
#include "prof.h"
#include "../../include/vqwnet_hip.h"

#define PC_C1 64             // conv1_x channels
#define PC_LOSS_BLOCKS 1024  // partial sums per window

__device__ __forceinline__ float pc_win(float x, const float* win) {
    return fminf(fmaxf(win[0] * x + win[1], win[2]), win[3]);
}

extern "C" int vqw_percep_supported(int N, int Cin, int H, int W) {
    if (N < 1 || (Cin != 1 && Cin != 3) || H < 2 || W < 2) return 0;
    return (long)N * H * W <= (1L << 40) ? 1 : 0;
}

// Thread = one pixel x 4 output channels: 16 threads store one pixel's 64 channels as one 256-byte row, a block of 256
// threads 16 consecutive pixels (4 KB contiguous).  The thread's 4 x 9 x CIN weights live in registers.
template <int CIN>
__global__ __launch_bounds__(256) void k_percep_stem_fwd(const float* __restrict__ sr, const float* __restrict__ hr,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ win, float* __restrict__ a1, int N, int nwin,
                                                         int H, int W, long P) {
    const long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (p >= P) return;
    const int q = threadIdx.x & 15;
    float wr[4][9][CIN];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) wr[j][t][ci] = w[((4 * q + j) * 9 + t) * CIN + ci];
    const long HW = (long)H * W;
    const long b = p / HW;
    const int r = (int)(p - b * HW), y = r / W, x = r - y * W;
    const long M = (long)nwin * N;
    const int half = (int)(b / M);
    const long m = b - half * M;
    const int wi = (int)(m / N);
    const long n = m - (long)wi * N;
    const float* src = (half ? hr : sr) + n * HW * CIN;
    float wv[4] = {1.f, 0.f, 0.f, 0.f};
    if (win) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = win[4 * wi + k];
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            float v = 0.f;
            if (in) {
                v = src[((long)yy * W + xx) * CIN + ci];
                if (win) v = pc_win(v, wv);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(wr[j][t][ci], v, acc[j]);
        }
    }
    float4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaxf(acc[j] + bias[4 * q + j], 0.f);
    *(float4_t*)(a1 + p * PC_C1 + 4 * q) = o;
}

extern "C" int vqw_percep_stem_fwd(const float* sr, const float* hr, const float* w, const float* bias, const float* win, float* a1,
                                   int N, int nwin, int Cin, int H, int W, void* stream) {
    VQW_CHECK(sr && hr && w && bias && a1, "vqw_percep_stem_fwd: bad arguments");
    VQW_CHECK(vqw_percep_supported(N, Cin, H, W), "vqw_percep_stem_fwd: unsupported shape N=%d Cin=%d H=%d W=%d", N, Cin, H, W);
    VQW_CHECK(nwin >= 1 && nwin <= 3 && (win || nwin == 1), "vqw_percep_stem_fwd: nwin=%d needs a window table (1..3)", nwin);
    const long P = 2L * nwin * N * H * W;
    ProfScope ps(2, 2.0 * P * PC_C1 * 9 * Cin, (hipStream_t)stream, 4.0 * (P * Cin / 2 + P * PC_C1));
    const long blocks = (P + 15) / 16;
    VQW_CHECK(blocks < (1L << 31), "vqw_percep_stem_fwd: batch too large");
    if (Cin == 1)
        k_percep_stem_fwd<1><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, hr, w, bias, win, a1, N, nwin, H, W, P);
    else
        k_percep_stem_fwd<3><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, hr, w, bias, win, a1, N, nwin, H, W, P);
    VQW_LAUNCH_CHECK("vqw_percep_stem_fwd");
    return VQW_OK;
}

__global__ void k_percep_diff(const float4_t* __restrict__ a, float4_t* __restrict__ d, long n4) {
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) d[i] = a[i] - a[i + n4];
}

extern "C" int vqw_percep_diff(const float* a2, float* d, long n, void* stream) {
    VQW_PROF_HBM(stream, 3, n);
    VQW_CHECK(a2 && d && n > 0 && n % 4 == 0, "vqw_percep_diff: bad arguments (n=%ld)", n);
    k_percep_diff<<<stream_grid(n / 4, 256), 256, 0, (hipStream_t)stream>>>((const float4_t*)a2, (float4_t*)d, n / 4);
    VQW_LAUNCH_CHECK("vqw_percep_diff");
    return VQW_OK;
}

extern "C" size_t vqw_percep_loss_ws_bytes(int nwin) { return (size_t)(nwin > 0 ? nwin : 1) * PC_LOSS_BLOCKS * sizeof(double); }

// grid (PC_LOSS_BLOCKS, nwin): block k of window w strides over the window's n elements in a fixed pattern
__global__ __launch_bounds__(256) void k_percep_sumsq(const float* __restrict__ y, double* __restrict__ part, long n) {
    __shared__ double sm[4];
    const float* yw = y + (long)blockIdx.y * n;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double v = (double)yw[i];
        acc += v * v;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(256) void k_percep_fold(const double* __restrict__ part, int nparts, double scale, float* __restrict__ loss) {
    __shared__ double sm[4];
    const double* pw = part + (long)blockIdx.x * nparts;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc += pw[i];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)(((sm[0] + sm[1]) + (sm[2] + sm[3])) * scale);
}

extern "C" int vqw_percep_loss_fwd(const float* y, float* loss, void* ws, size_t ws_bytes, int nwin, long per_window, void* stream) {
    VQW_PROF_HBM(stream, 1, (double)nwin * per_window);
    VQW_CHECK(y && loss && ws && nwin >= 1 && nwin <= 3 && per_window > 0, "vqw_percep_loss_fwd: bad arguments");
    VQW_CHECK(ws_bytes >= vqw_percep_loss_ws_bytes(nwin), "vqw_percep_loss_fwd: workspace too small");
    k_percep_sumsq<<<dim3(PC_LOSS_BLOCKS, nwin), 256, 0, (hipStream_t)stream>>>(y, (double*)ws, per_window);
    k_percep_fold<<<nwin, 256, 0, (hipStream_t)stream>>>((const double*)ws, PC_LOSS_BLOCKS, 1.0 / (double)per_window, loss);
    VQW_LAUNCH_CHECK("vqw_percep_loss_fwd");
    return VQW_OK;
}

// Thread = one input pixel x 4 of the 64 gradient channels, all windows: the 16 threads of a pixel read each tap's 256-byte
// row of dz1 together, and their partial sums over channels are combined by a fixed butterfly across the 16 lanes (the
// same bits every run).  dz1: [nwin * N][H][W][64], the gradient in front of the stem's ReLU (sr half).  Taps whose output
// position leaves the image contribute nothing (zero padding).
template <int CIN>
__global__ __launch_bounds__(256) void k_percep_stem_bwd(const float* __restrict__ sr, const float* __restrict__ w,
                                                         const float* __restrict__ win, const float* __restrict__ g0,
                                                         const float* __restrict__ g1, const float* __restrict__ g2,
                                                         const float* __restrict__ dz1, float* __restrict__ gsr, int N, int nwin,
                                                         int H, int W, float inv_numel2) {
    const int q = threadIdx.x & 15;
    const long HW = (long)H * W;
    const long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = p < (long)N * HW;          // whole 16-lane groups: every lane takes part in the shuffles
    float wr[4][9][CIN];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) wr[j][t][ci] = w[((4 * q + j) * 9 + t) * CIN + ci];
    const long n = live ? p / HW : 0;
    const int r = live ? (int)(p - n * HW) : 0, y = r / W, x = r - y * W;
    float g[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) g[ci] = 0.f;
    for (int wi = 0; wi < nwin; ++wi) {
        const float* gl = wi == 0 ? g0 : wi == 1 ? g1 : g2;
        const float s = gl[0] * inv_numel2;
        const float* dz = dz1 + ((long)wi * N + n) * HW * PC_C1 + 4 * q;
        float acc[CIN];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int oy = y + 1 - t / 3, ox = x + 1 - t % 3;
            if (!live || oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
            const float4_t v = *(const float4_t*)(dz + ((long)oy * W + ox) * PC_C1);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) acc[ci] = fmaf(wr[j][t][ci], v[j], acc[ci]);
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
            g[ci] = fmaf(acc[ci], f, g[ci]);
        }
    }
    if (live && q == 0) {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) gsr[p * CIN + ci] = g[ci];
    }
}

extern "C" int vqw_percep_stem_bwd(const float* sr, const float* w, const float* win, const float* g0, const float* g1, const float* g2,
                                   const float* dz1, float* gsr, int N, int nwin, int Cin, int H, int W, long numel, void* stream) {
    VQW_CHECK(sr && w && g0 && dz1 && gsr && numel > 0, "vqw_percep_stem_bwd: bad arguments");
    VQW_CHECK(vqw_percep_supported(N, Cin, H, W), "vqw_percep_stem_bwd: unsupported shape N=%d Cin=%d H=%d W=%d", N, Cin, H, W);
    VQW_CHECK(nwin >= 1 && nwin <= 3 && (win || nwin == 1) && (nwin < 2 || g1) && (nwin < 3 || g2),
              "vqw_percep_stem_bwd: nwin=%d needs a window table and one loss gradient per window", nwin);
    const long P = (long)N * H * W;
    ProfScope ps(2, 2.0 * P * nwin * PC_C1 * 9 * Cin, (hipStream_t)stream, 4.0 * (P * nwin * PC_C1 + 2.0 * P * Cin));
    const long blocks = (P + 15) / 16;
    VQW_CHECK(blocks < (1L << 31), "vqw_percep_stem_bwd: batch too large");
    const float s2 = (float)(2.0 / (double)numel);
    if (Cin == 1)
        k_percep_stem_bwd<1><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, w, win, g0, g1, g2, dz1, gsr, N, nwin, H, W, s2);
    else
        k_percep_stem_bwd<3><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(sr, w, win, g0, g1, g2, dz1, gsr, N, nwin, H, W, s2);
    VQW_LAUNCH_CHECK("vqw_percep_stem_bwd");
    return VQW_OK;
}
