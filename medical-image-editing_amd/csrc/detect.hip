// Anomaly detection with the code prior (trainers/prior.py PriorTrainer.detect, trainers/fit.py Fit.detect): the smoothed
// residual map of a restoration, the streaming histogram of its scores by an order-preserving 16-bit key, and AUROC / average
// precision / best Dice from that histogram.  fp32 in, no float atomics (the histogram's integer adds have no order), the same
// bits every run.
#include "common.h"
#include "../../include/vqwnet_hip.h"

// ------------------------------------------------------------------------------------------------ the map
// map = G_sigma(r o U(m)): r = mean_c |a - b|, U = bilinear up-sampling of the cell mask (half-pixel centres, clamped edges),
// G = the separable Gaussian with clamped borders.  ONE kernel: a workgroup owns an AM_TY x AM_TX tile of the map, computes
// r o U(m) for the tile and a halo of R = (K - 1) / 2 pixels straight into LDS (a halo pixel outside the picture is the clamped
// pixel, which IS the replicate border), runs the row pass and then the column pass in LDS and writes the tile: a and b are read
// once (plus the halo), the map is written once, nothing else touches HBM.  Both passes add their taps in ascending order.
#define AM_TY 32
#define AM_TX 64
#define AM_MAX_R 16            // the widest halo: K <= 33 taps, sigma <= 5.33 under K = 2 ceil(3 sigma) + 1

__global__ void __launch_bounds__(256) k_anomaly_map(const float* __restrict__ a, const float* __restrict__ b,
                                                     const uint8_t* __restrict__ cellmask, const float* __restrict__ taps,
                                                     float* __restrict__ map, int H, int W, int C, int h, int w, int K) {
    extern __shared__ float am_lds[];
    const int R = K / 2, SW = AM_TX + 2 * R, SH = AM_TY + 2 * R;
    float* s = am_lds;                      // [SH][SW]: r o U(m) of tile + halo
    float* t = s + SH * SW;                 // [SH][AM_TX]: after the row pass
    float* g = t + SH * AM_TX;              // [K]
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * AM_TY, x0 = blockIdx.x * AM_TX;
    for (int k = tid; k < K; k += 256) g[k] = taps[k];
    const float inv_c = 1.0f / (float)C, inv_fy = (float)h / (float)H, inv_fx = (float)w / (float)W;
    const float* an = a + (long)n * H * W * C;
    const float* bn = b + (long)n * H * W * C;
    const uint8_t* mn = cellmask ? cellmask + (long)n * h * w : nullptr;
    // e / SW by a multiply and a shift: exact while e SW < 2^20 (e < 64 * 96, SW <= 96)
    const unsigned inv_sw = ((1u << 20) + SW - 1) / SW;
    for (int e = tid; e < SH * SW; e += 256) {
        const int i = (int)(((unsigned)e * inv_sw) >> 20), j = e - i * SW;
        const int y = min(max(y0 - R + i, 0), H - 1), x = min(max(x0 - R + j, 0), W - 1);
        const float* pa = an + ((long)y * W + x) * C;
        const float* pb = bn + ((long)y * W + x) * C;
        float r = 0.0f;
        for (int c = 0; c < C; ++c) r += fabsf(pa[c] - pb[c]);
        r *= inv_c;
        if (mn) {       // F.interpolate(mode='bilinear', align_corners=False): src = max(0, (dst + 0.5) h / H - 0.5)
            const float sy = fmaxf(((float)y + 0.5f) * inv_fy - 0.5f, 0.0f), sx = fmaxf(((float)x + 0.5f) * inv_fx - 0.5f, 0.0f);
            const int cy0 = min((int)sy, h - 1), cx0 = min((int)sx, w - 1);
            const int cy1 = min(cy0 + 1, h - 1), cx1 = min(cx0 + 1, w - 1);
            const float ly = sy - (float)cy0, lx = sx - (float)cx0;
            const float m00 = mn[cy0 * w + cx0] ? 1.0f : 0.0f, m01 = mn[cy0 * w + cx1] ? 1.0f : 0.0f;
            const float m10 = mn[cy1 * w + cx0] ? 1.0f : 0.0f, m11 = mn[cy1 * w + cx1] ? 1.0f : 0.0f;
            r *= (1.0f - ly) * ((1.0f - lx) * m00 + lx * m01) + ly * ((1.0f - lx) * m10 + lx * m11);
        }
        s[e] = r;
    }
    __syncthreads();
    for (int e = tid; e < SH * AM_TX; e += 256) {
        const int i = e / AM_TX, j = e - i * AM_TX;
        const float* row = s + i * SW + j;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc += g[k] * row[k];
        t[e] = acc;
    }
    __syncthreads();
    float* out = map + (long)n * H * W;
    for (int e = tid; e < AM_TY * AM_TX; e += 256) {
        const int i = e / AM_TX, j = e - i * AM_TX;
        if (y0 + i >= H || x0 + j >= W) continue;
        const float* col = t + i * AM_TX + j;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc += g[k] * col[k * AM_TX];
        out[(long)(y0 + i) * W + x0 + j] = acc;
    }
}

extern "C" int vqw_anomaly_map(const float* a, const float* b, const uint8_t* cellmask, const float* taps, float* map, int N, int H,
                               int W, int C, int h, int w, int K, void* stream) {
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 1, "vqw_anomaly_map: N=%d, H=%d, W=%d, C=%d: empty tensors are refused", N, H, W, C);
    VQW_CHECK(a && b && taps && map, "vqw_anomaly_map: null pointer (only cellmask may be null)");
    VQW_CHECK(K >= 1 && (K & 1) && K / 2 <= AM_MAX_R,
              "vqw_anomaly_map: K=%d taps: an odd K of at most %d (a halo of %d pixels: sigma <= %.2f under K = 2 ceil(3 sigma) + 1) is "
              "what the %d x %d tile supports", K, 2 * AM_MAX_R + 1, AM_MAX_R, AM_MAX_R / 3.0, AM_TY, AM_TX);
    if (cellmask)
        VQW_CHECK(h >= 1 && w >= 1 && H % h == 0 && W % w == 0,
                  "vqw_anomaly_map: H=%d, W=%d must be integer multiples of the cell grid h=%d, w=%d", H, W, h, w);
    else
        h = w = 1;
    VQW_CHECK(N <= 65535, "vqw_anomaly_map: N=%d exceeds the 65535 images of one launch", N);
    VQW_CHECK(al16(a) && al16(b) && al16(map) && al16(taps), "vqw_anomaly_map: a, b, taps and map must be 16-byte aligned");
    const int R = K / 2;
    const size_t lds = ((size_t)(AM_TY + 2 * R) * (AM_TX + 2 * R) + (size_t)(AM_TY + 2 * R) * AM_TX + K) * sizeof(float);
    hipLaunchKernelGGL(k_anomaly_map, dim3(ceil_div(W, AM_TX), ceil_div(H, AM_TY), N), dim3(256), lds, (hipStream_t)stream, a, b,
                       cellmask, taps, map, H, W, C, h, w, K);
    VQW_LAUNCH_CHECK("vqw_anomaly_map");
    return VQW_OK;
}

// ------------------------------------------------------------------------------------------------ the histogram
// The key of a score: the top 16 bits below the sign of its fp32 pattern - 8 exponent and 8 mantissa bits, monotone
// non-decreasing in the score; -0 is 0; a NaN, an infinity or a negative score has no key (-1).
__device__ __forceinline__ int score_key(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0;
    return u >= 0x7F800000u ? -1 : (int)(u >> 15);
}

// Privatisation: a workgroup keeps 32-bit counters for a WINDOW of SH_WIN keys per label in LDS (24 exponents: the window ends
// one exponent above the largest key of the workgroup's first chunk), and two more for key 0 - the exact zero of an untouched
// pixel is the one value far below a map's other scores that many pixels share - and adds them to the 64-bit global counters once,
// at its end, skipping the zeros; any other key outside the window goes to the global counter at once.  Before any add a wave
// merges its most likely duplicates: the lanes whose key equals that of the first lane are counted per label by two ballots and
// added by that lane; what is left adds lane by lane.  A constant map is therefore two adds per wave-instruction, not 64 on one
// address.
#define SH_WIN 6144
#define SH_UNITS_PER_WG 2048           // units (4 scores each on the vector route) a workgroup takes at the least

__device__ __forceinline__ void sh_add(int combo, unsigned cnt, unsigned* win, int base, unsigned long long* hist) {
    const int key = combo & 0xFFFF, lab = combo >> 16, k = key - base;
    if ((unsigned)k < (unsigned)SH_WIN) atomicAdd(&win[lab * SH_WIN + k], cnt);
    else if (key == 0) atomicAdd(&win[2 * SH_WIN + lab], cnt);
    else atomicAdd(&hist[lab * 65536 + key], (unsigned long long)cnt);
}

// every lane of the wave calls it; combo = key | label << 16, or < 0: nothing to add
__device__ __forceinline__ void sh_wave_add(int combo, unsigned* win, int base, unsigned long long* hist) {
    bool todo = combo >= 0;
    const unsigned long long act = __ballot(todo);
    if (!act) return;
    const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
    const int k0 = __builtin_amdgcn_readlane(combo, lead) & 0xFFFF;
    const bool mine = todo && (combo & 0xFFFF) == k0;
    const unsigned long long same = __ballot(mine);
    if (__popcll(same) > 1) {          // the same in every lane
        const unsigned long long pos = __ballot(mine && (combo >> 16));
        if ((int)(threadIdx.x & 63) == lead) {
            const unsigned np = (unsigned)__popcll(pos), nn = (unsigned)__popcll(same) - np;
            if (nn) sh_add(k0, nn, win, base, hist);
            if (np) sh_add(k0 | 0x10000, np, win, base, hist);
        }
        todo = todo && !mine;
    }
    if (todo) sh_add(combo, 1u, win, base, hist);
}

struct ShUnit { float sc[4]; unsigned lb; int cnt; };

// VEC: a unit is 4 scores behind one 16-byte load and 4 labels behind one 4-byte load (the last unit may be short: scalar loads);
// else one score and one label
template <bool VEC>
__device__ __forceinline__ ShUnit sh_load(const float* __restrict__ scores, const uint8_t* __restrict__ labels, long u, long units, long n) {
    ShUnit r = {{0.f, 0.f, 0.f, 0.f}, 0u, 0};
    if (u >= units) return r;
    if (!VEC) {
        r.sc[0] = scores[u], r.lb = labels[u], r.cnt = 1;
        return r;
    }
    r.cnt = (int)min(4L, n - 4 * u);
    if (r.cnt == 4) {
        const float4 v = *(const float4*)(scores + 4 * u);
        r.sc[0] = v.x, r.sc[1] = v.y, r.sc[2] = v.z, r.sc[3] = v.w;
        r.lb = *(const unsigned*)(labels + 4 * u);
    } else {
        for (int q = 0; q < r.cnt; ++q) {
            r.sc[q] = scores[4 * u + q];
            r.lb |= (unsigned)labels[4 * u + q] << (8 * q);
        }
    }
    return r;
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_score_histogram(const float* __restrict__ scores, const uint8_t* __restrict__ labels,
                                                         unsigned long long* __restrict__ hist, unsigned long long* __restrict__ err,
                                                         long n, long units, int rounds) {
    __shared__ unsigned win[2 * SH_WIN + 2];
    __shared__ int s_max[4];
    constexpr int PER = VEC ? 4 : 1;
    const int tid = threadIdx.x;
    const long gid = (long)blockIdx.x * 256 + tid, gstride = (long)gridDim.x * 256;
    for (int k = tid; k < 2 * SH_WIN + 2; k += 256) win[k] = 0u;
    ShUnit cur = sh_load<VEC>(scores, labels, gid, units, n);
    // the window: from the largest key of the workgroup's first chunk
    int kmax = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q)
        if (q < cur.cnt) kmax = max(kmax, score_key(cur.sc[q]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = kmax;
    __syncthreads();
    kmax = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    const int base = max(0, min(((kmax >> 8) + 2) << 8, 65536) - SH_WIN);
    unsigned bad = 0;
    for (int it = 0; it < rounds; ++it) {           // the same trip count in every lane: the ballots need the whole wave
        ShUnit nxt = cur;
        if (it + 1 < rounds) nxt = sh_load<VEC>(scores, labels, (long)(it + 1) * gstride + gid, units, n);      // in flight during the adds
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int key = q < cur.cnt ? score_key(cur.sc[q]) : -1;
            bad += (q < cur.cnt && key < 0) ? 1u : 0u;
            sh_wave_add(key < 0 ? -1 : (key | (((cur.lb >> (8 * q)) & 0xFFu) ? 0x10000 : 0)), win, base, hist);
        }
        cur = nxt;
    }
    __syncthreads();
    for (int k = tid; k < 2 * SH_WIN + 2; k += 256) {
        const unsigned v = win[k];
        if (!v) continue;
        const int lab = k >= 2 * SH_WIN ? k - 2 * SH_WIN : (k >= SH_WIN ? 1 : 0);
        const int key = k >= 2 * SH_WIN ? 0 : base + k - lab * SH_WIN;
        atomicAdd(&hist[lab * 65536 + key], (unsigned long long)v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((tid & 63) == 0 && bad) atomicAdd(err, (unsigned long long)bad);
}

extern "C" int vqw_score_histogram(const float* scores, const uint8_t* labels, long* hist, long* err, long n, void* stream) {
    VQW_CHECK(scores && labels && hist && err, "vqw_score_histogram: null pointer");
    VQW_CHECK(n >= 1 && n <= (1L << 40), "vqw_score_histogram: n=%ld must satisfy 1 <= n <= 2^40 (an empty tensor is refused)", n);
    VQW_CHECK((((uintptr_t)scores) & 3) == 0 && (((uintptr_t)hist) & 7) == 0 && (((uintptr_t)err) & 7) == 0,
              "vqw_score_histogram: scores must be 4-byte, hist and err 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* hp = (unsigned long long*)hist;
    unsigned long long* ep = (unsigned long long*)err;
    const bool vec = al16(scores) && (((uintptr_t)labels) & 3) == 0;
    const long units = vec ? (n + 3) / 4 : n;
    long want = (units + SH_UNITS_PER_WG - 1) / SH_UNITS_PER_WG;
    const int grid = (int)(want > 2048 ? 2048 : want);
    const int rounds = (int)((units + (long)grid * 256 - 1) / ((long)grid * 256));
    if (vec) hipLaunchKernelGGL(k_score_histogram<true>, dim3(grid), dim3(256), 0, st, scores, labels, hp, ep, n, units, rounds);
    else hipLaunchKernelGGL(k_score_histogram<false>, dim3(grid), dim3(256), 0, st, scores, labels, hp, ep, n, units, rounds);
    VQW_LAUNCH_CHECK("vqw_score_histogram");
    return VQW_OK;
}

// ------------------------------------------------------------------------------------------------ the scores
// One workgroup of 1024 threads; thread t owns the 64 bins [65535 - 64 t - 63, 65535 - 64 t] and walks them downwards.  The
// counts and their running sums TP, FP are 64-bit integers (exact); every area term is formed in double from them (no integer
// product: P_b N_<b can pass 2^64) and summed in a fixed order: along the thread's bins, then a halving tree over the threads.
// Dice values are compared exactly, as fractions by 128-bit cross-multiplication, so a tie is a tie and goes to the higher bin.
#define DS_T 1024
#define DS_PER 64

struct DiceBest { unsigned long long num, den; int bin; };        // bin < 0: none yet

__device__ __forceinline__ bool dice_better(const DiceBest& x, const DiceBest& y) {      // x beats y
    if (x.bin < 0) return false;
    if (y.bin < 0) return true;
    const unsigned __int128 l = (unsigned __int128)x.num * y.den, r = (unsigned __int128)y.num * x.den;
    return l > r || (l == r && x.bin > y.bin);
}

__global__ void __launch_bounds__(DS_T) k_detection_scores(const long* __restrict__ hist, const long* __restrict__ err,
                                                           double* __restrict__ out) {
    __shared__ long sP[DS_T], sN[DS_T];
    __shared__ double sA[DS_T], sQ[DS_T];
    __shared__ DiceBest sD[DS_T];
    const int t = threadIdx.x, top = 65535 - DS_PER * t;
    const long* neg = hist;
    const long* pos = hist + 65536;
    long cp = 0, cn = 0;
    for (int q = 0; q < DS_PER; ++q) cp += pos[top - q], cn += neg[top - q];
    sP[t] = cp, sN[t] = cn;
    __syncthreads();
    for (int o = 1; o < DS_T; o <<= 1) {          // inclusive scan over the threads: bins in descending order
        const long ap = t >= o ? sP[t - o] : 0, an = t >= o ? sN[t - o] : 0;
        __syncthreads();
        sP[t] += ap, sN[t] += an;
        __syncthreads();
    }
    const long P = sP[DS_T - 1], N = sN[DS_T - 1];
    long tp = sP[t] - cp, fp = sN[t] - cn;          // the bins above this thread's
    double area = 0.0, prec = 0.0;
    DiceBest best = {0ull, 1ull, -1};
    for (int q = 0; q < DS_PER; ++q) {
        const int bin = top - q;
        const long pb = pos[bin], nb = neg[bin];
        if (pb == 0 && nb == 0) continue;
        tp += pb, fp += nb;
        area += (double)pb * ((double)(N - fp) + 0.5 * (double)nb);
        prec += (double)pb * ((double)tp / (double)(tp + fp));
        const DiceBest here = {2ull * (unsigned long long)tp, (unsigned long long)tp + (unsigned long long)fp + (unsigned long long)P, bin};
        if (here.den && (best.bin < 0 || (unsigned __int128)here.num * best.den > (unsigned __int128)best.num * here.den)) best = here;
    }
    sA[t] = area, sQ[t] = prec, sD[t] = best;
    __syncthreads();
    for (int o = DS_T / 2; o > 0; o >>= 1) {
        if (t < o) {
            sA[t] += sA[t + o], sQ[t] += sQ[t + o];
            if (dice_better(sD[t + o], sD[t])) sD[t] = sD[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool defined = P > 0 && N > 0 && sD[0].bin >= 0;
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        out[0] = defined ? sA[0] / ((double)P * (double)N) : nan;
        out[1] = defined ? sQ[0] / (double)P : nan;
        out[2] = defined ? (double)sD[0].num / (double)sD[0].den : nan;
        out[3] = defined ? (double)__uint_as_float((unsigned)sD[0].bin << 15) : nan;
        out[4] = (double)P;
        out[5] = (double)N;
        out[6] = (err == nullptr || err[0] == 0) ? 1.0 : 0.0;
        out[7] = 0.0;
    }
}

extern "C" int vqw_detection_scores(const long* hist, const long* err, double* out, void* stream) {
    VQW_CHECK(hist && out, "vqw_detection_scores: null pointer (only err may be null)");
    VQW_CHECK((((uintptr_t)hist) & 7) == 0 && (((uintptr_t)out) & 7) == 0 && (((uintptr_t)err) & 7) == 0,
              "vqw_detection_scores: hist, err and out must be 8-byte aligned");
    hipLaunchKernelGGL(k_detection_scores, dim3(1), dim3(DS_T), 0, (hipStream_t)stream, hist, err, out);
    VQW_LAUNCH_CHECK("vqw_detection_scores");
    return VQW_OK;
}
