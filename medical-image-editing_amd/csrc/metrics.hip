// Test-mode evaluation metrics of the reference's `_test_step` (trainers/single_window_trainer.py:781-827): MSE, SSIM and
// PSNR of (recon, image) as torchmetrics 0.6.2 computes them per batch (MeanSquaredError, StructuralSimilarityIndexMeasure,
// PeakSignalNoiseRatio, data_range=None), and the base-2 entropy of the VQ code usage (scipy.stats.entropy of
// bincount(ids, minlength=K+1)[1:]).
//
//   mse  = sum (p - t)^2 / numel
//   psnr = (2 ln(R_psnr) - ln(mse)) * 10 / ln(10),   R_psnr = max(max t, 0) - min(min t, 0)   (zero-seeded min/max states)
//   ssim = mean over every (n, c) plane and every VALID k x k window of
//          ((2 mu_p mu_t + C1)(2 s_pt + C2)) / ((mu_p^2 + mu_t^2 + C1)(s_p + s_t + C2)),  s = E_g[x y] - mu_x mu_y,
//          C1 = (k1 R)^2, C2 = (k2 R)^2, R = max(range p, range t) over the batch, g = normalised Gaussian (k, sigma)
//
// The package reflect-pads by (k-1)/2 and crops (k-1)/2 from every edge of the SSIM map: the two cancel, so only windows
// that lie inside the image contribute and no reflect indexing is needed.  A given data_range > 0 replaces both R.
//
// Launches (all on one stream, no host synchronisation, bit-identical from run to run: fixed-order folds, integer counts):
//   k_mt_stats   streaming pass: per-block min/max of p and t and sum (p-t)^2 in double; per-block LDS histogram of ids
//   k_mt_fold    one block: the record (ranges, SSE, C1, C2), the code counts and the entropy in double
//   k_mt_ssim    one output tile per workgroup: p, t tile + (k-1) halo in LDS, horizontal then vertical k-tap pass over
//                the five moments, per-block SSIM sums in double
//   k_mt_final   one block: fixed-order sum of the SSIM partials; mse, ssim, psnr into `out`
// The moments are formed on values shifted by one sample of the tile (E[x^2] - mu^2 is shift-invariant), which keeps the
// fp32 window sums clear of the cancellation a low-contrast plane suffers in the package's unshifted form.
#include "common.h"
#include "../../include/vqwnet_hip.h"

#define MT_BLOCK 256
#define MT_GRID_MAX 1024       // stats blocks (partials are sized for this many)
#define MT_MAX_BINS 4096       // K + 2 (bins 0..K and one for out-of-range ids)
#define MT_MAX_K 15            // largest SSIM window side
#define MT_TW 64               // SSIM output tile: MT_TW columns x MT_TH rows
#define MT_TH 32
#define MT_FOLD 1024           // threads of the fold kernel

// out[] layout (double), shared with hipops.ops
enum { MT_MSE = 0, MT_SSIM, MT_PSNR, MT_RANGE_SSIM, MT_RANGE_PSNR, MT_SSE, MT_TMIN, MT_TMAX, MT_ENTROPY, MT_BAD, MT_NIDS,
       MT_OUT };
// record in the workspace: R_ssim, R_psnr, SSE, C1, C2
enum { MT_R_SSIM = 0, MT_R_PSNR, MT_R_SSE, MT_R_C1, MT_R_C2, MT_REC };

struct MtArgs {
    const float* pred;
    const float* target;
    const int64_t* ids;
    double* out;
    int64_t* counts;          // [K + 1] (optional)
    double* rec;              // [MT_REC]
    double* img_part;         // [MT_GRID_MAX][5]
    int* hist_part;           // [MT_GRID_MAX][K + 2]
    double* ssim_part;        // [planes * tiles]
    long n;                   // numel of pred / target
    long n_ids;
    int K, grid;
    int N, C, H, W, ks, tiles_x, tiles_y;
    float data_range, k1, k2;
    float g[MT_MAX_K];
};

static long mt_ssim_tiles(int H, int W, int ks) {
    return (long)ceil_div(W - ks + 1, MT_TW) * ceil_div(H - ks + 1, MT_TH);
}

static size_t mt_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: rec | img_part | hist_part | ssim_part
static size_t mt_ws(int N, int C, int H, int W, int K, int ks, size_t* o_img, size_t* o_hist, size_t* o_ssim) {
    size_t off = mt_align(MT_REC * sizeof(double));
    *o_img = off;
    off += mt_align((size_t)MT_GRID_MAX * 5 * sizeof(double));
    *o_hist = off;
    if (K > 0) off += mt_align((size_t)MT_GRID_MAX * (K + 2) * sizeof(int));
    *o_ssim = off;
    if (N > 0 && ks > 0 && H >= ks && W >= ks) off += mt_align((size_t)N * C * mt_ssim_tiles(H, W, ks) * sizeof(double));
    return off;
}

extern "C" size_t vqw_recon_metrics_ws_bytes(int N, int C, int H, int W, int K) {
    if (N < 0 || C < 0 || H < 0 || W < 0 || K < 0) return 0;
    size_t a, b, c;
    return mt_ws(N, C, H, W, K, 1, &a, &b, &c);     // ks = 1: the most SSIM tiles any window size needs
}

// ---------------------------------------------------------------------------------------------------------------------
// block reductions (fixed order: butterfly inside a wave, then the waves in index order)
template <int NT>
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < NT / 64; ++i) s += sh[i];
    return s;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(MT_BLOCK) void k_mt_stats(MtArgs a) {
    __shared__ int hist[MT_MAX_BINS];
    __shared__ float smm[4][MT_BLOCK / 64];
    __shared__ double ssq[MT_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long stride = (long)a.grid * MT_BLOCK, gid = (long)blockIdx.x * MT_BLOCK + tid;
    if (a.pred) {
        float pmn = INFINITY, pmx = -INFINITY, tmn = INFINITY, tmx = -INFINITY;
        double sse = 0.0;
        long tail = 0;
        if (VEC) {
            const long n4 = a.n >> 2;
            const float4* p4 = (const float4*)a.pred;
            const float4* t4 = (const float4*)a.target;
            for (long i = gid; i < n4; i += stride) {
                const float4 p = p4[i], t = t4[i];
                pmn = fminf(pmn, fminf(fminf(p.x, p.y), fminf(p.z, p.w)));
                pmx = fmaxf(pmx, fmaxf(fmaxf(p.x, p.y), fmaxf(p.z, p.w)));
                tmn = fminf(tmn, fminf(fminf(t.x, t.y), fminf(t.z, t.w)));
                tmx = fmaxf(tmx, fmaxf(fmaxf(t.x, t.y), fmaxf(t.z, t.w)));
                const double d0 = (double)p.x - t.x, d1 = (double)p.y - t.y, d2 = (double)p.z - t.z, d3 = (double)p.w - t.w;
                sse += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
            }
            tail = n4 << 2;
        }
        for (long i = tail + gid; i < a.n; i += stride) {
            const float p = a.pred[i], t = a.target[i];
            pmn = fminf(pmn, p); pmx = fmaxf(pmx, p);
            tmn = fminf(tmn, t); tmx = fmaxf(tmx, t);
            const double d = (double)p - t;
            sse += d * d;
        }
        pmn = wave_min(pmn); pmx = wave_max_f(pmx); tmn = wave_min(tmn); tmx = wave_max_f(tmx);
        sse = wave_sum_d(sse);
        if (lane == 0) { smm[0][w] = pmn; smm[1][w] = pmx; smm[2][w] = tmn; smm[3][w] = tmx; ssq[w] = sse; }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < MT_BLOCK / 64; ++i) {
                pmn = fminf(pmn, smm[0][i]); pmx = fmaxf(pmx, smm[1][i]);
                tmn = fminf(tmn, smm[2][i]); tmx = fmaxf(tmx, smm[3][i]);
                s += ssq[i];
            }
            double* o = a.img_part + (long)blockIdx.x * 5;
            o[0] = pmn; o[1] = pmx; o[2] = tmn; o[3] = tmx; o[4] = s;
        }
    }
    if (a.ids) {
        const int nb = a.K + 2;                    // bins 0..K, then out of range
        for (int b = tid; b < nb; b += MT_BLOCK) hist[b] = 0;
        __syncthreads();
        for (long i = gid; i < a.n_ids; i += stride) {
            const int64_t v = a.ids[i];
            atomicAdd(&hist[(v >= 0 && v <= a.K) ? (int)v : a.K + 1], 1);
        }
        __syncthreads();
        int* o = a.hist_part + (long)blockIdx.x * nb;
        for (int b = tid; b < nb; b += MT_BLOCK) o[b] = hist[b];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_FOLD) void k_mt_fold(MtArgs a) {
    __shared__ float smm[4][MT_FOLD / 64];
    __shared__ double sh[MT_FOLD / 64];
    __shared__ long shl[MT_FOLD / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (a.pred) {
        float pmn = INFINITY, pmx = -INFINITY, tmn = INFINITY, tmx = -INFINITY;
        double sse = 0.0;
        for (int i = tid; i < a.grid; i += MT_FOLD) {
            const double* o = a.img_part + (long)i * 5;
            pmn = fminf(pmn, (float)o[0]); pmx = fmaxf(pmx, (float)o[1]);
            tmn = fminf(tmn, (float)o[2]); tmx = fmaxf(tmx, (float)o[3]);
            sse += o[4];
        }
        pmn = wave_min(pmn); pmx = wave_max_f(pmx); tmn = wave_min(tmn); tmx = wave_max_f(tmx);
        if (lane == 0) { smm[0][w] = pmn; smm[1][w] = pmx; smm[2][w] = tmn; smm[3][w] = tmx; }
        sse = block_sum_d<MT_FOLD>(sse, sh);        // its barriers also publish smm
        if (tid == 0) {
            for (int i = 0; i < MT_FOLD / 64; ++i) {
                pmn = fminf(pmn, smm[0][i]); pmx = fmaxf(pmx, smm[1][i]);
                tmn = fminf(tmn, smm[2][i]); tmx = fmaxf(tmx, smm[3][i]);
            }
            double rs = fmax((double)pmx - (double)pmn, (double)tmx - (double)tmn);
            double rp = fmax((double)tmx, 0.0) - fmin((double)tmn, 0.0);
            if (a.data_range > 0.f) rs = rp = (double)a.data_range;
            a.rec[MT_R_SSIM] = rs;
            a.rec[MT_R_PSNR] = rp;
            a.rec[MT_R_SSE] = sse;
            a.rec[MT_R_C1] = ((double)a.k1 * rs) * ((double)a.k1 * rs);
            a.rec[MT_R_C2] = ((double)a.k2 * rs) * ((double)a.k2 * rs);
            a.out[MT_RANGE_SSIM] = rs;
            a.out[MT_RANGE_PSNR] = rp;
            a.out[MT_SSE] = sse;
            a.out[MT_TMIN] = tmn;
            a.out[MT_TMAX] = tmx;
            const double mse = sse / (double)a.n;
            a.out[MT_MSE] = mse;
            a.out[MT_PSNR] = (2.0 * log(rp) - log(mse)) * (10.0 / log(10.0));
            a.out[MT_SSIM] = NAN;                    // k_mt_final fills it when the SSIM pass runs
        }
    } else if (tid == 0) {
        for (int i = MT_MSE; i <= MT_TMAX; ++i) a.out[i] = NAN;
    }
    if (a.ids) {
        // integer counts per bin in block order (exact), then H = ln S - sum c ln c / S in double, over bins 1..K
        const int nb = a.K + 2;
        long s = 0;
        double clc = 0.0;
        for (int b = tid; b < nb; b += MT_FOLD) {
            long c = 0;
            for (int i = 0; i < a.grid; ++i) c += a.hist_part[(long)i * nb + b];
            if (b <= a.K && a.counts) a.counts[b] = c;
            if (b >= 1 && b <= a.K) {
                s += c;
                if (c > 0) clc += (double)c * log((double)c);
            } else if (b == a.K + 1) {
                a.out[MT_BAD] = (double)c;
            }
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        __syncthreads();
        if (lane == 0) shl[w] = s;
        clc = block_sum_d<MT_FOLD>(clc, sh);
        if (tid == 0) {
            long S = 0;
            for (int i = 0; i < MT_FOLD / 64; ++i) S += shl[i];
            const double dS = (double)S;
            a.out[MT_ENTROPY] = S > 0 ? (log(dS) - clc / dS) / log(2.0) : NAN;
            a.out[MT_NIDS] = (double)a.n_ids;
        }
    } else if (tid == 0) {
        a.out[MT_ENTROPY] = NAN;
        a.out[MT_BAD] = 0.0;
        a.out[MT_NIDS] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// SSIM: grid (tiles, N * C).  LDS: the shifted p / t region (MT_TH + KS - 1) x (MT_TW + KS - 1), then the five
// horizontal moment rows (MT_TH + KS - 1) x MT_TW each.  Outputs beyond the valid (H - KS + 1) x (W - KS + 1) range are
// skipped; the region loads zeros past the image edge, which only such outputs read.
template <int KS>
__global__ __launch_bounds__(MT_BLOCK) void k_mt_ssim(MtArgs a) {
    constexpr int RH = MT_TH + KS - 1, RW = MT_TW + KS - 1, RWP = RW | 1;
    __shared__ float sp[RH][RWP], st[RH][RWP];
    __shared__ float sm[5][RH][MT_TW];
    __shared__ double sh[MT_BLOCK / 64];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x0 = tx * MT_TW, y0 = ty * MT_TH;
    const long plane = (long)blockIdx.y * a.H * a.W;
    const float* P = a.pred + plane;
    const float* T = a.target + plane;
    const int oh = a.H - KS + 1, ow = a.W - KS + 1;
    // shift: one sample inside the region (same for every window of the tile)
    const int cy = min(y0 + RH / 2, a.H - 1), cx = min(x0 + RW / 2, a.W - 1);
    const float shp = P[(long)cy * a.W + cx], sht = T[(long)cy * a.W + cx];
    for (int i = tid; i < RH * RW; i += MT_BLOCK) {
        const int r = i / RW, c = i - r * RW, y = y0 + r, x = x0 + c;
        float p = 0.f, t = 0.f;
        if (y < a.H && x < a.W) {
            p = P[(long)y * a.W + x] - shp;
            t = T[(long)y * a.W + x] - sht;
        }
        sp[r][c] = p;
        st[r][c] = t;
    }
    __syncthreads();
    for (int i = tid; i < RH * MT_TW; i += MT_BLOCK) {
        const int r = i / MT_TW, c = i - r * MT_TW;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float g = a.g[k], p = sp[r][c + k], t = st[r][c + k];
            const float gp = g * p, gt = g * t;
            m0 += gp; m1 += gt;
            m2 += gp * p; m3 += gt * t; m4 += gp * t;
        }
        sm[0][r][c] = m0; sm[1][r][c] = m1; sm[2][r][c] = m2; sm[3][r][c] = m3; sm[4][r][c] = m4;
    }
    __syncthreads();
    const double c1 = a.rec[MT_R_C1], c2 = a.rec[MT_R_C2];
    double acc = 0.0;
    for (int i = tid; i < MT_TH * MT_TW; i += MT_BLOCK) {
        const int r = i / MT_TW, c = i - r * MT_TW;
        if (y0 + r >= oh || x0 + c >= ow) continue;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float g = a.g[k];
            m0 += g * sm[0][r + k][c]; m1 += g * sm[1][r + k][c];
            m2 += g * sm[2][r + k][c]; m3 += g * sm[3][r + k][c]; m4 += g * sm[4][r + k][c];
        }
        // centred moments in double from the shifted sums (the products of two floats are exact in double)
        const double mp = m0, mt = m1;
        const double vp = (double)m2 - mp * mp, vt = (double)m3 - mt * mt, cpt = (double)m4 - mp * mt;
        const double up = mp + (double)shp, ut = mt + (double)sht;
        acc += ((2.0 * up * ut + c1) * (2.0 * cpt + c2)) / ((up * up + ut * ut + c1) * (vp + vt + c2));
    }
    acc = block_sum_d<MT_BLOCK>(acc, sh);
    if (tid == 0) a.ssim_part[(long)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

__global__ __launch_bounds__(MT_FOLD) void k_mt_final(MtArgs a, long nparts, double count) {
    __shared__ double sh[MT_FOLD / 64];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += MT_FOLD) s += a.ssim_part[i];
    s = block_sum_d<MT_FOLD>(s, sh);
    if (threadIdx.x == 0) a.out[MT_SSIM] = s / count;
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int vqw_recon_metrics(const float* pred, const float* target, const int64_t* ids, double* out, int64_t* counts,
                                 void* ws, size_t ws_bytes, int N, int C, int H, int W, long n_ids, int K, int ksize,
                                 float sigma, float k1, float k2, float data_range, void* stream) {
    const bool img = pred || target;
    VQW_CHECK(out && ws, "vqw_recon_metrics: bad arguments");
    VQW_CHECK(img || ids, "vqw_recon_metrics: nothing to compute (no images and no ids)");
    if (img) {
        VQW_CHECK(pred && target, "vqw_recon_metrics: pred and target go together");
        VQW_CHECK(N > 0 && C > 0 && H > 0 && W > 0, "vqw_recon_metrics: bad shape");
        VQW_CHECK((long)N * C * H * W < (1L << 40), "vqw_recon_metrics: tensor too large");
        VQW_CHECK(ksize == 0 || (ksize > 0 && ksize % 2 == 1 && ksize <= MT_MAX_K),
                  "vqw_recon_metrics: kernel_size must be odd and at most %d (got %d)", MT_MAX_K, ksize);
        VQW_CHECK(ksize == 0 || (H >= ksize && W >= ksize),
                  "vqw_recon_metrics: H=%d and W=%d must be at least kernel_size=%d", H, W, ksize);
        VQW_CHECK(ksize == 0 || sigma > 0.f, "vqw_recon_metrics: sigma must be > 0");
        VQW_CHECK(ksize == 0 || (long)N * C <= 65535, "vqw_recon_metrics: more than 65535 planes");
        VQW_CHECK(!(data_range != data_range), "vqw_recon_metrics: data_range is nan");
    }
    if (ids) {
        VQW_CHECK(n_ids > 0, "vqw_recon_metrics: no ids");
        VQW_CHECK(K >= 1 && K + 2 <= MT_MAX_BINS, "vqw_recon_metrics: K=%d out of [1, %d]", K, MT_MAX_BINS - 2);
    }
    size_t o_img, o_hist, o_ssim;
    const size_t need = mt_ws(img ? N : 0, C, H, W, ids ? K : 0, img ? ksize : 0, &o_img, &o_hist, &o_ssim);
    VQW_CHECK(ws_bytes >= need, "vqw_recon_metrics: workspace too small (%zu < %zu)", ws_bytes, need);

    MtArgs a;
    a.pred = img ? pred : nullptr;
    a.target = img ? target : nullptr;
    a.ids = ids;
    a.out = out;
    a.counts = counts;
    a.rec = (double*)ws;
    a.img_part = (double*)((char*)ws + o_img);
    a.hist_part = (int*)((char*)ws + o_hist);
    a.ssim_part = (double*)((char*)ws + o_ssim);
    a.n = img ? (long)N * C * H * W : 0;
    a.n_ids = ids ? n_ids : 0;
    a.K = K;
    a.N = N; a.C = C; a.H = H; a.W = W; a.ks = img ? ksize : 0;
    a.data_range = data_range; a.k1 = k1; a.k2 = k2;
    a.tiles_x = a.ks ? ceil_div(W - a.ks + 1, MT_TW) : 0;
    a.tiles_y = a.ks ? ceil_div(H - a.ks + 1, MT_TH) : 0;
    for (int k = 0; k < MT_MAX_K; ++k) a.g[k] = 0.f;
    if (a.ks) {                 // the package's _gaussian: exp(-(d / sigma)^2 / 2) over d = (1-k)/2 .. (k-1)/2, normalised
        double g[MT_MAX_K], s = 0.0;
        for (int k = 0; k < a.ks; ++k) {
            const double d = (double)(k - (a.ks - 1) / 2) / (double)sigma;
            g[k] = exp(-0.5 * d * d);
            s += g[k];
        }
        for (int k = 0; k < a.ks; ++k) a.g[k] = (float)(g[k] / s);
    }
    // stats grid: about four float4 (or id) loads per thread, at most MT_GRID_MAX blocks (grid-stride beyond)
    const long items = a.n / 4 > a.n_ids ? a.n / 4 : a.n_ids;
    const long blocks = (items + MT_BLOCK * 4 - 1) / (MT_BLOCK * 4);
    a.grid = (int)(blocks < 1 ? 1 : blocks > MT_GRID_MAX ? MT_GRID_MAX : blocks);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = img && ((((uintptr_t)pred) | ((uintptr_t)target)) & 15) == 0;
    if (vec)
        k_mt_stats<true><<<a.grid, MT_BLOCK, 0, st>>>(a);
    else
        k_mt_stats<false><<<a.grid, MT_BLOCK, 0, st>>>(a);
    k_mt_fold<<<1, MT_FOLD, 0, st>>>(a);
    if (a.ks) {
        const dim3 grid(a.tiles_x * a.tiles_y, N * C);
        switch (a.ks) {
            case 1: k_mt_ssim<1><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 3: k_mt_ssim<3><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 5: k_mt_ssim<5><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 7: k_mt_ssim<7><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 9: k_mt_ssim<9><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 11: k_mt_ssim<11><<<grid, MT_BLOCK, 0, st>>>(a); break;
            case 13: k_mt_ssim<13><<<grid, MT_BLOCK, 0, st>>>(a); break;
            default: k_mt_ssim<15><<<grid, MT_BLOCK, 0, st>>>(a); break;
        }
        const double count = (double)N * C * (double)(H - a.ks + 1) * (double)(W - a.ks + 1);
        k_mt_final<<<1, MT_FOLD, 0, st>>>(a, (long)grid.x * grid.y, count);
    }
    VQW_LAUNCH_CHECK("vqw_recon_metrics");
    return VQW_OK;
}

extern "C" int vqw_code_entropy(const int64_t* ids, double* out, int64_t* counts, void* ws, size_t ws_bytes, long n, int K,
                                void* stream) {
    VQW_CHECK(ids && out && ws, "vqw_code_entropy: bad arguments");
    return vqw_recon_metrics(nullptr, nullptr, ids, out, counts, ws, ws_bytes, 0, 0, 0, 0, n, K, 0, 0.f, 0.f, 0.f, 0.f,
                             stream);
}
