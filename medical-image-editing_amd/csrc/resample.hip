// Preprocessing kernels: a NIfTI volume as stored -> volume statistics, and -> the oriented, normalised, resampled slices
// the datasets read (the reference's src/preprocess scripts: numpy min / max / masked mean / std over a float64 copy of the
// volume, then one PIL Image.resize per slice).
//
// Bit-exactness is the contract, as in export.hip: every operation below is one IEEE double or float multiply, add,
// subtract or divide in a fixed order, so tests/test_gpu_preprocess.py compares with PIL's output byte for byte.  THIS FILE
// IS COMPILED WITH -ffp-contract=off (target-specific flag in the Makefile): PIL's resampler rounds `pixel * k` and
// `ss + product` separately, and nibabel rounds `v * slope` before adding the intercept.
//
// PIL's F-mode bilinear resize is two passes: horizontal (along the columns of the oriented slice) rounded to float32, then
// vertical; each output is sum_k float(pixel) * double(coefficient) accumulated in double in index order.  The normalised
// coefficient tables come from the host (built once per (in, out) size in double).
//   k_rows: a workgroup takes R oriented rows of one slice, reads them from the stored volume along its fastest axis x,
//           normalises each voxel and keeps the float32 values in LDS.  Under orientations 1 and 2 a row of the oriented
//           slice is a stored row read backwards; under orientation 0 the oriented rows run along y, so the workgroup
//           reads R consecutive x per y and the transposition happens in LDS.  Then each thread forms one output of the
//           horizontal pass from LDS and stores it along the output row.
//   k_cols: one thread per output pixel, threads along the output row, taps down the column of the horizontal pass.
// A pass that keeps its size is skipped as PIL skips it (k_rows then only normalises and orients).
//
// The work per volume is a few HBM passes; these kernels are here so that the dataset a user builds is the reference's
// dataset bit for bit without its host dependencies, not for speed: gzip and np.save dominate a command's time.
#include "common.h"
#include "../../include/vqwnet_hip.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kStatBlocks = 1024;        // partials of a statistics pass (fixed: the fold order depends on nothing else)
constexpr int kLdsFloats = 16384;        // 64 KiB of rows per workgroup in k_rows
constexpr int kMaxRows = 32;

enum { NORM_NONE = 0, NORM_MINMAX = 1, NORM_ZSCORE = 2 };
enum { ORIENT_NONE = 0, ORIENT_CRC = 1, ORIENT_BRATS = 2 };

struct Scale {
    double slope, inter;
    int scaled;
};

template <typename T>
__device__ __forceinline__ double voxel(const T* p, size_t i, const Scale& s) {
    const double v = (double)p[i];
    return s.scaled ? v * s.slope + s.inter : v;
}

// ---- statistics ------------------------------------------------------------------------------------------------------

// numpy's min / max: a NaN wins
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// tree over the workgroup's 256 values in LDS: the same order every run
template <int OP>
__device__ __forceinline__ double block_fold(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double a = sh[t], b = sh[t + s];
            sh[t] = OP == 0 ? a + b : OP == 1 ? nan_min(a, b) : nan_max(a, b);
        }
        __syncthreads();
    }
    return sh[0];
}

// part [4][kStatBlocks]: min, max, count, sum of the float32 values > 0
template <typename T>
__global__ void __launch_bounds__(kBlock) k_stats_sum(const T* __restrict__ vol, long n, Scale sc, double* __restrict__ part) {
    __shared__ double sh[kBlock];
    double mn = INFINITY, mx = -INFINITY, cnt = 0.0, sum = 0.0;
    const long step = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const double v = voxel(vol, (size_t)i, sc);
        mn = nan_min(mn, v);
        mx = nan_max(mx, v);
        const float f = (float)v;
        if (f > 0.f) {
            cnt += 1.0;
            sum += (double)f;
        }
    }
    mn = block_fold<1>(mn, sh);
    mx = block_fold<2>(mx, sh);
    cnt = block_fold<0>(cnt, sh);
    sum = block_fold<0>(sum, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mn;
        part[kStatBlocks + blockIdx.x] = mx;
        part[2 * kStatBlocks + blockIdx.x] = cnt;
        part[3 * kStatBlocks + blockIdx.x] = sum;
    }
}

// part [kStatBlocks]: sum of (float32 value - mean)^2 over the values > 0
template <typename T>
__global__ void __launch_bounds__(kBlock) k_stats_dev(const T* __restrict__ vol, long n, Scale sc, const double* __restrict__ stats,
                                                      double* __restrict__ part) {
    __shared__ double sh[kBlock];
    const double mean = stats[3];
    double sq = 0.0;
    const long step = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const float f = (float)voxel(vol, (size_t)i, sc);
        if (f > 0.f) {
            const double d = (double)f - mean;
            sq += d * d;
        }
    }
    sq = block_fold<0>(sq, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// one workgroup: thread t folds partials t, t + 256, ... in that order, then the tree
template <int OP>
__device__ __forceinline__ double fold_parts(const double* part, int G, double init, double* sh) {
    double v = init;
    for (int b = threadIdx.x; b < G; b += kBlock) {
        const double p = part[b];
        v = OP == 0 ? v + p : OP == 1 ? nan_min(v, p) : nan_max(v, p);
    }
    return block_fold<OP>(v, sh);
}

__global__ void __launch_bounds__(kBlock) k_stats_fold(const double* __restrict__ part, int G, double* __restrict__ stats, int phase) {
    __shared__ double sh[kBlock];
    if (phase == 0) {
        const double mn = fold_parts<1>(part, G, INFINITY, sh);
        const double mx = fold_parts<2>(part + kStatBlocks, G, -INFINITY, sh);
        const double cnt = fold_parts<0>(part + 2 * kStatBlocks, G, 0.0, sh);
        const double sum = fold_parts<0>(part + 3 * kStatBlocks, G, 0.0, sh);
        if (threadIdx.x == 0) {
            stats[0] = mn;
            stats[1] = mx;
            stats[2] = cnt;
            stats[3] = sum / cnt;
        }
    } else {
        const double sq = fold_parts<0>(part, G, 0.0, sh);
        if (threadIdx.x == 0) stats[4] = sqrt(sq / stats[2]);
    }
}

template <typename T>
int stats_launch(const void* vol, double* stats, double* ws, long n, Scale sc, hipStream_t s) {
    const int G = (int)((n + kBlock - 1) / kBlock < kStatBlocks ? (n + kBlock - 1) / kBlock : kStatBlocks);
    double* part2 = ws + 4 * kStatBlocks;
    k_stats_sum<T><<<G, kBlock, 0, s>>>((const T*)vol, n, sc, ws);
    k_stats_fold<<<1, kBlock, 0, s>>>(ws, G, stats, 0);
    k_stats_dev<T><<<G, kBlock, 0, s>>>((const T*)vol, n, sc, stats, part2);
    k_stats_fold<<<1, kBlock, 0, s>>>(part2, G, stats, 1);
    return VQW_OK;
}

// ---- normalise + orient + bilinear resample --------------------------------------------------------------------------

// oriented pixel (i, j) of a slice is the stored voxel off0 + i * si + j * sj of that slice; the oriented slice is h x w
struct Geo {
    long off0, si, sj;
    int h, w;
};

Geo geometry(int orient, int X, int Y) {
    Geo g;
    if (orient == ORIENT_CRC) {                    // np.rot90(s[::-1])[i, j] = s[X - 1 - j, Y - 1 - i]
        g.off0 = (long)(X - 1) + (long)X * (Y - 1);
        g.si = -X;
        g.sj = -1;
        g.h = Y;
        g.w = X;
    } else if (orient == ORIENT_BRATS) {           // np.rot90(s, k=3)[i, j] = s[X - 1 - j, i]
        g.off0 = X - 1;
        g.si = X;
        g.sj = -1;
        g.h = Y;
        g.w = X;
    } else {                                       // s[i, j]
        g.off0 = 0;
        g.si = 1;
        g.sj = X;
        g.h = X;
        g.w = Y;
    }
    return g;
}

template <typename T, int NORM>
__global__ void __launch_bounds__(kBlock) k_rows(const T* __restrict__ vol, const double* __restrict__ stats,
                                                 const double* __restrict__ kh, const int* __restrict__ bh,
                                                 float* __restrict__ dst, Geo g, int S, int ks, int R, Scale sc, long slice) {
    extern __shared__ float rows[];
    const int z = blockIdx.y;
    const int i0 = blockIdx.x * R;
    const int rn = min(R, g.h - i0);
    const int pitch = g.w + 1;
    const T* src = vol + (size_t)z * slice;
    double mn = 0.0, den = 1.0;
    float mean32 = 0.f, std32 = 1.f;
    if (NORM == NORM_MINMAX) {
        mn = stats[0];
        den = stats[1] - stats[0];
    } else if (NORM == NORM_ZSCORE) {
        mean32 = (float)stats[3];
        std32 = (float)stats[4];
    }
    const bool along_j = g.sj == 1 || g.sj == -1;  // which of (i, j) runs along the stored-fastest axis
    const int total = rn * g.w;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        int r, j;
        if (along_j) {
            r = idx / g.w;
            j = idx - r * g.w;
        } else {
            j = idx / rn;
            r = idx - j * rn;
        }
        const double v = voxel(src, (size_t)(g.off0 + (long)(i0 + r) * g.si + (long)j * g.sj), sc);
        float f;
        if (NORM == NORM_MINMAX) f = (float)(((v - mn) / den) * 255.0);
        else if (NORM == NORM_ZSCORE) f = __fdiv_rn(__fsub_rn((float)v, mean32), std32);
        else f = (float)v;
        rows[r * pitch + j] = f;
    }
    __syncthreads();
    const int outs = rn * S;
    for (int idx = threadIdx.x; idx < outs; idx += kBlock) {
        const int r = idx / S;
        const int xx = idx - r * S;
        const float* row = rows + r * pitch;
        float o;
        if (ks == 0) {
            o = row[xx];
        } else {
            const int x0 = bh[2 * xx], cnt = bh[2 * xx + 1];
            if (x0 < 0 || cnt < 0 || cnt > ks || x0 + cnt > g.w) {
                o = NAN;                           // a malformed table reads nothing
            } else {
                const double* k = kh + (size_t)xx * ks;
                double ss = 0.0;
                for (int x = 0; x < cnt; ++x) ss += (double)row[x0 + x] * k[x];
                o = (float)ss;
            }
        }
        dst[((size_t)z * g.h + (i0 + r)) * S + xx] = o;
    }
}

// tmp [Z][h][S] -> out [Z][S][S].  grid = (ceil(S / kBlock), S, Z)
__global__ void __launch_bounds__(kBlock) k_cols(const float* __restrict__ tmp, const double* __restrict__ kv,
                                                 const int* __restrict__ bv, float* __restrict__ out, int h, int S, int ks) {
    const int xx = blockIdx.x * kBlock + threadIdx.x;
    const int yy = blockIdx.y;
    const int z = blockIdx.z;
    if (xx >= S) return;
    const int y0 = bv[2 * yy], cnt = bv[2 * yy + 1];
    float o;
    if (y0 < 0 || cnt < 0 || cnt > ks || y0 + cnt > h) {
        o = NAN;
    } else {
        const double* k = kv + (size_t)yy * ks;
        const float* col = tmp + ((size_t)z * h + y0) * S + xx;
        double ss = 0.0;
        for (int y = 0; y < cnt; ++y) ss += (double)col[(size_t)y * S] * k[y];
        o = (float)ss;
    }
    out[((size_t)z * S + yy) * S + xx] = o;
}

template <typename T>
int slices_launch(const void* vol, const double* stats, const double* kh, const int* bh, const double* kv, const int* bv,
                  float* tmp, float* out, Geo g, int Z, int S, int ksh, int ksv, int norm, Scale sc, long slice, hipStream_t s) {
    const int R = imin(kMaxRows, kLdsFloats / (g.w + 1));
    dim3 grid(ceil_div(g.h, R), Z);
    const size_t shm = sizeof(float) * (size_t)R * (g.w + 1);
    float* dst = ksv ? tmp : out;
    const T* v = (const T*)vol;
    if (norm == NORM_MINMAX) k_rows<T, NORM_MINMAX><<<grid, kBlock, shm, s>>>(v, stats, kh, bh, dst, g, S, ksh, R, sc, slice);
    else if (norm == NORM_ZSCORE) k_rows<T, NORM_ZSCORE><<<grid, kBlock, shm, s>>>(v, stats, kh, bh, dst, g, S, ksh, R, sc, slice);
    else k_rows<T, NORM_NONE><<<grid, kBlock, shm, s>>>(v, stats, kh, bh, dst, g, S, ksh, R, sc, slice);
    if (ksv) k_cols<<<dim3(ceil_div(S, kBlock), S, Z), kBlock, 0, s>>>(tmp, kv, bv, out, g.h, S, ksv);
    return VQW_OK;
}

// ---- nearest resampling of label slices ------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock) k_label_scan(const int32_t* __restrict__ vol, long n, int32_t* __restrict__ err) {
    bool seen = false;
    const long step = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) seen |= vol[i] == 3;
    if (seen) *err = 1;
}

// out [Z][S][S].  Threads of a workgroup cover a 32 x 32 output tile, 32 x 8 at a time.  SWAP (orientation 0: the oriented
// columns run along stored y): the tile is read with lanes along the output ROWS, which run along stored x, and turned in LDS.
template <bool SWAP>
__global__ void __launch_bounds__(kBlock) k_labels(const int32_t* __restrict__ vol, const int* __restrict__ xtab,
                                                   const int* __restrict__ ytab, int32_t* __restrict__ out, Geo g, int S,
                                                   int relabel, long slice) {
    __shared__ int32_t tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int z = blockIdx.z;
    const int32_t* src = vol + (size_t)z * slice;
    int32_t* dst = out + (size_t)z * S * S;
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    if (SWAP) {
        const int yy = by + tx;
        for (int c = ty; c < 32; c += 8) {
            const int xx = bx + c;
            int32_t v = 0;
            if (yy < S && xx < S) {
                const int i = ytab[yy], j = xtab[xx];
                if (i >= 0 && i < g.h && j >= 0 && j < g.w) v = src[g.off0 + (long)i * g.si + (long)j * g.sj];
            }
            tile[c][tx] = v;                       // [column of the tile][row of the tile]
        }
        __syncthreads();
    }
    const int xx = bx + tx;
    for (int r = ty; r < 32; r += 8) {
        const int yy = by + r;
        if (yy >= S || xx >= S) continue;
        int32_t v = 0;
        if (SWAP) {
            v = tile[tx][r];
        } else {
            const int i = ytab[yy], j = xtab[xx];
            if (i >= 0 && i < g.h && j >= 0 && j < g.w) v = src[g.off0 + (long)i * g.si + (long)j * g.sj];
        }
        if (relabel && v == 4) v = 3;
        dst[(size_t)yy * S + xx] = v;
    }
}

int volume_checks(const char* name, int X, int Y, int Z, int S) {
    VQW_CHECK(X > 0 && Y > 0 && Z > 0 && S > 0, "%s: X, Y, Z, S must be positive (got %d, %d, %d, %d)", name, X, Y, Z, S);
    VQW_CHECK(Z <= 65535 && S <= 65535, "%s: at most 65535 slices and an output size of at most 65535 (got %d, %d)", name, Z, S);
    return VQW_OK;
}

}  // namespace

extern "C" long vqw_volume_stats_ws_bytes(void) { return (long)sizeof(double) * 5 * kStatBlocks; }

#define VQW_BY_DTYPE(fn, ...)                                        \
    switch (dtype) {                                                 \
        case 0: return fn<uint8_t>(__VA_ARGS__);                     \
        case 1: return fn<int16_t>(__VA_ARGS__);                     \
        case 2: return fn<uint16_t>(__VA_ARGS__);                    \
        case 3: return fn<int32_t>(__VA_ARGS__);                     \
        case 4: return fn<float>(__VA_ARGS__);                       \
        default: return fn<double>(__VA_ARGS__);                     \
    }

static int stats_by_dtype(int dtype, const void* vol, double* stats, double* ws, long n, Scale sc, hipStream_t s) {
    VQW_BY_DTYPE(stats_launch, vol, stats, ws, n, sc, s)
}

static int slices_by_dtype(int dtype, const void* vol, const double* stats, const double* kh, const int* bh, const double* kv,
                           const int* bv, float* tmp, float* out, Geo g, int Z, int S, int ksh, int ksv, int norm, Scale sc,
                           long slice, hipStream_t s) {
    VQW_BY_DTYPE(slices_launch, vol, stats, kh, bh, kv, bv, tmp, out, g, Z, S, ksh, ksv, norm, sc, slice, s)
}

extern "C" int vqw_volume_stats(const void* vol, double* stats, double* ws, int dtype, long n, double slope, double inter,
                                int scaled, void* stream) {
    VQW_CHECK(vol && stats && ws, "vqw_volume_stats: null pointer");
    VQW_CHECK(dtype >= 0 && dtype <= 5, "vqw_volume_stats: dtype must be 0..5 (got %d)", dtype);
    VQW_CHECK(n > 0, "vqw_volume_stats: empty volume");
    Scale sc = {slope, inter, scaled};
    stats_by_dtype(dtype, vol, stats, ws, n, sc, (hipStream_t)stream);
    VQW_LAUNCH_CHECK("vqw_volume_stats");
    return VQW_OK;
}

extern "C" int vqw_volume_to_slices(const void* vol, const double* stats, const double* kh, const int* bh, const double* kv,
                                    const int* bv, float* tmp, float* out, int dtype, int X, int Y, int Z, int S, int ksh,
                                    int ksv, int norm, int orient, double slope, double inter, int scaled, void* stream) {
    VQW_CHECK(vol && out, "vqw_volume_to_slices: null pointer");
    VQW_CHECK(dtype >= 0 && dtype <= 5, "vqw_volume_to_slices: dtype must be 0..5 (got %d)", dtype);
    VQW_CHECK(norm >= 0 && norm <= 2 && orient >= 0 && orient <= 2, "vqw_volume_to_slices: norm and orient must be 0..2 (got %d, %d)",
              norm, orient);
    VQW_CHECK(norm == NORM_NONE || stats, "vqw_volume_to_slices: normalisation needs the statistics");
    if (int rc = volume_checks("vqw_volume_to_slices", X, Y, Z, S)) return rc;
    const Geo g = geometry(orient, X, Y);
    VQW_CHECK(g.w + 1 <= kLdsFloats, "vqw_volume_to_slices: rows of at most %d pixels (got %d)", kLdsFloats - 1, g.w);
    VQW_CHECK(ksh >= 0 && ksv >= 0, "vqw_volume_to_slices: negative table width");
    VQW_CHECK(ksh ? (kh && bh) : g.w == S, "vqw_volume_to_slices: the horizontal pass needs its tables unless it keeps %d columns", g.w);
    VQW_CHECK(ksv ? (kv && bv && tmp) : g.h == S, "vqw_volume_to_slices: the vertical pass needs its tables and tmp unless it keeps %d rows", g.h);
    Scale sc = {slope, inter, scaled};
    slices_by_dtype(dtype, vol, stats, kh, bh, kv, bv, tmp, out, g, Z, S, ksh, ksv, norm, sc, (long)X * Y, (hipStream_t)stream);
    VQW_LAUNCH_CHECK("vqw_volume_to_slices");
    return VQW_OK;
}

extern "C" int vqw_label_slices(const int32_t* vol, const int* xtab, const int* ytab, int32_t* out, int32_t* err, int X, int Y,
                                int Z, int S, int orient, int relabel, void* stream) {
    VQW_CHECK(vol && xtab && ytab && out && err, "vqw_label_slices: null pointer");
    VQW_CHECK(orient >= 0 && orient <= 2, "vqw_label_slices: orient must be 0..2 (got %d)", orient);
    if (int rc = volume_checks("vqw_label_slices", X, Y, Z, S)) return rc;
    const Geo g = geometry(orient, X, Y);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(err, 0, sizeof(int32_t), s);
    VQW_CHECK(e == hipSuccess, "vqw_label_slices: memset failed: %s", hipGetErrorString(e));
    const long n = (long)X * Y * Z;
    if (relabel) k_label_scan<<<stream_grid(n, kBlock), kBlock, 0, s>>>(vol, n, err);
    dim3 grid(ceil_div(S, 32), ceil_div(S, 32), Z);
    if (orient == ORIENT_NONE) k_labels<true><<<grid, kBlock, 0, s>>>(vol, xtab, ytab, out, g, S, relabel, (long)X * Y);
    else k_labels<false><<<grid, kBlock, 0, s>>>(vol, xtab, ytab, out, g, S, relabel, (long)X * Y);
    VQW_LAUNCH_CHECK("vqw_label_slices");
    return VQW_OK;
}
