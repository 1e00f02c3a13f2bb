// 8-bit export kernels: float images -> grey bytes through display windows, id maps -> index / RGB planes and per-image
// counts.  What a validation mosaic, the inference export and a test-mode run copy to the host is then 1 byte (grey), 1-2
// bytes (index) or 3 bytes (RGB) per pixel instead of float32 images and int64 ids.
//
// The kernels stream: a thread takes four consecutive pixels of one plane (one 16-byte load of floats, two of ids), and
// stores four bytes per output plane as one dword.  Index arithmetic is 32-bit (B * H * W < 2^31 is checked on entry); the
// only divisions are the 32-bit row lookups a flipped store needs.  A plane size that is not a multiple of four (planes
// then start unaligned) and a flipped plane whose rows are not (a group of four then crosses rows) take the one-pixel forms
// of the same code: the arithmetic, and so every byte, is the same.
//
// Bit-exactness is part of the contract: one float32 rounding per operation, no fused multiply-add, so that
// tests/test_gpu_export.py can repeat the arithmetic operation by operation in numpy float32 and compare bytes.  HIP's
// __fmul_rn / __fadd_rn are plain operators that the compiler contracts like any other, and under the Makefile's global
// -ffp-contract=fast a `#pragma clang fp contract(off)` does not stop the fusion either (checked in the ISA: v_pk_fma_f32
// stays).  So THIS FILE IS COMPILED WITH -ffp-contract=off (target-specific flag in the Makefile); the fused multiply-adds
// left in its ISA are those of the correctly rounded division sequence.
#include "common.h"
#include "../../include/vqwnet_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxWin = 8;
constexpr int kWinStride = 6;            // alpha, beta, lo, hi, vmin, vmax - vmin
constexpr int kLdsBins = 4096;           // palette + histogram in LDS up to this many bins (32 KiB)

struct WinTable {
    float v[kMaxWin][kWinStride];
};

// u8 = min(255, floor(256 * clamp((clamp(alpha x + beta, lo, hi) - vmin) / (vmax - vmin), 0, 1)))
__device__ __forceinline__ unsigned grey_level(float x, const float* w) {
    float t = __fadd_rn(__fmul_rn(w[0], x), w[1]);
    t = fminf(fmaxf(t, w[2]), w[3]);
    float q = __fdiv_rn(__fsub_rn(t, w[4]), w[5]);
    q = fminf(fmaxf(q, 0.f), 1.f);
    float l = floorf(__fmul_rn(256.f, q));
    return (unsigned)fminf(l, 255.f);
}

// destination of plane pixel p (row-major, width W) in the vertically flipped plane
__device__ __forceinline__ unsigned flipped(unsigned p, unsigned H, unsigned W) {
    unsigned y = p / W;
    return (H - 1u - y) * W + (p - y * W);
}

// x: [B][HW] floats; out: [nwin][B][HW] bytes.  grid.y = image.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_export_grey(const float* __restrict__ x, const float* __restrict__ win,
                                                        uint8_t* __restrict__ out, int nwin, unsigned B, unsigned H,
                                                        unsigned W, int flip, int vec_store) {
    __shared__ WinTable tab;
    if (threadIdx.x < nwin * kWinStride) (&tab.v[0][0])[threadIdx.x] = win[threadIdx.x];
    __syncthreads();
    const unsigned HW = H * W;
    const unsigned b = blockIdx.y;
    const float* xp = x + (size_t)b * HW;
    const size_t wstride = (size_t)B * HW;
    uint8_t* op = out + (size_t)b * HW;
    const unsigned step = gridDim.x * kBlock;
    if (VEC) {
        const unsigned groups = HW >> 2;
        for (unsigned g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
            const unsigned p = g << 2;
            const float4_t v = *reinterpret_cast<const float4_t*>(xp + p);
            if (vec_store) {
                const unsigned d = flip ? flipped(p, H, W) : p;
                for (int w = 0; w < nwin; ++w) {
                    const float* t = tab.v[w];
                    const unsigned pk = grey_level(v[0], t) | (grey_level(v[1], t) << 8) | (grey_level(v[2], t) << 16) |
                                        (grey_level(v[3], t) << 24);
                    *reinterpret_cast<unsigned*>(op + w * wstride + d) = pk;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned d = flipped(p + j, H, W);
                    for (int w = 0; w < nwin; ++w) op[w * wstride + d] = (uint8_t)grey_level(v[j], tab.v[w]);
                }
            }
        }
    } else {
        for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < HW; p += step) {
            const float v = xp[p];
            const unsigned d = flip ? flipped(p, H, W) : p;
            for (int w = 0; w < nwin; ++w) op[w * wstride + d] = (uint8_t)grey_level(v, tab.v[w]);
        }
    }
}

struct LabelOut {
    uint8_t* idx8;
    uint16_t* idx16;
    uint8_t* rgb;
    int32_t* counts;
    int32_t* err;
};

// One id: range check (a bad id raises the flag and exports as 0), count, palette entry (packed r | g << 8 | b << 16).
template <bool LDS>
__device__ __forceinline__ unsigned take_id(int64_t id64, int K, const unsigned* pal_lds, const uint8_t* pal_glob,
                                            int* hist_lds, int32_t* counts_row, int32_t* err, bool want_rgb,
                                            unsigned* rgb) {
    unsigned id = (unsigned)id64;
    if (id64 < 0 || id64 > (int64_t)K) {
        *err = 1;
        id = 0;
    } else if (counts_row) {
        if (LDS) atomicAdd(&hist_lds[id], 1);
        else atomicAdd(&counts_row[id], 1);
    }
    if (want_rgb) {
        if (LDS) *rgb = pal_lds[id];
        else {
            const uint8_t* e = pal_glob + 3u * id;
            *rgb = (unsigned)e[0] | ((unsigned)e[1] << 8) | ((unsigned)e[2] << 16);
        }
    }
    return id;
}

// ids: [B][HW] int64.  grid.y = image.  LDS: the palette (packed dwords) and this workgroup's histogram live in LDS,
// the histogram's non-zero bins are added to counts[b] at the end; otherwise palette reads and count atomics go to memory.
template <bool VEC, bool LDS>
__global__ void __launch_bounds__(kBlock) k_export_labels(const int64_t* __restrict__ ids, const uint8_t* __restrict__ palette,
                                                          LabelOut o, unsigned H, unsigned W, int K, int flip,
                                                          int vec_store) {
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    const int bins = K + 1;
    unsigned* pal = lds;
    int* hist = reinterpret_cast<int*>(lds + (LDS ? bins : 0));
    const bool want_rgb = o.rgb != nullptr;
    if (LDS) {
        for (int k = threadIdx.x; k < bins; k += kBlock) {
            if (want_rgb) pal[k] = (unsigned)palette[3 * k] | ((unsigned)palette[3 * k + 1] << 8) | ((unsigned)palette[3 * k + 2] << 16);
            hist[k] = 0;
        }
        __syncthreads();
    }
    const unsigned HW = H * W;
    const unsigned b = blockIdx.y;
    const int64_t* ip = ids + (size_t)b * HW;
    const size_t base = (size_t)b * HW;
    int32_t* crow = o.counts ? o.counts + (size_t)b * bins : nullptr;
    const unsigned step = gridDim.x * kBlock;
    if (VEC) {
        typedef long long ll2 __attribute__((ext_vector_type(2)));
        const unsigned groups = HW >> 2;
        for (unsigned g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
            const unsigned p = g << 2;
            const ll2 a = *reinterpret_cast<const ll2*>(ip + p);
            const ll2 c = *reinterpret_cast<const ll2*>(ip + p + 2);
            const int64_t v[4] = {a[0], a[1], c[0], c[1]};
            unsigned id[4], col[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) id[j] = take_id<LDS>(v[j], K, pal, palette, hist, crow, o.err, want_rgb, &col[j]);
            if (vec_store) {
                const size_t d = base + (flip ? flipped(p, H, W) : p);
                if (o.idx8) *reinterpret_cast<unsigned*>(o.idx8 + d) = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
                if (o.idx16) {
                    uint2 pk;
                    pk.x = id[0] | (id[1] << 16);
                    pk.y = id[2] | (id[3] << 16);
                    *reinterpret_cast<uint2*>(o.idx16 + d) = pk;
                }
                if (want_rgb) {                    // 12 bytes at a multiple of 12: three dwords
                    unsigned* r = reinterpret_cast<unsigned*>(o.rgb + 3 * d);
                    r[0] = col[0] | (col[1] << 24);
                    r[1] = (col[1] >> 8) | (col[2] << 16);
                    r[2] = (col[2] >> 16) | (col[3] << 8);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t d = base + flipped(p + j, H, W);
                    if (o.idx8) o.idx8[d] = (uint8_t)id[j];
                    if (o.idx16) o.idx16[d] = (uint16_t)id[j];
                    if (want_rgb) {
                        o.rgb[3 * d] = (uint8_t)col[j];
                        o.rgb[3 * d + 1] = (uint8_t)(col[j] >> 8);
                        o.rgb[3 * d + 2] = (uint8_t)(col[j] >> 16);
                    }
                }
            }
        }
    } else {
        for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < HW; p += step) {
            unsigned col = 0;
            const unsigned id = take_id<LDS>(ip[p], K, pal, palette, hist, crow, o.err, want_rgb, &col);
            const size_t d = base + (flip ? flipped(p, H, W) : p);
            if (o.idx8) o.idx8[d] = (uint8_t)id;
            if (o.idx16) o.idx16[d] = (uint16_t)id;
            if (want_rgb) {
                o.rgb[3 * d] = (uint8_t)col;
                o.rgb[3 * d + 1] = (uint8_t)(col >> 8);
                o.rgb[3 * d + 2] = (uint8_t)(col >> 16);
            }
        }
    }
    if (LDS && crow) {
        __syncthreads();
        for (int k = threadIdx.x; k < bins; k += kBlock) {
            const int c = hist[k];
            if (c) atomicAdd(&crow[k], c);
        }
    }
}

// ---- per-image auto-ranged export: a range pass (per-workgroup partial minima / maxima of the finite values), then an export
// pass whose workgroups each fold their image's partials.  x is read twice, out written once; no floating-point atomics.
constexpr int kMaxRangeGroups = 64;      // partials per image: one wave folds them

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }      // false for NaN

__device__ __forceinline__ void take_range(float v, float& lo, float& hi) {
    if (finite_f(v)) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
}

__device__ __forceinline__ void wave_range(float& lo, float& hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
}

// workgroups per image of both passes (at most kMaxRangeGroups; fewer for many images)
int auto_groups(unsigned work, int B) {
    return imax(1, imin(imin(stream_grid(work, kBlock), kMaxRangeGroups), 2048 / imin(B, 2048)));
}

// x: [B][HW] floats; part: [B][gridDim.x][2] = this workgroup's (min, max) over the finite values it saw, (+inf, -inf) when
// it saw none.  grid.y = image.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_export_range(const float* __restrict__ x, float* __restrict__ part, unsigned HW) {
    __shared__ float red[2][kBlock / 64];
    const unsigned b = blockIdx.y;
    const float* xp = x + (size_t)b * HW;
    const unsigned step = gridDim.x * kBlock;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (VEC) {
        const unsigned groups = HW >> 2;
        for (unsigned g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
            const float4_t v = *reinterpret_cast<const float4_t*>(xp + (g << 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) take_range(v[j], lo, hi);
        }
    } else {
        for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < HW; p += step) take_range(xp[p], lo, hi);
    }
    wave_range(lo, hi);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kBlock / 64; ++i) {
            lo = fminf(lo, red[0][i]);
            hi = fmaxf(hi, red[1][i]);
        }
        float* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        o[0] = lo;
        o[1] = hi;
    }
}

// u8 = min(255, floor(256 * clamp((x - vmin) / (vmax - vmin), 0, 1))): grey_level with the identity window and the image's own
// (vmin, vmax - vmin); 0 for a non-finite x and for an image whose range is empty or a single value
__device__ __forceinline__ unsigned auto_level(float x, float vmin, float d) {
    if (!finite_f(x) || !(d > 0.f)) return 0u;
    float q = __fdiv_rn(__fsub_rn(x, vmin), d);
    q = fminf(fmaxf(q, 0.f), 1.f);
    float l = floorf(__fmul_rn(256.f, q));
    return (unsigned)fminf(l, 255.f);
}

// part: [B][nparts][2] from k_export_range; out: [B][HW] bytes; range (nullable): [B][2] = (vmin, vmax).  grid.y = image.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_export_grey_auto(const float* __restrict__ x, const float* __restrict__ part,
                                                             uint8_t* __restrict__ out, float* __restrict__ range, int nparts,
                                                             unsigned H, unsigned W, int flip, int vec_store) {
    __shared__ float rng[2];
    const unsigned b = blockIdx.y;
    if (threadIdx.x < 64) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        if ((int)threadIdx.x < nparts) {
            const float* q = part + ((size_t)b * nparts + threadIdx.x) * 2;
            lo = q[0];
            hi = q[1];
        }
        wave_range(lo, hi);
        if (threadIdx.x == 0) {
            rng[0] = lo;
            rng[1] = hi;
            if (range && blockIdx.x == 0) {
                range[2 * b] = lo;
                range[2 * b + 1] = hi;
            }
        }
    }
    __syncthreads();
    const float vmin = rng[0];
    const float d = __fsub_rn(rng[1], vmin);
    const unsigned HW = H * W;
    const float* xp = x + (size_t)b * HW;
    uint8_t* op = out + (size_t)b * HW;
    const unsigned step = gridDim.x * kBlock;
    if (VEC) {
        const unsigned groups = HW >> 2;
        for (unsigned g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += step) {
            const unsigned p = g << 2;
            const float4_t v = *reinterpret_cast<const float4_t*>(xp + p);
            if (vec_store) {
                const unsigned dst = flip ? flipped(p, H, W) : p;
                *reinterpret_cast<unsigned*>(op + dst) = auto_level(v[0], vmin, d) | (auto_level(v[1], vmin, d) << 8) |
                                                         (auto_level(v[2], vmin, d) << 16) | (auto_level(v[3], vmin, d) << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) op[flipped(p + j, H, W)] = (uint8_t)auto_level(v[j], vmin, d);
            }
        }
    } else {
        for (unsigned p = blockIdx.x * kBlock + threadIdx.x; p < HW; p += step)
            op[flip ? flipped(p, H, W) : p] = (uint8_t)auto_level(xp[p], vmin, d);
    }
}

int plane_checks(const char* name, int B, int H, int W) {
    VQW_CHECK(B > 0 && H > 0 && W > 0, "%s: B, H, W must be positive (got %d, %d, %d)", name, B, H, W);
    VQW_CHECK((long)B * H * W < (1L << 31), "%s: B * H * W = %ld does not fit 32-bit indices", name, (long)B * H * W);
    VQW_CHECK(B <= 65535, "%s: at most 65535 images per call (got %d)", name, B);
    return VQW_OK;
}

}  // namespace

extern "C" int vqw_export_grey(const float* x, const float* win, uint8_t* out, int nwin, int B, int H, int W, int flip,
                               void* stream) {
    VQW_CHECK(x && win && out, "vqw_export_grey: null pointer");
    VQW_CHECK(nwin >= 1 && nwin <= kMaxWin, "vqw_export_grey: 1..%d windows (got %d)", kMaxWin, nwin);
    if (int rc = plane_checks("vqw_export_grey", B, H, W)) return rc;
    const unsigned HW = (unsigned)H * W;
    const bool vec = HW % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 4) == 0;
    const int vec_store = !flip || W % 4 == 0;
    dim3 grid(imax(1, imin(stream_grid(vec ? HW / 4 : HW, kBlock), 2048 / imin(B, 2048))), B);
    hipStream_t s = (hipStream_t)stream;
    if (vec) k_export_grey<true><<<grid, kBlock, 0, s>>>(x, win, out, nwin, B, H, W, flip, vec_store);
    else k_export_grey<false><<<grid, kBlock, 0, s>>>(x, win, out, nwin, B, H, W, flip, 0);
    VQW_LAUNCH_CHECK("vqw_export_grey");
    return VQW_OK;
}

extern "C" size_t vqw_export_auto_ws_bytes(int B) { return sizeof(float) * 2 * kMaxRangeGroups * (size_t)imax(B, 1); }

extern "C" int vqw_export_grey_auto(const float* x, uint8_t* out, float* range, float* ws, size_t ws_bytes, int B, int H, int W,
                                    int flip, void* stream) {
    VQW_CHECK(x && out && ws, "vqw_export_grey_auto: null pointer");
    if (int rc = plane_checks("vqw_export_grey_auto", B, H, W)) return rc;
    VQW_CHECK(ws_bytes >= vqw_export_auto_ws_bytes(B), "vqw_export_grey_auto: workspace of %zu bytes, %zu needed", ws_bytes,
              vqw_export_auto_ws_bytes(B));
    const unsigned HW = (unsigned)H * W;
    const bool vec_load = HW % 4 == 0 && ((uintptr_t)x % 16) == 0;
    const bool vec = vec_load && ((uintptr_t)out % 4) == 0;
    const int vec_store = !flip || W % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    const int nparts = auto_groups(vec_load ? HW / 4 : HW, B);
    if (vec_load) k_export_range<true><<<dim3(nparts, B), kBlock, 0, s>>>(x, ws, HW);
    else k_export_range<false><<<dim3(nparts, B), kBlock, 0, s>>>(x, ws, HW);
    VQW_LAUNCH_CHECK("vqw_export_grey_auto (range)");
    dim3 grid(imax(1, imin(stream_grid(vec ? HW / 4 : HW, kBlock), 2048 / imin(B, 2048))), B);
    if (vec) k_export_grey_auto<true><<<grid, kBlock, 0, s>>>(x, ws, out, range, nparts, H, W, flip, vec_store);
    else k_export_grey_auto<false><<<grid, kBlock, 0, s>>>(x, ws, out, range, nparts, H, W, flip, 0);
    VQW_LAUNCH_CHECK("vqw_export_grey_auto");
    return VQW_OK;
}

extern "C" int vqw_export_labels(const int64_t* ids, const uint8_t* palette, void* index_out, uint8_t* rgb, int32_t* counts,
                                 int32_t* err, int B, int H, int W, int K, int flip, void* stream) {
    VQW_CHECK(ids && err, "vqw_export_labels: null pointer");
    VQW_CHECK(K >= 1 && K <= 65535, "vqw_export_labels: K must be in [1, 65535] (got %d)", K);
    VQW_CHECK(!rgb || palette, "vqw_export_labels: an RGB plane needs a palette");
    if (int rc = plane_checks("vqw_export_labels", B, H, W)) return rc;
    const unsigned HW = (unsigned)H * W;
    const int bins = K + 1;
    LabelOut o;
    o.idx8 = K <= 255 ? (uint8_t*)index_out : nullptr;
    o.idx16 = K <= 255 ? nullptr : (uint16_t*)index_out;
    o.rgb = rgb;
    o.counts = counts;
    o.err = err;
    const bool vec = HW % 4 == 0 && ((uintptr_t)ids % 16) == 0 && ((uintptr_t)index_out % 8) == 0 && ((uintptr_t)rgb % 4) == 0;
    const int vec_store = !flip || W % 4 == 0;
    const bool lds = bins <= kLdsBins;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(err, 0, sizeof(int32_t), s);
    if (e == hipSuccess && counts) e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)B * bins, s);
    VQW_CHECK(e == hipSuccess, "vqw_export_labels: memset failed: %s", hipGetErrorString(e));
    // few, long-lived workgroups per image where the histogram is flushed per workgroup
    const int cap = lds ? imax(1, 1024 / imin(B, 1024)) : imax(1, 2048 / imin(B, 2048));
    dim3 grid(imax(1, imin(stream_grid(vec ? HW / 4 : HW, kBlock), cap)), B);
    const size_t shm = lds ? sizeof(unsigned) * 2 * (size_t)bins : 0;
    if (vec && lds) k_export_labels<true, true><<<grid, kBlock, shm, s>>>(ids, palette, o, H, W, K, flip, vec_store);
    else if (vec) k_export_labels<true, false><<<grid, kBlock, shm, s>>>(ids, palette, o, H, W, K, flip, vec_store);
    else if (lds) k_export_labels<false, true><<<grid, kBlock, shm, s>>>(ids, palette, o, H, W, K, flip, 0);
    else k_export_labels<false, false><<<grid, kBlock, shm, s>>>(ids, palette, o, H, W, K, flip, 0);
    VQW_LAUNCH_CHECK("vqw_export_labels");
    return VQW_OK;
}
