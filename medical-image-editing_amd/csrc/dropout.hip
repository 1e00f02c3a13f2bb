// Dropout of the GPT prior outside the attention (networks/mingpt.py:104 res_drop, :112 the MLP's Dropout, :189 drop): the
// counter-based masks of dropout.h applied in one pass.  The mask is regenerated wherever it is needed - the backward is the same
// launch on the gradient under the same key - and written to memory only by the two *_mask entry points, which exist for tests
// and for looking at a mask.  fp32, no atomics, the same bits every run.  HBM-bound: the nine integer instructions per element
// (dropout.h) sit beside 8 or 12 bytes of traffic per element.
#include "common.h"
#include "prof.h"
#include "dropout.h"
#include "../../include/vqwnet_hip.h"

// a float4 of the walk holds the elements [4 i, 4 i + 4): one row key (a row of the index space is 2^32 elements), four draws
struct DropRow4 {
    uint32_t r0, r1, lo;
    __device__ __forceinline__ DropRow4(const DropKey& k, long i4) : lo((uint32_t)((unsigned long)i4 << 2)) {
        dk_row(k, (uint32_t)((unsigned long)i4 >> 30), r0, r1);
    }
    __device__ __forceinline__ float m(const DropKey& k, int e) const { return dk_keep_row(k, r0, r1, lo + e) ? k.scale : 0.f; }
};

// y = (ADD ? a : 0) + drop(x)
template <bool ADD>
__global__ void k_dropout(const float* __restrict__ a, const float* __restrict__ x, float* __restrict__ y, long n, DropKey k) {
    const long n4 = n >> 2, stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const DropRow4 d(k, i);
        const float4 v = ((const float4*)x)[i];
        float4 r = make_float4(v.x * d.m(k, 0), v.y * d.m(k, 1), v.z * d.m(k, 2), v.w * d.m(k, 3));
        if (ADD) {
            const float4 u = ((const float4*)a)[i];
            r.x += u.x; r.y += u.y; r.z += u.z; r.w += u.w;
        }
        ((float4*)y)[i] = r;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float r = x[i] * (dk_keep(k, (uint64_t)i) ? k.scale : 0.f);
        y[i] = ADD ? a[i] + r : r;
    }
}

__global__ void k_dropout_mask(unsigned char* __restrict__ out, long n, DropKey k) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = dk_keep(k, (uint64_t)i) ? 1 : 0;
}

// out [B n_head][Tq][Tk]: one thread per probability, through the attention's index (dk_attn_hi, lo = j)
__global__ void k_attention_dropout_mask(unsigned char* __restrict__ out, long rows, int Tq, int Tk, DropKey k) {
    const long n = rows * Tk, stride = (long)gridDim.x * blockDim.x;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const long row = e / Tk;                                  // (b n_head + h) Tq + i
        const int j = (int)(e - row * Tk);
        uint32_t r0, r1;
        dk_row(k, dk_attn_hi((uint32_t)(row / Tq), (uint32_t)Tq, (uint32_t)(row % Tq)), r0, r1);
        out[e] = dk_keep_row(k, r0, r1, (uint32_t)j) ? 1 : 0;
    }
}

static int drop_check(const char* name, long n, float p) {
    VQW_CHECK(n > 0, "%s: n=%ld must be positive", name, n);
    VQW_CHECK(p >= 0.f && p < 1.f, "%s: p=%g must lie in [0, 1)", name, (double)p);
    return VQW_OK;
}

extern "C" int vqw_dropout(const float* x, float* y, long n, float p, long seed, long call, int site, void* stream) {
    VQW_PROF_HBM(stream, 2, n);
    if (int rc = drop_check("vqw_dropout", n, p)) return rc;
    VQW_CHECK(x && y, "vqw_dropout: null pointer");
    VQW_CHECK(al16(x) && al16(y), "vqw_dropout: pointers must be 16-byte aligned");
    k_dropout<false><<<stream_grid((n + 3) / 4, 256), 256, 0, (hipStream_t)stream>>>(nullptr, x, y, n, dk_make(p, seed, call, site));
    VQW_LAUNCH_CHECK("vqw_dropout");
    return VQW_OK;
}

extern "C" int vqw_add_dropout(const float* a, const float* b, float* y, long n, float p, long seed, long call, int site, void* stream) {
    VQW_PROF_HBM(stream, 3, n);
    if (int rc = drop_check("vqw_add_dropout", n, p)) return rc;
    VQW_CHECK(a && b && y, "vqw_add_dropout: null pointer");
    VQW_CHECK(al16(a) && al16(b) && al16(y), "vqw_add_dropout: pointers must be 16-byte aligned");
    k_dropout<true><<<stream_grid((n + 3) / 4, 256), 256, 0, (hipStream_t)stream>>>(a, b, y, n, dk_make(p, seed, call, site));
    VQW_LAUNCH_CHECK("vqw_add_dropout");
    return VQW_OK;
}

extern "C" int vqw_dropout_mask(unsigned char* out, long n, float p, long seed, long call, int site, void* stream) {
    if (int rc = drop_check("vqw_dropout_mask", n, p)) return rc;
    VQW_CHECK(out, "vqw_dropout_mask: null pointer");
    k_dropout_mask<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(out, n, dk_make(p, seed, call, site));
    VQW_LAUNCH_CHECK("vqw_dropout_mask");
    return VQW_OK;
}

extern "C" int vqw_attention_dropout_mask(unsigned char* out, int B, int n_head, int Tq, int Tk, float p, long seed, long call, int site,
                                          void* stream) {
    VQW_CHECK(B >= 1 && n_head >= 1 && (long)B * n_head <= 65535 && Tq >= 1 && Tq <= 65536 && Tk >= 1 && Tk <= 65536,
              "vqw_attention_dropout_mask: B=%d, n_head=%d, Tq=%d, Tk=%d must satisfy 1 <= B * n_head <= 65535 and 1 <= T <= 65536", B, n_head, Tq, Tk);
    const long rows = (long)B * n_head * Tq;
    if (int rc = drop_check("vqw_attention_dropout_mask", rows * Tk, p)) return rc;
    VQW_CHECK(out, "vqw_attention_dropout_mask: null pointer");
    k_attention_dropout_mask<<<stream_grid(rows * Tk, 256), 256, 0, (hipStream_t)stream>>>(out, rows, Tq, Tk, dk_make(p, seed, call, site));
    VQW_LAUNCH_CHECK("vqw_attention_dropout_mask");
    return VQW_OK;
}
