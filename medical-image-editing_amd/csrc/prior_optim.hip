// What training the GPT code prior adds to the kernels (trainers/prior.py): the global gradient norm with its clip coefficient,
// AdamW with that coefficient applied on the fly, and the transformer's input tokens.  fp32 in and out, no float atomics: every
// sum has a fixed order, two runs give the same bits.
//
// Gradient norm.  The gradients arrive as vqw_adam_multi's chunk table.  Stage one: a workgroup per record; thread t owns the
// quads t, t + 256, ... of the chunk (a quad is four consecutive elements: one 16-byte load where the chunk is aligned, four
// 4-byte loads where it is not - the same additions in the same order either way) and sums g g in double; the 256 sums are
// folded by the fixed wave butterfly and the four wave sums in order; one double per record goes to the workspace.  Stage two:
// one workgroup of GN_FOLD_LANES threads, thread l the partials l, l + GN_FOLD_LANES, ... in ascending order, the same fold, then
// norm = (float)sqrt(sum) and coef = min(1, max_norm / (norm + 1e-6)) in fp32 - torch.nn.utils.clip_grad_norm_'s formula.
// Nothing is read by the host.
//
// AdamW.  torch.optim.AdamW: p *= 1 - lr wd; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2; p -= (lr / bc1) m / (sqrt(v) /
// sqrt(bc2) + eps), with g' = coef g and coef read from the device (stage two's output) - the gradient tensors are not rewritten.
// k_adam_multi's walk (elementwise.hip): a workgroup per record, 16-byte accesses where the four pointers allow.  28 B/param.
//
// Tokens.  inp[b][0] = sos, inp[b][t] = corrupted[b][t - 1]; corrupted = ids where u_keep < pkeep, else a uniform code
// min(V - 1, floor(u_rand V)).  A thread per element; pkeep >= 1 reads neither uniform array.
#include "common.h"
#include "../../include/vqwnet_hip.h"

// the 40-byte record of vqw_adam_multi's table (elementwise.hip): part of the ABI
struct OptChunk {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
};
static_assert(sizeof(OptChunk) == 40, "chunk table layout is part of the ABI: 4 pointers + int64 count");

// ---------------------------------------------------------------------------------------------------------- gradient norm
#define GN_FOLD_LANES 1024

// the 256 (or 1024) per-thread sums of a workgroup -> one double in thread 0; fixed order
template <int WAVES>
__device__ __forceinline__ double gn_block_sum(double s, double* wsum) {
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < WAVES; ++w) t += wsum[w];
    return t;
}

__global__ void __launch_bounds__(256) k_gn_partial(const OptChunk* __restrict__ chunks, double* __restrict__ part) {
    __shared__ double wsum[4];
    const OptChunk c = chunks[blockIdx.x];
    const float* g = c.g;
    const long n = c.n, quads = (n + 3) >> 2;
    const bool vec = (((uintptr_t)g) & 15) == 0;
    double s = 0.0;
    for (long q = threadIdx.x; q < quads; q += 256) {
        const long i = q << 2;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 4 <= n) {
            const float4 t = *(const float4*)(g + i);
            x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (i + k < n) x[k] = g[i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s += (double)x[k] * (double)x[k];
    }
    s = gn_block_sum<4>(s, wsum);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(GN_FOLD_LANES) k_gn_fold(const double* __restrict__ part, float* __restrict__ norm_out, int n_chunks,
                                                           float max_norm) {
    __shared__ double wsum[GN_FOLD_LANES / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += GN_FOLD_LANES) s += part[i];
    s = gn_block_sum<GN_FOLD_LANES / 64>(s, wsum);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        float coef = 1.f;
        if (max_norm > 0.f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c < 1.f || c != c ? c : 1.f;          // clamp(max = 1); a NaN norm stays a NaN coefficient, as torch's does
        }
        norm_out[0] = norm;
        norm_out[1] = coef;
    }
}

extern "C" size_t vqw_grad_norm_ws_bytes(int n_chunks) {
    if (n_chunks < 1) return 0;
    return (size_t)n_chunks * sizeof(double);
}

extern "C" int vqw_grad_norm_multi(const void* chunks_dev, int n_chunks, float max_norm, void* ws, size_t ws_bytes, float* norm_out,
                                   void* stream) {
    VQW_CHECK(n_chunks > 0, "vqw_grad_norm_multi: n_chunks=%d must be at least 1", n_chunks);
    VQW_CHECK(chunks_dev && ws && norm_out, "vqw_grad_norm_multi: null pointer");
    VQW_CHECK(ws_bytes >= vqw_grad_norm_ws_bytes(n_chunks), "vqw_grad_norm_multi: workspace of %zu bytes, %zu needed", ws_bytes,
              vqw_grad_norm_ws_bytes(n_chunks));
    VQW_CHECK((((uintptr_t)ws) & 7) == 0, "vqw_grad_norm_multi: the workspace must be 8-byte aligned");
    VQW_CHECK(max_norm == max_norm, "vqw_grad_norm_multi: max_norm is NaN");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gn_partial, dim3(n_chunks), dim3(256), 0, st, (const OptChunk*)chunks_dev, (double*)ws);
    hipLaunchKernelGGL(k_gn_fold, dim3(1), dim3(GN_FOLD_LANES), 0, st, (const double*)ws, norm_out, n_chunks, max_norm);
    VQW_LAUNCH_CHECK("vqw_grad_norm_multi");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- AdamW
// The step's scalars, each formed in double on the host and rounded once, as torch forms them in Python before its fp32 tensor
// operations: an fp32 beta would leave 1 - beta 2.4e-7 off, the same way in every element.
struct AdamWArgs {
    float decay;          // 1 - lr wd (torch's p.mul_(1 - lr * wd))
    float b1, b2;
    float omb1, omb2;     // 1 - beta1, 1 - beta2
    float eps;
    float step;           // lr / bias_corr1
    float bc2_sqrt;       // sqrt(bias_corr2)
};

// One rounding per operation as written: this file is compiled with -ffp-contract=off (csrc/Makefile), since contraction into
// fused multiply-adds comes out differently in the 16-byte walk, the scalar tail and the per-tensor kernel.  Every route gives
// a parameter the same bits.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float coef, const AdamWArgs& a) {
    g *= coef;
    p *= a.decay;
    m = m * a.b1 + a.omb1 * g;
    v = v * a.b2 + a.omb2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step * (m / denom);
}

__global__ void __launch_bounds__(256) k_adamw_multi(const OptChunk* __restrict__ chunks, const float* __restrict__ clip, AdamWArgs a) {
    const OptChunk c = chunks[blockIdx.x];
    const float coef = clip ? clip[0] : 1.f;
    long i0 = 0;
    if ((((uintptr_t)c.p | (uintptr_t)c.g | (uintptr_t)c.m | (uintptr_t)c.v) & 15) == 0) {
        const long n4 = c.n >> 2;
        float4* p4 = (float4*)c.p; const float4* g4 = (const float4*)c.g; float4* m4 = (float4*)c.m; float4* v4 = (float4*)c.v;
        for (long i = threadIdx.x; i < n4; i += 256) {
            const float4 gq = g4[i], pq = p4[i], mq = m4[i], vq = v4[i];
            float gi[4] = {gq.x, gq.y, gq.z, gq.w}, pi[4] = {pq.x, pq.y, pq.z, pq.w}, mi[4] = {mq.x, mq.y, mq.z, mq.w}, vi[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) adamw_elem(pi[k], gi[k], mi[k], vi[k], coef, a);
            p4[i] = make_float4(pi[0], pi[1], pi[2], pi[3]);
            m4[i] = make_float4(mi[0], mi[1], mi[2], mi[3]);
            v4[i] = make_float4(vi[0], vi[1], vi[2], vi[3]);
        }
        i0 = n4 << 2;
    }
    for (long i = i0 + threadIdx.x; i < c.n; i += 256) {
        float pi = c.p[i], mi = c.m[i], vi = c.v[i];
        adamw_elem(pi, c.g[i], mi, vi, coef, a);
        c.p[i] = pi;
        c.m[i] = mi;
        c.v[i] = vi;
    }
}

__global__ void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                        const float* __restrict__ clip, AdamWArgs a) {
    const float coef = clip ? clip[0] : 1.f;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_elem(pi, g[i], mi, vi, coef, a);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
    }
}

static int adamw_args(const char* name, double lr, double beta1, double beta2, double eps, double weight_decay, double bias_corr1,
                      double bias_corr2, AdamWArgs* a) {
    VQW_CHECK(bias_corr1 > 0.0 && bias_corr2 > 0.0, "%s: bias corrections must be positive", name);
    VQW_CHECK(lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0, "%s: lr, eps and weight_decay must not be negative", name);
    VQW_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas must lie in [0, 1)", name);
    a->decay = (float)(1.0 - lr * weight_decay);
    a->b1 = (float)beta1;
    a->b2 = (float)beta2;
    a->omb1 = (float)(1.0 - beta1);
    a->omb2 = (float)(1.0 - beta2);
    a->eps = (float)eps;
    a->step = (float)(lr / bias_corr1);
    a->bc2_sqrt = (float)sqrt(bias_corr2);
    return VQW_OK;
}

extern "C" int vqw_adamw_multi(const void* chunks_dev, int n_chunks, double lr, double beta1, double beta2, double eps,
                               double weight_decay, double bias_corr1, double bias_corr2, const float* clip, void* stream) {
    VQW_CHECK(chunks_dev && n_chunks > 0, "vqw_adamw_multi: bad arguments");
    AdamWArgs a;
    if (int rc = adamw_args("vqw_adamw_multi", lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, &a)) return rc;
    hipLaunchKernelGGL(k_adamw_multi, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const OptChunk*)chunks_dev, clip, a);
    VQW_LAUNCH_CHECK("vqw_adamw_multi");
    return VQW_OK;
}

extern "C" int vqw_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                              double weight_decay, double bias_corr1, double bias_corr2, const float* clip, void* stream) {
    VQW_CHECK(p && g && m && v && n > 0, "vqw_adamw_step: bad arguments");
    AdamWArgs a;
    if (int rc = adamw_args("vqw_adamw_step", lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, &a)) return rc;
    hipLaunchKernelGGL(k_adamw, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, clip, a);
    VQW_LAUNCH_CHECK("vqw_adamw_step");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- input tokens
__global__ void __launch_bounds__(256) k_prior_tokens(const long* __restrict__ ids, const float* __restrict__ u_keep,
                                                      const float* __restrict__ u_rand, long* __restrict__ inp, long total, int T, int V,
                                                      long sos, float pkeep, int corrupt) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    long out = sos;
    if (t > 0) {
        const long j = i - 1;          // (b, t - 1)
        out = ids[j];
        if (corrupt && !(u_keep[j] < pkeep)) {
            const long r = (long)floorf(u_rand[j] * (float)V);
            out = r < V - 1 ? r : (long)V - 1;
        }
    }
    inp[i] = out;
}

extern "C" int vqw_prior_tokens(const long* ids, const float* u_keep, const float* u_rand, long* inp, int B, int T, int V, long sos,
                                float pkeep, void* stream) {
    VQW_CHECK(B >= 1 && T >= 1, "vqw_prior_tokens: B=%d and T=%d must be at least 1", B, T);
    VQW_CHECK(V >= 1, "vqw_prior_tokens: V=%d must be at least 1", V);
    VQW_CHECK(pkeep == pkeep, "vqw_prior_tokens: pkeep is NaN");
    VQW_CHECK(ids && inp, "vqw_prior_tokens: null pointer");
    const int corrupt = pkeep < 1.f ? 1 : 0;
    VQW_CHECK(!corrupt || (u_keep && u_rand), "vqw_prior_tokens: pkeep=%g below 1 needs u_keep and u_rand", (double)pkeep);
    const long total = (long)B * T;
    hipLaunchKernelGGL(k_prior_tokens, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, ids, u_keep, u_rand, inp, total, T, V,
                       sos, pkeep, corrupt);
    VQW_LAUNCH_CHECK("vqw_prior_tokens");
    return VQW_OK;
}
