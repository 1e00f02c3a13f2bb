// The kernel families around the minGPT blocks that make the code prior (networks/mingpt.py GPT :122-224): the token /
// position embedding, the cross-entropy over the last axis, top-k sampling, and the sample-or-force step of masked resampling.  fp32, dense, no float atomics: every sum has a
// fixed order, two runs give the same bits.
//
// Embedding.  x[b][t] = (t < Te ? prefix[b][t] : tok[idx[b][t - Te]]) + pos[t0 + t]: one wave per row, one add per element.  An
// index outside [0, V) reads nothing and writes a NaN row.  Backward: gpos[t0 + t] = sum_b gx[b][t] with b ascending (a thread per
// float4 column of a position; the other rows of gpos are zeroed), and gtok by ownership: a wave owns a vocabulary row, walks the
// B Ti indices 64 at a time, ballots the matches and adds the matching rows of gx in ascending (b, t) order into registers
// (E / 64 floats per lane, as float4s) - V B Ti index reads from L2, no sort, no atomics; an index outside [0, V) matches no row.
//
// Cross-entropy.  One wave owns a row of z [rows][V]: up to XE_REG_V columns the row is read once into registers (maximum, then
// sum of exp(z - max)); above it the row is walked with an online maximum and sum per lane, merged over the wave at the end.
// The terms exp(z - max) are fp32; their sum and the row's two scalars are double and rounded once: lse = max + log(sum),
// loss = (max - z[target]) + log(sum) - the difference is taken before the logarithm is added, so a row that sits far off zero
// loses nothing to the size of its lse.  A workgroup owns XE_WG_ROWS rows (wave w the rows w, w + 4, ...) and leaves the sum of
// their losses, in double, in the workspace; a second kernel folds the partials in index order in double (XE_FOLD_LANES threads,
// thread l the partials l, l + XE_FOLD_LANES, ...), divides by rows and rounds once.  Backward:
// gz = (exp(z - lse) - [c == target]) w_r, w_r = g[0] / rows (the mean; g is read on the device) or gloss[r].
//
// Sampling.  One workgroup of 256 threads per row of logits [B][V]; s = z / temperature.  The k-th largest s is found by a
// four-pass 8-bit radix select on the order-preserving integer image of the floats (LDS histogram; integer atomics - counts do
// not depend on order); every entry at or above it is kept, ties included.  p = exp(s - max) over the kept entries; thread t sums
// the contiguous chunk t of the row, thread 0 adds the 256 chunk sums in order, finds the first chunk whose running sum exceeds
// u total and walks it serially.  The row is read from global memory on every pass (L2-resident at these sizes).
//
// Sample or force (vqw_sample_filtered, the step of GPT.generate_masked).  The same kernel, k_sample, with what vqw_sample_topk
// leaves off: a nucleus threshold found by the same radix walk on integer MASSES per bin, a forced token per row in place of the
// draw, and the token's log-probability under the unfiltered distribution at temperature 1 (the cross-entropy's rule: fp32
// terms, a double sum in a fixed order, rounded once).  Details above the kernel.
//
// Guided sampling (vqw_sample_guided, the guided step of GPT.generate_masked).  Still the same kernel: k_sample takes its logits
// source as a template parameter, and the guided source mixes the conditional and the unconditional row of a sample entry by entry,
// z = fmaf(scale, z_c - z_u, z_u), in every pass - nothing of the size of the logits is written.  Details above the two sources.
#include "common.h"
#include "gpt_math.h"
#include "../../include/vqwnet_hip.h"

// ---------------------------------------------------------------------------------------------------------- embedding
#define EM_MIN_E 4
#define EM_MAX_E 4096
#define EM_SMALL_E 1024     // up to here a lane of the gtok kernel holds 4 float4 columns of its row, above 16

// grid ceil(B T / 4): wave w of workgroup g writes row 4 g + w
__global__ void __launch_bounds__(256) k_embed_fwd(const long* __restrict__ idx, const float* __restrict__ tok, const float* __restrict__ pos,
                                                   const float* __restrict__ prefix, float* __restrict__ x, long rows, int Ti, int Te, int E,
                                                   int V, int t0) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, E4 = E >> 2, T = Te + Ti;
    const long b = r / T;
    const int t = (int)(r - b * T);
    const float* src;
    bool ok = true;
    if (t < Te) src = prefix + (b * Te + t) * E;
    else {
        const long id = idx[b * Ti + (t - Te)];
        ok = id >= 0 && id < V;
        src = tok + (ok ? id : 0) * E;
    }
    const float* pp = pos + (long)(t0 + t) * E;
    float* xr = x + r * E;
    const float nan = quiet_nan();
    for (int c4 = lane; c4 < E4; c4 += 64) {
        const float4 a = *(const float4*)(src + 4 * c4), p = *(const float4*)(pp + 4 * c4);
        *(float4*)(xr + 4 * c4) = ok ? make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w) : make_float4(nan, nan, nan, nan);
    }
}

// grid-stride over block_size x E / 4: position p, float4 column c4
__global__ void __launch_bounds__(256) k_embed_gpos(const float* __restrict__ gx, float* __restrict__ gpos, int B, int T, int E, int block_size,
                                                    int t0) {
    const int E4 = E >> 2;
    const long n = (long)block_size * E4, step = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const int p = (int)(i / E4), c4 = (int)(i - (long)p * E4), t = p - t0;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) {
            for (int b = 0; b < B; ++b) {
                const float4 g = *(const float4*)(gx + ((long)b * T + t) * E + 4 * c4);
                s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
            }
        }
        *(float4*)(gpos + (long)p * E + 4 * c4) = s;
    }
}

// grid ceil(V / 4): wave w of workgroup g owns the vocabulary row 4 g + w
template <int NV>
__global__ void __launch_bounds__(256) k_embed_gtok(const long* __restrict__ idx, const float* __restrict__ gx, float* __restrict__ gtok, int B,
                                                    int Ti, int Te, int E, int V) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= V) return;
    const int lane = threadIdx.x & 63, E4 = E >> 2, T = Te + Ti;
    const long n = (long)B * Ti;
    float4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i0 = 0; i0 < n; i0 += 64) {
        const long i = i0 + lane;
        unsigned long long hit = __ballot(i < n && idx[i] == (long)v);
        while (hit) {                                   // wave-uniform: the set bits in ascending order
            const long j = i0 + (__ffsll((long long)hit) - 1);
            hit &= hit - 1;
            const long b = j / Ti;
            const float* g = gx + (b * T + Te + (j - b * Ti)) * E;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int c4 = lane + 64 * k;
                if (c4 < E4) {
                    const float4 a = *(const float4*)(g + 4 * c4);
                    acc[k].x += a.x; acc[k].y += a.y; acc[k].z += a.z; acc[k].w += a.w;
                }
            }
        }
    }
    float* o = gtok + (long)v * E;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c4 = lane + 64 * k;
        if (c4 < E4) *(float4*)(o + 4 * c4) = acc[k];
    }
}

static int em_check(const char* name, int B, int Ti, int Te, int E, int V, int block_size, int t0) {
    VQW_CHECK(E % 4 == 0 && E >= EM_MIN_E && E <= EM_MAX_E, "%s: E=%d must be a multiple of 4 with %d <= E <= %d", name, E, EM_MIN_E, EM_MAX_E);
    VQW_CHECK(V >= 1, "%s: V=%d must be at least 1", name, V);
    VQW_CHECK(Ti >= 0, "%s: Ti=%d must not be negative", name, Ti);
    VQW_CHECK(B >= 1 && Te >= 0 && (long)Te + Ti >= 1, "%s: B=%d, Te=%d, Ti=%d must satisfy B >= 1, Te >= 0, Te + Ti >= 1", name, B, Te, Ti);
    VQW_CHECK(t0 >= 0 && block_size >= 1 && (long)t0 + Te + Ti <= block_size, "%s: t0 + T = %d + %d exceeds block_size=%d", name, t0, Te + Ti,
              block_size);
    VQW_CHECK((long)B * ((long)Te + Ti) <= (1L << 31) - 4, "%s: B * T = %ld rows are too many", name, (long)B * ((long)Te + Ti));
    return VQW_OK;
}

extern "C" int vqw_embed_fwd(const long* idx, const float* tok, const float* pos, const float* prefix, float* x, int B, int Ti, int Te, int E,
                             int V, int block_size, int t0, void* stream) {
    if (int rc = em_check("vqw_embed_fwd", B, Ti, Te, E, V, block_size, t0)) return rc;
    VQW_CHECK(tok && pos && x && (idx || Ti == 0), "vqw_embed_fwd: null pointer");
    VQW_CHECK((prefix != nullptr) == (Te > 0), "vqw_embed_fwd: prefix must be given exactly when Te=%d is positive", Te);
    VQW_CHECK(al16(tok) && al16(pos) && al16(prefix) && al16(x), "vqw_embed_fwd: tensors must be 16-byte aligned");
    const long rows = (long)B * (Te + Ti);
    hipLaunchKernelGGL(k_embed_fwd, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, idx, tok, pos, prefix, x, rows, Ti, Te, E, V, t0);
    VQW_LAUNCH_CHECK("vqw_embed_fwd");
    return VQW_OK;
}

extern "C" int vqw_embed_bwd(const long* idx, const float* gx, float* gtok, float* gpos, int B, int Ti, int Te, int E, int V, int block_size,
                             int t0, void* stream) {
    if (int rc = em_check("vqw_embed_bwd", B, Ti, Te, E, V, block_size, t0)) return rc;
    VQW_CHECK(gx && gtok && gpos && (idx || Ti == 0), "vqw_embed_bwd: null pointer");
    VQW_CHECK(al16(gx) && al16(gtok) && al16(gpos), "vqw_embed_bwd: tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_embed_gpos, dim3(stream_grid((long)block_size * (E >> 2), 256)), dim3(256), 0, st, gx, gpos, B, Te + Ti, E, block_size, t0);
    if (E <= EM_SMALL_E) hipLaunchKernelGGL((k_embed_gtok<EM_SMALL_E / 256>), dim3(ceil_div(V, 4)), dim3(256), 0, st, idx, gx, gtok, B, Ti, Te, E, V);
    else hipLaunchKernelGGL((k_embed_gtok<EM_MAX_E / 256>), dim3(ceil_div(V, 4)), dim3(256), 0, st, idx, gx, gtok, B, Ti, Te, E, V);
    VQW_LAUNCH_CHECK("vqw_embed_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- cross-entropy
#define XE_MAX_V 65536
#define XE_REG_V 1024        // up to here a row lives in registers (16 floats per lane) and is read once; above: online max / sum
#define XE_WG_ROWS 32        // rows per workgroup of the forward: one partial sum of losses each
#define XE_FOLD_LANES 256    // threads of the fold: thread l adds the partials l, l + XE_FOLD_LANES, ...

extern "C" size_t vqw_xent_ws_bytes(long rows) {
    if (rows < 1) return 0;
    return (size_t)ceil_div(rows, XE_WG_ROWS) * sizeof(double);
}

// grid ceil(rows / XE_WG_ROWS); part (may be null): the workgroup's sum of losses
template <bool REG>
__global__ void __launch_bounds__(256) k_xe_fwd(const float* __restrict__ z, const long* __restrict__ target, float* __restrict__ loss,
                                                float* __restrict__ lse, double* __restrict__ part, long rows, int V) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.x * XE_WG_ROWS;
    const long r1 = r0 + XE_WG_ROWS < rows ? r0 + XE_WG_ROWS : rows;
    double acc = 0.0;
    for (long r = r0 + wv; r < r1; r += 4) {
        const float* zr = z + r * V;
        float m = -INFINITY;
        double s = 0.0;
        if (REG) {
            float v[XE_REG_V / 64];
#pragma unroll
            for (int i = 0; i < XE_REG_V / 64; ++i) {
                const int c = lane + 64 * i;
                v[i] = c < V ? zr[c] : -INFINITY;
                m = fmaxf(m, v[i]);
            }
            m = wave_max_f(m);
#pragma unroll
            for (int i = 0; i < XE_REG_V / 64; ++i) s += (lane + 64 * i < V) ? (double)expf(v[i] - m) : 0.0;
        } else {
            for (int c = lane; c < V; c += 64) {        // V > XE_REG_V: every lane sees a column
                const float x = zr[c];
                if (x > m) { s = s * (double)expf(m - x) + 1.0; m = x; }
                else s += (double)expf(x - m);
            }
            const float mw = wave_max_f(m);
            s *= (double)expf(m - mw);
            m = mw;
        }
        // the terms are fp32, their sum and the row's scalars are double: lse and loss are rounded once
        s = wave_sum_d(s);
        const long t = target[r];
        const bool ok = t >= 0 && t < V;
        const double ls = log(s);
        const float l = ok ? (float)(((double)m - (double)zr[ok ? t : 0]) + ls) : quiet_nan();
        if (lane == 0) { lse[r] = (float)((double)m + ls); loss[r] = l; }
        acc += (double)l;
    }
    if (part) {
        if (lane == 0) wsum[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// one workgroup: mean = (sum of the G partials, in double) / rows, rounded once
__global__ void __launch_bounds__(XE_FOLD_LANES) k_xe_mean(const double* __restrict__ part, float* __restrict__ mean, int G, long rows) {
    __shared__ double lanes[XE_FOLD_LANES];
    double s = 0.0;
    for (int g = threadIdx.x; g < G; g += XE_FOLD_LANES) s += part[g];
    lanes[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = 0.0;
        for (int k = 0; k < XE_FOLD_LANES; ++k) s += lanes[k];
        mean[0] = (float)(s / (double)rows);
    }
}

// grid ceil(rows / 4): wave w of workgroup g writes row 4 g + w
__global__ void __launch_bounds__(256) k_xe_bwd(const float* __restrict__ z, const long* __restrict__ target, const float* __restrict__ lse,
                                                const float* __restrict__ gw, float* __restrict__ gz, long rows, int V, int mean) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const long t = target[r];
    const bool ok = t >= 0 && t < V;
    const float w = mean ? gw[0] / (float)rows : gw[r], L = lse[r];
    const float* zr = z + r * V;
    float* gr = gz + r * V;
    for (int c = lane; c < V; c += 64) {
        const float p = expf(zr[c] - L);
        gr[c] = ok ? (c == t ? p - 1.f : p) * w : quiet_nan();
    }
}

static int xe_check(const char* name, long rows, int V) {
    VQW_CHECK(V >= 1 && V <= XE_MAX_V, "%s: V=%d must satisfy 1 <= V <= %d", name, V, XE_MAX_V);
    VQW_CHECK(rows >= 1 && rows <= (1L << 31) - 4, "%s: bad row count %ld (rows >= 1)", name, rows);
    return VQW_OK;
}

extern "C" int vqw_xent_fwd(const float* z, const long* target, float* loss, float* lse, float* mean, void* ws, size_t ws_bytes, long rows, int V,
                            void* stream) {
    if (int rc = xe_check("vqw_xent_fwd", rows, V)) return rc;
    VQW_CHECK(z && target && loss && lse, "vqw_xent_fwd: null pointer");
    VQW_CHECK(!mean || (ws && ws_bytes >= vqw_xent_ws_bytes(rows)), "vqw_xent_fwd: workspace of %zu bytes, %zu needed for the mean",
              ws ? ws_bytes : (size_t)0, vqw_xent_ws_bytes(rows));
    VQW_CHECK(!mean || (((uintptr_t)ws) & 7) == 0, "vqw_xent_fwd: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int G = ceil_div(rows, XE_WG_ROWS);
    double* part = mean ? (double*)ws : nullptr;
    if (V <= XE_REG_V) hipLaunchKernelGGL(k_xe_fwd<true>, dim3(G), dim3(256), 0, st, z, target, loss, lse, part, rows, V);
    else hipLaunchKernelGGL(k_xe_fwd<false>, dim3(G), dim3(256), 0, st, z, target, loss, lse, part, rows, V);
    if (mean) hipLaunchKernelGGL(k_xe_mean, dim3(1), dim3(XE_FOLD_LANES), 0, st, part, mean, G, rows);
    VQW_LAUNCH_CHECK("vqw_xent_fwd");
    return VQW_OK;
}

extern "C" int vqw_xent_bwd(const float* z, const long* target, const float* lse, const float* gw, float* gz, long rows, int V, int mean,
                            void* stream) {
    if (int rc = xe_check("vqw_xent_bwd", rows, V)) return rc;
    VQW_CHECK(z && target && lse && gw && gz, "vqw_xent_bwd: null pointer");
    hipLaunchKernelGGL(k_xe_bwd, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, z, target, lse, gw, gz, rows, V, mean ? 1 : 0);
    VQW_LAUNCH_CHECK("vqw_xent_bwd");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- sampling
#define ST_MAX_V 65536

// One kernel draws for vqw_sample_topk (forced = logp = null, top_p = 1) and vqw_sample_filtered.  The row maximum of s, the radix
// select of the k-th largest key and the chunked inverse-CDF draw are as the file's header describes; a forced row skips the
// filter and the draw; the row's log-probability (and the maximum of z it needs) is taken only where logp is given.
//
// Nucleus.  Entry c of K1 (the top-k kept set) stays iff G(c) = the mass of the entries of K1 strictly greater than it is
// <= top_p total.  G falls as the key rises, so the kept set is {key >= thr2} and thr2 is found like the k-th largest entry: byte
// by byte from the top, on a histogram of MASSES per bin.  The masses are p = exp(s - max) in 2^-40 fixed point (p <= 1 and
// V <= 2^16: a 64-bit sum cannot overflow; p 2^40 is exact in fp32, the conversion truncates below 2^-40): integer additions have
// no order, so the LDS atomics leave the same bits every run.  The bins are walked downwards while the mass above the next
// bin stays within the limit (wave 0, four bins a lane); the bin the walk stops in holds thr2 and is refined by the next byte.
// An empty bin may be chosen: thr2 need not be a key of the row.
#define SF_FIX 0x1p40f

// The logits source of k_sample, a template parameter: what entry c of the row of workgroup b is.
//   PlainLogits   logits [B][V]: the entry itself; the log-probability is that of the same row.
//   GuidedLogits  logits [2B][V], classifier-free guidance: row b is the conditional z_c, row B + b the unconditional z_u of the same
//                 sample, and the entry is sg_mix(z_c, z_u, scale) = z_u + scale (z_c - z_u): one fp32 subtraction and one EXPLICIT
//                 fused multiply-add (the file is built with -ffp-contract=fast: a + s * d would leave the fusing to the back end).
//                 ONE function for every pass - the maximum, the radix select, the mass histogram, the chunk sums and the walk see
//                 the same bits for an entry, so tied entries share one fate.  Nothing [B][V] is written: each pass reads both rows
//                 again (L2-resident at these sizes).  The log-probabilities are those of the two rows themselves: logp under z_c,
//                 logp_u under z_u, each in the plain kernel's form.
__device__ __forceinline__ float sg_mix(float zc, float zu, float scale) { return fmaf(scale, zc - zu, zu); }

struct PlainLogits {
    static constexpr bool GUIDED = false;
    const float* __restrict__ logits;
    struct Row {
        const float* __restrict__ z;
        __device__ __forceinline__ float operator()(int c) const { return z[c]; }
        __device__ __forceinline__ float cond(int c) const { return z[c]; }
        __device__ __forceinline__ float uncond(int c) const { return z[c]; }
    };
    __device__ __forceinline__ Row row(unsigned b, unsigned B, int V) const { return Row{logits + (long)b * V}; }
    __device__ __forceinline__ float* logp_uncond() const { return nullptr; }
};

struct GuidedLogits {
    static constexpr bool GUIDED = true;
    const float* __restrict__ logits;
    float* __restrict__ logp_u;
    float scale;
    struct Row {
        const float* __restrict__ zc;
        const float* __restrict__ zu;
        float scale;
        __device__ __forceinline__ float operator()(int c) const { return sg_mix(zc[c], zu[c], scale); }
        __device__ __forceinline__ float cond(int c) const { return zc[c]; }
        __device__ __forceinline__ float uncond(int c) const { return zu[c]; }
    };
    __device__ __forceinline__ Row row(unsigned b, unsigned B, int V) const { return Row{logits + (long)b * V, logits + ((long)B + b) * V, scale}; }
    __device__ __forceinline__ float* logp_uncond() const { return logp_u; }
};

// grid B, 256 threads: one row (GuidedLogits: one pair of rows) each; out [B], GuidedLogits: [2B] with out[B + b] = out[b]
template <bool NUCLEUS, class SRC>
__global__ void __launch_bounds__(256) k_sample(const SRC src, const float* __restrict__ u, const long* __restrict__ forced,
                                                long* __restrict__ out, float* __restrict__ logp, int V, float temperature, int top_k,
                                                float top_p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long mass[256];
    __shared__ float csum[256];
    __shared__ int clast[256];
    __shared__ float wmax[4], wzmax[4], wzmaxu[4];
    __shared__ double wsum[4], wsumu[4];
    __shared__ unsigned sel[2];
    __shared__ unsigned long long sabove;
    const int tid = threadIdx.x;
    const typename SRC::Row z = src.row(blockIdx.x, gridDim.x, V);
    float* const logp_u = src.logp_uncond();        // GuidedLogits only: null otherwise
    const long f = forced ? forced[blockIdx.x] : -1;
    const bool force = f >= 0 && f < V;             // the same for the whole workgroup

    float m = -INFINITY, zm = -INFINITY, zmu = -INFINITY;      // the maxima of s = z / temperature and, for logp (logp_u), of z_c (z_u)
    for (int c = tid; c < V; c += 256) {
        const float x = z(c);
        if (logp) zm = fmaxf(zm, SRC::GUIDED ? z.cond(c) : x);      // the same for the whole workgroup
        if (SRC::GUIDED && logp_u) zmu = fmaxf(zmu, z.uncond(c));
        m = fmaxf(m, x / temperature);
    }
    m = wave_max_f(m);
    if (logp) zm = wave_max_f(zm);
    if (SRC::GUIDED && logp_u) zmu = wave_max_f(zmu);
    if ((tid & 63) == 0) {
        wmax[tid >> 6] = m;
        wzmax[tid >> 6] = zm;
        if (SRC::GUIDED) wzmaxu[tid >> 6] = zmu;
    }
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));

    // sum_c exp(z_c - max z): fp32 terms, thread t the columns t, t + 256, ... in double, a butterfly per wave, the four waves in order
    if (logp) {
        zm = fmaxf(fmaxf(wzmax[0], wzmax[1]), fmaxf(wzmax[2], wzmax[3]));
        double s = 0.0;
        for (int c = tid; c < V; c += 256) s += (double)expf(z.cond(c) - zm);
        s = wave_sum_d(s);
        if ((tid & 63) == 0) wsum[tid >> 6] = s;
    }
    if (SRC::GUIDED && logp_u) {
        zmu = fmaxf(fmaxf(wzmaxu[0], wzmaxu[1]), fmaxf(wzmaxu[2], wzmaxu[3]));
        double s = 0.0;
        for (int c = tid; c < V; c += 256) s += (double)expf(z.uncond(c) - zmu);
        s = wave_sum_d(s);
        if ((tid & 63) == 0) wsumu[tid >> 6] = s;
    }

    int pick = (int)f;
    if (!force) {
        // the key of the k-th largest entry: byte by byte from the top, among the entries that share the bytes chosen so far
        unsigned thr = 0;
        if (top_k > 0 && top_k < V) {
            unsigned prefix = 0, pmask = 0, kk = (unsigned)top_k;
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[tid] = 0;
                __syncthreads();
                for (int c = tid; c < V; c += 256) {
                    const unsigned key = st_key(z(c) / temperature);
                    if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    int bin = 255;
                    for (; bin > 0; --bin) {
                        const unsigned cnt = hist[bin];
                        if (cnt >= kk) break;
                        kk -= cnt;
                    }
                    sel[0] = prefix | ((unsigned)bin << shift);
                    sel[1] = kk;
                }
                __syncthreads();
                prefix = sel[0];
                kk = sel[1];
                pmask |= 0xffu << shift;
                __syncthreads();
            }
            thr = prefix;
        }

        if (NUCLEUS) {
            unsigned prefix = 0, pmask = 0;
            unsigned long long above = 0, limit = 0;          // wave 0's: the mass above the chosen bin, floor(top_p total)
            for (int shift = 24; shift >= 0; shift -= 8) {
                mass[tid] = 0;
                __syncthreads();
                for (int c = tid; c < V; c += 256) {
                    const float x = z(c) / temperature;
                    const unsigned key = st_key(x);
                    if (key >= thr && (key & pmask) == prefix)
                        atomicAdd(&mass[(key >> shift) & 255u], (unsigned long long)(expf(x - m) * SF_FIX));
                }
                __syncthreads();
                // the walk "bin = 255; while (bin > 0 && above + mass[bin] <= limit) above += mass[bin--]" by wave 0: lane l owns
                // the bins 255 - 4 l ... 252 - 4 l, an integer scan over the lanes finds the lane the walk stops in
                if (tid < 64) {
                    const int hi = 255 - 4 * tid;
                    unsigned long long mb[4], own = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { mb[j] = mass[hi - j]; own += mb[j]; }
                    unsigned long long inc = own;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned long long t = __shfl_up(inc, o, 64);
                        if (tid >= o) inc += t;
                    }
                    if (shift == 24) limit = (unsigned long long)((double)top_p * (double)__shfl(inc, 63, 64));
                    const unsigned long long over = __ballot(above + inc > limit);
                    const int stop = over ? __ffsll((long long)over) - 1 : 63;
                    if (tid == stop) {
                        unsigned long long a = above + (inc - own);
                        int bin = hi;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (bin == hi - j && bin > 0 && a + mb[j] <= limit) { a += mb[j]; --bin; }
                        sel[0] = prefix | ((unsigned)bin << shift);
                        sabove = a;
                    }
                }
                __syncthreads();
                prefix = sel[0];
                above = sabove;
                pmask |= 0xffu << shift;
                __syncthreads();
            }
            if (prefix > thr) thr = prefix;
        }

        // the draw: chunk sums of p = exp(s - max) over the kept entries, and each chunk's last kept index
        const int chunk = (V + 255) / 256, c0 = tid * chunk, c1 = c0 + chunk < V ? c0 + chunk : V;
        float s = 0.f;
        int last = -1;
        for (int c = c0; c < c1; ++c) {
            const float x = z(c) / temperature;
            if (st_key(x) >= thr) { s += expf(x - m); last = c; }
        }
        csum[tid] = s;
        clast[tid] = last;
        __syncthreads();
        if (tid == 0) {
            float total = 0.f;
            for (int t = 0; t < 256; ++t) total += csum[t];
            const float goal = u[blockIdx.x] * total;
            float run = 0.f;
            int t = 0;
            pick = -1;
            for (; t < 256; ++t) {
                const float nx = run + csum[t];
                if (nx > goal) break;
                run = nx;
            }
            if (t < 256) {
                const int e = (t + 1) * chunk < V ? (t + 1) * chunk : V;
                for (int c = t * chunk; c < e; ++c) {
                    const float x = z(c) / temperature;
                    if (st_key(x) >= thr) {
                        run += expf(x - m);
                        if (run > goal) { pick = c; break; }
                    }
                }
                if (pick < 0) pick = clast[t];              // rounding: the chunk's own sum crossed, the running sum did not
            } else {
                for (t = 255; t >= 0 && pick < 0; --t) pick = clast[t];      // rounding left no such index: the last kept one
            }
            if (pick < 0) pick = 0;                         // only with NaN logits
        }
    } else {
        __syncthreads();                                    // wsum
    }
    if (tid == 0) {
        out[blockIdx.x] = pick;
        if (SRC::GUIDED) out[gridDim.x + blockIdx.x] = pick;      // the next decode step's idx for both halves
        if (logp) {                                         // k_xe_fwd's form: the difference first, then the logarithm, rounded once
            const double ls = log(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
            logp[blockIdx.x] = f >= V ? quiet_nan() : -(float)(((double)zm - (double)z.cond(pick)) + ls);
        }
        if (SRC::GUIDED && logp_u) {
            const double ls = log(((wsumu[0] + wsumu[1]) + wsumu[2]) + wsumu[3]);
            logp_u[blockIdx.x] = f >= V ? quiet_nan() : -(float)(((double)zmu - (double)z.uncond(pick)) + ls);
        }
    }
}

extern "C" int vqw_sample_filtered(const float* logits, const float* u, const long* forced, long* out, float* logp, int B, int V,
                                   float temperature, int top_k, float top_p, void* stream) {
    VQW_CHECK(V >= 1 && V <= ST_MAX_V, "vqw_sample_filtered: V=%d must satisfy 1 <= V <= %d", V, ST_MAX_V);
    VQW_CHECK(B >= 1, "vqw_sample_filtered: B=%d must be at least 1", B);
    VQW_CHECK(temperature > 0.f, "vqw_sample_filtered: temperature=%g must be positive", (double)temperature);
    VQW_CHECK(top_k >= 0, "vqw_sample_filtered: top_k=%d must not be negative (0: no filter)", top_k);
    VQW_CHECK(top_p > 0.f, "vqw_sample_filtered: top_p=%g must be positive (>= 1: no filter)", (double)top_p);
    VQW_CHECK(logits && u && out, "vqw_sample_filtered: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const PlainLogits src{logits};
    if (top_p < 1.f) hipLaunchKernelGGL((k_sample<true, PlainLogits>), dim3(B), dim3(256), 0, st, src, u, forced, out, logp, V, temperature, top_k, top_p);
    else hipLaunchKernelGGL((k_sample<false, PlainLogits>), dim3(B), dim3(256), 0, st, src, u, forced, out, logp, V, temperature, top_k, top_p);
    VQW_LAUNCH_CHECK("vqw_sample_filtered");
    return VQW_OK;
}

extern "C" int vqw_sample_guided(const float* logits, const float* u, const long* forced, long* out, float* logp, float* logp_u, int B, int V,
                                 float scale, float temperature, int top_k, float top_p, void* stream) {
    VQW_CHECK(V >= 1 && V <= ST_MAX_V, "vqw_sample_guided: V=%d must satisfy 1 <= V <= %d", V, ST_MAX_V);
    VQW_CHECK(B >= 1 && B <= (1 << 30), "vqw_sample_guided: B=%d must lie in [1, 2^30] (logits has 2 B rows)", B);
    VQW_CHECK(temperature > 0.f, "vqw_sample_guided: temperature=%g must be positive", (double)temperature);
    VQW_CHECK(top_k >= 0, "vqw_sample_guided: top_k=%d must not be negative (0: no filter)", top_k);
    VQW_CHECK(top_p > 0.f, "vqw_sample_guided: top_p=%g must be positive (>= 1: no filter)", (double)top_p);
    VQW_CHECK(scale >= 0.f && scale < INFINITY, "vqw_sample_guided: scale=%g must be finite and not negative", (double)scale);
    VQW_CHECK(logits && u && out, "vqw_sample_guided: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const GuidedLogits src{logits, logp_u, scale};
    if (top_p < 1.f) hipLaunchKernelGGL((k_sample<true, GuidedLogits>), dim3(B), dim3(256), 0, st, src, u, forced, out, logp, V, temperature, top_k, top_p);
    else hipLaunchKernelGGL((k_sample<false, GuidedLogits>), dim3(B), dim3(256), 0, st, src, u, forced, out, logp, V, temperature, top_k, top_p);
    VQW_LAUNCH_CHECK("vqw_sample_guided");
    return VQW_OK;
}

extern "C" int vqw_sample_topk(const float* logits, const float* u, long* out, int B, int V, float temperature, int top_k, void* stream) {
    VQW_CHECK(V >= 1 && V <= ST_MAX_V, "vqw_sample_topk: V=%d must satisfy 1 <= V <= %d", V, ST_MAX_V);
    VQW_CHECK(B >= 1, "vqw_sample_topk: B=%d must be at least 1", B);
    VQW_CHECK(temperature > 0.f, "vqw_sample_topk: temperature=%g must be positive", (double)temperature);
    VQW_CHECK(top_k >= 0, "vqw_sample_topk: top_k=%d must not be negative (0: no filter)", top_k);
    VQW_CHECK(logits && u && out, "vqw_sample_topk: null pointer");
    hipLaunchKernelGGL((k_sample<false, PlainLogits>), dim3(B), dim3(256), 0, (hipStream_t)stream, PlainLogits{logits}, u, (const long*)nullptr, out,
                       (float*)nullptr, V, temperature, top_k, 1.f);
    VQW_LAUNCH_CHECK("vqw_sample_topk");
    return VQW_OK;
}
