// The bidirectional masked code prior (networks/gpt.py MaskedGPT, trainers/masked_prior.py; MaskGIT's recipe): the corruption of a
// training step and one iteration of parallel decoding.  Both are "mark the n lowest of a row", so both stand on one device
// routine, select_lowest, which vqw_select_lowest exposes on its own.
//
// select_lowest.  One workgroup of 256 threads owns a row of T 32-bit keys.  Among the eligible entries it takes exactly
// min(max(n, 0), count) with the smallest (key, position): the n-th smallest key is found byte by byte from the top on an LDS
// histogram of integer counters (k_sample's walk for the k-th largest, turned round), every eligible entry below that threshold
// is taken, and the entries EQUAL to it are taken in ascending position until n is reached - their rank is a workgroup prefix count
// over the positions (a ballot per wave, the four waves' counts in wave order, a running total per chunk of 256 positions), so a
// tie never depends on which wave came first.  Integer LDS atomics only: counts have no order, the same bits every run.  The
// routine reads a key through a functor as often as it has passes (six at most) and keeps nothing per entry: a row of any T in
// [1, 65536] needs the same 1 KB of LDS.  A functor must return the same bits for the same position every time it is asked.
//
// Keys of floats: the order-preserving image of the fp32 bits - negative numbers with all bits flipped, the others with the sign
// bit set - so -0 < +0, the infinities order as numbers and a NaN with a clear sign bit lies above +inf.
#include <math.h>
#include "common.h"
#include "dropout.h"
#include "../../include/vqwnet_hip.h"

#define MASK_RATIO_SITE (-2)          // the draw of sample b's masking ratio: element b under this site
#define MASK_KEY_SITE (-3)            // the draw of position (b, t)'s key: element b T + t under this site

__device__ __forceinline__ unsigned float_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelectLds {
    unsigned hist[256];
    unsigned sel[2];
    unsigned wcnt[4];
};

// All 256 threads of the workgroup call it with the same T and n.  key(t) -> unsigned, elig(t) -> bool, emit(t, taken) is called
// exactly once for every t in [0, T).  Returns the number of eligible entries.
template <class KEY, class ELIG, class EMIT>
__device__ __forceinline__ int select_lowest(SelectLds& s, int T, int n, KEY key, ELIG elig, EMIT emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c = 0;
    for (int t = tid; t < T; t += 256) c += elig(t) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();                                  // the routine may be entered twice: nobody still reads wcnt
    if (lane == 0) s.wcnt[wave] = (unsigned)c;
    __syncthreads();
    const int count = (int)(s.wcnt[0] + s.wcnt[1] + s.wcnt[2] + s.wcnt[3]);
    const int take = n < 0 ? 0 : (n > count ? count : n);
    if (take == 0 || take == count) {                 // nothing or everything: no threshold
        for (int t = tid; t < T; t += 256) emit(t, take != 0 && elig(t));
        return count;
    }

    // the key of the take-th smallest eligible entry, byte by byte from the top, among the entries that share the bytes chosen so far
    unsigned prefix = 0, pmask = 0, kk = (unsigned)take;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s.hist[tid] = 0;                              // thread 0's reads of the previous pass lie in front of that pass's last barrier
        __syncthreads();
        for (int t = tid; t < T; t += 256) {
            if (!elig(t)) continue;
            const unsigned k = key(t);
            if ((k & pmask) == prefix) atomicAdd(&s.hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int bin = 0;
            for (; bin < 255; ++bin) {
                const unsigned cnt = s.hist[bin];
                if (cnt >= kk) break;
                kk -= cnt;
            }
            s.sel[0] = prefix | ((unsigned)bin << shift);
            s.sel[1] = kk;
        }
        __syncthreads();
        prefix = s.sel[0];
        kk = s.sel[1];
        pmask |= 0xffu << shift;
    }
    const unsigned thr = prefix;                      // kk >= 1 of the entries equal to thr are taken, the first in position

    unsigned before = 0;                              // the entries equal to thr in front of this chunk of 256 positions
    for (int base = 0; base < T; base += 256) {
        const int t = base + tid;
        bool e = false, below = false, tie = false;
        if (t < T && (e = elig(t))) {
            const unsigned k = key(t);
            below = k < thr;
            tie = k == thr;
        }
        const unsigned long long ball = __ballot(tie);
        __syncthreads();                              // the previous chunk's reads of wcnt are done
        if (lane == 0) s.wcnt[wave] = (unsigned)__popcll(ball);
        __syncthreads();
        unsigned rank = before + (unsigned)__popcll(ball & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += s.wcnt[w];
        if (t < T) emit(t, e && (below || (tie && rank < kk)));
        before += s.wcnt[0] + s.wcnt[1] + s.wcnt[2] + s.wcnt[3];
    }
    return count;
}

// ------------------------------------------------------------------------------------------------ vqw_select_lowest
__global__ void __launch_bounds__(256) k_select_lowest(const float* __restrict__ keys, const uint8_t* __restrict__ eligible,
                                                       const int* __restrict__ n, uint8_t* __restrict__ out, int T) {
    __shared__ SelectLds lds;
    const long row = (long)blockIdx.x * T;
    const float* kr = keys + row;
    const uint8_t* er = eligible ? eligible + row : nullptr;
    uint8_t* orow = out + row;
    select_lowest(lds, T, n[blockIdx.x],
                  [&](int t) { return float_key(kr[t]); },
                  [&](int t) { return er ? er[t] != 0 : true; },
                  [&](int t, bool taken) { orow[t] = taken ? 1 : 0; });
}

// ------------------------------------------------------------------------------------------------ vqw_mask_tokens
// the number of masked positions of a sample: clamp(ceil(r T), 1, T) in double, r = cos(pi/2 u) of the sample's draw or the fixed ratio
__device__ __forceinline__ int masked_count(double r, int T) {
    const double c = ceil(r * (double)T);
    return c < 1.0 ? 1 : (c > (double)T ? T : (int)c);
}

__global__ void __launch_bounds__(256) k_mask_tokens(const long* __restrict__ ids, long* __restrict__ inp, uint8_t* __restrict__ masked,
                                                     int* __restrict__ n_out, int T, long mask_token, double ratio, DropKey kratio,
                                                     DropKey kkey) {
    __shared__ SelectLds lds;
    const unsigned b = blockIdx.x;
    uint32_t r0, r1;
    double r = ratio;
    if (!(ratio > 0.0)) {                             // the cosine schedule: u = the sample's draw / 2^32
        dk_row(kratio, 0u, r0, r1);
        r = cos(1.5707963267948966 * ((double)dk_draw(r0, r1, b) * (1.0 / 4294967296.0)));
    }
    const int n = masked_count(r, T);
    dk_row(kkey, 0u, r0, r1);                         // B T <= 2^32: the high word of every element index is 0
    const unsigned e0 = b * (unsigned)T;
    const long row = (long)b * T;
    select_lowest(lds, T, n,
                  [&](int t) { return dk_draw(r0, r1, e0 + (unsigned)t); },
                  [&](int) { return true; },
                  [&](int t, bool taken) {
                      masked[row + t] = taken ? 1 : 0;
                      inp[row + t] = taken ? mask_token : ids[row + t];
                  });
    if (threadIdx.x == 0) n_out[b] = n;
}

// ------------------------------------------------------------------------------------------------ vqw_unmask_step
// The confidence of a masked position.  ONE body (never inlined): every pass of the select and the conf output get the same bits.
__device__ __noinline__ float unmask_confidence(float logp, const float* __restrict__ u, long i, float tau) {
    if (tau == 0.f) return logp;
    const float lo = 5.9604644775390625e-8f, hi = 1.f - 5.9604644775390625e-8f;       // 2^-24, 1 - 2^-24
    const float uc = fminf(fmaxf(u[i], lo), hi);
    const float g = -logf(-logf(uc));
    return logp + tau * g;
}

__global__ void __launch_bounds__(256) k_unmask_step(const long* __restrict__ tokens, const float* __restrict__ logp,
                                                     const uint8_t* __restrict__ masked, const float* __restrict__ u,
                                                     const int* __restrict__ m0, long* __restrict__ ids_out, uint8_t* __restrict__ masked_out,
                                                     float* __restrict__ fixed_logp, float* __restrict__ conf, int T, double gamma, float tau,
                                                     long mask_token) {
    __shared__ SelectLds lds;
    __shared__ int s_cur;
    const long row = (long)blockIdx.x * T;
    const int tid = threadIdx.x;
    // cur, the masked count now -> n_keep = gamma <= 0 ? 0 : max(0, min(cur - 1, floor(gamma m0)))
    int c = 0;
    for (int t = tid; t < T; t += 256) c += masked[row + t] ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (tid == 0) s_cur = 0;
    __syncthreads();
    if ((tid & 63) == 0) atomicAdd(&s_cur, c);
    __syncthreads();
    const int cur = s_cur;
    int n_keep = 0;
    if (gamma > 0.0) {
        const double f = floor(gamma * (double)m0[blockIdx.x]);
        const int lim = cur - 1;
        n_keep = f < (double)lim ? (int)f : lim;
        if (n_keep < 0) n_keep = 0;
    }
    select_lowest(lds, T, n_keep,
                  [&](int t) { return float_key(unmask_confidence(logp[row + t], u, row + t, tau)); },
                  [&](int t) { return masked[row + t] != 0; },
                  [&](int t, bool keep) {
                      const long i = row + t;
                      const bool was = masked[i] != 0;
                      if (conf) conf[i] = was ? unmask_confidence(logp[i], u, i, tau) : INFINITY;
                      if (was && !keep) fixed_logp[i] = logp[i];
                      masked_out[i] = keep ? 1 : 0;
                      ids_out[i] = keep ? mask_token : tokens[i];
                  });
}

// ------------------------------------------------------------------------------------------------ the entry points
static int rows_check(const char* name, int B, int T) {
    VQW_CHECK(B >= 1 && B <= 65535, "%s: B=%d must lie in [1, 65535] (one workgroup per sample)", name, B);
    VQW_CHECK(T >= 1 && T <= 65536, "%s: T=%d must lie in [1, 65536]", name, T);
    return VQW_OK;
}
static inline bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
static inline bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

extern "C" int vqw_select_lowest(const float* keys, const uint8_t* eligible, const int* n, uint8_t* out, int B, int T, void* stream) {
    if (int rc = rows_check("vqw_select_lowest", B, T)) return rc;
    VQW_CHECK(keys && n && out, "vqw_select_lowest: null pointer (keys, n and out are required; eligible may be null)");
    VQW_CHECK(al4(keys) && al4(n), "vqw_select_lowest: keys and n must be 4-byte aligned");
    hipLaunchKernelGGL(k_select_lowest, dim3(B), dim3(256), 0, (hipStream_t)stream, keys, eligible, n, out, T);
    VQW_LAUNCH_CHECK("vqw_select_lowest");
    return VQW_OK;
}

extern "C" int vqw_mask_tokens(const long* ids, long* inp, uint8_t* masked, int* n, int B, int T, long mask_token, double ratio, long seed,
                               long call, void* stream) {
    if (int rc = rows_check("vqw_mask_tokens", B, T)) return rc;
    VQW_CHECK(mask_token >= 0, "vqw_mask_tokens: mask_token=%ld must not be negative", mask_token);
    VQW_CHECK(ratio == 0.0 || (ratio > 0.0 && ratio <= 1.0), "vqw_mask_tokens: ratio=%g must lie in (0, 1], or be 0 for the cosine schedule", ratio);
    VQW_CHECK(ids && inp && masked && n, "vqw_mask_tokens: null pointer");
    VQW_CHECK(al8(ids) && al8(inp) && al4(n), "vqw_mask_tokens: ids and inp must be 8-byte, n 4-byte aligned");
    hipLaunchKernelGGL(k_mask_tokens, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, inp, masked, n, T, mask_token, ratio,
                       dk_make(0.f, seed, call, MASK_RATIO_SITE), dk_make(0.f, seed, call, MASK_KEY_SITE));
    VQW_LAUNCH_CHECK("vqw_mask_tokens");
    return VQW_OK;
}

extern "C" int vqw_unmask_step(const long* tokens, const float* logp, const uint8_t* masked, const float* u, const int* m0, long* ids_out,
                               uint8_t* masked_out, float* fixed_logp, float* conf, int B, int T, double gamma, float tau, long mask_token,
                               void* stream) {
    if (int rc = rows_check("vqw_unmask_step", B, T)) return rc;
    VQW_CHECK(mask_token >= 0, "vqw_unmask_step: mask_token=%ld must not be negative", mask_token);
    VQW_CHECK(isfinite(gamma), "vqw_unmask_step: gamma=%g must be finite", gamma);
    VQW_CHECK(isfinite(tau) && tau >= 0.f, "vqw_unmask_step: tau=%g must be finite and not negative", (double)tau);
    VQW_CHECK(tokens && logp && masked && m0 && ids_out && masked_out && fixed_logp,
              "vqw_unmask_step: null pointer (only u, with tau = 0, and conf may be null)");
    VQW_CHECK(u || tau == 0.f, "vqw_unmask_step: u is null with tau=%g; only tau = 0 reads no uniforms", (double)tau);
    VQW_CHECK(al8(tokens) && al8(ids_out) && al4(logp) && al4(u) && al4(m0) && al4(fixed_logp) && al4(conf),
              "vqw_unmask_step: tokens and ids_out must be 8-byte, the fp32 and int32 tensors 4-byte aligned");
    VQW_CHECK((const void*)masked != (const void*)masked_out && (const void*)tokens != (const void*)ids_out,
              "vqw_unmask_step: masked_out and ids_out must not alias masked and tokens (a pass reads what another has written)");
    hipLaunchKernelGGL(k_unmask_step, dim3(B), dim3(256), 0, (hipStream_t)stream, tokens, logp, masked, u, m0, ids_out, masked_out,
                       fixed_logp, conf, T, gamma, tau, mask_token);
    VQW_LAUNCH_CHECK("vqw_unmask_step");
    return VQW_OK;
}
