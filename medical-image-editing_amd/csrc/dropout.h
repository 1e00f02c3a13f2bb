// Counter-based dropout masks: whether an element is kept is a pure integer function of (seed, call, site, element index),
// computed in registers where the mask is used and never written to memory.  Integer arithmetic only (all of it modulo 2^32 or
// 2^64), so tests/dropout_ref.py restates it in numpy bit for bit.  Shared by dropout.hip and the causal kernels of attention.hip.
//
//   key     (seed, call, site) -> two 32-bit words: three splitmix64 steps on the host, once per launch.
//             z = sm(sm(sm(seed) ^ call) ^ site),  sm(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
//             x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^= x >> 31;      k0 = low word of z, k1 = high word
//   index   64 bits, as (hi, lo).  Element-wise sites: the linear index into the dense tensor, hi = index >> 32.  Attention:
//           hi = (b n_head + h) Tq + i, lo = j - the logical position of the probability, nothing of tiles, waves or lanes
//           (B n_head <= 65535 and Tq <= 65536 keep hi below 2^32).
//   row     hi -> two words, once per row of 2^32 elements (a query row of the attention; a thread or an LDS slot holds them):
//             r0 = mix(hi ^ k0), r1 = mix(r0 ^ k1),  mix = lowbias32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
//             x ^= x >> 16
//   draw    (r0, r1, lo) -> r, a two-round multiply-xorshift mix with a row word entering each round:
//             x = (lo ^ r0) * 0x7feb352d;  x ^= x >> 15;  x = (x ^ r1) * 0x846ca68b;  r = x ^ x >> 16
//           Two rows whose r0 are close hold the same first-round values in permuted order; the second word separates them.
//   keep    r >= threshold, threshold = round-to-even(p 2^32) of the float32 p in double: the full 32 bits, no coarser quantisation
//           of p (p < 1 in float32 keeps it below 2^32).  scale = float32(1 / (1 - p)), the quotient in double, rounded once.
//
// Cost per element where the mask is used, as compiled for gfx950: v_xor, v_mul_lo_u32, v_lshrrev, v_xor, v_xor, v_mul_lo_u32,
// v_xor (SDWA: the shift by 16 is a word select), v_cmp, v_cndmask - nine vector instructions, two of them the quarter-rate
// 32-bit multiplies - plus the multiply by the scale.  A Philox4x32 round is two 32 x 32 -> 64 multiplies (four quarter-rate instructions) and delivers four draws only
// to a thread that owns four elements of one counter; the attention's element-wise stage owns columns 8 apart, and the two tile
// orientations would have to agree on the grouping.  It was not built.
#pragma once
#include <stdint.h>
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

struct DropKey {
    uint32_t k0, k1, thr;
    float scale;
};

static inline uint64_t dk_sm64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// host side, once per launch; p in [0, 1) is the caller's to check
static inline DropKey dk_make(float p, long seed, long call, int site) {
    const uint64_t z = dk_sm64(dk_sm64(dk_sm64((uint64_t)seed) ^ (uint64_t)call) ^ (uint64_t)(int64_t)site);
    DropKey k;
    k.k0 = (uint32_t)z;
    k.k1 = (uint32_t)(z >> 32);
    k.thr = (uint32_t)llrint((double)p * 4294967296.0);
    k.scale = (float)(1.0 / (1.0 - (double)p));
    return k;
}

__host__ __device__ static inline uint32_t dk_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    return x ^ (x >> 16);
}
__host__ __device__ static inline void dk_row(const DropKey& k, uint32_t hi, uint32_t& r0, uint32_t& r1) {
    r0 = dk_mix(hi ^ k.k0);
    r1 = dk_mix(r0 ^ k.k1);
}
__host__ __device__ static inline uint32_t dk_draw(uint32_t r0, uint32_t r1, uint32_t lo) {
    uint32_t x = (lo ^ r0) * 0x7feb352du;
    x ^= x >> 15;
    x = (x ^ r1) * 0x846ca68bu;
    return x ^ (x >> 16);
}
__host__ __device__ static inline bool dk_keep_row(const DropKey& k, uint32_t r0, uint32_t r1, uint32_t lo) { return dk_draw(r0, r1, lo) >= k.thr; }
// keep(key, index): the whole function, for a 64-bit element index
__host__ __device__ static inline bool dk_keep(const DropKey& k, uint64_t index) {
    uint32_t r0, r1;
    dk_row(k, (uint32_t)(index >> 32), r0, r1);
    return dk_keep_row(k, r0, r1, (uint32_t)index);
}
// the attention's index of probability (bh, i, j) of a (.., Tq, Tk) score matrix: hi of query row i of head bh; lo = j
__host__ __device__ static inline uint32_t dk_attn_hi(uint32_t bh, uint32_t Tq, uint32_t i) { return bh * Tq + i; }
