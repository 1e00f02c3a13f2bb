// Device helpers shared by the MFMA convolution kernels (conv_mfma.hip, conv_halo.hip, conv_dil.hip, conv_wino*.hip).
#pragma once
#include "common.h"

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// Bijective XCD-aware remap: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a contiguous run
// of tiles (neighbouring pixel tiles share halo rows and all N tiles of a pixel tile share the A operand in L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    int q = nwg >> 3, r = nwg & 7;
    int xcd = bid & 7, idx = bid >> 3;
    int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// Raw buffer loads: 32-bit byte offsets against a wave-uniform descriptor; an offset >= num_records returns 0 in
// hardware, which is the conv zero padding / tile masking for free (no exec-mask branches, no 64-bit address math).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, unsigned nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, nbytes, 0x00020000);
}
// (soff: a wave-uniform byte offset added after the range check of byte_off)
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, unsigned soff = 0) {
    u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, (int)soff, 0);
    float4 f;     // (index, then convert: __builtin_bit_cast on a vector element mis-reads element 0 with this clang)
    unsigned a = v[0], b = v[1], c = v[2], d = v[3];
    f.x = __uint_as_float(a); f.y = __uint_as_float(b); f.z = __uint_as_float(c); f.w = __uint_as_float(d);
    return f;
}

__device__ __forceinline__ void buf_st4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, float4 f) {
    u32x4 v;
    v[0] = __float_as_uint(f.x); v[1] = __float_as_uint(f.y); v[2] = __float_as_uint(f.z); v[3] = __float_as_uint(f.w);
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)byte_off, 0, 0);
}

// A value the compiler cannot see through: LDS base addresses kept in registers of their own (no ds_read2 merging, no
// re-derivation from a common base inside an MFMA loop).
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }
// Its float twin: a constant (+1, -1, a wave's sign) held in a VGPR the compiler cannot see through.  The Winograd transforms
// write their add / sub as fma with such a constant: x + 1 * y and x - 1 * y round exactly like the add / sub they stand
// for, but the vector combiner cannot pair them into v_pk_add_f32 over the two channels of a ds_read_b64 (which holds the
// vector issue port 2-3 times as long beside MFMAs: 10-15 matrix-pipe cycles instead of 2 x 4.4), an SGPR operand would cost
// 1.5 x, and - unlike v_add / v_sub written in inline asm - the fma is an ordinary instruction to the compiler's hazard
// recogniser (a VALU write inside inline asm followed closely by the MFMA that reads it gave a stale operand in the
// weight-gradient kernel of conv_wino.hip).  The v_mov is the whole asm: nothing that feeds an MFMA is computed in it.
__device__ __forceinline__ float opaque_f(float x) { float r; asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }

// Walk over the regions of a tensor in the order (image, region column, region row): the cursor of region number sp, and its
// successor.  tilesY / tilesX = regions per image column / row.
__device__ __forceinline__ void region_start(int sp, int tilesY, int tilesX, int& n, int& tx, int& ty) {
    const int per_img = tilesY * tilesX;
    n = sp / per_img;
    const int rem = sp - n * per_img;
    tx = rem / tilesY;
    ty = rem - tx * tilesY;
}
// (step = 0 / 1: stay / move on - selects, no branch: see sel_u32)
__device__ __forceinline__ void region_step(int step, int tilesY, int tilesX, int& n, int& tx, int& ty) {
    const int ty1 = ty + step, wy = ty1 == tilesY ? 1 : 0;
    ty = wy ? 0 : ty1;
    const int tx1 = tx + wy, wx = tx1 == tilesX ? 1 : 0;
    tx = wx ? 0 : tx1;
    n += wx;
}
__device__ __forceinline__ void region_next(int tilesY, int tilesX, int& n, int& tx, int& ty) { region_step(1, tilesY, tilesX, n, tx, ty); }

// A select between two values that are both evaluated.  Written as `c ? f(x) : k` the address arithmetic of f lands in
// an exec-masked block of its own; basic-block boundaries inside an MFMA loop keep the scheduler from spreading the
// prefetch / store instructions between the MFMAs (they end up in one run during which the matrix pipe idles).
__device__ __forceinline__ unsigned sel_u32(bool c, unsigned a, unsigned b) { return c ? a : b; }

// Per-tile statistics the conv epilogues leave for the following normalisation: (sum, M2) with M2 = sum (x - tile mean)^2,
// merged pairwise (Chan et al.) so that no fp32 quantity ever holds sum(x^2): var = E[x^2] - mean^2 from fp32 sums loses
// (mean / sigma)^2 * 6e-8 - 3e-4 of the output on a plane that sits 60 sigma off zero (profiles/r02_stats_precision.txt).
// lane_stats: m values held by one lane.  stat_merge_eq: two groups of n elements EACH (inv2n = 1 / (2 n)).
// stat_merge: groups of na and nb elements.
template <int M>
__device__ __forceinline__ void lane_stats(const float* v, float& s, float& m2) {
    s = 0.f;
#pragma unroll
    for (int i = 0; i < M; ++i) s += v[i];
    const float mean = s * (1.f / M);
    m2 = 0.f;
#pragma unroll
    for (int i = 0; i < M; ++i) { const float d = v[i] - mean; m2 = fmaf(d, d, m2); }
}
__device__ __forceinline__ void stat_merge_eq(float& s, float& m2, float so, float m2o, float inv2n) {
    const float d = so - s;
    m2 = (m2 + m2o) + d * d * inv2n;
    s += so;
}
__device__ __forceinline__ void stat_merge(float& s, float& m2, float na, float so, float m2o, float nb) {
    const float d = so / nb - s / na;
    m2 = (m2 + m2o) + d * d * (na * nb / (na + nb));
    s += so;
}
