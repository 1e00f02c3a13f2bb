// The row math the GPT prior's kernels share (mingpt.hip, gpt_head.hip, gpt_decode.hip): each formula stands here once, every
// kernel keeps its own storage, loop and unrolling around it.  fp32; nothing here adds across lanes.
#pragma once
#include "common.h"

// what a row with an index outside its range is filled with
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// a float4 as a tree: (x + y) + (z + w)
__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// The exact GELU 0.5 x (1 + erf(x / sqrt 2)) and its gradient Phi(x) + x phi(x), with the device erff / expf: the fp32 form passes
// the accuracy gate on every case (within 1.11 of the host's fp32 error) at 2.3 times the speed of an evaluation in double, which
// was measured too.
__device__ __forceinline__ float gelu_y(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_dx(float x, float gy) {
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
    return gy * fmaf(x, pdf, cdf);
}

// the order-preserving integer image of a float: a < b iff key(a) < key(b); -0 and +0 share a key
__device__ __forceinline__ unsigned st_key(float x) {
    if (x == 0.f) x = 0.f;
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// LayerNorm forward of a row of C floats, a float4 at a time; the sums between the steps are the caller's (one fixed butterfly
// each).  mean = mu0 + delta with mu0 = sum(x) / C and delta the mean of x - mu0: on a row that sits far off zero x - mu0 is exact
// and delta carries what the fp32 sum lost, so the centred values do not inherit the rounding of the mean.  The variance comes
// from the centred values (never E[x^2] - mean^2):
//   mu0 = sum(sum4(v)) / C;  ln_centre(v, mu0);  delta = sum(sum4(v)) / C;  ln_centre(v, delta);  m2 = ln_m2(v, m2);
//   rs = 1 / sqrt(sum(m2) / C + eps);  y = ln_affine(v, rs, gamma, beta)
__device__ __forceinline__ void ln_centre(float4& v, float c) { v.x -= c; v.y -= c; v.z -= c; v.w -= c; }
__device__ __forceinline__ float ln_m2(const float4& v, float m2) {
    m2 = fmaf(v.x, v.x, m2); m2 = fmaf(v.y, v.y, m2); m2 = fmaf(v.z, v.z, m2);
    return fmaf(v.w, v.w, m2);
}
__device__ __forceinline__ float4 ln_affine(const float4& v, float rs, const float4& g, const float4& b) {
    return make_float4(fmaf(v.x * rs, g.x, b.x), fmaf(v.y * rs, g.y, b.y), fmaf(v.z * rs, g.z, b.z), fmaf(v.w * rs, g.w, b.w));
}
