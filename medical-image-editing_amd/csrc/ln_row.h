// LayerNorm forward of ONE row by ONE wave: the body of vqw_layernorm_fwd's kernel (mingpt.hip), shared with the kernels that
// normalise a row they pick themselves (pseudo_nll.hip gathers it from another tensor).  Lane l holds the float4 columns l,
// l + 64, ... of the row in registers, the row is read once; gpt_math.h's steps under three fixed butterflies.  One body, so every
// caller gets the same bits for the same row.
#pragma once
#include "common.h"
#include "gpt_math.h"

__device__ __forceinline__ float4 ln_ld(const float* p, int c4, int C4) {
    return c4 < C4 ? *(const float4*)(p + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// xr, yr: the row read and the row written ([C] floats each, 16-byte aligned); every lane of the wave calls it; mu and rs (the
// mean and 1 / sqrt(var + eps)) come back in every lane.  NV: the float4 columns a lane holds, C <= 256 NV.
template <int NV>
__device__ __forceinline__ void ln_row_fwd(const float* __restrict__ xr, const float* __restrict__ gamma, const float* __restrict__ beta,
                                           float* __restrict__ yr, int lane, int C, float eps, float& mu, float& rs) {
    const int C4 = C >> 2;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { v[i] = ln_ld(xr, lane + 64 * i, C4); s += sum4(v[i]); }
    const float mu0 = wave_sum_f(s) / (float)C;
    float s0 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < C4) { ln_centre(v[i], mu0); s0 += sum4(v[i]); }
    }
    const float delta = wave_sum_f(s0) / (float)C;
    mu = mu0 + delta;
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < C4) { ln_centre(v[i], delta); m2 = ln_m2(v[i], m2); }
    }
    rs = 1.f / sqrtf(wave_sum_f(m2) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) *(float4*)(yr + 4 * c4) = ln_affine(v[i], rs, *(const float4*)(gamma + 4 * c4), *(const float4*)(beta + 4 * c4));
    }
}
