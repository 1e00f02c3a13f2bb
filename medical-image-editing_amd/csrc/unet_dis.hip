// U-Net discriminator of the second training step (reference: networks/unet_discriminator.py:386-627, its BigGAN blocks
// networks/biggan/layers.py:416-506, the step trainers/single_window_trainer.py:264-432).  The 3x3 / 1x1 convolutions are the
// operators of conv.hip; this file holds what sits between them.  NHWC fp32.
//
//   down-block tail   out = avgpool2(a) (+ s)            s: the 1x1 shortcut, run on the pooled block input (it commutes with
//                     relu_out = relu(out)               the pool)
//   up-block tail     out = h + up2x(s)                  s: the 1x1 shortcut at the low resolution (it commutes with nearest x2)
//                     cat[.., c] = relu(out), cat[.., C + c'] = relu(res), channel stride C + Cr: the rectified concat
//                     buffer that the NEXT up block's collapsed up-sampled 3x3 reads as a single source
//   bottleneck head   bottleneck[n] = bias + sum_c w[c] * sum_p relu(h[n, p, c])
//   CutMix select     image outside the rectangle, recon inside (swapped when `flip`)
//   losses            hinge (maps and bottlenecks), CutMix hinge, consistency MSE in one pass; the mask is the rectangle
//
// Reductions: thread-strided double partials in a fixed order, wave butterfly, wave totals added in order, per-workgroup
// partials summed in order by one workgroup - the same bits every run, no atomics.  A tail moves each element once: a thread
// owns one pooled / low-resolution pixel and 1 or 4 channels (float4 when every channel count is a multiple of 4 and the
// tensors are 16-byte aligned).
#include "common.h"
#include "../../include/vqwnet_hip.h"

namespace {

template <int V> struct Vec { float v[V]; };
template <int V> __device__ __forceinline__ Vec<V> ld(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void st(float* p, const Vec<V>& r) {
    if constexpr (V == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

__device__ __forceinline__ double block_sum_d(double v, double* sm) {      // 256 threads; every thread gets the total
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// ---- down-block tail ------------------------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) k_dtail_fwd(const float* __restrict__ a, const float* __restrict__ s, float* __restrict__ out,
                                                   float* __restrict__ relu_out, long total, int Ho, int Wo, int C) {
    const int CV = C / V, W = 2 * Wo;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const int c = (int)(i % CV) * V;
        const long p = i / CV;
        const int xo = (int)(p % Wo);
        const long q = p / Wo;                                   // n * Ho + yo
        const long base = ((2 * q) * W + 2 * xo) * C + c;        // (n * H + 2 yo) * W + 2 xo, H = 2 Ho
        const long rowC = (long)W * C;
        const Vec<V> t0 = ld<V>(a + base), t1 = ld<V>(a + base + C), t2 = ld<V>(a + base + rowC), t3 = ld<V>(a + base + rowC + C);
        Vec<V> o, r;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = 0.25f * ((t0.v[k] + t1.v[k]) + (t2.v[k] + t3.v[k]));
        if (s) {
            const Vec<V> sv = ld<V>(s + p * C + c);
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] += sv.v[k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = fmaxf(o.v[k], 0.f);
        if (out) st<V>(out + p * C + c, o);
        if (relu_out) st<V>(relu_out + p * C + c, r);
    }
}

template <int V>
__global__ void __launch_bounds__(256) k_dtail_bwd(const float* __restrict__ relu_out, const float* __restrict__ g_out,
                                                   const float* __restrict__ g_relu, float* __restrict__ g_full,
                                                   float* __restrict__ g_low, long total, int Ho, int Wo, int C) {
    const int CV = C / V, W = 2 * Wo;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const int c = (int)(i % CV) * V;
        const long p = i / CV;
        const int xo = (int)(p % Wo);
        const long q = p / Wo;
        Vec<V> g;
#pragma unroll
        for (int k = 0; k < V; ++k) g.v[k] = 0.f;
        if (g_out) g = ld<V>(g_out + p * C + c);
        if (g_relu) {
            const Vec<V> m = ld<V>(relu_out + p * C + c), gr = ld<V>(g_relu + p * C + c);
#pragma unroll
            for (int k = 0; k < V; ++k) g.v[k] += m.v[k] > 0.f ? gr.v[k] : 0.f;
        }
        if (g_low) st<V>(g_low + p * C + c, g);
        if (g_full) {
#pragma unroll
            for (int k = 0; k < V; ++k) g.v[k] *= 0.25f;
            const long base = ((2 * q) * W + 2 * xo) * C + c, rowC = (long)W * C;
            st<V>(g_full + base, g);
            st<V>(g_full + base + C, g);
            st<V>(g_full + base + rowC, g);
            st<V>(g_full + base + rowC + C, g);
        }
    }
}

// ---- up-block tail: a thread owns (full-resolution pixel, channel group) of the C block channels or the Cr residual ones -------
template <int V>
__global__ void __launch_bounds__(256) k_utail_fwd(const float* __restrict__ h, const float* __restrict__ s, const float* __restrict__ res,
                                                   float* __restrict__ out, float* __restrict__ cat, long total, int H, int W, int C,
                                                   int Cr) {
    const int CV = C / V, G = CV + Cr / V, Wl = W / 2, Hl = H / 2, ld_r = C + Cr;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const int g = (int)(i % G);
        const long p = i / G;
        if (g < CV) {
            const int c = g * V;
            const int x = (int)(p % W);
            const long q = p / W;
            const int y = (int)(q % H);
            const long n = q / H;
            const long pl = (n * Hl + (y >> 1)) * Wl + (x >> 1);
            Vec<V> o = ld<V>(h + p * C + c);
            const Vec<V> sv = ld<V>(s + pl * C + c);
            Vec<V> r;
#pragma unroll
            for (int k = 0; k < V; ++k) { o.v[k] += sv.v[k]; r.v[k] = fmaxf(o.v[k], 0.f); }
            if (out) st<V>(out + p * C + c, o);
            if (cat) st<V>(cat + p * ld_r + c, r);
        } else {
            const int c = (g - CV) * V;
            Vec<V> r = ld<V>(res + p * Cr + c);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = fmaxf(r.v[k], 0.f);
            st<V>(cat + p * ld_r + C + c, r);
        }
    }
}

// a thread owns (low-resolution pixel, channel group): the four positions of its 2x2 window
template <int V>
__global__ void __launch_bounds__(256) k_utail_bwd(const float* __restrict__ cat, const float* __restrict__ g_out, const float* __restrict__ g_cat,
                                                   float* __restrict__ g_h, float* __restrict__ g_s, float* __restrict__ g_res, long total,
                                                   int Hl, int Wl, int C, int Cr) {
    const int CV = C / V, G = CV + (g_res ? Cr / V : 0), W = 2 * Wl, ld_r = C + Cr;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const int gi = (int)(i % G);
        const long pl = i / G;
        const int xl = (int)(pl % Wl);
        const long q = pl / Wl;                                  // n * Hl + yl
        const long p00 = (2 * q) * W + 2 * xl;
        const long pf[4] = {p00, p00 + 1, p00 + W, p00 + W + 1};
        if (gi < CV) {
            const int c = gi * V;
            Vec<V> sum;
#pragma unroll
            for (int k = 0; k < V; ++k) sum.v[k] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Vec<V> g;
#pragma unroll
                for (int k = 0; k < V; ++k) g.v[k] = 0.f;
                if (g_out) g = ld<V>(g_out + pf[j] * C + c);
                if (g_cat) {
                    const Vec<V> m = ld<V>(cat + pf[j] * ld_r + c), gr = ld<V>(g_cat + pf[j] * ld_r + c);
#pragma unroll
                    for (int k = 0; k < V; ++k) g.v[k] += m.v[k] > 0.f ? gr.v[k] : 0.f;
                }
                st<V>(g_h + pf[j] * C + c, g);
#pragma unroll
                for (int k = 0; k < V; ++k) sum.v[k] += g.v[k];
            }
            st<V>(g_s + pl * C + c, sum);
        } else {
            const int c = (gi - CV) * V;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Vec<V> m = ld<V>(cat + pf[j] * ld_r + C + c), gr = ld<V>(g_cat + pf[j] * ld_r + C + c);
                Vec<V> g;
#pragma unroll
                for (int k = 0; k < V; ++k) g.v[k] = m.v[k] > 0.f ? gr.v[k] : 0.f;
                st<V>(g_res + pf[j] * Cr + c, g);
            }
        }
    }
}

// ---- bottleneck head --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bottleneck_fwd(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ y, int HW, int C) {
    __shared__ double sm[4];
    const float* hn = h + (long)blockIdx.x * HW * C;
    double a = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        float sp = 0.f;
        for (int p = 0; p < HW; ++p) sp += fmaxf(hn[(long)p * C + c], 0.f);
        a += (double)w[c] * (double)sp;
    }
    a = block_sum_d(a, sm);
    if (threadIdx.x == 0) y[blockIdx.x] = (float)(a + (bias ? (double)bias[0] : 0.0));
}
// thread = channel: g_h for every (n, p), g_w[c] = sum_n g[n] * sum_p relu(h); block 0 / thread 0 also sums g_bias
__global__ void __launch_bounds__(256) k_bottleneck_bwd(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ gy,
                                                  float* __restrict__ g_h, float* __restrict__ g_w, float* __restrict__ g_bias, int N,
                                                  int HW, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        const float wc = w[c];
        double gw = 0.0;
        for (int n = 0; n < N; ++n) {
            const float g = gy[n];
            float sp = 0.f;
            for (int p = 0; p < HW; ++p) {
                const long e = ((long)n * HW + p) * C + c;
                const float v = h[e];
                sp += fmaxf(v, 0.f);
                if (g_h) g_h[e] = v > 0.f ? g * wc : 0.f;
            }
            gw += (double)g * (double)sp;
        }
        if (g_w) g_w[c] = (float)gw;
    }
    if (g_bias && blockIdx.x == 0 && threadIdx.x == 0) {
        double gb = 0.0;
        for (int n = 0; n < N; ++n) gb += (double)gy[n];
        g_bias[0] = (float)gb;
    }
}

// ---- CutMix ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool takes_source(int y, int x, int y0, int y1, int x0, int x1, int flip) {
    const bool inside = y >= y0 && y < y1 && x >= x0 && x < x1;         // mask = 0 inside, 1 outside; flip: 1 - mask
    return inside == (flip != 0);                                       // mask == 1: the source (image / real map)
}

__global__ void __launch_bounds__(256) k_cutmix_select(const float* __restrict__ image, const float* __restrict__ recon,
                                                       float* __restrict__ out, long total, int H, int W, int C, int y0, int y1, int x0,
                                                       int x1, int flip) {
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gstride) {
        const long p = i / C;
        const int x = (int)(p % W), y = (int)((p / W) % H);
        out[i] = takes_source(y, x, y0, y1, x0, x1, flip) ? image[i] : recon[i];
    }
}

constexpr int LOSS_BLOCKS = 256;       // partials per sum

// part[blockIdx][4]: sum relu(1 - r), sum relu(1 + f), sum relu(1 - (2m - 1) c), sum (c - (m r + (1 - m) f))^2
__global__ void __launch_bounds__(256) k_dis_losses_part(const float* __restrict__ r, const float* __restrict__ f, const float* __restrict__ cm,
                                                         double* __restrict__ part, long n, int H, int W, int y0, int y1, int x0, int x1,
                                                         int flip) {
    __shared__ double sm[4];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const long gstride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += gstride) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const bool src = takes_source(y, x, y0, y1, x0, x1, flip);
        const float rv = r[i], fv = f[i], cv = cm[i];
        a0 += (double)fmaxf(1.f - rv, 0.f);
        a1 += (double)fmaxf(1.f + fv, 0.f);
        a2 += (double)fmaxf(src ? 1.f - cv : 1.f + cv, 0.f);
        const float d = cv - (src ? rv : fv);
        a3 += (double)d * (double)d;
    }
    a0 = block_sum_d(a0, sm);
    a1 = block_sum_d(a1, sm);
    a2 = block_sum_d(a2, sm);
    a3 = block_sum_d(a3, sm);
    if (threadIdx.x == 0) {
        double* o = part + 4 * (long)blockIdx.x;
        o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
    }
}
__global__ void __launch_bounds__(256) k_dis_losses_final(const double* __restrict__ part, int nblocks, const float* __restrict__ rb,
                                                          const float* __restrict__ fb, const float* __restrict__ cb, int B, long n,
                                                          float* __restrict__ l_dis, float* __restrict__ l_cutmix, float* __restrict__ l_cons) {
    __shared__ double sm[4];
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += 256)
        for (int k = 0; k < 4; ++k) a[k] += part[4 * (long)i + k];
    for (int i = threadIdx.x; i < B; i += 256) {
        b[0] += (double)fmaxf(1.f - rb[i], 0.f);
        b[1] += (double)fmaxf(1.f + fb[i], 0.f);
        b[2] += (double)fmaxf(1.f + cb[i], 0.f);
    }
    for (int k = 0; k < 4; ++k) a[k] = block_sum_d(a[k], sm);
    for (int k = 0; k < 3; ++k) b[k] = block_sum_d(b[k], sm);
    if (threadIdx.x == 0) {
        const double dn = (double)n, dB = (double)B;
        l_dis[0] = (float)(0.5 * (a[0] / dn + a[1] / dn) + 0.5 * (b[0] / dB + b[1] / dB));
        l_cutmix[0] = (float)(b[2] / dB + a[2] / dn);
        l_cons[0] = (float)(a[3] / dn);
    }
}
// gd, gm, gk: dL / d(l_dis, l_cutmix, l_consistency), device scalars (NULL = 0)
__global__ void __launch_bounds__(256) k_dis_losses_bwd(const float* __restrict__ r, const float* __restrict__ f, const float* __restrict__ cm,
                                                        const float* __restrict__ rb, const float* __restrict__ fb, const float* __restrict__ cb,
                                                        const float* __restrict__ gd_, const float* __restrict__ gm_, const float* __restrict__ gk_,
                                                        float* __restrict__ g_r, float* __restrict__ g_f, float* __restrict__ g_c,
                                                        float* __restrict__ g_rb, float* __restrict__ g_fb, float* __restrict__ g_cb, long n, int B,
                                                        int H, int W, int y0, int y1, int x0, int x1, int flip) {
    const float gd = gd_ ? gd_[0] : 0.f, gm = gm_ ? gm_[0] : 0.f, gk = gk_ ? gk_[0] : 0.f;
    const float hd = 0.5f * gd / (float)n, hm = gm / (float)n, hk = 2.f * gk / (float)n;
    const long gstride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += gstride) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const bool src = takes_source(y, x, y0, y1, x0, x1, flip);
        const float rv = r[i], fv = f[i], cv = cm[i];
        const float dk = hk * (cv - (src ? rv : fv));
        g_r[i] = (1.f - rv > 0.f ? -hd : 0.f) - (src ? dk : 0.f);
        g_f[i] = (1.f + fv > 0.f ? hd : 0.f) - (src ? 0.f : dk);
        g_c[i] = (src ? (1.f - cv > 0.f ? -hm : 0.f) : (1.f + cv > 0.f ? hm : 0.f)) + dk;
    }
    if (blockIdx.x == 0) {
        const float bd = 0.5f * gd / (float)B, bm = gm / (float)B;
        for (int i = threadIdx.x; i < B; i += 256) {
            g_rb[i] = 1.f - rb[i] > 0.f ? -bd : 0.f;
            g_fb[i] = 1.f + fb[i] > 0.f ? bd : 0.f;
            g_cb[i] = 1.f + cb[i] > 0.f ? bm : 0.f;
        }
    }
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
int loss_blocks(long n) {
    long b = (n + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > LOSS_BLOCKS ? LOSS_BLOCKS : b));
}
bool rect_ok(int H, int W, int y0, int y1, int x0, int x1) { return 0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W; }

}  // namespace

extern "C" int vqw_unet_dtail_fwd(const float* a, const float* s_low, float* out, float* relu_out, int N, int H, int W, int C,
                                  void* stream) {
    VQW_CHECK(a && (out || relu_out) && N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0,
              "vqw_unet_dtail_fwd: bad arguments (N=%d H=%d W=%d C=%d; H, W even)", N, H, W, C);
    const bool v4 = C % 4 == 0 && aligned16(a) && aligned16(s_low) && aligned16(out) && aligned16(relu_out);
    const long total = (long)N * (H / 2) * (W / 2) * (v4 ? C / 4 : C);
    hipStream_t st = (hipStream_t)stream;
    if (v4) k_dtail_fwd<4><<<stream_grid(total, 256), 256, 0, st>>>(a, s_low, out, relu_out, total, H / 2, W / 2, C);
    else k_dtail_fwd<1><<<stream_grid(total, 256), 256, 0, st>>>(a, s_low, out, relu_out, total, H / 2, W / 2, C);
    VQW_LAUNCH_CHECK("vqw_unet_dtail_fwd");
    return VQW_OK;
}

extern "C" int vqw_unet_dtail_bwd(const float* relu_out, const float* g_out, const float* g_relu, float* g_full, float* g_low, int N,
                                  int H, int W, int C, void* stream) {
    VQW_CHECK((g_out || g_relu) && (g_full || g_low) && (!g_relu || relu_out) && N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 &&
                  W % 2 == 0,
              "vqw_unet_dtail_bwd: bad arguments (N=%d H=%d W=%d C=%d; H, W even; g_relu needs relu_out)", N, H, W, C);
    const bool v4 = C % 4 == 0 && aligned16(g_out) && aligned16(g_full) && aligned16(g_low) && aligned16(relu_out) && aligned16(g_relu);
    const long total = (long)N * (H / 2) * (W / 2) * (v4 ? C / 4 : C);
    hipStream_t st = (hipStream_t)stream;
    if (v4) k_dtail_bwd<4><<<stream_grid(total, 256), 256, 0, st>>>(relu_out, g_out, g_relu, g_full, g_low, total, H / 2, W / 2, C);
    else k_dtail_bwd<1><<<stream_grid(total, 256), 256, 0, st>>>(relu_out, g_out, g_relu, g_full, g_low, total, H / 2, W / 2, C);
    VQW_LAUNCH_CHECK("vqw_unet_dtail_bwd");
    return VQW_OK;
}

extern "C" int vqw_unet_utail_fwd(const float* h, const float* s_low, const float* res, float* out, float* cat, int N, int H, int W,
                                  int C, int Cr, void* stream) {
    VQW_CHECK(h && s_low && (out || cat) && (Cr == 0 || (res && cat)) && N > 0 && H > 0 && W > 0 && C > 0 && Cr >= 0 && H % 2 == 0 &&
                  W % 2 == 0,
              "vqw_unet_utail_fwd: bad arguments (N=%d H=%d W=%d C=%d Cr=%d; H, W even; a residual needs cat)", N, H, W, C, Cr);
    const bool v4 = C % 4 == 0 && Cr % 4 == 0 && aligned16(h) && aligned16(s_low) && aligned16(res) && aligned16(out) && aligned16(cat);
    const int V = v4 ? 4 : 1;
    const long total = (long)N * H * W * (C / V + Cr / V);
    hipStream_t st = (hipStream_t)stream;
    if (v4) k_utail_fwd<4><<<stream_grid(total, 256), 256, 0, st>>>(h, s_low, res, out, cat, total, H, W, C, Cr);
    else k_utail_fwd<1><<<stream_grid(total, 256), 256, 0, st>>>(h, s_low, res, out, cat, total, H, W, C, Cr);
    VQW_LAUNCH_CHECK("vqw_unet_utail_fwd");
    return VQW_OK;
}

extern "C" int vqw_unet_utail_bwd(const float* cat, const float* g_out, const float* g_cat, float* g_h, float* g_s_low, float* g_res,
                                  int N, int H, int W, int C, int Cr, void* stream) {
    VQW_CHECK((g_out || g_cat) && g_h && g_s_low && (!g_cat || cat) && (!g_res || (g_cat && Cr > 0)) && N > 0 && H > 0 && W > 0 &&
                  C > 0 && Cr >= 0 && H % 2 == 0 && W % 2 == 0,
              "vqw_unet_utail_bwd: bad arguments (N=%d H=%d W=%d C=%d Cr=%d; H, W even; g_res needs g_cat)", N, H, W, C, Cr);
    const bool v4 = C % 4 == 0 && Cr % 4 == 0 && aligned16(g_out) && aligned16(g_h) && aligned16(g_s_low) && aligned16(g_res) &&
                    aligned16(cat) && aligned16(g_cat);
    const int V = v4 ? 4 : 1;
    const long total = (long)N * (H / 2) * (W / 2) * (C / V + (g_res ? Cr / V : 0));
    hipStream_t st = (hipStream_t)stream;
    if (v4) k_utail_bwd<4><<<stream_grid(total, 256), 256, 0, st>>>(cat, g_out, g_cat, g_h, g_s_low, g_res, total, H / 2, W / 2, C, Cr);
    else k_utail_bwd<1><<<stream_grid(total, 256), 256, 0, st>>>(cat, g_out, g_cat, g_h, g_s_low, g_res, total, H / 2, W / 2, C, Cr);
    VQW_LAUNCH_CHECK("vqw_unet_utail_bwd");
    return VQW_OK;
}

extern "C" int vqw_unet_head_fwd(const float* h, const float* w, const float* bias, float* y, int N, int HW, int C, void* stream) {
    VQW_CHECK(h && w && y && N > 0 && HW > 0 && C > 0, "vqw_unet_head_fwd: bad arguments");
    k_bottleneck_fwd<<<N, 256, 0, (hipStream_t)stream>>>(h, w, bias, y, HW, C);
    VQW_LAUNCH_CHECK("vqw_unet_head_fwd");
    return VQW_OK;
}

extern "C" int vqw_unet_head_bwd(const float* h, const float* w, const float* gy, float* g_h, float* g_w, float* g_bias, int N, int HW,
                                 int C, void* stream) {
    VQW_CHECK(h && w && gy && (g_h || g_w || g_bias) && N > 0 && HW > 0 && C > 0, "vqw_unet_head_bwd: bad arguments");
    k_bottleneck_bwd<<<ceil_div(C, 256), 256, 0, (hipStream_t)stream>>>(h, w, gy, g_h, g_w, g_bias, N, HW, C);
    VQW_LAUNCH_CHECK("vqw_unet_head_bwd");
    return VQW_OK;
}

extern "C" int vqw_cutmix_select(const float* image, const float* recon, float* out, int N, int H, int W, int C, int y0, int y1, int x0,
                                 int x1, int flip, void* stream) {
    VQW_CHECK(image && recon && out && N > 0 && H > 0 && W > 0 && C > 0 && rect_ok(H, W, y0, y1, x0, x1),
              "vqw_cutmix_select: bad arguments (rectangle [%d, %d) x [%d, %d) in %d x %d)", y0, y1, x0, x1, H, W);
    const long total = (long)N * H * W * C;
    k_cutmix_select<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(image, recon, out, total, H, W, C, y0, y1, x0, x1, flip);
    VQW_LAUNCH_CHECK("vqw_cutmix_select");
    return VQW_OK;
}

extern "C" size_t vqw_unet_dis_losses_ws_bytes(long n) { return n > 0 ? (size_t)loss_blocks(n) * 4 * sizeof(double) : 0; }

extern "C" int vqw_unet_dis_losses_fwd(const float* r_map, const float* f_map, const float* c_map, const float* r_bottle,
                                       const float* f_bottle, const float* c_bottle, float* l_dis, float* l_cutmix, float* l_consistency,
                                       void* ws, size_t ws_bytes, int B, int H, int W, int y0, int y1, int x0, int x1, int flip,
                                       void* stream) {
    VQW_CHECK(r_map && f_map && c_map && r_bottle && f_bottle && c_bottle && l_dis && l_cutmix && l_consistency && ws && B > 0 && H > 0 &&
                  W > 0 && rect_ok(H, W, y0, y1, x0, x1),
              "vqw_unet_dis_losses_fwd: bad arguments (rectangle [%d, %d) x [%d, %d) in %d x %d)", y0, y1, x0, x1, H, W);
    const long n = (long)B * H * W;
    VQW_CHECK(ws_bytes >= vqw_unet_dis_losses_ws_bytes(n) && aligned16(ws), "vqw_unet_dis_losses_fwd: workspace too small");
    const int nb = loss_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    k_dis_losses_part<<<nb, 256, 0, st>>>(r_map, f_map, c_map, (double*)ws, n, H, W, y0, y1, x0, x1, flip);
    k_dis_losses_final<<<1, 256, 0, st>>>((const double*)ws, nb, r_bottle, f_bottle, c_bottle, B, n, l_dis, l_cutmix, l_consistency);
    VQW_LAUNCH_CHECK("vqw_unet_dis_losses_fwd");
    return VQW_OK;
}

extern "C" int vqw_unet_dis_losses_bwd(const float* r_map, const float* f_map, const float* c_map, const float* r_bottle,
                                       const float* f_bottle, const float* c_bottle, const float* g_dis, const float* g_cutmix,
                                       const float* g_consistency, float* g_r_map, float* g_f_map, float* g_c_map, float* g_r_bottle,
                                       float* g_f_bottle, float* g_c_bottle, int B, int H, int W, int y0, int y1, int x0, int x1,
                                       int flip, void* stream) {
    VQW_CHECK(r_map && f_map && c_map && r_bottle && f_bottle && c_bottle && g_r_map && g_f_map && g_c_map && g_r_bottle && g_f_bottle &&
                  g_c_bottle && B > 0 && H > 0 && W > 0 && rect_ok(H, W, y0, y1, x0, x1),
              "vqw_unet_dis_losses_bwd: bad arguments (rectangle [%d, %d) x [%d, %d) in %d x %d)", y0, y1, x0, x1, H, W);
    const long n = (long)B * H * W;
    k_dis_losses_bwd<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, g_dis, g_cutmix,
                                                                            g_consistency, g_r_map, g_f_map, g_c_map, g_r_bottle, g_f_bottle,
                                                                            g_c_bottle, n, B, H, W, y0, y1, x0, x1, flip);
    VQW_LAUNCH_CHECK("vqw_unet_dis_losses_bwd");
    return VQW_OK;
}
