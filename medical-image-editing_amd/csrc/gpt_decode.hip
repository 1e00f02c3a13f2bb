// Cached generation for the GPT code prior (networks/gpt.py GPT.decode_step / generate): the kernels of one decode step - one new
// token per batch row behind a preallocated key / value cache - and the host function that launches the whole step from C.  fp32
// in, fp32 out, fp32 accumulation, no float atomics, no scratch: every sum has a fixed order, two runs give the same bits.
//
// Skinny fused linear.  y[m][n] = act(sum_k LN?(x[m])[k] W[n][k] + bias[n]) (+ residual[m][n]) for M rows (the batch of a decode
// step) against a weight [N][K] as nn.Linear stores it.  The kernel is weight-bandwidth-bound: a wave owns one output column n, reads
// row n of W once (a float4 per lane and step, 1 KB per wave and step, coalesced) and uses it for all rows of its row group; a
// workgroup is four waves = four columns.  Rows are tiled in groups of DEC_ROWS (grid.y): the rows of a group sit in LDS as
// [DEC_ROWS][chunk], chunk = min(K, DEC_KC), staged once per workgroup (rows past M as zeros) and read as ds_read_b128 at
// consecutive lanes.  With M <= DEC_ROWS every weight element is read exactly once per launch.  Optional LayerNorm of the input
// row: K <= DEC_KC, so the whole row is in LDS; wave w normalises the rows w, w + 4, ... in place by the steps k_ln_fwd takes on
// registers, gpt_math.h's (the mean plus the mean of the residuals, the variance from the centred values, fixed butterflies).
// The 64 lane partials of a column are folded by one fixed butterfly per row; lane m then owns row m: bias, the exact erf GELU
// (gelu_y), residual, one store.  The output is addressed through up to three column segments (pointer, row stride): one launch over the
// packed [3E][E] weight writes q to a buffer and k, v into row t of the cache planes.
//
// Decode attention.  One query row per (b, head) against the cache rows [0, Tk): one workgroup per (b, head), no mask (the
// layer_past route, mingpt.py:79-80).  Wave w takes the key chunks w, w + 4, ... of DA_CHUNK keys: lane j scores key j (q from LDS
// as a broadcast, its key row as float4s straight to registers), the wave keeps an online softmax (running maximum m, sum l) and
// its lanes, as 64 / (hs / 4) key groups x hs / 4 float4 columns, accumulate p v over the chunk's keys with independent float4 loads.
// The (m, l, acc) partials are merged through LDS in (wave, key group) order.  A lane whose key index is at or beyond Tk issues no
// load: rows past Tk are never read.
//
// The step.  vqw_gpt_decode_step: embedding of idx[b] at position t (vqw_embed_fwd with Ti = 1, t0 = t), per layer ln1 + q|k|v
// (k, v into cache row t), attention over the rows [0, t], proj + residual, ln2 + fc1 + GELU, fc2 + residual, then ln_f + head:
// 2 + 5 n_layer launches, no allocation, no synchronisation, no host read.
#include "common.h"
#include "gpt_math.h"
#include "../../include/vqwnet_hip.h"

// ---------------------------------------------------------------------------------------------------------- skinny fused linear
#define DEC_ROWS 8          // rows of x a workgroup serves: one row group
#define DEC_KC 4096         // floats of a row staged in LDS at a time; the LayerNorm needs the whole row: K <= DEC_KC
#define DEC_MAX_K 16384
#define DEC_WG_COLS 4       // output columns per workgroup: one per wave

// where output column n of row m goes: segment s = n / seg_n, p[s] + m ld[s] + (n - s seg_n)
struct DecOut {
    float* p[3];
    long ld[3];
    int seg_n;
};

static inline int dec_lds_bytes(int K) { return DEC_ROWS * imin(K, DEC_KC) * (int)sizeof(float); }

// grid (ceil(N / DEC_WG_COLS), ceil(M / DEC_ROWS)), 256 threads, dynamic LDS dec_lds_bytes(K)
template <bool LN>
__global__ void __launch_bounds__(256) k_dec_linear(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    const float* __restrict__ residual, DecOut out, int M, int K, int N, int gelu, float eps) {
    extern __shared__ __align__(16) float xs[];          // [DEC_ROWS][kc]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m0 = blockIdx.y * DEC_ROWS, rows = M - m0 < DEC_ROWS ? M - m0 : DEC_ROWS;
    const int n = blockIdx.x * DEC_WG_COLS + wv;
    const int kc = K < DEC_KC ? K : DEC_KC;
    float acc[DEC_ROWS];
#pragma unroll
    for (int m = 0; m < DEC_ROWS; ++m) acc[m] = 0.f;

    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc, kn4 = kn >> 2;          // this chunk's floats / float4s of a row
        __syncthreads();          // the previous chunk's readers are done
        for (int i = threadIdx.x; i < DEC_ROWS * kn4; i += 256) {
            const int m = i / kn4, c4 = i - m * kn4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < rows) v = *(const float4*)(x + (long)(m0 + m) * K + k0 + 4 * c4);
            *(float4*)(xs + m * kc + 4 * c4) = v;
        }
        __syncthreads();
        if (LN) {          // K <= DEC_KC: this is the only chunk and holds whole rows
            for (int m = wv; m < rows; m += 4) {
                float* xr = xs + m * kc;
                float s = 0.f;
                for (int c4 = lane; c4 < kn4; c4 += 64) s += sum4(*(const float4*)(xr + 4 * c4));
                const float mu0 = wave_sum_f(s) / (float)K;
                float s0 = 0.f;
                for (int c4 = lane; c4 < kn4; c4 += 64) {
                    float4 v = *(const float4*)(xr + 4 * c4);
                    ln_centre(v, mu0);
                    s0 += sum4(v);
                }
                const float delta = wave_sum_f(s0) / (float)K;
                float m2 = 0.f;
                for (int c4 = lane; c4 < kn4; c4 += 64) {
                    float4 v = *(const float4*)(xr + 4 * c4);
                    ln_centre(v, mu0); ln_centre(v, delta);
                    m2 = ln_m2(v, m2);
                }
                const float rs = 1.f / sqrtf(wave_sum_f(m2) / (float)K + eps);
                for (int c4 = lane; c4 < kn4; c4 += 64) {          // a lane rewrites only what it read itself
                    float4 v = *(const float4*)(xr + 4 * c4);
                    ln_centre(v, mu0); ln_centre(v, delta);
                    *(float4*)(xr + 4 * c4) = ln_affine(v, rs, *(const float4*)(gamma + 4 * c4), *(const float4*)(beta + 4 * c4));
                }
            }
            __syncthreads();
        }
        if (n < N) {
            const float* wr = W + (long)n * K + k0;
#pragma unroll 2
            for (int c4 = lane; c4 < kn4; c4 += 64) {
                const float4 w = *(const float4*)(wr + 4 * c4);
#pragma unroll
                for (int m = 0; m < DEC_ROWS; ++m) {
                    const float4 v = *(const float4*)(xs + m * kc + 4 * c4);
                    acc[m] = fmaf(w.x, v.x, acc[m]); acc[m] = fmaf(w.y, v.y, acc[m]); acc[m] = fmaf(w.z, v.z, acc[m]); acc[m] = fmaf(w.w, v.w, acc[m]);
                }
            }
        }
    }
    if (n >= N) return;
    float r = 0.f;
#pragma unroll
    for (int m = 0; m < DEC_ROWS; ++m) {
        const float s = wave_sum_f(acc[m]);
        if (lane == m) r = s;
    }
    if (lane < rows) {          // lane m owns row m0 + m of column n
        const long row = m0 + lane;
        if (bias) r += bias[n];
        if (gelu) r = gelu_y(r);
        if (residual) r += residual[row * N + n];
        const int s = n / out.seg_n;
        out.p[s][row * out.ld[s] + (n - s * out.seg_n)] = r;
    }
}

static int dec_linear_check(const char* name, int M, int K, int N, bool ln) {
    VQW_CHECK(K % 4 == 0 && K >= 4 && K <= DEC_MAX_K, "%s: K=%d must be a multiple of 4 with 4 <= K <= %d", name, K, DEC_MAX_K);
    VQW_CHECK(!ln || K <= DEC_KC, "%s: the LayerNorm of the input row needs K=%d <= %d", name, K, DEC_KC);
    VQW_CHECK(N >= 1, "%s: N=%d must be at least 1", name, N);
    VQW_CHECK(M >= 1 && M <= 65535 * DEC_ROWS, "%s: M=%d must satisfy 1 <= M <= %d", name, M, 65535 * DEC_ROWS);
    return VQW_OK;
}

// the launch, after every check
static int dec_linear_launch(const char* name, const float* x, const float* W, const float* bias, const float* gamma, const float* beta,
                             const float* residual, const DecOut& out, int M, int K, int N, int gelu, float eps, hipStream_t st) {
    const dim3 grid(ceil_div(N, DEC_WG_COLS), ceil_div(M, DEC_ROWS));
    if (gamma) {
        if (int rc = lds_opt_in<k_dec_linear<true>>(dec_lds_bytes(DEC_KC), name)) return rc;
        hipLaunchKernelGGL(k_dec_linear<true>, grid, dim3(256), dec_lds_bytes(K), st, x, W, bias, gamma, beta, residual, out, M, K, N, gelu, eps);
    } else {
        if (int rc = lds_opt_in<k_dec_linear<false>>(dec_lds_bytes(DEC_KC), name)) return rc;
        hipLaunchKernelGGL(k_dec_linear<false>, grid, dim3(256), dec_lds_bytes(K), st, x, W, bias, gamma, beta, residual, out, M, K, N, gelu, eps);
    }
    return VQW_OK;
}

extern "C" int vqw_dec_linear(const float* x, const float* w, const float* bias, const float* ln_gamma, const float* ln_beta,
                              const float* residual, float* y, int M, int K, int N, long ldy, long y_col, int gelu, float eps, void* stream) {
    if (int rc = dec_linear_check("vqw_dec_linear", M, K, N, ln_gamma != nullptr)) return rc;
    VQW_CHECK(x && w && y, "vqw_dec_linear: null pointer");
    VQW_CHECK((ln_gamma != nullptr) == (ln_beta != nullptr), "vqw_dec_linear: ln_gamma and ln_beta must be given together");
    VQW_CHECK(y_col >= 0 && ldy >= y_col + N, "vqw_dec_linear: the output columns [%ld, %ld) do not fit the row stride ldy=%ld", y_col, y_col + N, ldy);
    VQW_CHECK(al16(x) && al16(w) && al16(ln_gamma) && al16(ln_beta), "vqw_dec_linear: x, w and the LayerNorm parameters must be 16-byte aligned");
    VQW_CHECK((((uintptr_t)y) & 3) == 0 && (((uintptr_t)bias) & 3) == 0 && (((uintptr_t)residual) & 3) == 0,
              "vqw_dec_linear: y, bias and residual must be 4-byte aligned");
    VQW_CHECK((const float*)y != x, "vqw_dec_linear: y must not be x (y may be residual: the add is in place)");
    VQW_CHECK(!residual || (const float*)y != residual || (ldy == N && y_col == 0),
              "vqw_dec_linear: an in-place residual needs the dense output (ldy == N, y_col == 0)");
    DecOut out;
    for (int s = 0; s < 3; ++s) { out.p[s] = y + y_col; out.ld[s] = ldy; }
    out.seg_n = N;
    if (int rc = dec_linear_launch("vqw_dec_linear", x, w, bias, ln_gamma, ln_beta, residual, out, M, K, N, gelu ? 1 : 0, eps, (hipStream_t)stream)) return rc;
    VQW_LAUNCH_CHECK("vqw_dec_linear");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- decode attention
#define DA_CHUNK 64         // keys per chunk: one per lane
#define DA_MAX_HS 128
#define DA_MAX_T 65536

// grid B n_head, 256 threads.  q, o [B][E]; k, v [B][capacity][E]; head h in the columns [h hs, (h + 1) hs), hs = 4 HS4.  All four
// waves walk the same number of rounds of 4 DA_CHUNK keys (a wave whose chunk lies at or beyond Tk adds nothing in that round), so the
// workgroup barriers inside the walk are met by every wave.  P V: lane (g, c4) = (lane / HS4, lane % HS4) adds the keys g, g + G, ...
// of the chunk, G = 64 / HS4, into the float4 column c4: DA_CHUNK / G independent float4 loads per lane and chunk.
template <int HS4>
__global__ void __launch_bounds__(256) k_dec_attention(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                       float* __restrict__ o, int Tk, int capacity, int nh, float scale) {
    constexpr int HS = 4 * HS4, G = 64 / HS4, NI = (DA_CHUNK + G - 1) / G, NB = 8;          // NB loads in flight per lane
    __shared__ __align__(16) float qs[HS];
    __shared__ float ps[4][DA_CHUNK];                  // a wave's softmax numerators of the current chunk
    __shared__ float pm[4], pl[4];
    __shared__ __align__(16) float pacc[4][G][HS];     // the (wave, key group) partial outputs
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / nh, h = blockIdx.x - b * nh, E = nh * HS;
    const float* kb = k + (long)b * capacity * E + h * HS;
    const float* vb = v + (long)b * capacity * E + h * HS;
    if (threadIdx.x < HS) qs[threadIdx.x] = q[(long)b * E + h * HS + threadIdx.x];
    __syncthreads();
    const int g = lane / HS4, c4 = lane - g * HS4;
    float m = -INFINITY, l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r0 = 0; r0 < Tk; r0 += 4 * DA_CHUNK) {
        const int j0 = r0 + wv * DA_CHUNK;
        const int nk = Tk - j0 < DA_CHUNK ? Tk - j0 : DA_CHUNK;          // <= 0: this wave has no chunk in this round
        float a = 1.f;
        if (nk > 0) {
            float s = -INFINITY;
            if (lane < nk) {
                const float* kr = kb + (long)(j0 + lane) * E;
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);          // four chains of hs / 4 terms, added as a tree: shorter than one of hs
#pragma unroll
                for (int c = 0; c < HS4; ++c) {
                    const float4 kk = *(const float4*)(kr + 4 * c), qq = *(const float4*)(qs + 4 * c);
                    d.x = fmaf(qq.x, kk.x, d.x); d.y = fmaf(qq.y, kk.y, d.y); d.z = fmaf(qq.z, kk.z, d.z); d.w = fmaf(qq.w, kk.w, d.w);
                }
                s = scale * sum4(d);
            }
            const float mn = fmaxf(m, wave_max_f(s));          // finite: the chunk has a key
            const float p = lane < nk ? expf(s - mn) : 0.f;
            a = expf(m - mn);                                    // 0 on the wave's first chunk (m = -inf)
            l = fmaf(l, a, wave_sum_f(p));
            m = mn;
            ps[wv][lane] = p;
        }
        __syncthreads();
        if (nk > 0 && g < G) {
            acc.x *= a; acc.y *= a; acc.z *= a; acc.w *= a;
#pragma unroll 1
            for (int i0 = 0; i0 < NI; i0 += NB) {
                float4 vv[NB];
                float pj[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) {          // a key at or beyond Tk is not loaded
                    const int j = g + G * (i0 + i);
                    const bool ok = j < nk;
                    vv[i] = ok ? *(const float4*)(vb + (long)(j0 + j) * E + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    pj[i] = ok ? ps[wv][j] : 0.f;
                }
                // the batch's NB products as a tree, then one add into the accumulator: the chain per lane is DA_CHUNK / (G NB) adds long
#pragma unroll
                for (int i = 0; i < NB; ++i) { vv[i].x *= pj[i]; vv[i].y *= pj[i]; vv[i].z *= pj[i]; vv[i].w *= pj[i]; }
#pragma unroll
                for (int w = 1; w < NB; w *= 2) {
#pragma unroll
                    for (int i = 0; i < NB; i += 2 * w) {
                        vv[i].x += vv[i + w].x; vv[i].y += vv[i + w].y; vv[i].z += vv[i + w].z; vv[i].w += vv[i + w].w;
                    }
                }
                acc.x += vv[0].x; acc.y += vv[0].y; acc.z += vv[0].z; acc.w += vv[0].w;
            }
        }
        __syncthreads();          // ps is rewritten in the next round
    }
    if (lane == 0) { pm[wv] = m; pl[wv] = l; }
    if (g < G) *(float4*)(&pacc[wv][g][4 * c4]) = acc;
    __syncthreads();
    // the partials, merged in (wave, key group) order; a wave that never had a chunk left (-inf, 0, 0): its factor is exp(-inf) = 0
    if (threadIdx.x < HS) {
        const float mm = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));          // wave 0 always has a chunk
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = expf(pm[w] - mm);
            L = fmaf(pl[w], f, L);
            float ow = 0.f;
#pragma unroll
            for (int gg = 0; gg < G; ++gg) ow += pacc[w][gg][threadIdx.x];
            O = fmaf(ow, f, O);
        }
        o[(long)b * E + h * HS + threadIdx.x] = O / L;
    }
}

// the launch, after every check: one instantiation per head size
static void dec_attention_launch(const float* q, const float* k, const float* v, float* o, int B, int Tk, int capacity, int nh, int hs, float scale,
                                 hipStream_t st) {
    const dim3 grid(B * nh), block(256);
    switch (hs) {
        case 32: hipLaunchKernelGGL(k_dec_attention<8>, grid, block, 0, st, q, k, v, o, Tk, capacity, nh, scale); break;
        case 64: hipLaunchKernelGGL(k_dec_attention<16>, grid, block, 0, st, q, k, v, o, Tk, capacity, nh, scale); break;
        case 96: hipLaunchKernelGGL(k_dec_attention<24>, grid, block, 0, st, q, k, v, o, Tk, capacity, nh, scale); break;
        default: hipLaunchKernelGGL(k_dec_attention<32>, grid, block, 0, st, q, k, v, o, Tk, capacity, nh, scale); break;
    }
}

static int dec_attention_check(const char* name, int B, int Tk, int capacity, int nh, int hs) {
    VQW_CHECK(hs % 32 == 0 && hs >= 32 && hs <= DA_MAX_HS, "%s: head size hs=%d must be a multiple of 32 with 32 <= hs <= %d", name, hs, DA_MAX_HS);
    VQW_CHECK(B >= 1 && nh >= 1 && (long)B * nh <= 65535, "%s: B=%d, n_head=%d must satisfy 1 <= B * n_head <= 65535", name, B, nh);
    VQW_CHECK(capacity >= 1 && capacity <= DA_MAX_T, "%s: capacity=%d must satisfy 1 <= capacity <= %d", name, capacity, DA_MAX_T);
    VQW_CHECK(Tk >= 1 && Tk <= capacity, "%s: Tk=%d must satisfy 1 <= Tk <= capacity=%d", name, Tk, capacity);
    return VQW_OK;
}

extern "C" int vqw_dec_attention(const float* q, const float* k, const float* v, float* o, int B, int Tk, int capacity, int n_head, int hs,
                                 float scale, void* stream) {
    if (int rc = dec_attention_check("vqw_dec_attention", B, Tk, capacity, n_head, hs)) return rc;
    VQW_CHECK(q && k && v && o, "vqw_dec_attention: null pointer");
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o), "vqw_dec_attention: tensors must be 16-byte aligned");
    dec_attention_launch(q, k, v, o, B, Tk, capacity, n_head, hs, scale, (hipStream_t)stream);
    VQW_LAUNCH_CHECK("vqw_dec_attention");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------- the step
// floats of one layer in the packed buffer: ln1 (2E), W_qkv (3E E), b_qkv (3E), W_proj (E E), b_proj (E), ln2 (2E), W_fc1 (4E E),
// b_fc1 (4E), W_fc2 (E 4E), b_fc2 (E)
static inline long dec_layer_floats(long E) { return 12 * E * E + 13 * E; }

extern "C" long vqw_gpt_decode_pack_floats(int n_layer, int E, int V) {
    if (n_layer < 1 || E < 1 || V < 1) return 0;
    return (long)n_layer * dec_layer_floats(E) + 2L * E + (long)V * E;
}

// x, q, att [B][E] and h [B][4E]
extern "C" size_t vqw_gpt_decode_ws_bytes(int B, int E, int V) {
    if (B < 1 || E < 1 || V < 1) return 0;
    return (size_t)B * 7 * E * sizeof(float);
}

extern "C" int vqw_gpt_decode_step(const float* packed, const float* tok, const float* pos, const long* idx, float* kv, float* logits, void* ws,
                                   size_t ws_bytes, int B, int t, int capacity, int n_layer, int n_head, int E, int V, int block_size, float eps,
                                   void* stream) {
    const char* name = "vqw_gpt_decode_step";
    VQW_CHECK(packed && tok && pos && idx && kv && logits && ws, "%s: null pointer", name);
    VQW_CHECK(n_layer >= 1 && V >= 1, "%s: n_layer=%d, V=%d must be at least 1", name, n_layer, V);
    VQW_CHECK(E % 4 == 0 && E >= 4 && E <= DEC_KC, "%s: E=%d must be a multiple of 4 with 4 <= E <= %d", name, E, DEC_KC);
    VQW_CHECK(n_head >= 1 && E % n_head == 0, "%s: E=%d is not divisible by n_head=%d", name, E, n_head);
    if (int rc = dec_attention_check(name, B, 1, imax(capacity, 1), n_head, E / n_head)) return rc;
    VQW_CHECK(capacity >= 1 && capacity <= DA_MAX_T, "%s: capacity=%d must satisfy 1 <= capacity <= %d", name, capacity, DA_MAX_T);
    VQW_CHECK(t >= 0, "%s: t=%d must not be negative", name, t);
    VQW_CHECK(t < capacity, "%s: t=%d: the cache of capacity=%d rows is full", name, t, capacity);
    VQW_CHECK(block_size >= 1 && t < block_size, "%s: t + 1 = %d exceeds block_size=%d", name, t + 1, block_size);
    VQW_CHECK(ws_bytes >= vqw_gpt_decode_ws_bytes(B, E, V), "%s: workspace of %zu bytes, %zu needed", name, ws_bytes, vqw_gpt_decode_ws_bytes(B, E, V));
    VQW_CHECK(al16(packed) && al16(tok) && al16(pos) && al16(kv) && al16(logits) && al16(ws), "%s: tensors must be 16-byte aligned", name);
    VQW_CHECK((((uintptr_t)idx) & 7) == 0, "%s: idx must be 8-byte aligned", name);
    if (int rc = dec_linear_check(name, B, 4 * E, V, false)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const long e = E, plane = (long)B * capacity * E;
    const int hs = E / n_head;
    const float scale = 1.f / sqrtf((float)hs);
    float* x = (float*)ws;
    float* q = x + B * e;
    float* att = q + B * e;
    float* hbuf = att + B * e;
    auto dense = [](float* p, long ld, int N) {
        DecOut o;
        for (int s = 0; s < 3; ++s) { o.p[s] = p; o.ld[s] = ld; }
        o.seg_n = N;
        return o;
    };

    // x[b] = tok[idx[b]] + pos[t]: the embedding's own launch with one token per row (what it checks has been checked above)
    if (int rc = vqw_embed_fwd(idx, tok, pos, nullptr, x, B, 1, 0, E, V, block_size, t, stream)) return rc;
    const float* p = packed;
    for (int l = 0; l < n_layer; ++l, p += dec_layer_floats(e)) {
        const float *ln1w = p, *ln1b = ln1w + e, *wqkv = ln1b + e, *bqkv = wqkv + 3 * e * e, *wproj = bqkv + 3 * e, *bproj = wproj + e * e;
        const float *ln2w = bproj + e, *ln2b = ln2w + e, *wfc1 = ln2b + e, *bfc1 = wfc1 + 4 * e * e, *wfc2 = bfc1 + 4 * e, *bfc2 = wfc2 + 4 * e * e;
        float* kplane = kv + (long)(2 * l) * plane;
        float* vplane = kplane + plane;
        DecOut qkv;          // q | k | v: q to its buffer, k and v into row t of batch row m's cache rows
        qkv.p[0] = q; qkv.ld[0] = e;
        qkv.p[1] = kplane + (long)t * e; qkv.ld[1] = (long)capacity * e;
        qkv.p[2] = vplane + (long)t * e; qkv.ld[2] = (long)capacity * e;
        qkv.seg_n = E;
        if (int rc = dec_linear_launch(name, x, wqkv, bqkv, ln1w, ln1b, nullptr, qkv, B, E, 3 * E, 0, eps, st)) return rc;
        dec_attention_launch(q, kplane, vplane, att, B, t + 1, capacity, n_head, hs, scale, st);
        if (int rc = dec_linear_launch(name, att, wproj, bproj, nullptr, nullptr, x, dense(x, e, E), B, E, E, 0, eps, st)) return rc;
        if (int rc = dec_linear_launch(name, x, wfc1, bfc1, ln2w, ln2b, nullptr, dense(hbuf, 4 * e, 4 * E), B, E, 4 * E, 1, eps, st)) return rc;
        if (int rc = dec_linear_launch(name, hbuf, wfc2, bfc2, nullptr, nullptr, x, dense(x, e, E), B, 4 * E, E, 0, eps, st)) return rc;
    }
    if (int rc = dec_linear_launch(name, x, p + 2 * e, nullptr, p, p + e, nullptr, dense(logits, V, V), B, E, V, 0, eps, st)) return rc;
    VQW_LAUNCH_CHECK(name);
    return VQW_OK;
}
