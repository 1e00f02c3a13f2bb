// Softmax attention, forward and backward, for the two layouts of the library: the VQGAN's single-head self-attention over a
// feature map (networks/vqgan.py: AttnBlock :125-180) and the minGPT's multi-head attention with a causal mask and an unmasked
// prefix (networks/mingpt.py: CausalSelfAttention :34-90).  fp32.  One tile engine serves both; what differs between them is
// held by two compile-time policies (below), never by a run-time branch on the caller.  A third policy adds dropout on the
// probabilities (mingpt.py:83) to the causal kernels: the instantiations without it are the code they were before it existed.
//
// o = softmax(scale q k^T) v.  All five matrix products (q k^T and p v forward; recomputed q k^T, dO v^T, dS k, dS^T q and
// p^T dO backward) are one of two forms on the exact-fp32 32x32x2 MFMA:
//   at_gemm_nt: T[32][64] = A[32 rows][W] . B[64 rows][W]^T   (operands staged in LDS in chunks of <= 128 channels)
//   pv:         acc[32][W] += P[32][64] (LDS) . B[64 rows][W]  (the value / output policy's)
// A workgroup owns 32 "tile rows" (queries forward and for dQ; keys for dK / dV, where the transposed score tile is computed
// directly as k q^T - no transposed LDS reads) and walks the other axis in tiles of 64.  The score matrix never leaves LDS.
// No atomics anywhere: every output element is written by one thread, sums run in a fixed order.
//
// Query i sees key j iff j <= limit(i).  Steps that lie wholly outside a tile's limits are not walked, the others are masked
// element by element.
//
// Contraction.  The library is built with -ffp-contract=fast, under which clang disregards `#pragma clang fp contract`
// (DESIGN 6k), so the compiler may fuse any multiply here into a following add - in particular the scaled score
// s = scale (T0 + T1) into the subtraction that follows it - and may do so differently in the forward and in the backward.
// Both attention families have always been compiled this way; whether the backward's recomputed score has to match the
// forward's bit for bit is an open item of DESIGN 6r.  The explicit fmaf calls and the MFMAs are not affected.
#include <type_traits>
#include "common.h"
#include "mfma_util.h"
#include "dropout.h"
#include "../../include/vqwnet_hip.h"

#define AT_BM 32           // tile rows a workgroup owns
#define AT_BN 64           // tile columns per step of the walk
#define AT_KC 128          // channels per staged chunk
#define AT_LDS (AT_BN + 4) // LDS row stride of a score tile
#define AT_MAX_C 512       // spatial: widest value / output column window one workgroup keeps in registers
#define AT_MAX_C2 1024     // spatial: two such windows, the grid's z dimension
#define AT_MAX_T 65536     // causal: longest sequence

__device__ __forceinline__ int at_min(int a, int b) { return a < b ? a : b; }

// LDS carve-up (floats).  A: staged 32-row operand chunk; B: staged 64-row operand chunk; T0 / T1: two score tiles as two
// half-sums each (T0 at the end of a key-split kernel: the four waves' partial accumulators); P0 / P1: the element-wise stage's
// results (the A operand of pv); V: 4 x 64 floats of row / column vectors.  A staged operand row is `ld` floats, ld = 4 mod 32
// (ds_read_b128 of 32 consecutive rows conflict-free): 128 + 4 for the spatial kernels, hs + 4 for a head of hs channels, so
// that several workgroups of narrow heads share a CU.  A forward uses neither T1 nor P1: they lie last and it need not ask for
// them (the spatial forward still does: its request is the backward's).
#define AT_T_FLOATS (2 * AT_BM * AT_LDS)
#define AT_P_FLOATS (AT_BM * AT_LDS)
struct AtLds {
    int ld;
    float *A, *B, *T0, *P0, *V, *T1, *P1;
    __device__ __forceinline__ AtLds(float* base, int ld_) : ld(ld_) {
        A = base; B = A + AT_BM * ld; T0 = B + AT_BN * ld; P0 = T0 + AT_T_FLOATS; V = P0 + AT_P_FLOATS; T1 = V + 4 * AT_BN; P1 = T1 + AT_T_FLOATS;
    }
};
static inline int at_lds_bytes(int ld, bool bwd) {
    return ((AT_BM + AT_BN) * ld + AT_T_FLOATS + AT_P_FLOATS + 4 * AT_BN + (bwd ? AT_T_FLOATS + AT_P_FLOATS : 0)) * 4;
}

// ------------------------------------------------------------------------------------------- geometry / visibility policies
// base(rows): this workgroup's offset into a tensor of `rows` rows per batch element; ld: the row stride; width: the
// contraction and value width W; lds_ld: the staged-row stride; limit(i): the last key query i sees (it grows with i);
// last_key(i0): the largest limit of the query tile at i0; first_query(j0): the first query step that sees a key of the tile
// at j0; d_index(r): where the row-dot of row segment r goes; row(src, row0, r, ld): the address of row row0 + r (r < 64) of a
// tile that starts at row0, for the stager.  The two families want different forms of that one address (same-run A/B against
// the previous copies): with the other family's form the spatial C = 512 kernels are 0.4 ... 0.7 % slower and the
// causal hs = 128 forward 0.4 %.
// Spatial: q, k, v [B][N][C], one head of all C channels, no mask - limit is a constant and costs nothing.
template <bool FOLD_>
struct AtSpatial {
    static constexpr bool FOLD = FOLD_;            // above 512 channels: at_gemm_nt's second accumulator
    static constexpr bool ONE_CHUNK = false;
    int N, C;
    using RowDot = AtSpatial<false>;               // the row-dot does not depend on FOLD: one instantiation
    RowDot rowdot() const { return RowDot{N, C}; }
    __device__ __forceinline__ int Tq() const { return N; }
    __device__ __forceinline__ int Tk() const { return N; }
    __device__ __forceinline__ long base(int rows) const { return (long)blockIdx.y * rows * C; }
    __device__ __forceinline__ int ld() const { return C; }
    // the 64-bit part is the tile's own row0 * ld, a scalar; a thread adds r * ld <= 2^16 in 32 bits
    static __device__ __forceinline__ const float* row(const float* src, int row0, int r, int ld) { return src + (long)row0 * ld + r * ld; }
    __device__ __forceinline__ int width() const { return C; }
    __device__ __forceinline__ int lds_ld() const { return AT_KC + 4; }
    __device__ __forceinline__ int limit(int) const { return N - 1; }
    __device__ __forceinline__ int last_key(int) const { return N - 1; }
    __device__ __forceinline__ int first_query(int) const { return 0; }
    __device__ __forceinline__ long d_index(long r) const { return r; }
};
// Causal: q [B][Tq][E], k, v [B][Tk][E], E = n_head hs, head h in the columns [h hs, (h + 1) hs) - the layout the three
// projections leave; blockIdx.y = b n_head + h.  limit(i) = (i < n_unmasked ? n_unmasked - 1 : i) under the causal mask and
// Tk - 1 without.  hs <= 128: a single staged chunk.  lse and D are [B][n_head][T].
struct AtCausal {
    static constexpr bool FOLD = false;
    static constexpr bool ONE_CHUNK = true;
    int tq, tk, nh, hs, causal, nu;
    using RowDot = AtCausal;
    RowDot rowdot() const { return *this; }
    __device__ __forceinline__ int Tq() const { return tq; }
    __device__ __forceinline__ int Tk() const { return tk; }
    __device__ __forceinline__ long base(int rows) const {
        const int b = blockIdx.y / nh, h = blockIdx.y - b * nh;
        return (long)b * rows * (nh * hs) + h * hs;
    }
    __device__ __forceinline__ int ld() const { return nh * hs; }
    // one 32 x 32 -> 64-bit multiply-add per thread
    static __device__ __forceinline__ const float* row(const float* src, int row0, int r, int ld) { return src + (long)(row0 + r) * ld; }
    __device__ __forceinline__ int width() const { return hs; }
    __device__ __forceinline__ int lds_ld() const { return hs + 4; }
    __device__ __forceinline__ int limit(int i) const { return causal ? at_min(i < nu ? nu - 1 : i, tk - 1) : tk - 1; }
    __device__ __forceinline__ int last_key(int i0) const { return limit(at_min(i0 + AT_BM, tq) - 1); }
    // step 0 when the tile's first key lies in the unmasked prefix (or without a mask), else the step that holds its first key
    __device__ __forceinline__ int first_query(int j0) const { return (!causal || j0 < nu) ? 0 : (j0 / AT_BN) * AT_BN; }
    __device__ __forceinline__ long d_index(long r) const {          // r = (b T + t) n_head + h
        const int h = (int)(r % nh);
        const long bt = r / nh;
        return ((bt / tq) * nh + h) * tq + bt % tq;
    }
};

// --------------------------------------------------------------------------------------------------------- dropout policies
// Dropout on the probabilities, between the softmax and the P . V product: o = (P o M) v with M = keep / (1 - p).  The mask is the
// counter-based one of dropout.h at the LOGICAL position of a probability - index hi = (b n_head + h) Tq + i, lo = j - so that
// the three kernels, which meet an element in different tile orientations, regenerate the same mask and nothing is stored.
// A query row's two key words are made once per row: by the row's thread (forward) or into the row / column vector in LDS
// beside lse and D (backward); an element then costs the nine vector instructions dropout.h counts and the multiply by M.
// AtNoDrop is empty and every use of a policy sits behind `if constexpr (DP::ON)`: no run-time flag reaches the element-wise
// stage (at_gemm_nt's comment says what one costs).  A kernel takes the policy as a trailing parameter PACK: without dropout the
// pack is empty and the kernel's argument list - its kernarg segment and the loads in front of its body - is the one it had.
struct AtNoDrop {
    static constexpr bool ON = false;
};
struct AtDrop {
    static constexpr bool ON = true;
    DropKey key;
    __device__ __forceinline__ void row(int Tq, int i, uint32_t& r0, uint32_t& r1) const {
        dk_row(key, dk_attn_hi(blockIdx.y, (uint32_t)Tq, (uint32_t)i), r0, r1);
    }
    // M of key j in the row of (r0, r1)
    __device__ __forceinline__ float m(uint32_t r0, uint32_t r1, int j) const { return dk_keep_row(key, r0, r1, (uint32_t)j) ? key.scale : 0.f; }
};
__device__ __forceinline__ AtNoDrop at_policy() { return {}; }
__device__ __forceinline__ const AtDrop& at_policy(const AtDrop& dp) { return dp; }
#define AT_VEC_R0 (2 * AT_BN)          // the backward's vector: lse, D, then the queries' two key words (drop policy only)
#define AT_VEC_R1 (3 * AT_BN)

// --------------------------------------------------------------------------------------------------------- the tile engine
// rows [row0, row0 + R) x columns [c0, c0 + wt) of src (row stride ld) -> dst [R][sld]; rows at or past n_rows are zeros
template <class G>
__device__ __forceinline__ void at_stage(float* dst, int sld, const float* __restrict__ src, int row0, int n_rows, int R, int c0, int wt, int ld) {
    const int w4 = wt >> 2;
    for (int i = threadIdx.x; i < R * w4; i += 256) {
        const int r = i / w4, c4 = i - r * w4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < n_rows) v = *(const float4*)(G::row(src, row0, r, ld) + c0 + c4 * 4);
        *(float4*)(dst + r * sld + c4 * 4) = v;
    }
}

// T[32][64] = A[a0 .. a0+32) . B[b0 .. b0+64)^T over W channels, left in LDS as two half-sums T[0], T[1] ([32][AT_LDS] each; the
// consumer adds them): wave w takes the 32 columns (w & 1) and half (w >> 1) of every chunk's channels.
// Lane l feeds row / column l % 32; its four consecutive channels 8 s + 4 (l / 32) + {0..3} go to four MFMAs.
// FOLD (the kernels above 512 channels): every chunk's sum is added to a second accumulator, so that no chain of dependent
// roundings is longer than at 128 channels (a single chain over 1024 channels left lse twice as far from float64 as torch's
// fp32 bmm is).  ONE_CHUNK (W <= 128, the causal heads): no chunk loop, and stage_a = false says that A is still staged from
// the previous call.  Both are compile-time facts of the geometry G because a run-time trip count or a run-time `stage_a` around the staging of A
// cost the kernels 14 to 34 registers and an occupancy step each.
template <class G>
__device__ __forceinline__ void at_gemm_nt(const AtLds& L, float* T, const float* __restrict__ A, int a0, int na, const float* __restrict__ B, int b0,
                                           int nb, int W, int ld, bool stage_a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kb = wv & 1, hf = wv >> 1;
    const int lr = lane & 31, lh = lane >> 5;
    constexpr bool FOLD = G::FOLD, ONE_CHUNK = G::ONE_CHUNK;
    f32x16 acc = {0}, tot = {0};
    for (int c0 = 0; c0 < (ONE_CHUNK ? 1 : W); c0 += AT_KC) {
        const int wt = ONE_CHUNK ? W : at_min(AT_KC, W - c0);
        __syncthreads();                      // the previous users of the staging buffers and of T are done
        if (!ONE_CHUNK || stage_a) at_stage<G>(L.A, L.ld, A, a0, na, AT_BM, c0, wt, ld);
        at_stage<G>(L.B, L.ld, B, b0, nb, AT_BN, c0, wt, ld);
        __syncthreads();
        const int half = wt >> 1;             // a multiple of 16
        const float* pa = L.A + lr * L.ld + hf * half + lh * 4;
        const float* pb = L.B + (kb * 32 + lr) * L.ld + hf * half + lh * 4;
        for (int s = 0; s < half; s += 8) {
            const float4 a = *(const float4*)(pa + s), b = *(const float4*)(pb + s);
            acc = MFMA32(a.x, b.x, acc);
            acc = MFMA32(a.y, b.y, acc);
            acc = MFMA32(a.z, b.z, acc);
            acc = MFMA32(a.w, b.w, acc);
        }
        if constexpr (FOLD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
        }
    }
    if constexpr (FOLD) acc = tot;
    float* t = T + hf * (AT_BM * AT_LDS) + kb * 32 + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[((r & 3) + 8 * (r >> 2) + 4 * lh) * AT_LDS] = acc[r];
    __syncthreads();
}

// element-wise stage: thread -> row tid / 8, columns tid % 8 + 8 e (e = 0..7): the eight threads of a row are neighbours
#define AT_EW_ROW (threadIdx.x >> 3)
#define AT_EW_COL(e) ((threadIdx.x & 7) + 8 * (e))
// row of element r of a lane's 32x32 MFMA accumulator
#define AT_ACC_ROW(r, lh) (((r) & 3) + 8 * ((r) >> 2) + 4 * (lh))
__device__ __forceinline__ float at_row8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
    return v;
}
__device__ __forceinline__ float at_row8_sum(float v) {       // fixed butterfly: the same bits in all eight lanes, every run
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    return v;
}
__device__ __forceinline__ float at_score(const float* T, int row, int col) {       // the two half-sums
    return T[row * AT_LDS + col] + T[AT_BM * AT_LDS + row * AT_LDS + col];
}

// One online-softmax step on the score tile T0 of the keys [j0, j0 + 64): the running row maximum m and sum l live in the row's
// eight threads; P0 = exp(s - m); returns this step's rescale of what the row has accumulated.  Every row - a padding row of
// the last tile too - sees key 0, so m is finite after the first step, and a masked entry (s = -inf) gives exp(-inf - m) = 0
// exactly.  (Selecting the constant 0 for it instead gives the same bits and cost every forward about 1 %, measured.)
// Drop policy: m and l come from the undropped p - lse does not know of the dropout - and P0 = p M, the row's key words in (r0, r1).
template <class DP>
__device__ __forceinline__ float at_softmax_step(const AtLds& L, int j0, int lim, float scale, float& m, float& l, const DP& dp, uint32_t r0,
                                                 uint32_t r1) {
    const int row = AT_EW_ROW;
    float s[8], mt = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s[e] = (j0 + AT_EW_COL(e) <= lim) ? scale * at_score(L.T0, row, AT_EW_COL(e)) : -INFINITY;
        mt = fmaxf(mt, s[e]);
    }
    const float mn = fmaxf(m, at_row8_max(mt));
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float p = expf(s[e] - mn);
        if constexpr (DP::ON) L.P0[row * AT_LDS + AT_EW_COL(e)] = p * dp.m(r0, r1, j0 + AT_EW_COL(e));
        else L.P0[row * AT_LDS + AT_EW_COL(e)] = p;
        ps += p;
    }
    const float a = expf(m - mn);
    l = fmaf(l, a, at_row8_sum(ps));
    m = mn;
    return a;
}

// The backward's element-wise stage on T0 = (q k^T or k q^T) and T1 = (dO v^T or v dO^T): P = exp(scale S - lse) -> P0 (if
// wanted), dS = scale P (dP - D) -> P1 where the query exists and sees the key, 0 elsewhere.  lse / D are indexed by the QUERY:
// the tile row (ROWS_ARE_QUERIES) or column.  vec: lse at [0, 64), D at [64, 128) of the tile's query range.
// Drop policy, M the mask of (query, key) from the query's key words at [128, 256) of vec: P0 = P o M (what dV multiplies),
// dS = scale P (M dP - D).
template <bool ROWS_ARE_QUERIES, class G, class DP>
__device__ __forceinline__ void at_bwd_stage(const AtLds& L, const float* vec, int r0, int c0, const G& g, float scale, bool want_p, const DP& dp) {
    const int row = AT_EW_ROW;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int col = AT_EW_COL(e), qi = ROWS_ARE_QUERIES ? row : col;
        const int iq = ROWS_ARE_QUERIES ? r0 + row : c0 + col, jk = ROWS_ARE_QUERIES ? c0 + col : r0 + row;
        const bool ok = iq < g.Tq() && jk <= g.limit(iq);
        const float sc = scale * at_score(L.T0, row, col);
        const float dpv = at_score(L.T1, row, col);
        const float p = ok ? expf(sc - vec[qi]) : 0.f;
        if constexpr (DP::ON) {
            const uint32_t* kw = (const uint32_t*)vec;
            const float mk = dp.m(kw[AT_VEC_R0 + qi], kw[AT_VEC_R1 + qi], jk);
            if (want_p) L.P0[row * AT_LDS + col] = p * mk;
            L.P1[row * AT_LDS + col] = ok ? scale * p * (mk * dpv - vec[AT_BN + qi]) : 0.f;
        } else {
            if (want_p) L.P0[row * AT_LDS + col] = p;
            L.P1[row * AT_LDS + col] = ok ? scale * p * (dpv - vec[AT_BN + qi]) : 0.f;
        }
    }
    __syncthreads();
}

// vec <- lse | D of the n queries from i0 (zeros past T); drop policy: and the queries' key words
template <class DP>
__device__ __forceinline__ void at_load_vec(float* vec, const float* __restrict__ lse, const float* __restrict__ D, int i0, int n, int T, const DP& dp) {
    if (threadIdx.x < n) {
        const bool ok = i0 + threadIdx.x < T;
        vec[threadIdx.x] = ok ? lse[i0 + threadIdx.x] : 0.f;
        vec[AT_BN + threadIdx.x] = ok ? D[i0 + threadIdx.x] : 0.f;
        if constexpr (DP::ON) {
            uint32_t* kw = (uint32_t*)vec;
            dp.row(T, i0 + threadIdx.x, kw[AT_VEC_R0 + threadIdx.x], kw[AT_VEC_R1 + threadIdx.x]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ value / output policies
// Two different algorithms, each with its own order of sums.  acc += P[32][64] . src[b0 .. b0+64)[W columns, row stride ld];
// store: out[row0 + row][c] = acc * f(row) for the valid rows; the 64-bit part of its addresses is the tile's row0 * ld, a
// scalar, and a thread adds row * ld < 2^31 in 32 bits (row < 32).
//
// Column windows (spatial): the workgroup works on a window of Cw = W / gridDim.z columns starting at column blockIdx.z Cw
// (one window = the whole row up to 512 channels, two halves above).  Wave w keeps the 32 x 32 blocks of the columns
// 128 t + 32 w, t < CT, of the window, each over all 64 keys of a step, and stores them straight from registers.
template <int CT>
struct AtWindows {
    f32x16 acc[CT];
    static __device__ __forceinline__ int col0(int W) { return (int)blockIdx.z * (W / (int)gridDim.z); }
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[t] = (f32x16){0};
    }
    __device__ __forceinline__ void rescale(const float* alpha) {
        const int lh = (threadIdx.x & 63) >> 5;
        float ar[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ar[r] = alpha[AT_ACC_ROW(r, lh)];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] *= ar[r];
    }
    template <class G>
    __device__ __forceinline__ void pv(const AtLds& L, const float* P, const float* __restrict__ src, int b0, int nb, int W, int ld) {
        const int Cw = W / (int)gridDim.z;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int lr = lane & 31, lh = lane >> 5;
        src += col0(W);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const int c0 = t * AT_KC, wt = at_min(AT_KC, Cw - c0);
            __syncthreads();
            at_stage<G>(L.B, L.ld, src, b0, nb, AT_BN, c0, wt, ld);
            __syncthreads();
            if (wv * 32 < wt) {
                const float* pa = P + lr * AT_LDS + lh * 4;
                const float* pb = L.B + (lh * 4) * L.ld + wv * 32 + lr;
#pragma unroll
                for (int s = 0; s < AT_BN; s += 8) {
                    const float4 a = *(const float4*)(pa + s);
                    acc[t] = MFMA32(a.x, pb[(s + 0) * L.ld], acc[t]);
                    acc[t] = MFMA32(a.y, pb[(s + 1) * L.ld], acc[t]);
                    acc[t] = MFMA32(a.z, pb[(s + 2) * L.ld], acc[t]);
                    acc[t] = MFMA32(a.w, pb[(s + 3) * L.ld], acc[t]);
                }
            }
        }
    }
    template <class RowScale>
    __device__ __forceinline__ void store(const AtLds&, float* __restrict__ out, int row0, int n_rows, int W, int ld, RowScale rs) const {
        const int Cw = W / (int)gridDim.z;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int lr = lane & 31, lh = lane >> 5;
        out += (long)row0 * ld + col0(W);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const int c = t * AT_KC + wv * 32;
            if (c < Cw) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = AT_ACC_ROW(r, lh);
                    if (row0 + row < n_rows) out[row * ld + c + lr] = acc[t][r] * rs(row);
                }
            }
        }
    }
};

// Column blocks x key splits (causal, W = hs <= 128): with ncb = hs / 32 column blocks and ksn = 4 / ncb key splits, wave w takes
// column block w % ncb and the keys [64 / ksn * (w / ncb), 64 / ksn * (w / ncb + 1)) of a step.  The per-wave partial
// accumulators are linear in everything the walk does to them and are added once, in split order, at the end (through T0).
static_assert(4 * AT_BM * 32 <= AT_T_FLOATS, "the partial accumulators fit in T0");
struct AtKeySplits {
    f32x16 acc;
    __device__ __forceinline__ void zero() { acc = (f32x16){0}; }
    __device__ __forceinline__ void rescale(const float* alpha) {
        const int lh = (threadIdx.x & 63) >> 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= alpha[AT_ACC_ROW(r, lh)];
    }
    template <class G>
    __device__ __forceinline__ void pv(const AtLds& L, const float* P, const float* __restrict__ src, int b0, int nb, int hs, int ld) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int lr = lane & 31, lh = lane >> 5;
        const int ncb = hs >> 5, ksn = 4 / ncb, cb = wv % ncb, ks = wv / ncb, kw = AT_BN / ksn;
        __syncthreads();
        at_stage<G>(L.B, L.ld, src, b0, nb, AT_BN, 0, hs, ld);
        __syncthreads();
        if (ks < ksn) {
            const float* pa = P + lr * AT_LDS + ks * kw + lh * 4;
            const float* pb = L.B + (ks * kw + lh * 4) * L.ld + cb * 32 + lr;
            for (int s = 0; s < kw; s += 8) {
                const float4 a = *(const float4*)(pa + s);
                acc = MFMA32(a.x, pb[(s + 0) * L.ld], acc);
                acc = MFMA32(a.y, pb[(s + 1) * L.ld], acc);
                acc = MFMA32(a.z, pb[(s + 2) * L.ld], acc);
                acc = MFMA32(a.w, pb[(s + 3) * L.ld], acc);
            }
        }
    }
    template <class RowScale>
    __device__ __forceinline__ void store(const AtLds& L, float* __restrict__ out, int row0, int n_rows, int hs, int ld, RowScale rs) const {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int lr = lane & 31, lh = lane >> 5;
        const int ncb = hs >> 5, ksn = 4 / ncb;
        float* red = L.T0;
        out += (long)row0 * ld;
        __syncthreads();                      // the readers of T0 - a previous store's too - are done
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wv * 1024 + AT_ACC_ROW(r, lh) * 32 + lr] = acc[r];
        __syncthreads();
        for (int i = threadIdx.x; i < AT_BM * hs; i += 256) {
            const int row = i / hs, c = i - row * hs, cb = c >> 5;
            float s = red[cb * 1024 + row * 32 + (c & 31)];
            for (int ks = 1; ks < ksn; ++ks) s += red[(ks * ncb + cb) * 1024 + row * 32 + (c & 31)];
            if (row0 + row < n_rows) out[row * ld + c] = s * rs(row);
        }
    }
};

// ------------------------------------------------------------------------------------------------------------- the kernels
// grid (ceil(Tq / 32), batch x heads, column windows).  o and lse [batch x heads][Tq] of a tile of 32 queries, over the key
// steps up to the tile's largest limit.  A single-chunk geometry re-uses the staged q tile after the first step.
template <class G, class VO, class... DPs>
__global__ void __launch_bounds__(256) k_attn_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                  float* __restrict__ o, float* __restrict__ lse, G g, float scale, DPs... dps) {
    extern __shared__ __align__(16) float lds[];
    const auto dp = at_policy(dps...);
    using DP = std::remove_cv_t<decltype(dp)>;
    const AtLds L(lds, g.lds_ld());
    const int Tq = g.Tq(), Tk = g.Tk(), W = g.width(), ld = g.ld();
    q += g.base(Tq); o += g.base(Tq); k += g.base(Tk); v += g.base(Tk);
    const int i0 = blockIdx.x * AT_BM;
    float* alpha = L.V;          // [32] this step's rescale of the accumulated rows
    VO acc;
    acc.zero();
    float m = -INFINITY, l = 0.f;
    const int row = AT_EW_ROW;
    const int lim = g.limit(i0 + row), jmax = g.last_key(i0);
    uint32_t r0 = 0, r1 = 0;     // drop policy: the key words of this thread's query row
    if constexpr (DP::ON) dp.row(Tq, i0 + row, r0, r1);
    for (int j0 = 0; j0 <= jmax; j0 += AT_BN) {
        at_gemm_nt<G>(L, L.T0, q, i0, Tq, k, j0, Tk, W, ld, j0 == 0);
        const float a = at_softmax_step(L, j0, lim, scale, m, l, dp, r0, r1);
        if ((threadIdx.x & 7) == 0) alpha[row] = a;
        __syncthreads();
        acc.rescale(alpha);
        acc.template pv<G>(L, L.P0, v, j0, Tk, W, ld);
    }
    float* rinv = L.V + AT_BN;
    if ((threadIdx.x & 7) == 0) {
        rinv[row] = 1.f / l;
        if (i0 + row < Tq && blockIdx.z == 0) lse[(long)blockIdx.y * Tq + i0 + row] = m + logf(l);
    }
    __syncthreads();
    acc.store(L, o, i0, Tq, W, ld, [&](int r) { return rinv[r]; });
}

// D[d_index(r)] = sum_c dO O over row segment r of `W` contiguous floats (a row of [B][N][C]; the (b, t, h) head segment of
// [B][T][n_head hs]): one wave per segment, fixed butterfly
template <class G>
__global__ void __launch_bounds__(256) k_attn_rowdot(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, long rows, G g) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, W = g.width();
    float s = 0.f;
    for (int c = lane * 4; c < W; c += 256) {
        const float4 x = *(const float4*)(a + r * W + c), y = *(const float4*)(b + r * W + c);
        s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
    s = wave_sum_f(s);
    if (lane == 0) d[g.d_index(r)] = s;
}

// same grid: dQ = scale (P o (dO v^T - D)) k for a tile of 32 queries, over the key steps the forward walked
template <class G, class VO, class... DPs>
__global__ void __launch_bounds__(256) k_attn_dq(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                 const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                                 float* __restrict__ gq, G g, float scale, DPs... dps) {
    extern __shared__ __align__(16) float lds[];
    const auto dp = at_policy(dps...);
    const AtLds L(lds, g.lds_ld());
    const int T = g.Tq(), W = g.width(), ld = g.ld();
    const long off = g.base(T);
    q += off; k += off; v += off; go += off; gq += off;
    lse += (long)blockIdx.y * T; D += (long)blockIdx.y * T;
    const int i0 = blockIdx.x * AT_BM;
    float* vec = L.V;
    at_load_vec(vec, lse, D, i0, AT_BM, T, dp);
    VO acc;
    acc.zero();
    const int jmax = g.last_key(i0);
    for (int j0 = 0; j0 <= jmax; j0 += AT_BN) {
        at_gemm_nt<G>(L, L.T0, q, i0, T, k, j0, T, W, ld, true);
        at_gemm_nt<G>(L, L.T1, go, i0, T, v, j0, T, W, ld, true);
        at_bwd_stage<true>(L, vec, i0, j0, g, scale, false, dp);
        acc.template pv<G>(L, L.P1, k, j0, T, W, ld);
    }
    acc.store(L, gq, i0, T, W, ld, [](int) { return 1.f; });
}

// same grid: dK = scale (P o (dO v^T - D))^T q and dV = P^T dO for a tile of 32 keys, over the query steps from the first one
// that sees one of its keys
template <class G, class VO, class... DPs>
__global__ void __launch_bounds__(256) k_attn_dkdv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                   const float* __restrict__ go, const float* __restrict__ lse, const float* __restrict__ D,
                                                   float* __restrict__ gk, float* __restrict__ gv, G g, float scale, DPs... dps) {
    extern __shared__ __align__(16) float lds[];
    const auto dp = at_policy(dps...);
    const AtLds L(lds, g.lds_ld());
    const int T = g.Tq(), W = g.width(), ld = g.ld();
    const long off = g.base(T);
    q += off; k += off; v += off; go += off; gk += off; gv += off;
    lse += (long)blockIdx.y * T; D += (long)blockIdx.y * T;
    const int j0 = blockIdx.x * AT_BM;
    float* vec = L.V;
    VO ak, av;
    ak.zero();
    av.zero();
    for (int i0 = g.first_query(j0); i0 < T; i0 += AT_BN) {
        __syncthreads();                      // the previous step's readers of vec are done
        at_load_vec(vec, lse, D, i0, AT_BN, T, dp);
        at_gemm_nt<G>(L, L.T0, k, j0, T, q, i0, T, W, ld, true);
        at_gemm_nt<G>(L, L.T1, v, j0, T, go, i0, T, W, ld, true);
        at_bwd_stage<false>(L, vec, j0, i0, g, scale, true, dp);
        av.template pv<G>(L, L.P0, go, i0, T, W, ld);
        ak.template pv<G>(L, L.P1, q, i0, T, W, ld);
    }
    ak.store(L, gk, j0, T, W, ld, [](int) { return 1.f; });
    av.store(L, gv, j0, T, W, ld, [](int) { return 1.f; });
}

// ---------------------------------------------------------------------------------------------------------------- the host
// lds_max: the largest request of this instantiation (the opt-in is made once), lds: this launch's
template <class G, class VO, class... DPs>
static int at_fwd_launch(const char* name, const G& g, dim3 grid, int lds_max, int lds, const float* q, const float* k, const float* v, float* o,
                         float* lse, float scale, hipStream_t st, DPs... dps) {
    if (int rc = lds_opt_in<k_attn_fwd<G, VO, DPs...>>(lds_max, name)) return rc;
    hipLaunchKernelGGL((k_attn_fwd<G, VO, DPs...>), grid, dim3(256), lds, st, q, k, v, o, lse, g, scale, dps...);
    return VQW_OK;
}
template <class G, class VO, class... DPs>
static int at_bwd_launch(const char* name, const G& g, dim3 grid, int lds_max, int lds, long segments, const float* q, const float* k,
                         const float* v, const float* o, const float* go, const float* lse, float* D, float* gq, float* gk, float* gv, float scale,
                         hipStream_t st, DPs... dps) {
    if (int rc = lds_opt_in<k_attn_dq<G, VO, DPs...>>(lds_max, name)) return rc;
    if (int rc = lds_opt_in<k_attn_dkdv<G, VO, DPs...>>(lds_max, name)) return rc;
    hipLaunchKernelGGL((k_attn_rowdot<typename G::RowDot>), dim3(ceil_div(segments, 4)), dim3(256), 0, st, go, o, D, segments, g.rowdot());
    hipLaunchKernelGGL((k_attn_dq<G, VO, DPs...>), grid, dim3(256), lds, st, q, k, v, go, lse, D, gq, g, scale, dps...);
    hipLaunchKernelGGL((k_attn_dkdv<G, VO, DPs...>), grid, dim3(256), lds, st, q, k, v, go, lse, D, gk, gv, g, scale, dps...);
    return VQW_OK;
}

static int at_spatial_check(const char* name, int B, int N, int C) {
    VQW_CHECK(B >= 1 && B <= 65535 && N >= 1 && N <= (1 << 20), "%s: bad shape B=%d N=%d", name, B, N);
    VQW_CHECK(C >= 32 && ((C % 32 == 0 && C <= AT_MAX_C) || (C % 64 == 0 && C <= AT_MAX_C2)),
              "%s: C=%d must be a multiple of 32 up to %d or a multiple of 64 up to %d", name, C, AT_MAX_C, AT_MAX_C2);
    return VQW_OK;
}
// column windows of the value / output side (the grid's z dimension), and the 128-channel blocks of one window
static inline int at_windows(int C) { return C > AT_MAX_C ? 2 : 1; }
static inline int at_ct(int C) { return ceil_div(C / at_windows(C), AT_KC); }
// the spatial instantiations: up to 512 channels one window of one to four blocks; 576 ... 1024 channels two windows of
// 288 ... 512, three or four blocks, with the folded score sums.  f(geometry, CT) launches.
template <class F>
static int at_spatial_dispatch(int N, int C, F f) {
    if (at_windows(C) == 2) {
        const AtSpatial<true> g{N, C};
        return at_ct(C) == 3 ? f(g, std::integral_constant<int, 3>()) : f(g, std::integral_constant<int, 4>());
    }
    const AtSpatial<false> g{N, C};
    switch (at_ct(C)) {
        case 1: return f(g, std::integral_constant<int, 1>());
        case 2: return f(g, std::integral_constant<int, 2>());
        case 3: return f(g, std::integral_constant<int, 3>());
        default: return f(g, std::integral_constant<int, 4>());
    }
}

extern "C" int vqw_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int C, float scale,
                                 void* stream) {
    VQW_CHECK(q && k && v && o && lse, "vqw_attention_fwd: null pointer");
    if (int rc = at_spatial_check("vqw_attention_fwd", B, N, C)) return rc;
    VQW_CHECK(al16(q) && al16(k) && al16(v), "vqw_attention_fwd: tensors must be 16-byte aligned");
    const dim3 grid(ceil_div(N, AT_BM), B, at_windows(C));
    const int lds = at_lds_bytes(AT_KC + 4, true);
    if (int rc = at_spatial_dispatch(N, C, [&](auto g, auto ct) {
            return at_fwd_launch<decltype(g), AtWindows<decltype(ct)::value>>("vqw_attention_fwd", g, grid, lds, lds, q, k, v, o, lse, scale, (hipStream_t)stream);
        }))
        return rc;
    VQW_LAUNCH_CHECK("vqw_attention_fwd");
    return VQW_OK;
}

extern "C" int vqw_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                 float* d_ws, float* gq, float* gk, float* gv, int B, int N, int C, float scale, void* stream) {
    VQW_CHECK(q && k && v && o && lse && go && d_ws && gq && gk && gv, "vqw_attention_bwd: null pointer");
    if (int rc = at_spatial_check("vqw_attention_bwd", B, N, C)) return rc;
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && al16(go), "vqw_attention_bwd: tensors must be 16-byte aligned");
    const dim3 grid(ceil_div(N, AT_BM), B, at_windows(C));
    const int lds = at_lds_bytes(AT_KC + 4, true);
    if (int rc = at_spatial_dispatch(N, C, [&](auto g, auto ct) {
            return at_bwd_launch<decltype(g), AtWindows<decltype(ct)::value>>("vqw_attention_bwd", g, grid, lds, lds, (long)B * N, q, k, v, o, go, lse, d_ws, gq, gk, gv,
                                                            scale, (hipStream_t)stream);
        }))
        return rc;
    VQW_LAUNCH_CHECK("vqw_attention_bwd");
    return VQW_OK;
}

static int at_causal_check(const char* name, int B, int Tq, int Tk, int nh, int hs, int causal, int nu) {
    VQW_CHECK(hs % 32 == 0 && hs >= 32 && hs <= AT_KC, "%s: head size hs=%d must be a multiple of 32 with 32 <= hs <= %d", name, hs, AT_KC);
    VQW_CHECK(Tq >= 1 && Tq <= AT_MAX_T && Tk >= 1 && Tk <= AT_MAX_T, "%s: Tq=%d, Tk=%d must satisfy 1 <= T <= %d", name, Tq, Tk, AT_MAX_T);
    VQW_CHECK(B >= 1 && nh >= 1 && (long)B * nh <= 65535, "%s: B=%d, n_head=%d must satisfy 1 <= B * n_head <= 65535", name, B, nh);
    VQW_CHECK(!causal || Tq == Tk, "%s: the causal mask needs Tq == Tk (got Tq=%d, Tk=%d)", name, Tq, Tk);
    VQW_CHECK(nu >= 0 && nu <= Tk && (causal || nu == 0), "%s: n_unmasked=%d must satisfy 0 <= n_unmasked <= T=%d (and be 0 without the causal mask)",
              name, nu, Tk);
    return VQW_OK;
}

extern "C" int vqw_causal_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Tq, int Tk, int n_head,
                                        int hs, float scale, int causal, int n_unmasked, void* stream) {
    if (int rc = at_causal_check("vqw_causal_attention_fwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    VQW_CHECK(q && k && v && o && lse, "vqw_causal_attention_fwd: null pointer");
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o), "vqw_causal_attention_fwd: tensors must be 16-byte aligned");
    const AtCausal g{Tq, Tk, n_head, hs, causal ? 1 : 0, n_unmasked};
    if (int rc = at_fwd_launch<AtCausal, AtKeySplits>("vqw_causal_attention_fwd", g, dim3(ceil_div(Tq, AT_BM), B * n_head),
                                                      at_lds_bytes(AT_KC + 4, false), at_lds_bytes(hs + 4, false), q, k, v, o, lse, scale,
                                                      (hipStream_t)stream))
        return rc;
    VQW_LAUNCH_CHECK("vqw_causal_attention_fwd");
    return VQW_OK;
}

extern "C" int vqw_causal_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                        float* d_ws, float* gq, float* gk, float* gv, int B, int Tq, int Tk, int n_head, int hs, float scale,
                                        int causal, int n_unmasked, void* stream) {
    if (int rc = at_causal_check("vqw_causal_attention_bwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    VQW_CHECK(Tq == Tk, "vqw_causal_attention_bwd: the backward needs Tq == Tk (got Tq=%d, Tk=%d): the layer_past route is forward only", Tq, Tk);
    VQW_CHECK(q && k && v && o && lse && go && d_ws && gq && gk && gv, "vqw_causal_attention_bwd: null pointer");
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && al16(go) && al16(gq) && al16(gk) && al16(gv),
              "vqw_causal_attention_bwd: tensors must be 16-byte aligned");
    const AtCausal g{Tq, Tk, n_head, hs, causal ? 1 : 0, n_unmasked};
    if (int rc = at_bwd_launch<AtCausal, AtKeySplits>("vqw_causal_attention_bwd", g, dim3(ceil_div(Tq, AT_BM), B * n_head),
                                                      at_lds_bytes(AT_KC + 4, true), at_lds_bytes(hs + 4, true), (long)B * Tq * n_head, q, k, v, o, go,
                                                      lse, d_ws, gq, gk, gv, scale, (hipStream_t)stream))
        return rc;
    VQW_LAUNCH_CHECK("vqw_causal_attention_bwd");
    return VQW_OK;
}

// ---- the same two passes with dropout on the probabilities (the drop policy): the contract and the checks of the functions above
static int at_drop_check(const char* name, int Tq, int Tk, float p) {
    VQW_CHECK(Tq == Tk, "%s: dropout needs Tq == Tk (got Tq=%d, Tk=%d): the layer_past route is inference only", name, Tq, Tk);
    VQW_CHECK(p >= 0.f && p < 1.f, "%s: p=%g must lie in [0, 1)", name, (double)p);
    return VQW_OK;
}

extern "C" int vqw_causal_attention_drop_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int Tq, int Tk,
                                             int n_head, int hs, float scale, int causal, int n_unmasked, float p, long seed, long call,
                                             int site, void* stream) {
    if (int rc = at_causal_check("vqw_causal_attention_drop_fwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    if (int rc = at_drop_check("vqw_causal_attention_drop_fwd", Tq, Tk, p)) return rc;
    VQW_CHECK(q && k && v && o && lse, "vqw_causal_attention_drop_fwd: null pointer");
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o), "vqw_causal_attention_drop_fwd: tensors must be 16-byte aligned");
    const AtCausal g{Tq, Tk, n_head, hs, causal ? 1 : 0, n_unmasked};
    if (int rc = at_fwd_launch<AtCausal, AtKeySplits, AtDrop>("vqw_causal_attention_drop_fwd", g, dim3(ceil_div(Tq, AT_BM), B * n_head),
                                                              at_lds_bytes(AT_KC + 4, false), at_lds_bytes(hs + 4, false), q, k, v, o, lse, scale,
                                                              (hipStream_t)stream, AtDrop{dk_make(p, seed, call, site)}))
        return rc;
    VQW_LAUNCH_CHECK("vqw_causal_attention_drop_fwd");
    return VQW_OK;
}

extern "C" int vqw_causal_attention_drop_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* go,
                                             float* d_ws, float* gq, float* gk, float* gv, int B, int Tq, int Tk, int n_head, int hs, float scale,
                                             int causal, int n_unmasked, float p, long seed, long call, int site, void* stream) {
    if (int rc = at_causal_check("vqw_causal_attention_drop_bwd", B, Tq, Tk, n_head, hs, causal, n_unmasked)) return rc;
    if (int rc = at_drop_check("vqw_causal_attention_drop_bwd", Tq, Tk, p)) return rc;
    VQW_CHECK(q && k && v && o && lse && go && d_ws && gq && gk && gv, "vqw_causal_attention_drop_bwd: null pointer");
    VQW_CHECK(al16(q) && al16(k) && al16(v) && al16(o) && al16(go) && al16(gq) && al16(gk) && al16(gv),
              "vqw_causal_attention_drop_bwd: tensors must be 16-byte aligned");
    const AtCausal g{Tq, Tk, n_head, hs, causal ? 1 : 0, n_unmasked};
    if (int rc = at_bwd_launch<AtCausal, AtKeySplits, AtDrop>("vqw_causal_attention_drop_bwd", g, dim3(ceil_div(Tq, AT_BM), B * n_head),
                                                              at_lds_bytes(AT_KC + 4, true), at_lds_bytes(hs + 4, true), (long)B * Tq * n_head, q, k, v,
                                                              o, go, lse, d_ws, gq, gk, gv, scale, (hipStream_t)stream,
                                                              AtDrop{dk_make(p, seed, call, site)}))
        return rc;
    VQW_LAUNCH_CHECK("vqw_causal_attention_drop_bwd");
    return VQW_OK;
}
