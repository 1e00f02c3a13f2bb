// Scores of a generative prior's samples over feature rows X[N][D] (fp32, dense): the double moments behind a Frechet distance
// and the two N x M nearest-neighbour problems behind precision / recall (Kynkaanniemi et al. 2019) and density / coverage
// (Naeem et al. 2020).  The reference has nothing of this; tests/sample_scores_ref.py restates it in float64.
//
// Every kernel uses a row as y = fp32(x - shift): one fp32 subtraction per element while staging, shift = NULL means 0.
//
//   vqw_feature_moments   sum[D] += sum_n y, outer[D][D] += sum_n y y^T, both double.  Plain double FMAs (the product of two
//                         fp32 values is exact in double): a workgroup owns a 64 x 64 tile of the upper triangle and one split
//                         of the rows, a thread a 4 x 4 block of it, and walks its rows in order; the splits are folded in
//                         index order by a second kernel that writes both triangles from the one folded value.  No atomics.
//   vqw_knn_radius        r2[i] = the k-th smallest d2(i, j) over j != i (by index).
//   vqw_ball_counts       cnt_q[q] = #{i : d2(q, a_i) <= r2[i]}, hit_a[i] = #{q : d2(q, a_i) <= r2[i]}.
//
// The two distance kernels are one tile engine, k_ss_engine<MODE>: a workgroup owns 64 queries and walks the centres 64 at a
// time.  Up to 512 columns the query tile is staged once and stays in LDS (136 KB at 512) while the centre tiles stream through in
// chunks of 32 columns; above, both tiles go through LDS chunk by chunk.  Tails are zero-padded in LDS and the products run on the
// exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32).  The centres are the A operand and the queries the B operand, so a lane holds ONE query and 16
// centres of a 32 x 32 block: the row reduction - a running 8-smallest list, or a count - stays in the lane's registers while the
// centres stream by and is merged across the four partial lists of a query through LDS once, at the end.  The N x M distances
// never reach memory; the workspace holds the N + M squared norms and nothing else.
//
//   d2 = max(0, |q|^2 + |a|^2 - 2 q.a)
//
// Bit-identical rows have distance exactly 0: the squared norms are the engine's own diagonal Gram entries - k_ss_norms runs the
// same instruction over the same column order with the row as both operands - so |q|^2, |a|^2 and q.a are one fp32 value s and
// 2 s - 2 s cancels exactly (with or without contraction of the last two operations).
#include "common.h"
#include "mfma_util.h"
#include "../../include/vqwnet_hip.h"

#define SS_MAX_D 2048
#define SS_MAX_K 8
#define SS_MAX_ROWS (1L << 30)     // N, M: int32 counts and the grid (rows / 64 workgroups) hold well beyond it
#define SS_BLOCK 256
#define SS_BM 64                   // queries per workgroup
#define SS_BN 64                   // centres per step
#define SS_KC 32                   // columns per LDS chunk
#define SS_LD (SS_KC + 1)          // padded row: the 32 rows a wave reads land in different banks
#define SS_RES_MAX_D 512           // the query tile stays in LDS up to this many columns
#define SS_RES_LDS_MAX ((SS_BM * (SS_RES_MAX_D + 33) + SS_BN * SS_LD) * 4)     // 147968 bytes + 9 KB static of the 160 KB

#define FM_T 64                    // outer-product tile side
#define FM_RC 16                   // rows staged per step
#define FM_MAX_SPLITS 16
#define FM_WG_TARGET 512           // workgroups aimed at: tiles x splits

static size_t ss_align(size_t b) { return (b + 255) & ~(size_t)255; }
static bool al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
static bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// moments
static int fm_tiles(int D) { return ceil_div(D, FM_T); }
static int fm_splits(long N, int D) {
    const int nt = fm_tiles(D), ntu = nt * (nt + 1) / 2;
    long s = ceil_div(FM_WG_TARGET, ntu);
    const long by_rows = (N + FM_RC - 1) / FM_RC;
    if (s > by_rows) s = by_rows;
    if (s > FM_MAX_SPLITS) s = FM_MAX_SPLITS;
    return (int)(s < 1 ? 1 : s);
}

extern "C" size_t vqw_feature_moments_ws_bytes(long N, int D) {
    if (N < 1 || D < 1 || D > SS_MAX_D) return 0;
    const int nt = fm_tiles(D), ntu = nt * (nt + 1) / 2, S = fm_splits(N, D);
    return ss_align((size_t)S * ntu * FM_T * FM_T * sizeof(double)) + ss_align((size_t)S * D * sizeof(double));
}

// upper-triangle tile number -> (ti, tj), ti <= tj, rows of tiles in order
__device__ __forceinline__ void fm_tile(int t, int nt, int& ti, int& tj) {
    ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    tj = ti + t;
}

// grid (upper tiles, splits): part[s][tile][64][64] = sum over the rows of split s, in row order, of y_i y_j
__global__ __launch_bounds__(SS_BLOCK) void k_fm_outer(const float* __restrict__ X, const float* __restrict__ shift,
                                                       double* __restrict__ part, long N, int D, int nt, long rows_per_split) {
    __shared__ __attribute__((aligned(16))) float sI[FM_RC][FM_T];
    __shared__ __attribute__((aligned(16))) float sJ[FM_RC][FM_T];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int ti, tj;
    fm_tile(blockIdx.x, nt, ti, tj);
    const long n0 = (long)blockIdx.y * rows_per_split;
    const long n1 = n0 + rows_per_split < N ? n0 + rows_per_split : N;
    const int col = tid & 63, r0 = tid >> 6;
    const int di = ti * FM_T + col, dj = tj * FM_T + col;
    const float shi = (shift && di < D) ? shift[di] : 0.f, shj = (shift && dj < D) ? shift[dj] : 0.f;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (long nb = n0; nb < n1; nb += FM_RC) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < FM_RC / 4; ++i) {
            const int r = r0 + 4 * i;
            const long n = nb + r;
            const bool ok = n < n1;
            sI[r][col] = (ok && di < D) ? X[n * D + di] - shi : 0.f;
            sJ[r][col] = (ok && dj < D) ? X[n * D + dj] - shj : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < FM_RC; ++r) {
            const float4 vi = *(const float4*)&sI[r][ty * 4];
            const float4 vj = *(const float4*)&sJ[r][tx * 4];
            const double a4[4] = {(double)vi.x, (double)vi.y, (double)vi.z, (double)vi.w};
            const double b4[4] = {(double)vj.x, (double)vj.y, (double)vj.z, (double)vj.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(a4[a], b4[b], acc[a][b]);
        }
    }
    double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (FM_T * FM_T);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) o[(ty * 4 + a) * FM_T + tx * 4 + b] = acc[a][b];
}

// grid (ceil(D / 256), splits): psum[s][d] = sum over the rows of split s, in row order, of y_d
__global__ __launch_bounds__(SS_BLOCK) void k_fm_colsum(const float* __restrict__ X, const float* __restrict__ shift,
                                                        double* __restrict__ psum, long N, int D, long rows_per_split) {
    const int d = blockIdx.x * SS_BLOCK + threadIdx.x;
    if (d >= D) return;
    const long n0 = (long)blockIdx.y * rows_per_split;
    const long n1 = n0 + rows_per_split < N ? n0 + rows_per_split : N;
    const float sh = shift ? shift[d] : 0.f;
    double s = 0.0;
    for (long n = n0; n < n1; ++n) s += (double)(X[n * D + d] - sh);
    psum[(size_t)blockIdx.y * D + d] = s;
}

// grid (upper tiles): the splits in index order, added to what `outer` / `sum` hold; both triangles get the one folded value
__global__ __launch_bounds__(SS_BLOCK) void k_fm_fold(const double* __restrict__ part, const double* __restrict__ psum,
                                                      double* __restrict__ sum, double* __restrict__ outer, int D, int nt, int S) {
    int ti, tj;
    fm_tile(blockIdx.x, nt, ti, tj);
    for (int e = threadIdx.x; e < FM_T * FM_T; e += SS_BLOCK) {
        const int i = ti * FM_T + (e >> 6), j = tj * FM_T + (e & 63);
        if (i >= D || j >= D) continue;
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += part[((size_t)s * gridDim.x + blockIdx.x) * (FM_T * FM_T) + e];
        const double r = outer[(size_t)i * D + j] + v;
        outer[(size_t)i * D + j] = r;
        if (ti != tj) outer[(size_t)j * D + i] = r;
    }
    if (blockIdx.x == 0)
        for (int d = threadIdx.x; d < D; d += SS_BLOCK) {
            double v = 0.0;
            for (int s = 0; s < S; ++s) v += psum[(size_t)s * D + d];
            sum[d] += v;
        }
}

extern "C" int vqw_feature_moments(const float* x, const float* shift, double* sum, double* outer, void* ws, size_t ws_bytes,
                                   long N, int D, void* stream) {
    VQW_CHECK(D >= 1 && D <= SS_MAX_D, "vqw_feature_moments: D=%d out of [1, %d]", D, SS_MAX_D);
    VQW_CHECK(N >= 1 && N <= SS_MAX_ROWS, "vqw_feature_moments: N=%ld out of [1, %ld]", N, SS_MAX_ROWS);
    VQW_CHECK(x && sum && outer && ws, "vqw_feature_moments: x, sum, outer and ws must not be null");
    VQW_CHECK(al4(x) && al4(shift), "vqw_feature_moments: x and shift must be 4-byte aligned");
    VQW_CHECK(al8(sum) && al8(outer) && al8(ws), "vqw_feature_moments: sum, outer and ws must be 8-byte aligned");
    const size_t need = vqw_feature_moments_ws_bytes(N, D);
    VQW_CHECK(ws_bytes >= need, "vqw_feature_moments: workspace too small (%zu < %zu)", ws_bytes, need);
    const int nt = fm_tiles(D), ntu = nt * (nt + 1) / 2, S = fm_splits(N, D);
    long rps = (N + S - 1) / S;
    rps = (rps + FM_RC - 1) / FM_RC * FM_RC;
    double* part = (double*)ws;
    double* psum = (double*)((char*)ws + ss_align((size_t)S * ntu * FM_T * FM_T * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    k_fm_outer<<<dim3(ntu, S), SS_BLOCK, 0, st>>>(x, shift, part, N, D, nt, rps);
    k_fm_colsum<<<dim3(ceil_div(D, SS_BLOCK), S), SS_BLOCK, 0, st>>>(x, shift, psum, N, D, rps);
    k_fm_fold<<<ntu, SS_BLOCK, 0, st>>>(part, psum, sum, outer, D, nt, S);
    VQW_LAUNCH_CHECK("vqw_feature_moments");
    return VQW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// squared norms: the diagonal of the 32 x 32 Gram block of a wave's rows, through the engine's instruction in the engine's
// column order (columns 2 s and 2 s + 1 in step s, from 0)
__global__ __launch_bounds__(SS_BLOCK) void k_ss_norms(const float* __restrict__ X, const float* __restrict__ shift,
                                                       float* __restrict__ nrm, long N, int D) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const long row = ((long)blockIdx.x * (SS_BLOCK / 64) + w) * 32 + c;
    const bool ok = row < N;
    const float* p = X + (ok ? row : 0) * D;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < D; k0 += 2) {
        const int k = k0 + h;
        const float y = (ok && k < D) ? p[k] - (shift ? shift[k] : 0.f) : 0.f;
        acc = MFMA32(y, y, acc);
    }
    // element (c, c) of the block: register (c & 3) + 4 (c >> 3) of the lane half (c >> 2) & 1
    const int want = (c & 3) + 4 * (c >> 3);
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) v = (i == want) ? acc[i] : v;
    if (ok && h == ((c >> 2) & 1)) nrm[row] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
struct SsArgs {
    const float* Q;        // [M][D] queries
    const float* A;        // [N][D] centres
    const float* shift;    // [D] or null
    const float* nq;       // [M] squared norms
    const float* na;       // [N]
    const float* r2;       // [N] (ball counts)
    float* out_r2;         // [M] (knn)
    int* cnt_q;            // [M]
    int* hit_a;            // [N]
    long M, N;
    int D, k;
};

// MODE 0: the k-th smallest distance of every query to the centres other than itself (Q == A).  MODE 1: ball counts.
// RES: the query tile is staged ONCE, all D columns of it (row stride ldq floats), and stays in LDS while the centre tiles stream by
// (D <= SS_RES_MAX_D: 64 rows of 512 columns are 136 KB); otherwise it is staged again with every chunk, like the centres.  Both
// feed the matrix cores the same values in the same order: the same bits.
// Dynamic LDS: the query tile [64][ldq], then the centre chunk [64][SS_LD].
template <int MODE, bool RES>
__global__ __launch_bounds__(SS_BLOCK) void k_ss_engine(SsArgs a, int ldq) {
    extern __shared__ float ss_dyn[];
    float* const sQ = ss_dyn;
    float* const sA = ss_dyn + SS_BM * ldq;
    __shared__ float sbest[SS_BM][4][SS_MAX_K];
    __shared__ int scnt[SS_BM][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wq = w & 1, wc = w >> 1, c = lane & 31, h = lane >> 5;
    const long q0 = (long)blockIdx.x * SS_BM;
    const long q = q0 + wq * 32 + c;                  // this lane's query
    const bool qok = q < a.M;
    const float nqv = qok ? a.nq[q] : 0.f;
    const int D = a.D;
    const int scol = tid & 31, srow = tid >> 5;       // staging: 8 rows of each tile per thread, one column
    float best[SS_MAX_K];
#pragma unroll
    for (int t = 0; t < SS_MAX_K; ++t) best[t] = INFINITY;
    int cnt = 0;
    if (RES) {                                        // the whole query tile, columns padded with zeros to a multiple of SS_KC
        const int Dp = (D + SS_KC - 1) / SS_KC * SS_KC;
        for (int idx = tid; idx < SS_BM * Dp; idx += SS_BLOCK) {
            const int r = idx / Dp, kk = idx - r * Dp;
            const long gq = q0 + r;
            sQ[r * ldq + kk] = (kk < D && gq < a.M) ? a.Q[gq * D + kk] - (a.shift ? a.shift[kk] : 0.f) : 0.f;
        }
    }
    for (long a0 = 0; a0 < a.N; a0 += SS_BN) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int k0 = 0; k0 < D; k0 += SS_KC) {
            const int kk = k0 + scol;
            const bool kok = kk < D;
            const float sh = (a.shift && kok) ? a.shift[kk] : 0.f;
            __syncthreads();                          // the previous chunk has been read
#pragma unroll
            for (int i = 0; i < SS_BM / 8; ++i) {
                const int r = srow + 8 * i;
                const long gq = q0 + r, ga = a0 + r;
                if (!RES) sQ[r * ldq + scol] = (kok && gq < a.M) ? a.Q[gq * D + kk] - sh : 0.f;
                sA[r * SS_LD + scol] = (kok && ga < a.N) ? a.A[ga * D + kk] - sh : 0.f;
            }
            __syncthreads();
            const float* pa = &sA[(wc * 32 + c) * SS_LD + h];
            const float* pq = &sQ[(wq * 32 + c) * ldq + (RES ? k0 : 0) + h];
#pragma unroll
            for (int s = 0; s < SS_KC / 2; ++s) acc = MFMA32(pa[2 * s], pq[2 * s], acc);
        }
        // the block: column = this lane's query, register i = centre (i & 3) + 8 (i >> 2) + 4 h of the wave's 32
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long ci = a0 + wc * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool cok = ci < a.N;
            const float nav = cok ? a.na[ci] : 0.f;
            const float d2 = fmaxf(0.f, (nqv + nav) - 2.f * acc[i]);
            if (MODE == 0) {
                if (cok && ci != q && d2 < best[SS_MAX_K - 1]) {
                    float v = d2;
#pragma unroll
                    for (int t = 0; t < SS_MAX_K; ++t) {
                        const float lo = fminf(best[t], v);
                        v = fmaxf(best[t], v);
                        best[t] = lo;
                    }
                }
            } else {
                const bool inside = cok && qok && d2 <= a.r2[ci];          // a NaN radius contains nobody
                cnt += inside ? 1 : 0;
                const unsigned long long m = __ballot(inside);
                if (lane == 0) {
                    const int lo = __popc((unsigned)(m & 0xffffffffu)), hi = __popc((unsigned)(m >> 32));
                    const long base = a0 + wc * 32 + (i & 3) + 8 * (i >> 2);
                    if (lo) atomicAdd(&a.hit_a[base], lo);
                    if (hi) atomicAdd(&a.hit_a[base + 4], hi);
                }
            }
        }
    }
    // the four partial results of a query: two lane halves of two waves
    const int ql = wq * 32 + c, src = wc * 2 + h;
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < SS_MAX_K; ++t) sbest[ql][src][t] = best[t];
        __syncthreads();
        if (tid < SS_BM && q0 + tid < a.M) {
            float m8[SS_MAX_K];
#pragma unroll
            for (int t = 0; t < SS_MAX_K; ++t) m8[t] = INFINITY;
            for (int s = 0; s < 4; ++s)
                for (int u = 0; u < SS_MAX_K; ++u) {
                    float v = sbest[tid][s][u];
#pragma unroll
                    for (int t = 0; t < SS_MAX_K; ++t) {
                        const float lo = fminf(m8[t], v);
                        v = fmaxf(m8[t], v);
                        m8[t] = lo;
                    }
                }
            float r = m8[0];
#pragma unroll
            for (int t = 1; t < SS_MAX_K; ++t) r = (t == a.k - 1) ? m8[t] : r;
            a.out_r2[q0 + tid] = r;
        }
    } else {
        scnt[ql][src] = cnt;
        __syncthreads();
        if (tid < SS_BM && q0 + tid < a.M) a.cnt_q[q0 + tid] = (scnt[tid][0] + scnt[tid][1]) + (scnt[tid][2] + scnt[tid][3]);
    }
}

// One launch of the engine over `rows` queries: the resident form up to SS_RES_MAX_D columns (its dynamic LDS limit is raised once,
// to the largest tile), else the re-staging form.
template <int MODE>
static int ss_launch(const SsArgs& g, long rows, const char* name, hipStream_t st) {
    const int Dp = ceil_div(g.D, SS_KC) * SS_KC;
    const bool res = g.D <= SS_RES_MAX_D;
    const int ldq = res ? (Dp % 64 == 0 ? Dp + 33 : Dp + 1) : SS_LD;          // an odd multiple of 33 modulo 64 banks either way
    const int bytes = (SS_BM * ldq + SS_BN * SS_LD) * (int)sizeof(float);
    const int grid = ceil_div(rows, SS_BM);
    if (res) {
        if (lds_opt_in<k_ss_engine<MODE, true>>(SS_RES_LDS_MAX, name) != VQW_OK) return VQW_ERR_HIP;
        k_ss_engine<MODE, true><<<grid, SS_BLOCK, bytes, st>>>(g, ldq);
    } else {
        k_ss_engine<MODE, false><<<grid, SS_BLOCK, bytes, st>>>(g, ldq);
    }
    return VQW_OK;
}

static int ss_check_rows(const char* name, const char* what, long n) {
    VQW_CHECK(n >= 1 && n <= SS_MAX_ROWS, "%s: %s=%ld out of [1, %ld] (int32 counts, one workgroup per 64 rows)", name, what, n,
              SS_MAX_ROWS);
    return VQW_OK;
}

extern "C" size_t vqw_knn_radius_ws_bytes(long N) {
    return N < 1 ? 0 : ss_align((size_t)N * sizeof(float));
}

extern "C" size_t vqw_ball_counts_ws_bytes(long M, long N) {
    return (M < 1 || N < 1) ? 0 : ss_align((size_t)M * sizeof(float)) + ss_align((size_t)N * sizeof(float));
}

extern "C" int vqw_knn_radius(const float* a, const float* shift, float* r2, void* ws, size_t ws_bytes, long N, int D, int k,
                              void* stream) {
    VQW_CHECK(D >= 1 && D <= SS_MAX_D, "vqw_knn_radius: D=%d out of [1, %d]", D, SS_MAX_D);
    VQW_CHECK(k >= 1 && k <= SS_MAX_K, "vqw_knn_radius: k=%d out of [1, %d]", k, SS_MAX_K);
    VQW_CHECK(N >= (long)k + 1, "vqw_knn_radius: N=%ld must be at least k + 1 = %d (self is excluded)", N, k + 1);
    if (ss_check_rows("vqw_knn_radius", "N", N) != VQW_OK) return VQW_ERR_ARG;
    VQW_CHECK(a && r2 && ws, "vqw_knn_radius: a, r2 and ws must not be null");
    VQW_CHECK(al4(a) && al4(shift) && al4(r2) && al4(ws), "vqw_knn_radius: a, shift, r2 and ws must be 4-byte aligned");
    const size_t need = vqw_knn_radius_ws_bytes(N);
    VQW_CHECK(ws_bytes >= need, "vqw_knn_radius: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* na = (float*)ws;
    k_ss_norms<<<ceil_div(N, 128), SS_BLOCK, 0, st>>>(a, shift, na, N, D);
    SsArgs g = {};
    g.Q = a; g.A = a; g.shift = shift; g.nq = na; g.na = na; g.out_r2 = r2; g.M = N; g.N = N; g.D = D; g.k = k;
    if (ss_launch<0>(g, N, "vqw_knn_radius", st) != VQW_OK) return VQW_ERR_HIP;
    VQW_LAUNCH_CHECK("vqw_knn_radius");
    return VQW_OK;
}

extern "C" int vqw_ball_counts(const float* q, const float* a, const float* r2, const float* shift, int32_t* cnt_q, int32_t* hit_a,
                               void* ws, size_t ws_bytes, long M, long N, int D, void* stream) {
    VQW_CHECK(D >= 1 && D <= SS_MAX_D, "vqw_ball_counts: D=%d out of [1, %d]", D, SS_MAX_D);
    if (ss_check_rows("vqw_ball_counts", "M", M) != VQW_OK || ss_check_rows("vqw_ball_counts", "N", N) != VQW_OK) return VQW_ERR_ARG;
    VQW_CHECK(q && a && r2 && cnt_q && hit_a && ws, "vqw_ball_counts: q, a, r2, cnt_q, hit_a and ws must not be null");
    VQW_CHECK(al4(q) && al4(a) && al4(r2) && al4(shift) && al4(cnt_q) && al4(hit_a) && al4(ws),
              "vqw_ball_counts: every pointer must be 4-byte aligned");
    const size_t need = vqw_ball_counts_ws_bytes(M, N);
    VQW_CHECK(ws_bytes >= need, "vqw_ball_counts: workspace too small (%zu < %zu)", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* nq = (float*)ws;
    float* na = (float*)((char*)ws + ss_align((size_t)M * sizeof(float)));
    if (hipMemsetAsync(hit_a, 0, sizeof(int32_t) * (size_t)N, st) != hipSuccess) {
        vqw_set_error("vqw_ball_counts: clearing hit_a failed");
        return VQW_ERR_HIP;
    }
    k_ss_norms<<<ceil_div(M, 128), SS_BLOCK, 0, st>>>(q, shift, nq, M, D);
    k_ss_norms<<<ceil_div(N, 128), SS_BLOCK, 0, st>>>(a, shift, na, N, D);
    SsArgs g = {};
    g.Q = q; g.A = a; g.shift = shift; g.nq = nq; g.na = na; g.r2 = r2; g.cnt_q = cnt_q; g.hit_a = hit_a;
    g.M = M; g.N = N; g.D = D; g.k = 0;
    if (ss_launch<1>(g, M, "vqw_ball_counts", st) != VQW_OK) return VQW_ERR_HIP;
    VQW_LAUNCH_CHECK("vqw_ball_counts");
    return VQW_OK;
}
