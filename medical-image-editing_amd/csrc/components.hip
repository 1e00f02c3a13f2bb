// Lesion-wise detection scores (functions/lesion_scores.py LesionScores, trainers/fit.py Fit.detect): connected components of a
// thresholded score map or a mask, their areas, and the matching of predicted components against ground-truth components.  The
// definitions are in include/vqwnet_hip.h.  Integer atomics only (a minimum and a count have no order): the same bits every run.
//
// No workgroup ever waits for another: there is no flag, no spin and no cooperative launch; kernel boundaries order the passes.
// Every find / union loop walks a strictly decreasing index (a parent is never larger than its child), so it ends; on top of that
// each walk counts its steps against a bound and past it stops and sets the error word - a wrong kernel fails a test, it does not
// hold a card.
#include "common.h"
#include "../../include/vqwnet_hip.h"

#define CC_TY 32
#define CC_TX 64
#define CC_TILE (CC_TY * CC_TX)
#define CC_CHUNK 1024            // pixels of one numbering chunk: 256 threads x 4 consecutive pixels
#define CC_BG (-1)               // background in the parent array

#define CC_ERR_TILE 1            // a walk inside a tile passed its bound
#define CC_ERR_SEAM 2            // a walk of the seam pass passed its bound
#define CC_ERR_FLATTEN 4         // a walk of the flatten pass passed its bound
#define CC_ERR_CAP 8             // component_areas met a label outside [0, cap]

// ------------------------------------------------------------------------------------------------ pass 1: one tile in LDS
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// union of the tile-local indices a and b by the minimum rule; steps: the walk's budget (every hop and every retry takes one)
__device__ __forceinline__ bool lds_unite(int* p, int a, int b) {
    int steps = 0;
    for (;;) {
        for (int q; (q = lds_ld(p + a)) != a && steps <= 4 * CC_TILE; a = q) ++steps;          // q < a: strictly decreasing
        for (int q; (q = lds_ld(p + b)) != b && steps <= 4 * CC_TILE; b = q) ++steps;
        if (steps > 4 * CC_TILE) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return true;          // a was still a root: linked
        a = old;                            // it was not: old < a, go on from there (p[a] is now min(old, b): both lie in the component)
        ++steps;
    }
}

__global__ void __launch_bounds__(256) k_cc_tile(const uint8_t* __restrict__ mask, const float* __restrict__ scores, float thr,
                                                 int* __restrict__ P, int* __restrict__ err, int H, int W, int tilesX, int tilesY,
                                                 int conn8) {
    __shared__ int p[CC_TILE];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / (tilesX * tilesY), rem = blockIdx.x - n * (tilesX * tilesY);
    const int ty = rem / tilesX, tx = rem - ty * tilesX;
    const int y0 = ty * CC_TY, x0 = tx * CC_TX, base = n * H * W;
    unsigned fg = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid + 256 * k, y = y0 + (e >> 6), x = x0 + (e & 63);
        bool f = false;
        if (y < H && x < W) {
            const int g = base + y * W + x;
            f = mask ? mask[g] != 0 : scores[g] >= thr;          // a NaN compares false: background
        }
        fg |= (f ? 1u : 0u) << k;
        p[e] = f ? e : CC_BG;
    }
    __syncthreads();
    // rows first: a pixel points at its left neighbour, then six rounds of pointer jumping reach the start of its run (a racing
    // read sees a newer, smaller ancestor of the same run: harmless)
    unsigned left = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid + 256 * k;
        if (((fg >> k) & 1u) && (e & 63) && p[e - 1] >= 0) left |= 1u << k;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((left >> k) & 1u) p[tid + 256 * k] = tid + 256 * k - 1;
    __syncthreads();
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = tid + 256 * k;
            if ((fg >> k) & 1u) {
                const int q = lds_ld(p + lds_ld(p + e));
                __hip_atomic_store(p + e, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
    }
    // then the row above.  N joins NW and NE already (they are in one run), and with W and NW set W has joined the row above.
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid + 256 * k, col = e & 63;
        if (!((fg >> k) & 1u) || e < CC_TX) continue;
        const bool w = col > 0 && lds_ld(p + e - 1) >= 0, nw = col > 0 && lds_ld(p + e - CC_TX - 1) >= 0;
        if (lds_ld(p + e - CC_TX) >= 0) {
            if (!(w && nw)) ok = lds_unite(p, e, e - CC_TX) && ok;
        } else if (conn8) {
            if (nw && !w) ok = lds_unite(p, e, e - CC_TX - 1) && ok;
            if (col < CC_TX - 1 && lds_ld(p + e - CC_TX + 1) >= 0) ok = lds_unite(p, e, e - CC_TX + 1) && ok;
        }
    }
    __syncthreads();
    // the provisional label: the GLOBAL index of the tile-local root (raster order in the tile is the global order restricted to it)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid + 256 * k, y = y0 + (e >> 6), x = x0 + (e & 63);
        if (y >= H || x >= W) continue;
        int out = CC_BG;
        if ((fg >> k) & 1u) {
            int r = e, steps = 0;
            for (int q; (q = p[r]) != r && steps <= CC_TILE; r = q) ++steps;
            ok = ok && steps <= CC_TILE;
            out = base + (y0 + (r >> 6)) * W + x0 + (r & 63);
        }
        P[base + y * W + x] = out;
    }
    if (!ok) atomicOr(err, CC_ERR_TILE);
}

// ------------------------------------------------------------------------------------------------ pass 2: the seams
// Parents are read with relaxed agent-scope atomic loads.  A plain load could see an old parent from a CU-local cache line; even
// that would be harmless here, because an old parent is still an ancestor and the decision to stop is taken only on the value the
// agent-scope atomicMin returned - the atomic has the last word.
__device__ __forceinline__ int g_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bound: the pixel count of the launch.  Each of the two walkers only ever descends through pixel indices, so together they take
// fewer than 2 bound steps; past that the walk gives up and the caller sets the error word.
__device__ __forceinline__ bool g_unite(int* P, int a0, int b0, int bound) {
    int a = a0, b = b0;
    unsigned steps = 0;
    const unsigned lim = 2u * (unsigned)bound;
    for (;;) {
        for (int q; (q = g_ld(P + a)) != a && steps <= lim; a = q) ++steps;          // q < a: strictly decreasing
        for (int q; (q = g_ld(P + b)) != b && steps <= lim; b = q) ++steps;
        if (steps > lim) return false;
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) break;                // a was still a root: linked under b
        a = old;                            // no longer a root: go on from the value the atomic returned (old < a)
        ++steps;
    }
    // shorten the two chains we walked: b is a smaller member of the same component, so the minimum keeps every invariant
    __hip_atomic_fetch_min(P + a0, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(P + b0, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// threads 0..63: the tile's top row against the row above (N, else NW and NE); threads 64..95: its left column against the column to
// the left (W, else NW and SW - the SW neighbour lies in the left tile and no other seam pixel of THIS tile visits it).  At a corner
// the diagonal neighbours lie in the diagonal tiles: the addresses are global, so they are reached like any other.
__global__ void __launch_bounds__(128) k_cc_seam(int* __restrict__ P, int* __restrict__ err, int H, int W, int tilesX, int tilesY,
                                                 int conn8, int bound) {
    const int t = threadIdx.x;
    const int n = blockIdx.x / (tilesX * tilesY), rem = blockIdx.x - n * (tilesX * tilesY);
    const int ty = rem / tilesX, tx = rem - ty * tilesX;
    const int y0 = ty * CC_TY, x0 = tx * CC_TX, base = n * H * W;
    bool ok = true;
    if (t < CC_TX) {
        const int x = x0 + t;
        if (y0 > 0 && x < W) {
            const int i = base + y0 * W + x, up = i - W;
            if (g_ld(P + i) >= 0) {
                if (g_ld(P + up) >= 0) ok = g_unite(P, i, up, bound);
                else if (conn8) {
                    if (x > 0 && g_ld(P + up - 1) >= 0) ok = g_unite(P, i, up - 1, bound);
                    if (x + 1 < W && g_ld(P + up + 1) >= 0) ok = g_unite(P, i, up + 1, bound) && ok;
                }
            }
        }
    } else if (t < CC_TX + CC_TY) {
        const int y = y0 + t - CC_TX;
        if (x0 > 0 && y < H) {
            const int i = base + y * W + x0, l = i - 1;
            if (g_ld(P + i) >= 0) {
                if (g_ld(P + l) >= 0) ok = g_unite(P, i, l, bound);
                else if (conn8) {
                    if (y > 0 && g_ld(P + l - W) >= 0) ok = g_unite(P, i, l - W, bound);
                    if (y + 1 < H && g_ld(P + l + W) >= 0) ok = g_unite(P, i, l + W, bound) && ok;
                }
            }
        }
    }
    if (!ok) atomicOr(err, CC_ERR_SEAM);
}

// ------------------------------------------------------------------------------------------------ pass 3: flatten, number, write
// exclusive prefix of v over the 256 threads of the workgroup, in thread order; total: the sum, in every thread
__device__ __forceinline__ int block_excl_scan(int v, int& total) {
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();          // s_w may still be read from an earlier call
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < 4; ++k) before += k < wv ? s_w[k] : 0;
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + inc - v;
}

// a workgroup owns chunk c of image n: pixels [c CC_CHUNK, (c + 1) CC_CHUNK) of the image, four consecutive ones per thread
__global__ void __launch_bounds__(256) k_cc_flatten(int* __restrict__ P, int* __restrict__ chunk_count, int* __restrict__ err, int HW,
                                                    int cpi, int bound) {
    const int n = blockIdx.x / cpi, c = blockIdx.x - n * cpi, base = n * HW;
    const int j0 = c * CC_CHUNK + 4 * threadIdx.x;
    int roots = 0;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j >= HW) break;
        const int i = base + j;
        int r = g_ld(P + i);
        if (r < 0) continue;
        if (r == i) { ++roots; continue; }
        int steps = 0;
        for (int v; (v = g_ld(P + r)) != r && steps <= bound; r = v) ++steps;          // roots do not change in this pass
        ok = ok && steps <= bound;
        // another walk may read this slot meanwhile: it sees the old parent or the root, both ancestors
        __hip_atomic_store(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int total;
    block_excl_scan(roots, total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
    if (!ok) atomicOr(err, CC_ERR_FLATTEN);
}

// one workgroup per image: the exclusive prefix of its chunk counts, in chunk order, and counts[n]
__global__ void __launch_bounds__(256) k_cc_scan(const int* __restrict__ chunk_count, int* __restrict__ chunk_off, int* __restrict__ counts,
                                                 int cpi) {
    const int n = blockIdx.x;
    int carry = 0;
    for (int c0 = 0; c0 < cpi; c0 += 256) {
        const int c = c0 + threadIdx.x, v = c < cpi ? chunk_count[n * cpi + c] : 0;
        int total;
        const int ex = block_excl_scan(v, total);
        if (c < cpi) chunk_off[n * cpi + c] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) counts[n] = carry;
}

// a root takes its number: the count of roots before it in raster order, plus 1, stored as -(number) - 1 <= -2
__global__ void __launch_bounds__(256) k_cc_number(int* __restrict__ P, const int* __restrict__ chunk_off, int HW, int cpi) {
    const int n = blockIdx.x / cpi, c = blockIdx.x - n * cpi, base = n * HW;
    const int j0 = c * CC_CHUNK + 4 * threadIdx.x;
    unsigned isroot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (j0 + q < HW && P[base + j0 + q] == base + j0 + q) isroot |= 1u << q;
    int total;
    int rank = chunk_off[blockIdx.x] + block_excl_scan(__popc(isroot), total);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if ((isroot >> q) & 1u) P[base + j0 + q] = -(++rank) - 1;
}

__global__ void __launch_bounds__(256) k_cc_write(const int* __restrict__ P, int* __restrict__ labels, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int v = P[i];
    if (v >= 0) v = P[v];          // flattened: one hop to the root, which holds its number
    labels[i] = v == CC_BG ? 0 : -v - 1;
}

static inline int cc_chunks(int H, int W) { return (int)(((long)H * W + CC_CHUNK - 1) / CC_CHUNK); }

extern "C" long vqw_label_components_ws_ints(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (long)N * H * W >= (1L << 31)) return 0;
    return (long)N * H * W + 2L * N * cc_chunks(H, W);
}

extern "C" int vqw_label_components(const uint8_t* mask, const float* scores, float threshold, int* labels, int* counts, int* err,
                                    int* ws, long ws_ints, int N, int H, int W, int connectivity, void* stream) {
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1, "vqw_label_components: N=%d, H=%d, W=%d: empty tensors are refused", N, H, W);
    VQW_CHECK(connectivity == 4 || connectivity == 8, "vqw_label_components: connectivity=%d must be 4 or 8", connectivity);
    VQW_CHECK((long)N * H * W < (1L << 31), "vqw_label_components: N H W = %ld must stay below 2^31 (32-bit pixel indices)", (long)N * H * W);
    VQW_CHECK((mask != nullptr) != (scores != nullptr),
              "vqw_label_components: exactly one of mask (bytes, foreground = non-zero) and scores (fp32, foreground = score >= threshold) is given");
    VQW_CHECK(labels && counts && err && ws, "vqw_label_components: null pointer (labels, counts, err and ws are needed)");
    VQW_CHECK(scores == nullptr || threshold == threshold, "vqw_label_components: the threshold is NaN");
    VQW_CHECK(((((uintptr_t)scores) | ((uintptr_t)labels) | ((uintptr_t)counts) | ((uintptr_t)err) | ((uintptr_t)ws)) & 3) == 0,
              "vqw_label_components: scores, labels, counts, err and ws must be 4-byte aligned");
    VQW_CHECK(ws_ints >= vqw_label_components_ws_ints(N, H, W), "vqw_label_components: a workspace of %ld ints, %ld are needed", ws_ints,
              vqw_label_components_ws_ints(N, H, W));
    hipStream_t st = (hipStream_t)stream;
    const int tilesX = ceil_div(W, CC_TX), tilesY = ceil_div(H, CC_TY), cpi = cc_chunks(H, W), total = N * H * W, conn8 = connectivity == 8;
    const long tiles = (long)N * tilesX * tilesY;
    VQW_CHECK(tiles < (1L << 31) && (long)N * cpi < (1L << 31), "vqw_label_components: too many tiles for one launch");
    int* P = ws;
    int* chunk_count = ws + total;
    int* chunk_off = chunk_count + (long)N * cpi;
    hipLaunchKernelGGL(k_cc_tile, dim3((unsigned)tiles), dim3(256), 0, st, mask, scores, threshold, P, err, H, W, tilesX, tilesY, conn8);
    if (tilesX > 1 || tilesY > 1)
        hipLaunchKernelGGL(k_cc_seam, dim3((unsigned)tiles), dim3(128), 0, st, P, err, H, W, tilesX, tilesY, conn8, total);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)(N * cpi)), dim3(256), 0, st, P, chunk_count, err, H * W, cpi, total);
    hipLaunchKernelGGL(k_cc_scan, dim3(N), dim3(256), 0, st, chunk_count, chunk_off, counts, cpi);
    hipLaunchKernelGGL(k_cc_number, dim3((unsigned)(N * cpi)), dim3(256), 0, st, P, chunk_off, H * W, cpi);
    hipLaunchKernelGGL(k_cc_write, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, P, labels, total);
    VQW_LAUNCH_CHECK("vqw_label_components");
    return VQW_OK;
}

// ------------------------------------------------------------------------------------------------ areas
// Labels are constant along runs: the lanes of a wave that share the label of its first active lane are merged into one add by a
// ballot, the others add one by one.  An all-foreground image is one add per wave-instruction, not 64 on one address.
__device__ __forceinline__ void cc_wave_add(int l, int* row) {          // every lane of the wave calls it; l < 1: nothing to add
    bool todo = l >= 1;
    const unsigned long long act = __ballot(todo);
    if (!act) return;
    const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
    const int l0 = __builtin_amdgcn_readlane(l, lead);
    const bool mine = todo && l == l0;
    const unsigned long long same = __ballot(mine);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(row + l0 - 1, __popcll(same));
    if (todo && !mine) atomicAdd(row + l - 1, 1);
}

__global__ void __launch_bounds__(256) k_cc_areas(const int* __restrict__ labels, int* __restrict__ areas, int* __restrict__ err, int HW,
                                                  int cap, int bpi, int rounds) {
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const int* lab = labels + (long)n * HW;
    int* row = areas + (long)n * cap;
    bool bad = false;
    for (int it = 0; it < rounds; ++it) {          // the same trip count in every lane: the ballots need the whole wave
        const long j = ((long)it * bpi + b) * 256 + threadIdx.x;
        int l = j < HW ? lab[j] : 0;
        if (l < 0 || l > cap) bad = true, l = 0;          // never written: the row has cap entries
        cc_wave_add(l, row);
    }
    if (bad) atomicOr(err, CC_ERR_CAP);
}

static inline void cc_stream_plan(int HW, int& bpi, int& rounds) {
    bpi = imin(imax(ceil_div(HW, 1024), 1), 256);
    rounds = ceil_div(HW, (long)bpi * 256);
}

extern "C" int vqw_component_areas(const int* labels, int* areas, int* err, int N, int H, int W, int cap, void* stream) {
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1, "vqw_component_areas: N=%d, H=%d, W=%d: empty tensors are refused", N, H, W);
    VQW_CHECK((long)N * H * W < (1L << 31), "vqw_component_areas: N H W = %ld must stay below 2^31 (32-bit pixel indices)", (long)N * H * W);
    VQW_CHECK(cap >= 1 && (long)N * cap < (1L << 31), "vqw_component_areas: cap=%d must be at least 1 with N cap below 2^31", cap);
    VQW_CHECK(labels && areas && err, "vqw_component_areas: null pointer");
    VQW_CHECK(((((uintptr_t)labels) | ((uintptr_t)areas) | ((uintptr_t)err)) & 3) == 0, "vqw_component_areas: labels, areas and err must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(areas, 0, (size_t)N * cap * sizeof(int), st) != hipSuccess) {
        vqw_set_error("vqw_component_areas: clearing the areas failed");
        return VQW_ERR_HIP;
    }
    int bpi, rounds;
    cc_stream_plan(H * W, bpi, rounds);
    hipLaunchKernelGGL(k_cc_areas, dim3((unsigned)(N * bpi)), dim3(256), 0, st, labels, areas, err, H * W, cap, bpi, rounds);
    VQW_LAUNCH_CHECK("vqw_component_areas");
    return VQW_OK;
}

// ------------------------------------------------------------------------------------------------ matching
__device__ __forceinline__ long wave_sum_l(long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// hits: same-value byte stores (every writer stores 1); the three pixel counts: one 64-bit add per wave that has any
__global__ void __launch_bounds__(256) k_cc_match(const int* __restrict__ pl, const int* __restrict__ pc, const int* __restrict__ pa,
                                                  const int* __restrict__ gl, const int* __restrict__ gc, uint8_t* __restrict__ phit,
                                                  uint8_t* __restrict__ ghit, unsigned long long* __restrict__ acc, int HW, int pcap,
                                                  int gcap, int min_size, int bpi, int rounds) {
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const int np = min(pc[n], pcap), ng = min(gc[n], gcap);
    long inter = 0, pp = 0, gp = 0;
    for (int it = 0; it < rounds; ++it) {
        const long j = ((long)it * bpi + b) * 256 + threadIdx.x;
        if (j >= HW) continue;
        const int p = pl[(long)n * HW + j], g = gl[(long)n * HW + j];
        const bool kept = p >= 1 && p <= np && pa[(long)n * pcap + p - 1] >= min_size;
        const bool truth = g >= 1 && g <= ng;
        pp += kept, gp += truth;
        if (kept && truth) {
            ++inter;
            phit[(long)n * pcap + p - 1] = 1;
            ghit[(long)n * gcap + g - 1] = 1;
        }
    }
    inter = wave_sum_l(inter), pp = wave_sum_l(pp), gp = wave_sum_l(gp);
    if ((threadIdx.x & 63) == 0) {
        if (inter) atomicAdd(acc + 5, (unsigned long long)inter);
        if (pp) atomicAdd(acc + 6, (unsigned long long)pp);
        if (gp) atomicAdd(acc + 7, (unsigned long long)gp);
    }
}

// one workgroup per image folds the flags, the kept test and the counts into acc
__global__ void __launch_bounds__(256) k_cc_fold(const int* __restrict__ pc, const int* __restrict__ pa, const int* __restrict__ gc,
                                                 const uint8_t* __restrict__ phit, const uint8_t* __restrict__ ghit,
                                                 unsigned long long* __restrict__ acc, int pcap, int gcap, int min_size) {
    __shared__ long s[3][4];
    const int n = blockIdx.x, np = min(pc[n], pcap), ng = min(gc[n], gcap);
    long det = 0, comps = 0, fls = 0;
    for (int l = threadIdx.x; l < np; l += 256) {
        const bool kept = pa[(long)n * pcap + l] >= min_size;
        comps += kept;
        fls += kept && !phit[(long)n * pcap + l];
    }
    for (int g = threadIdx.x; g < ng; g += 256) det += ghit[(long)n * gcap + g] != 0;
    det = wave_sum_l(det), comps = wave_sum_l(comps), fls = wave_sum_l(fls);
    if ((threadIdx.x & 63) == 0) s[0][threadIdx.x >> 6] = det, s[1][threadIdx.x >> 6] = comps, s[2][threadIdx.x >> 6] = fls;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(acc + 0, 1ull);
        atomicAdd(acc + 1, (unsigned long long)max(gc[n], 0));
        atomicAdd(acc + 2, (unsigned long long)(s[0][0] + s[0][1] + s[0][2] + s[0][3]));
        atomicAdd(acc + 3, (unsigned long long)(s[1][0] + s[1][1] + s[1][2] + s[1][3]));
        atomicAdd(acc + 4, (unsigned long long)(s[2][0] + s[2][1] + s[2][2] + s[2][3]));
    }
}

extern "C" long vqw_lesion_match_ws_bytes(int N, int pcap, int gcap) {
    if (N < 1 || pcap < 1 || gcap < 1) return 0;
    return (((long)N * ((long)pcap + gcap)) + 15) / 16 * 16;
}

extern "C" int vqw_lesion_match(const int* pred_labels, const int* pred_counts, const int* pred_areas, const int* gt_labels,
                                const int* gt_counts, long* acc, uint8_t* ws, long ws_bytes, int N, int H, int W, int pcap, int gcap,
                                int min_size, void* stream) {
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1, "vqw_lesion_match: N=%d, H=%d, W=%d: empty tensors are refused", N, H, W);
    VQW_CHECK((long)N * H * W < (1L << 31), "vqw_lesion_match: N H W = %ld must stay below 2^31 (32-bit pixel indices)", (long)N * H * W);
    VQW_CHECK(min_size >= 1, "vqw_lesion_match: min_size=%d must be at least 1", min_size);
    VQW_CHECK(pcap >= 1 && gcap >= 1 && (long)N * pcap < (1L << 31) && (long)N * gcap < (1L << 31),
              "vqw_lesion_match: pcap=%d and gcap=%d must be at least 1 with N cap below 2^31", pcap, gcap);
    VQW_CHECK(pred_labels && pred_counts && pred_areas && gt_labels && gt_counts && acc && ws, "vqw_lesion_match: null pointer");
    VQW_CHECK(((((uintptr_t)pred_labels) | ((uintptr_t)pred_counts) | ((uintptr_t)pred_areas) | ((uintptr_t)gt_labels) | ((uintptr_t)gt_counts)) & 3) == 0 &&
                  (((uintptr_t)acc) & 7) == 0,
              "vqw_lesion_match: the int32 tensors must be 4-byte and acc 8-byte aligned");
    VQW_CHECK(ws_bytes >= vqw_lesion_match_ws_bytes(N, pcap, gcap), "vqw_lesion_match: a workspace of %ld bytes, %ld are needed", ws_bytes,
              vqw_lesion_match_ws_bytes(N, pcap, gcap));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)vqw_lesion_match_ws_bytes(N, pcap, gcap), st) != hipSuccess) {
        vqw_set_error("vqw_lesion_match: clearing the hit flags failed");
        return VQW_ERR_HIP;
    }
    uint8_t* phit = ws;
    uint8_t* ghit = ws + (long)N * pcap;
    unsigned long long* a = (unsigned long long*)acc;
    int bpi, rounds;
    cc_stream_plan(H * W, bpi, rounds);
    hipLaunchKernelGGL(k_cc_match, dim3((unsigned)(N * bpi)), dim3(256), 0, st, pred_labels, pred_counts, pred_areas, gt_labels, gt_counts,
                       phit, ghit, a, H * W, pcap, gcap, min_size, bpi, rounds);
    hipLaunchKernelGGL(k_cc_fold, dim3(N), dim3(256), 0, st, pred_counts, pred_areas, gt_counts, phit, ghit, a, pcap, gcap, min_size);
    VQW_LAUNCH_CHECK("vqw_lesion_match");
    return VQW_OK;
}
