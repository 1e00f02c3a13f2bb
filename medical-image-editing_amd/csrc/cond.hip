// Conditioning the code prior on label maps (networks/label_condition.py, trainers/cond_prior.py): a label map becomes one token per
// latent cell, two label maps become the mask of the cells that differ, and the tokens are looked up in a table of their own.
// Integers only in the two map kernels: counts do not depend on the order of accumulation, the same bits every run.  No float
// atomics, no inline assembly.
//
// Cell labels.  label [B][H][W] (1-, 4- or 8-byte integers), fy = H / h, fx = W / w.  A workgroup takes one row of cells of one
// image - or CW of its w cells, when the counters of a whole row would not fit or the grid would be too small - reads the fy image
// rows of its cells in 16-byte units and counts into LDS counters [CW][L] with integer LDS atomics (a lane adds a run of equal
// (cell, label) pixels of its unit at once).  A wave then takes a cell: the maximum over the packed key (count << 8 | 255 - label)
// is the largest count and, among equal counts, the smallest label.  A pixel outside [0, L) counts for nothing; a cell with no
// counted pixel gets -1.  purity = float(count) / float(fy fx).
//
// A unit is 16 bytes at a 16-byte aligned ADDRESS: a row of 40 bytes starts its units 8 bytes into the row above's.  A unit that
// straddles an end of the row segment is read element by element, and only the elements inside the segment.
//
// Cells changed.  The same walk over two maps: out[b][cy][cx] = 1 iff any pixel of the cell differs.
//
// Table lookup.  out[r] = table[idx[r]], a wave per row; an index outside [0, L) writes a NaN row (vqw_embed_fwd's rule).  Its
// gradient is vqw_embed_bwd's: nothing here.
//
// Table lookup with the condition dropped per sample (classifier-free guidance's training side).  Sample b = r / rows_per_sample is
// dropped iff the draw of dropout.h for element b of the site COND_DROP_SITE under (seed, call) falls below round(p 2^32) - the mask
// is never stored, the same bits every run - and every row of a dropped sample reads table[null_index].  eff[r] is the index read:
// the gradient is vqw_embed_bwd's gtok over eff.
//
// Conditioned embedding (vqw_embed_cond_fwd, the input stem of the label-conditioned MaskedGPT).  The label token of cell t is ADDED
// to the embedding of position t: x[b][t] = (tok[idx[b][t]] + pos[t]) + ctab[e], two fp32 additions in this order, e the effective
// label of the row - cond_effective() below, the one place where the drop is decided, shared with the lookup above.  One streaming
// pass, a wave per row, 16-byte accesses, every element of x written once; the looked-up condition is never stored.
#include "common.h"
#include "gpt_math.h"
#include "dropout.h"
#include "../../include/vqwnet_hip.h"

#define CL_MAX_LABELS 256
#define CL_LDS_INTS 8192          // 32 KB of counters per workgroup
#define CL_MIN_BLOCKS 512         // below this many (image, cell row) pairs the columns are split over the grid as well

// Element j of a 16-byte unit / of memory, as a long: 1-byte labels are unsigned (torch.uint8), the others signed.
template <int ES> __device__ __forceinline__ long unit_elem(const uint4& u, int j);
template <> __device__ __forceinline__ long unit_elem<1>(const uint4& u, int j) {
    const unsigned word = (j >> 2) == 0 ? u.x : (j >> 2) == 1 ? u.y : (j >> 2) == 2 ? u.z : u.w;
    return (long)((word >> (8 * (j & 3))) & 255u);
}
template <> __device__ __forceinline__ long unit_elem<4>(const uint4& u, int j) {
    return (long)(int)(j == 0 ? u.x : j == 1 ? u.y : j == 2 ? u.z : u.w);
}
template <> __device__ __forceinline__ long unit_elem<8>(const uint4& u, int j) {
    return j == 0 ? (long)((unsigned long long)u.x | ((unsigned long long)u.y << 32)) : (long)((unsigned long long)u.z | ((unsigned long long)u.w << 32));
}
template <int ES> __device__ __forceinline__ long mem_elem(const void* p, long e);
template <> __device__ __forceinline__ long mem_elem<1>(const void* p, long e) { return (long)((const uint8_t*)p)[e]; }
template <> __device__ __forceinline__ long mem_elem<4>(const void* p, long e) { return (long)((const int*)p)[e]; }
template <> __device__ __forceinline__ long mem_elem<8>(const void* p, long e) { return ((const long*)p)[e]; }

// The 16-byte units of the row segments [x0, x1) of the image rows y0 .. y0 + fy - 1 of image b, dealt to the threads of the
// workgroup: f(e0, x, jlo, jhi) with e0 the element index of the unit's first element, x the column of that element (it may lie
// left of x0) and [jlo, jhi) the elements of the unit inside the segment; the unit is whole iff jlo == 0 and jhi == 16 / ES.
template <int ES, class F>
__device__ __forceinline__ void walk_units(const void* base, long b, int H, int W, int y0, int fy, int x0, int x1, F f) {
    constexpr int EPU = 16 / ES;
    const long base_e = (long)((uintptr_t)base / ES);          // the base address in elements (base is a multiple of ES)
    const int units = (x1 - x0 + EPU - 1) / EPU + 1;           // an upper bound per row: the segment may start inside a unit
    const int total = fy * units;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int ry = i / units, k = i - ry * units;
        const long r = (b * H + y0 + ry) * (long)W;            // element index of (b, y, 0)
        const int m = (int)((base_e + r + x0) % EPU);          // elements between the unit's start and the segment's
        const int x = x0 - m + k * EPU;
        const int jlo = x < x0 ? x0 - x : 0, jhi = x1 - x < EPU ? x1 - x : EPU;
        if (jhi > jlo) f(r + x, x, jlo, jhi);
    }
}

// grid (ceil(w / CW), h, B); dynamic LDS: CW * L ints
template <int ES>
__global__ void __launch_bounds__(256) k_cell_labels(const void* __restrict__ label, long* __restrict__ tokens, float* __restrict__ purity,
                                                     int H, int W, int h, int w, int L, int CW) {
    extern __shared__ __attribute__((aligned(16))) int cl_count[];
    constexpr int EPU = 16 / ES;
    const int fy = H / h, fx = W / w;
    const int c0 = blockIdx.x * CW, c1 = min(w, c0 + CW), cy = blockIdx.y;
    const long b = blockIdx.z;
    const int ncell = c1 - c0;
    for (int i = threadIdx.x; i < ncell * L; i += blockDim.x) cl_count[i] = 0;
    __syncthreads();
    walk_units<ES>(label, b, H, W, cy * fy, fy, c0 * fx, c1 * fx, [&](long e0, int x, int jlo, int jhi) {
        int slot = -1, run = 0;                                  // a run of pixels that share a counter
        auto count = [&](long v, int xx) {
            const int s = (v >= 0 && v < L) ? (xx / fx - c0) * L + (int)v : -1;
            if (s != slot) {
                if (slot >= 0) atomicAdd(&cl_count[slot], run);
                slot = s;
                run = 0;
            }
            ++run;
        };
        if (jlo == 0 && jhi == EPU) {
            const uint4 u = *(const uint4*)((const char*)label + e0 * ES);
#pragma unroll
            for (int j = 0; j < EPU; ++j) count(unit_elem<ES>(u, j), x + j);
        } else {
            for (int j = jlo; j < jhi; ++j) count(mem_elem<ES>(label, e0 + j), x + j);
        }
        if (slot >= 0) atomicAdd(&cl_count[slot], run);
    });
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    for (int c = wave; c < ncell; c += nwave) {
        unsigned long long key = 0;                              // (count, 255 - label): the smallest label wins a tie
        for (int l = lane; l < L; l += 64) {
            const unsigned long long k = ((unsigned long long)(unsigned)cl_count[c * L + l] << 8) | (unsigned)(255 - l);
            key = k > key ? k : key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long k = __shfl_xor(key, o, 64);
            key = k > key ? k : key;
        }
        if (lane == 0) {
            const int count = (int)(key >> 8);
            const long o = (b * h + cy) * (long)w + c0 + c;
            tokens[o] = count > 0 ? (long)(255 - (int)(key & 255)) : -1L;
            if (purity) purity[o] = (float)count / (float)(fy * fx);
        }
    }
}

// grid (ceil(w / CW), h, B); static LDS: a flag per cell of the chunk
#define CC_MAX_CW 4096
template <int ES, bool VEC>
__global__ void __launch_bounds__(256) k_cells_changed(const void* __restrict__ a, const void* __restrict__ bmap, uint8_t* __restrict__ out, int H,
                                                       int W, int h, int w, int CW) {
    __shared__ int cc_flag[CC_MAX_CW];
    constexpr int EPU = 16 / ES;
    const int fy = H / h, fx = W / w;
    const int c0 = blockIdx.x * CW, c1 = min(w, c0 + CW), cy = blockIdx.y;
    const long b = blockIdx.z;
    for (int i = threadIdx.x; i < c1 - c0; i += blockDim.x) cc_flag[i] = 0;
    __syncthreads();
    walk_units<ES>(a, b, H, W, cy * fy, fy, c0 * fx, c1 * fx, [&](long e0, int x, int jlo, int jhi) {
        const bool whole = VEC && jlo == 0 && jhi == EPU;
        uint4 ua = make_uint4(0u, 0u, 0u, 0u), ub = ua;
        if (whole) {
            ua = *(const uint4*)((const char*)a + e0 * ES);
            ub = *(const uint4*)((const char*)bmap + e0 * ES);
            if (ua.x == ub.x && ua.y == ub.y && ua.z == ub.z && ua.w == ub.w) return;
        }
        for (int j = jlo; j < jhi; ++j) {
            const bool differ = whole ? unit_elem<ES>(ua, j) != unit_elem<ES>(ub, j) : mem_elem<ES>(a, e0 + j) != mem_elem<ES>(bmap, e0 + j);
            if (differ) atomicOr(&cc_flag[(x + j) / fx - c0], 1);
        }
    });
    __syncthreads();
    for (int i = threadIdx.x; i < c1 - c0; i += blockDim.x) out[(b * h + cy) * (long)w + c0 + i] = (uint8_t)(cc_flag[i] != 0);
}

// grid ceil(rows / 4): wave w of workgroup g writes row 4 g + w
__global__ void __launch_bounds__(256) k_embed_lookup(const long* __restrict__ idx, const float* __restrict__ table, float* __restrict__ out,
                                                      long rows, int E, int L) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, E4 = E >> 2;
    const long id = idx[r];
    const bool ok = id >= 0 && id < L;
    const float* src = table + (ok ? id : 0) * E;
    const float nan = quiet_nan();
    for (int c4 = lane; c4 < E4; c4 += 64)
        *(float4*)(out + r * E + 4 * c4) = ok ? *(const float4*)(src + 4 * c4) : make_float4(nan, nan, nan, nan);
}

// The dropout site of the condition drop: GPT.seed_dropout numbers its sites upwards from 0, so a negative site is never one of them.
#define COND_DROP_SITE (-1)

// The index row r of a conditioned lookup reads: its own, or null_index when its sample r / rows_per_sample is dropped - the same
// for every row of a sample.
__device__ __forceinline__ long cond_effective(const long* __restrict__ idx, long r, int rows_per_sample, long null_index, const DropKey& key) {
    return dk_keep(key, (uint64_t)(r / rows_per_sample)) ? idx[r] : null_index;
}

// grid ceil(rows / 4): wave w of workgroup g writes row 4 g + w
__global__ void __launch_bounds__(256) k_embed_lookup_drop(const long* __restrict__ idx, const float* __restrict__ table, float* __restrict__ out,
                                                           long* __restrict__ eff, long rows, int rows_per_sample, int E, int L, long null_index,
                                                           DropKey key) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, E4 = E >> 2;
    const long id = cond_effective(idx, r, rows_per_sample, null_index, key);
    const bool ok = id >= 0 && id < L;
    const float* src = table + (ok ? id : 0) * E;
    const float nan = quiet_nan();
    if (lane == 0) eff[r] = id;
    for (int c4 = lane; c4 < E4; c4 += 64)
        *(float4*)(out + r * E + 4 * c4) = ok ? *(const float4*)(src + 4 * c4) : make_float4(nan, nan, nan, nan);
}

// grid ceil(B T / 4): wave w of workgroup g writes row 4 g + w.  A key with thr = 0 keeps every sample (p = 0).
__global__ void __launch_bounds__(256) k_embed_cond_fwd(const long* __restrict__ idx, const float* __restrict__ tok, const float* __restrict__ pos,
                                                        const long* __restrict__ cidx, const float* __restrict__ ctab, float* __restrict__ x,
                                                        long* __restrict__ eff, long rows, int T, int E, int V, int L, long null_index, DropKey key) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, E4 = E >> 2;
    const int t = (int)(r % T);
    const long id = idx[r], e = cond_effective(cidx, r, T, null_index, key);
    const bool ok = id >= 0 && id < V && e >= 0 && e < L;
    const float* ta = tok + (ok ? id : 0) * E;
    const float* pp = pos + (long)t * E;
    const float* cc = ctab + (ok ? e : 0) * E;
    float* xr = x + r * E;
    const float nan = quiet_nan();
    if (eff && lane == 0) eff[r] = e;
    for (int c4 = lane; c4 < E4; c4 += 64) {
        const float4 a = *(const float4*)(ta + 4 * c4), p = *(const float4*)(pp + 4 * c4), c = *(const float4*)(cc + 4 * c4);
        *(float4*)(xr + 4 * c4) = ok ? make_float4((a.x + p.x) + c.x, (a.y + p.y) + c.y, (a.z + p.z) + c.z, (a.w + p.w) + c.w)
                                     : make_float4(nan, nan, nan, nan);
    }
}

static int cell_check(const char* name, int B, int H, int W, int h, int w, int elem_bytes) {
    VQW_CHECK(B >= 1 && H >= 1 && W >= 1, "%s: B=%d, H=%d, W=%d must be positive", name, B, H, W);
    VQW_CHECK(h >= 1 && w >= 1 && H % h == 0 && W % w == 0, "%s: H=%d, W=%d must be multiples of the cell grid h=%d, w=%d", name, H, W, h, w);
    VQW_CHECK(elem_bytes == 1 || elem_bytes == 4 || elem_bytes == 8, "%s: elem_bytes=%d must be 1, 4 or 8 (uint8, int32, int64)", name, elem_bytes);
    VQW_CHECK(B <= 65535 && h <= 65535, "%s: B=%d and h=%d must not exceed 65535 (the grid's limits)", name, B, h);
    VQW_CHECK((long)(H / h) * ((long)W + 32) < (1L << 31), "%s: a row of cells of %d x %d pixels is too large for the 32-bit unit walk", name, H / h, W);
    VQW_CHECK((long)(H / h) * (W / w) <= (1L << 24), "%s: a cell of %d x %d pixels exceeds 2^24 (an exact fp32 count)", name, H / h, W / w);
    return VQW_OK;
}

// cells of a row per workgroup: at most `cap`, and few enough that the grid has CL_MIN_BLOCKS workgroups where w allows it
static int cells_per_block(int B, int h, int w, int cap) {
    const long pairs = (long)B * h;
    const int split = pairs >= CL_MIN_BLOCKS ? 1 : imin(w, ceil_div(CL_MIN_BLOCKS, pairs));
    return imax(1, imin(cap, ceil_div(w, split)));
}

extern "C" int vqw_cell_labels(const void* label, long* tokens, float* purity, int B, int H, int W, int h, int w, int n_labels, int elem_bytes,
                               void* stream) {
    if (int rc = cell_check("vqw_cell_labels", B, H, W, h, w, elem_bytes)) return rc;
    VQW_CHECK(n_labels >= 1 && n_labels <= CL_MAX_LABELS, "vqw_cell_labels: n_labels=%d must lie in [1, %d]", n_labels, CL_MAX_LABELS);
    VQW_CHECK(label && tokens, "vqw_cell_labels: null pointer");
    VQW_CHECK((uintptr_t)label % elem_bytes == 0, "vqw_cell_labels: label must be aligned to its element size %d", elem_bytes);
    const int CW = cells_per_block(B, h, w, CL_LDS_INTS / n_labels);
    const dim3 grid(ceil_div(w, CW), h, B);
    const size_t lds = (size_t)CW * n_labels * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 1) hipLaunchKernelGGL(k_cell_labels<1>, grid, dim3(256), lds, st, label, tokens, purity, H, W, h, w, n_labels, CW);
    else if (elem_bytes == 4) hipLaunchKernelGGL(k_cell_labels<4>, grid, dim3(256), lds, st, label, tokens, purity, H, W, h, w, n_labels, CW);
    else hipLaunchKernelGGL(k_cell_labels<8>, grid, dim3(256), lds, st, label, tokens, purity, H, W, h, w, n_labels, CW);
    VQW_LAUNCH_CHECK("vqw_cell_labels");
    return VQW_OK;
}

template <int ES>
static void launch_cells_changed(const void* a, const void* b, uint8_t* out, int B, int H, int W, int h, int w, hipStream_t st) {
    const int CW = cells_per_block(B, h, w, CC_MAX_CW);
    const dim3 grid(ceil_div(w, CW), h, B);
    if ((((uintptr_t)a ^ (uintptr_t)b) & 15) == 0) hipLaunchKernelGGL((k_cells_changed<ES, true>), grid, dim3(256), 0, st, a, b, out, H, W, h, w, CW);
    else hipLaunchKernelGGL((k_cells_changed<ES, false>), grid, dim3(256), 0, st, a, b, out, H, W, h, w, CW);
}

extern "C" int vqw_cells_changed(const void* a, const void* b, uint8_t* out, int B, int H, int W, int h, int w, int elem_bytes, void* stream) {
    if (int rc = cell_check("vqw_cells_changed", B, H, W, h, w, elem_bytes)) return rc;
    VQW_CHECK(a && b && out, "vqw_cells_changed: null pointer");
    VQW_CHECK((uintptr_t)a % elem_bytes == 0 && (uintptr_t)b % elem_bytes == 0, "vqw_cells_changed: the maps must be aligned to their element size %d",
              elem_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 1) launch_cells_changed<1>(a, b, out, B, H, W, h, w, st);
    else if (elem_bytes == 4) launch_cells_changed<4>(a, b, out, B, H, W, h, w, st);
    else launch_cells_changed<8>(a, b, out, B, H, W, h, w, st);
    VQW_LAUNCH_CHECK("vqw_cells_changed");
    return VQW_OK;
}

extern "C" int vqw_embed_lookup(const long* idx, const float* table, float* out, long rows, int E, int L, void* stream) {
    VQW_CHECK(rows >= 1 && rows <= (1L << 31) - 4, "vqw_embed_lookup: rows=%ld must lie in [1, 2^31 - 4]", rows);
    VQW_CHECK(E % 4 == 0 && E >= 4 && E <= 4096, "vqw_embed_lookup: E=%d must be a multiple of 4 with 4 <= E <= 4096", E);
    VQW_CHECK(L >= 1, "vqw_embed_lookup: L=%d must be at least 1", L);
    VQW_CHECK(idx && table && out, "vqw_embed_lookup: null pointer");
    VQW_CHECK(al16(table) && al16(out), "vqw_embed_lookup: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_embed_lookup, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, idx, table, out, rows, E, L);
    VQW_LAUNCH_CHECK("vqw_embed_lookup");
    return VQW_OK;
}

extern "C" int vqw_embed_lookup_drop(const long* idx, const float* table, float* out, long* eff, long rows, int rows_per_sample, int E, int L,
                                     long null_index, float p, long seed, long call, void* stream) {
    VQW_CHECK(rows >= 1 && rows <= (1L << 31) - 4, "vqw_embed_lookup_drop: rows=%ld must lie in [1, 2^31 - 4]", rows);
    VQW_CHECK(rows_per_sample >= 1 && rows % rows_per_sample == 0, "vqw_embed_lookup_drop: rows=%ld must be a multiple of rows_per_sample=%d >= 1", rows,
              rows_per_sample);
    VQW_CHECK(E % 4 == 0 && E >= 4 && E <= 4096, "vqw_embed_lookup_drop: E=%d must be a multiple of 4 with 4 <= E <= 4096", E);
    VQW_CHECK(L >= 1, "vqw_embed_lookup_drop: L=%d must be at least 1", L);
    VQW_CHECK(null_index >= 0 && null_index < L, "vqw_embed_lookup_drop: null_index=%ld must be a row of the table, [0, L = %d)", null_index, L);
    VQW_CHECK(p >= 0.f && p < 1.f, "vqw_embed_lookup_drop: p=%g must lie in [0, 1)", (double)p);
    VQW_CHECK(idx && table && out && eff, "vqw_embed_lookup_drop: null pointer");
    VQW_CHECK(al16(table) && al16(out), "vqw_embed_lookup_drop: tensors must be 16-byte aligned");
    hipLaunchKernelGGL(k_embed_lookup_drop, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, idx, table, out, eff, rows, rows_per_sample, E, L,
                       null_index, dk_make(p, seed, call, COND_DROP_SITE));
    VQW_LAUNCH_CHECK("vqw_embed_lookup_drop");
    return VQW_OK;
}

extern "C" int vqw_embed_cond_fwd(const long* idx, const float* tok, const float* pos, const long* cidx, const float* ctab, float* x, long* eff,
                                  int B, int T, int E, int V, int L, int block_size, long null_index, float p, long seed, long call,
                                  void* stream) {
    VQW_CHECK(E % 4 == 0 && E >= 4 && E <= 4096, "vqw_embed_cond_fwd: E=%d must be a multiple of 4 with 4 <= E <= 4096", E);
    VQW_CHECK(V >= 1, "vqw_embed_cond_fwd: V=%d must be at least 1", V);
    VQW_CHECK(L >= 1, "vqw_embed_cond_fwd: L=%d must be at least 1", L);
    VQW_CHECK(B >= 1 && T >= 1, "vqw_embed_cond_fwd: B=%d, T=%d must be at least 1", B, T);
    VQW_CHECK(block_size >= 1 && T <= block_size, "vqw_embed_cond_fwd: T = %d exceeds block_size=%d", T, block_size);
    VQW_CHECK((long)B * T <= (1L << 31) - 4, "vqw_embed_cond_fwd: B * T = %ld rows are too many", (long)B * T);
    VQW_CHECK(p >= 0.f && p < 1.f, "vqw_embed_cond_fwd: p=%g must lie in [0, 1)", (double)p);
    VQW_CHECK(p == 0.f || (null_index >= 0 && null_index < L), "vqw_embed_cond_fwd: null_index=%ld must be a row of the table, [0, L = %d), when p > 0",
              null_index, L);
    VQW_CHECK(idx && tok && pos && cidx && ctab && x, "vqw_embed_cond_fwd: null pointer");
    VQW_CHECK(al16(tok) && al16(pos) && al16(ctab) && al16(x), "vqw_embed_cond_fwd: tensors must be 16-byte aligned");
    const long rows = (long)B * T;
    // p = 0 reads neither seed nor call: the key of (0, 0) with threshold 0 keeps every sample
    const DropKey key = p > 0.f ? dk_make(p, seed, call, COND_DROP_SITE) : dk_make(0.f, 0, 0, COND_DROP_SITE);
    hipLaunchKernelGGL(k_embed_cond_fwd, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, idx, tok, pos, cidx, ctab, x, eff, rows, T, E, V,
                       L, null_index, key);
    VQW_LAUNCH_CHECK("vqw_embed_cond_fwd");
    return VQW_OK;
}
