// Device code shared by the Winograd convolution kernels (conv_wino.hip, conv_wino64.hip, conv_wino_up.hip): the walk of a
// workgroup over its run of regions, the halo stager of the 10-float LDS pixel, the direct global -> LDS load and the
// transforms.  DESIGN section 6v is the description; the kernels keep what distinguishes them (tile geometry, slot positions,
// operand builds, epilogues).
#pragma once
#include "mfma_util.h"
#include <type_traits>

namespace wino {

using P0 = std::integral_constant<int, 0>;
using P1 = std::integral_constant<int, 1>;

// ---- the run of a workgroup -----------------------------------------------------------------------------------------
// Workgroup -> (cout tile, run of kt consecutive regions from sp0): the cout tiles of a run are neighbours on one XCD.
struct RegionRun {
    int tile_n, sp0, my_tiles;         // my_tiles <= 0: nothing to do (uniform per workgroup)
};
__device__ __forceinline__ RegionRun region_run(int ntn, int kt, int nsp) {
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    RegionRun r;
    r.tile_n = lb % ntn;
    r.sp0 = (lb / ntn) * kt;
    r.my_tiles = min(kt, nsp - r.sp0);
    return r;
}

// Item = (region, 8-channel chunk).  The cursor holds the (image, strip, region row, chunk) of the items i, i+1 and i+2: item
// i is multiplied while the patch of item i+1 is transformed and the halo of item i+2 is fetched.  Items past the
// workgroup's share name another region or none: their loads return data that is never consumed, or 0.  `advance` is
// region_step behind the chunk counter - selects only, like everything that runs inside an MFMA loop (see sel_u32).
template <class Args>                  // the kernel's argument struct: its tilesY, tilesX, nch are read where they are needed
struct ItemCursor {
    const Args& a;
    int cn, ctx, cty, ch;              // item i
    int n1, tx1, ty1, ch1;             // item i+1
    int n2, tx2, ty2, ch2;             // item i+2
    __device__ __forceinline__ void advance(int& n, int& tx, int& ty, int& c) const {     // the item after (n, tx, ty, c)
        const int adv = c + 1 == a.nch ? 1 : 0;
        c = adv ? 0 : c + 1;
        region_step(adv, a.tilesY, a.tilesX, n, tx, ty);
    }
    __device__ __forceinline__ ItemCursor(const Args& a_, int sp0) : a(a_) {
        region_start(sp0, a.tilesY, a.tilesX, cn, ctx, cty);
        ch = 0;
        n1 = cn; tx1 = ctx; ty1 = cty; ch1 = 0;
        advance(n1, tx1, ty1, ch1);
        n2 = n1; tx2 = tx1; ty2 = ty1; ch2 = ch1;
        advance(n2, tx2, ty2, ch2);
    }
    __device__ __forceinline__ void shift() {          // item i+1 becomes the current item
        cn = n1; ctx = tx1; cty = ty1; ch = ch1;
        n1 = n2; tx1 = tx2; ty1 = ty2; ch1 = ch2;
        advance(n2, tx2, ty2, ch2);
    }
};

// The regions of a run, each as nch / 2 (even, odd) item pairs (nch is even): body(parity, first) is one item, a barrier
// after each publishes the halo of item i+2 and the U chunk of item i+1; the first pair starts the accumulators from the
// MFMA's inline 0.  offsets(n, tx, ty) prepares the halo offsets of a region when item i+2 opens it; epilogue() ends the
// region at the cursor.  (Explicit region / pair loops rather than one item loop with an `if (first)` diamond: with 128
// accumulators live the diamond's PHIs cost register copies and spills.)  Every branch is uniform per workgroup.
template <class Cursor, class Body, class Offsets, class Epilogue>
__device__ __forceinline__ void region_loop(int my_tiles, int nch, Cursor& it, Body&& body, Offsets&& offsets, Epilogue&& epilogue) {
    for (int reg = 0; reg < my_tiles; ++reg) {
        body(P0{}, std::true_type{});
        __syncthreads();
        it.shift();
        body(P1{}, std::false_type{});
        __syncthreads();
        for (int c = 2; c < nch; c += 2) {
            it.shift();
            if (it.ch2 == 0) offsets(it.n2, it.tx2, it.ty2);
            body(P0{}, std::false_type{});
            __syncthreads();
            it.shift();
            body(P1{}, std::false_type{});
            __syncthreads();
        }
        epilogue();                    // region (cn, ctx, cty) is complete
        it.shift();
        if (it.ch2 == 0) offsets(it.n2, it.tx2, it.ty2);
    }
}

// ---- halo stager of the 10-float LDS pixel ----------------------------------------------------------------------------
// Pixel (n, y, x) -> pixel index of the tensor.  Dense: NHWC as it lies.  Pitched: the fields of W64Args (dense tensors or
// the four phase images of a dilation-2 layer), see there.
struct DensePix {
    unsigned H, W;
    __device__ __forceinline__ unsigned operator()(int n, int yy, int xx) const { return ((unsigned)n * H + (unsigned)yy) * W + (unsigned)xx; }
};
struct PitchedPix {
    unsigned img_px, rowb_px, rpx, ppx;
    int n_sh, n_m;
    __device__ __forceinline__ unsigned base(int n) const {      // (scalar: n is uniform)
        return (unsigned)(n >> n_sh) * img_px + (unsigned)((n >> 1) & n_m) * rowb_px + (unsigned)(n & n_m);
    }
    __device__ __forceinline__ unsigned operator()(int n, int yy, int xx) const { return base(n) + (unsigned)yy * rpx + (unsigned)xx * ppx; }
};

constexpr int KPH = 10;                // floats per halo pixel in LDS (8 channels + 2: conflict-free ds_read_b64 patches)

// The (HR x HWV)-pixel halo of a region's 8-channel chunk as float4 slots fixed per thread: float4 f = tid + NT j -> halo
// pixel f / 2 (LDS row stride HWS pixels), channel quad f % 2; the last slot of the threads past the end repeats another
// thread's slot (same address, same data: a benign duplicate instead of a masked store).  A slot's byte offset is computed
// once per REGION with the padding / edge select folded in (an invalid lane holds an out-of-range offset: the buffer load
// returns 0); the chunk is the load's scalar offset, which is not part of the range check.
template <int NT, int HR, int HWV, int HWS, class Pix>
struct HaloStager {
    static constexpr int HF = HR * HWV * 2;            // float4 per halo chunk
    static constexpr int LH = (HF + NT - 1) / NT;      // slots per thread
    static_assert(HF > (LH - 1) * NT && HF >= NT, "every halo slot but the last is full");
    Pix pix;
    int tid, c4;
    int h_lds[LH];
    unsigned h_voff[LH];               // byte offsets of the slots in the region whose halo is fetched next
    float4 rh[LH];
    __device__ __forceinline__ void halo_pixel(int j, int& hy, int& hx) const {     // (recomputed where needed: a division by a constant, no register held)
        int f = tid + j * NT;
        if (f >= HF) f -= HF;
        const int hp = f >> 1;
        hy = hp / HWV;
        hx = hp - hy * HWV;
    }
    __device__ __forceinline__ void init(int tid_, const Pix& pix_) {
        tid = tid_; c4 = tid_ & 1; pix = pix_;
#pragma unroll
        for (int j = 0; j < LH; ++j) {
            int hy, hx;
            halo_pixel(j, hy, hx);
            h_lds[j] = (hy * HWS + hx) * KPH + c4 * 4;
        }
    }
    // region whose first output pixel is (y0 + 1, x0 + 1) of image n, on an H x W map of C channels
    __device__ __forceinline__ void region_offsets(int n, int y0, int x0, int H, int W, int C) {
#pragma unroll
        for (int j = 0; j < LH; ++j) {
            int hy, hx;
            halo_pixel(j, hy, hx);
            const int yy = y0 + hy, xx = x0 + hx;
            const bool ok = ((unsigned)yy < (unsigned)H) & ((unsigned)xx < (unsigned)W);
            h_voff[j] = sel_u32(ok, pix(n, yy, xx) * (unsigned)C * 4u + (unsigned)c4 * 16u, 0xFFFFFFFFu);
        }
    }
    __device__ __forceinline__ void issue_h(__amdgpu_buffer_rsrc_t rs, int j, int chunk) { rh[j] = buf_ld4(rs, h_voff[j], chunk * 32); }
    __device__ __forceinline__ void commit_h(int j, float* Hb) {      // a halo pixel is 40 bytes: two 8-byte-aligned halves
        float* p = Hb + h_lds[j];
        f32x2 lo, hi;
        lo.x = rh[j].x; lo.y = rh[j].y; hi.x = rh[j].z; hi.y = rh[j].w;
        *(f32x2*)p = lo;
        *(f32x2*)(p + 2) = hi;
    }
};

// ---- direct global -> LDS load ------------------------------------------------------------------------------------------
// 16 bytes per lane straight into LDS (buffer_load_dwordx4 ... offen lds): no VGPR destination, no ds_write.  The wave's
// 64 x 16 bytes land in a row at lds_wave (wave-uniform; the hardware adds lane * 16): a layout that is not lane-linear is
// reached through the per-lane SOURCE offset.  byte_off is range-checked like buf_ld4's (an out-of-range lane writes 0), soff
// is not.  The load counts on vmcnt like any other; its data may be read only behind a wait that covers it (dma_wait) AND
// the barrier behind that wait.
__device__ __forceinline__ void buf_ld4_lds(__amdgpu_buffer_rsrc_t r, float* lds_wave, unsigned byte_off, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave, 16, (int)byte_off, (int)soff, 0, 0);
}
// s_waitcnt vmcnt(0) alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt 6:4 and lgkmcnt 11:8 stay at their maxima)
__device__ __forceinline__ void dma_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// ---- transforms -------------------------------------------------------------------------------------------------------
// Row r of B^T d = (d0 - d2, d1 + d2, d2 - d1, d1 - d3); r is a constant after unrolling, so a call is one instruction.
// bt_row: as fma with the hidden constants pone = opaque_f(1), mone = opaque_f(-1) (see opaque_f); bt_row_plain: - / +.
// The nine-product kernels use the rows (0, 1, 3).
__device__ __forceinline__ float bt_row(int r, float d0, float d1, float d2, float d3, float pone, float mone) {
    return r == 0 ? __builtin_fmaf(mone, d2, d0) : r == 1 ? __builtin_fmaf(pone, d2, d1) : r == 2 ? __builtin_fmaf(mone, d1, d2) : __builtin_fmaf(mone, d3, d1);
}
__device__ __forceinline__ float bt_row_plain(int r, float d0, float d1, float d2, float d3) {
    return r == 0 ? d0 - d2 : r == 1 ? d1 + d2 : r == 2 ? d2 - d1 : d1 - d3;
}

// u = G g G^T in double, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
__device__ __forceinline__ void weight_transform(const double g[3][3], double u[4][4]) {
    double t[4][3];
    for (int kx = 0; kx < 3; ++kx) {
        t[0][kx] = g[0][kx];
        t[1][kx] = 0.5 * (g[0][kx] + g[1][kx] + g[2][kx]);
        t[2][kx] = 0.5 * (g[0][kx] - g[1][kx] + g[2][kx]);
        t[3][kx] = g[2][kx];
    }
    for (int i = 0; i < 4; ++i) {
        u[i][0] = t[i][0];
        u[i][1] = 0.5 * (t[i][0] + t[i][1] + t[i][2]);
        u[i][2] = 0.5 * (t[i][0] - t[i][1] + t[i][2]);
        u[i][3] = t[i][2];
    }
}

}  // namespace wino
