// The seamless composite of an edit (trainers/prior.py PriorTrainer.edit with blend="pyramid"): Burt-Adelson multi-band blending of
// the difference picture d = edit - image (or edit - recon) onto the scan under the Gaussian pyramid of the cell mask.  NHWC fp32
// pictures, forward only, no atomics, bounded loops, the same bits every run.
//
//   REDUCE(x)[i][j] = sum_m sum_n w[m] w[n] x[clamp(2i+m)][clamp(2j+n)], m, n = -2..2, w = [1, 4, 6, 4, 1] / 16
//   EXPAND(x), along each axis in turn: [2k] = (x[k-1] + 6 x[k] + x[k+1]) / 8, [2k+1] = (x[k] + x[k+1]) / 2, indices clamped
//   M_0 = the cell mask at pixels (0 / 1), M_{l+1} = REDUCE(M_l); G_0 = d, G_{l+1} = REDUCE(G_l)
//   R_L = M_L G_L; R_l = M_l (G_l - EXPAND(G_{l+1})) + EXPAND(R_{l+1}); out = image + R_0
//
// Every filter runs the row pass (along x) first, then the column pass (along y), taps in ascending order, one fp32 rounding per
// operation (the Makefile builds this file with -ffp-contract=off), so tests/blend_ref.py restates it operation by operation.
//
// Plan: L reduce launches (level l -> l + 1, the C planes of G and the plane of M through one LDS tile) and L collapse launches
// (level l from level l + 1).  Level 0 is never stored: the first reduce forms d and M_0 while it loads, the last collapse reads the
// pictures again and writes out.  The workspace holds, plane by plane, G_l and M_l for l = 1..L and R_l for l = 1..L-1.
#include "common.h"
#include "../../include/vqwnet_hip.h"

#define BL_MAX_LEVELS 12
// reduce: a workgroup owns BL_RTY x BL_RTX outputs of one plane and stages the (2 BL_RTY + 3) x (2 BL_RTX + 3) inputs under them -
// the 2-pixel halo on each side - with the even and the odd columns of a row in two runs, so that the stride-2 taps of the row pass
// are unit-stride LDS reads; the odd run starts 48 floats in (16 banks off the even run: the staging writes of a wave do not collide)
#define BL_RTY 16
#define BL_RTX 32
#define BL_RIH (2 * BL_RTY + 3)
#define BL_RIW (2 * BL_RTX + 3)
#define BL_ODD 48
#define BL_RROW 82
// collapse: a workgroup owns BL_CTY x BL_CTX outputs of one plane and stages the (BL_CTY / 2 + 2) x (BL_CTX / 2 + 2) samples of the
// level below that EXPAND reads
#define BL_CTY 16
#define BL_CTX 64
#define BL_CKH (BL_CTY / 2 + 2)
#define BL_CKW (BL_CTX / 2 + 2)

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// FIRST: level 0 -> 1, the input formed from the pictures (plane p < C: edit - base at channel p; plane C: the mask);
// else src -> dst, both [N][C + 1] planes of the workspace.  grid (tiles, C + 1, N).
template <bool FIRST>
__global__ void __launch_bounds__(256) k_blend_reduce(const float* __restrict__ edit, const float* __restrict__ base,
                                                      const uint8_t* __restrict__ cellmask, const float* __restrict__ src,
                                                      float* __restrict__ dst, int Hi, int Wi, int C, int h, int w, int fy, int fx,
                                                      int tiles_x) {
    __shared__ float s[BL_RIH * BL_RROW];
    __shared__ float t[BL_RIH * BL_RTX];
    const int tid = threadIdx.x, p = blockIdx.y, n = blockIdx.z;
    const int Ho = Hi / 2, Wo = Wi / 2;
    const int oy0 = (blockIdx.x / tiles_x) * BL_RTY, ox0 = (blockIdx.x % tiles_x) * BL_RTX;
    const int iy0 = 2 * oy0 - 2, ix0 = 2 * ox0 - 2;
    const float* plane = FIRST ? nullptr : src + ((long)n * (C + 1) + p) * Hi * Wi;
    for (int e = tid; e < BL_RIH * BL_RIW; e += 256) {
        const int i = e / BL_RIW, c = e - i * BL_RIW;
        const int y = clampi(iy0 + i, Hi - 1), x = clampi(ix0 + c, Wi - 1);
        float v;
        if (FIRST) {
            if (p < C) {
                const long at = (((long)n * Hi + y) * Wi + x) * C + p;
                v = edit[at] - base[at];
            } else {
                v = cellmask[((long)n * h + y / fy) * w + x / fx] ? 1.0f : 0.0f;
            }
        } else {
            v = plane[y * Wi + x];
        }
        s[i * BL_RROW + ((c & 1) ? BL_ODD : 0) + (c >> 1)] = v;
    }
    __syncthreads();
    const float w0 = 0.0625f, w1 = 0.25f, w2 = 0.375f;
    for (int e = tid; e < BL_RIH * BL_RTX; e += 256) {      // row pass: output column j reads the staged columns 2j .. 2j + 4
        const int i = e / BL_RTX, j = e - i * BL_RTX;
        const float* r = s + i * BL_RROW + j;
        float acc = w0 * r[0];
        acc += w1 * r[BL_ODD];
        acc += w2 * r[1];
        acc += w1 * r[BL_ODD + 1];
        acc += w0 * r[2];
        t[e] = acc;
    }
    __syncthreads();
    float* out = dst + ((long)n * (C + 1) + p) * Ho * Wo;
    for (int e = tid; e < BL_RTY * BL_RTX; e += 256) {      // column pass: output row i reads the rows 2i .. 2i + 4
        const int i = e / BL_RTX, j = e - i * BL_RTX;
        if (oy0 + i >= Ho || ox0 + j >= Wo) continue;
        const float* q = t + 2 * i * BL_RTX + j;
        float acc = w0 * q[0];
        acc += w1 * q[BL_RTX];
        acc += w2 * q[2 * BL_RTX];
        acc += w1 * q[3 * BL_RTX];
        acc += w0 * q[4 * BL_RTX];
        out[(oy0 + i) * Wo + ox0 + j] = acc;
    }
}

// EXPAND along one axis from three neighbours a = x[k-1], b = x[k], c = x[k+1] for the even sample 2k, b, c for the odd one
__device__ __forceinline__ float expand_tap(bool odd, float a, float b, float c) {
    return odd ? (b + c) * 0.5f : ((a + 6.0f * b) + c) * 0.125f;
}

// The collapse of level l (Hl x Wl) from level l + 1: R_l = M_l (G_l - EXPAND(G_{l+1})) + EXPAND(R_{l+1}).  gm_lo: the [N][C + 1]
// planes of G_{l+1} and M_{l+1}; r_lo: the [N][C] planes of R_{l+1}, or null at the top, where R_L = M_L G_L is formed while
// staging.  LAST (l = 0): G_0 and M_0 come from the pictures and out = image + R_0 is written; else gm_hi holds G_l and M_l and
// r_hi receives R_l.  grid (tiles, C, N).
template <bool LAST>
__global__ void __launch_bounds__(256) k_blend_collapse(const float* __restrict__ gm_lo, const float* __restrict__ r_lo,
                                                        const float* __restrict__ gm_hi, float* __restrict__ r_hi,
                                                        const float* __restrict__ image, const float* __restrict__ edit,
                                                        const float* __restrict__ base, const uint8_t* __restrict__ cellmask,
                                                        float* __restrict__ out, int Hl, int Wl, int C, int h, int w, int fy, int fx,
                                                        int tiles_x) {
    __shared__ float cg[BL_CKH * BL_CKW], cr[BL_CKH * BL_CKW];
    __shared__ float hg[BL_CKH * BL_CTX], hr[BL_CKH * BL_CTX];
    const int tid = threadIdx.x, c = blockIdx.y, n = blockIdx.z;
    const int Hc = Hl / 2, Wc = Wl / 2;
    const int y0 = (blockIdx.x / tiles_x) * BL_CTY, x0 = (blockIdx.x % tiles_x) * BL_CTX;
    const int ky0 = y0 / 2 - 1, kx0 = x0 / 2 - 1;
    const float* g_lo = gm_lo + ((long)n * (C + 1) + c) * Hc * Wc;
    const float* m_lo = gm_lo + ((long)n * (C + 1) + C) * Hc * Wc;
    const float* rr_lo = r_lo ? r_lo + ((long)n * C + c) * Hc * Wc : nullptr;
    for (int e = tid; e < BL_CKH * BL_CKW; e += 256) {
        const int a = e / BL_CKW, b = e - a * BL_CKW;
        const int at = clampi(ky0 + a, Hc - 1) * Wc + clampi(kx0 + b, Wc - 1);
        const float g = g_lo[at];
        cg[e] = g;
        cr[e] = rr_lo ? rr_lo[at] : m_lo[at] * g;
    }
    __syncthreads();
    for (int e = tid; e < BL_CKH * BL_CTX; e += 256) {      // row pass: column x0 + j reads the staged columns j / 2 .. j / 2 + 2
        const int a = e / BL_CTX, j = e - a * BL_CTX;
        const int at = a * BL_CKW + (j >> 1);
        const bool odd = j & 1;
        hg[e] = expand_tap(odd, cg[at], cg[at + 1], cg[at + 2]);
        hr[e] = expand_tap(odd, cr[at], cr[at + 1], cr[at + 2]);
    }
    __syncthreads();
    for (int e = tid; e < BL_CTY * BL_CTX; e += 256) {      // column pass, then the band's own term
        const int i = e / BL_CTX, j = e - i * BL_CTX;
        const int y = y0 + i, x = x0 + j;
        if (y >= Hl || x >= Wl) continue;
        const int at = (i >> 1) * BL_CTX + j;
        const bool odd = i & 1;
        const float eg = expand_tap(odd, hg[at], hg[at + BL_CTX], hg[at + 2 * BL_CTX]);
        const float er = expand_tap(odd, hr[at], hr[at + BL_CTX], hr[at + 2 * BL_CTX]);
        if (LAST) {
            const long px = (((long)n * Hl + y) * Wl + x) * C + c;
            const float m = cellmask[((long)n * h + y / fy) * w + x / fx] ? 1.0f : 0.0f;
            const float g = edit[px] - base[px];
            out[px] = image[px] + (m * (g - eg) + er);
        } else {
            const float g = gm_hi[((long)n * (C + 1) + c) * Hl * Wl + y * Wl + x];
            const float m = gm_hi[((long)n * (C + 1) + C) * Hl * Wl + y * Wl + x];
            r_hi[((long)n * C + c) * Hl * Wl + y * Wl + x] = m * (g - eg) + er;
        }
    }
}

// floats of the planes of G and M (gm) and of R (r) at level l >= 1
static inline long blend_gm_floats(int N, int H, int W, int C, int l) { return (long)N * (C + 1) * (H >> l) * (W >> l); }
static inline long blend_r_floats(int N, int H, int W, int C, int l) { return (long)N * C * (H >> l) * (W >> l); }

extern "C" long vqw_blend_cells_workspace(int N, int H, int W, int C, int levels) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || levels < 1 || levels > BL_MAX_LEVELS) return 0;
    if ((long)N * H >= (1L << 31) || (long)N * H * W >= (1L << 31) || (long)N * H * W * (C + 1) >= (1L << 31)) return 0;
    long total = 0;
    for (int l = 1; l <= levels; ++l) total += blend_gm_floats(N, H, W, C, l);
    for (int l = 1; l < levels; ++l) total += blend_r_floats(N, H, W, C, l);
    return total;
}

extern "C" int vqw_blend_cells(const float* image, const float* edit, const float* recon, const uint8_t* cellmask, float* out,
                               float* workspace, long workspace_floats, int N, int H, int W, int C, int h, int w, int levels,
                               void* stream) {
    VQW_CHECK(image && edit && cellmask && out && workspace, "vqw_blend_cells: null pointer (only recon may be null)");
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 1, "vqw_blend_cells: N=%d, H=%d, W=%d, C=%d must be positive", N, H, W, C);
    VQW_CHECK(levels >= 1 && levels <= BL_MAX_LEVELS, "vqw_blend_cells: levels=%d must lie in [1, %d]", levels, BL_MAX_LEVELS);
    VQW_CHECK(h >= 1 && w >= 1 && H % h == 0 && W % w == 0, "vqw_blend_cells: H=%d, W=%d must be multiples of the cell grid h=%d, w=%d", H, W, h, w);
    VQW_CHECK(H % (1L << levels) == 0 && W % (1L << levels) == 0, "vqw_blend_cells: 2^levels = %ld must divide H=%d and W=%d", 1L << levels, H, W);
    VQW_CHECK(N <= 65535, "vqw_blend_cells: N=%d exceeds the 65535 images of one launch", N);
    VQW_CHECK(C <= 65534, "vqw_blend_cells: C=%d exceeds the 65534 channels of one launch", C);
    long total = (long)N * H;                       // factor by factor: the product of four ints can leave a long
    if (total < (1L << 31)) total *= W;
    if (total < (1L << 31)) total *= C + 1;
    VQW_CHECK(total < (1L << 31), "vqw_blend_cells: N * H * W * (C + 1) = %d * %d * %d * %d elements need 32-bit indices", N, H, W, C + 1);
    const long need = vqw_blend_cells_workspace(N, H, W, C, levels);
    VQW_CHECK(workspace_floats >= need, "vqw_blend_cells: workspace of %ld floats, %ld needed (vqw_blend_cells_workspace)", workspace_floats, need);
    VQW_CHECK(al16(image) && al16(edit) && al16(recon) && al16(out) && al16(workspace),
              "vqw_blend_cells: image, edit, recon, out and workspace must be 16-byte aligned");
    const float* base = recon ? recon : image;
    const int fy = H / h, fx = W / w;
    hipStream_t st = (hipStream_t)stream;
    float* gm[BL_MAX_LEVELS + 1];
    float* r[BL_MAX_LEVELS + 1];
    float* at = workspace;
    gm[0] = r[0] = r[levels] = nullptr;
    for (int l = 1; l <= levels; ++l) { gm[l] = at; at += blend_gm_floats(N, H, W, C, l); }
    for (int l = 1; l < levels; ++l) { r[l] = at; at += blend_r_floats(N, H, W, C, l); }
    for (int l = 0; l < levels; ++l) {              // G_{l+1}, M_{l+1} from level l
        const int Hi = H >> l, Wi = W >> l, tx = ceil_div(Wi / 2, BL_RTX), ty = ceil_div(Hi / 2, BL_RTY);
        const dim3 grid(tx * ty, C + 1, N);
        if (l == 0)
            hipLaunchKernelGGL(k_blend_reduce<true>, grid, dim3(256), 0, st, edit, base, cellmask, (const float*)nullptr, gm[1], Hi, Wi, C, h, w, fy, fx, tx);
        else
            hipLaunchKernelGGL(k_blend_reduce<false>, grid, dim3(256), 0, st, (const float*)nullptr, (const float*)nullptr,
                               (const uint8_t*)nullptr, (const float*)gm[l], gm[l + 1], Hi, Wi, C, h, w, fy, fx, tx);
        VQW_LAUNCH_CHECK("vqw_blend_cells (reduce)");
    }
    for (int l = levels - 1; l >= 0; --l) {         // R_l from level l + 1; R_0 goes into out
        const int Hl = H >> l, Wl = W >> l, tx = ceil_div(Wl, BL_CTX), ty = ceil_div(Hl, BL_CTY);
        const dim3 grid(tx * ty, C, N);
        if (l == 0)
            hipLaunchKernelGGL(k_blend_collapse<true>, grid, dim3(256), 0, st, (const float*)gm[1], (const float*)r[1], (const float*)nullptr,
                               (float*)nullptr, image, edit, base, cellmask, out, Hl, Wl, C, h, w, fy, fx, tx);
        else
            hipLaunchKernelGGL(k_blend_collapse<false>, grid, dim3(256), 0, st, (const float*)gm[l + 1], (const float*)r[l + 1],
                               (const float*)gm[l], r[l], (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                               (const uint8_t*)nullptr, (float*)nullptr, Hl, Wl, C, h, w, fy, fx, tx);
        VQW_LAUNCH_CHECK("vqw_blend_cells (collapse)");
    }
    return VQW_OK;
}
