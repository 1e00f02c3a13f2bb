// The pseudo-likelihood map of the bidirectional masked code prior (networks/gpt.py MaskedGPT.pseudo_nll): what the model thinks of
// a slice code by code, -log p(code | the other codes).  A latent grid h x w (T = h w, raster order) is split by a lattice of
// stride (sy, sx) into S = sy sx groups, g(t) = (y mod sy) sx + (x mod sx) for t = y w + x; pass s feeds the slice with the mask
// token at every position of group s, and position t is read off pass g(t).  The passes of a sample run side by side as batch
// rows, in chunks [s0, s0 + ns): chunk row r = b ns + (s - s0).  Two kernels, both forward only, integers and fp32, no atomics:
// the same bits every run.
//
// Lattice inputs.  inp[b ns + (s - s0)][t] = mask_token where g(t) = s, ids[b][t] elsewhere: one streaming pass over the B ns T
// output elements, 8 bytes per access (a code is a long), grid-strided; no mask tensor from the host.
//
// Gathering LayerNorm.  y[b][t][:] = LayerNorm(x[b ns + g(t) - s0][t][:]) for the (b, t) whose group lies in the chunk; every other
// row of y is left as it is, so successive chunks fill one y and ln_f, the head and the cross-entropy behind it run over B T rows,
// not B S T.  One wave per OUTPUT row; the row index is made wave-uniform (readfirstlane), so the group and the source row are
// scalar arithmetic, once per row.  The row's body is ln_row.h's - vqw_layernorm_fwd's own - so y has the bits of
// vqw_layernorm_fwd on the gathered row.  No statistics are written.
#include "common.h"
#include "ln_row.h"
#include "../../include/vqwnet_hip.h"

#define PN_MIN_E 4
#define PN_MAX_E 4096
#define PN_SMALL_E 1024     // vqw_layernorm_fwd's tiers: up to here a lane holds 4 float4 columns of a row, above 16

// the group of position t = y w + x
__device__ __forceinline__ int lattice_group(int t, int w, int sy, int sx) {
    const int y = t / w, x = t - y * w;
    return (y % sy) * sx + (x % sx);
}

// grid-strided over the n = B ns T elements of inp
__global__ void __launch_bounds__(256) k_lattice_inputs(const long* __restrict__ ids, long* __restrict__ inp, long n, int T, int w, int sy,
                                                        int sx, int s0, int ns, long mask_token) {
    const long step = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const long r = i / T;
        const int t = (int)(i - r * T);
        const long b = r / ns;
        const int s = s0 + (int)(r - b * ns);
        inp[i] = lattice_group(t, w, sy, sx) == s ? mask_token : ids[b * T + t];
    }
}

// grid ceil(B T / 4): wave v of workgroup g owns output row 4 g + v
template <int NV>
__global__ void __launch_bounds__(256) k_lattice_gather_ln(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ y, long rows, int T, int w, int E,
                                                           int sy, int sx, int s0, int ns, float eps) {
    const long r = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= rows) return;
    const long b = r / T;
    const int t = (int)(r - b * T);
    const int g = lattice_group(t, w, sy, sx) - s0;
    if (g < 0 || g >= ns) return;                    // another chunk's row: untouched
    const long src = (b * ns + g) * T + t;           // < B ns T, the rows of x
    float mu, rs;
    ln_row_fwd<NV>(x + src * E, gamma, beta, y + r * E, (int)(threadIdx.x & 63), E, eps, mu, rs);
}

static inline bool pn_al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// the checks both entry points share: the grid, the lattice and the chunk
static int lattice_check(const char* name, int B, int h, int w, int sy, int sx, int s0, int ns) {
    VQW_CHECK(B >= 1 && h >= 1 && w >= 1, "%s: B=%d, h=%d, w=%d must be at least 1", name, B, h, w);
    VQW_CHECK((long)h * w <= 65536, "%s: T = h w = %ld must not exceed 65536", name, (long)h * w);
    VQW_CHECK(sy >= 1 && sy <= h && sx >= 1 && sx <= w, "%s: stride (sy=%d, sx=%d) must lie in [1, h=%d] x [1, w=%d]", name, sy, sx, h, w);
    VQW_CHECK(s0 >= 0 && ns >= 1 && (long)s0 + ns <= (long)sy * sx, "%s: the chunk [s0=%d, s0 + ns=%ld) must be a non-empty part of the S = sy sx = %ld passes",
              name, s0, (long)s0 + ns, (long)sy * sx);
    VQW_CHECK((long)B * ns * h * w <= (1L << 31) - 4, "%s: B ns T = %ld chunk rows times positions are too many", name, (long)B * ns * h * w);
    return VQW_OK;
}

extern "C" int vqw_lattice_inputs(const long* ids, long* inp, int B, int h, int w, int sy, int sx, int s0, int ns, long mask_token,
                                  void* stream) {
    if (int rc = lattice_check("vqw_lattice_inputs", B, h, w, sy, sx, s0, ns)) return rc;
    VQW_CHECK(mask_token >= 0, "vqw_lattice_inputs: mask_token=%ld must not be negative", mask_token);
    VQW_CHECK(ids && inp, "vqw_lattice_inputs: null pointer");
    VQW_CHECK(pn_al8(ids) && pn_al8(inp), "vqw_lattice_inputs: ids and inp must be 8-byte aligned");
    VQW_CHECK((const void*)ids != (const void*)inp, "vqw_lattice_inputs: inp must not be ids itself");
    const int T = h * w;
    const long n = (long)B * ns * T;
    hipLaunchKernelGGL(k_lattice_inputs, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, ids, inp, n, T, w, sy, sx, s0, ns, mask_token);
    VQW_LAUNCH_CHECK("vqw_lattice_inputs");
    return VQW_OK;
}

extern "C" int vqw_lattice_gather_ln(const float* x, const float* gamma, const float* beta, float* y, int B, int h, int w, int E, int sy,
                                     int sx, int s0, int ns, float eps, void* stream) {
    if (int rc = lattice_check("vqw_lattice_gather_ln", B, h, w, sy, sx, s0, ns)) return rc;
    VQW_CHECK(E % 4 == 0 && E >= PN_MIN_E && E <= PN_MAX_E, "vqw_lattice_gather_ln: E=%d must be a multiple of 4 with %d <= E <= %d", E, PN_MIN_E,
              PN_MAX_E);
    VQW_CHECK(x && gamma && beta && y, "vqw_lattice_gather_ln: null pointer");
    VQW_CHECK(al16(x) && al16(gamma) && al16(beta) && al16(y), "vqw_lattice_gather_ln: tensors must be 16-byte aligned");
    VQW_CHECK((const void*)x != (const void*)y, "vqw_lattice_gather_ln: y must not be x itself (a row is read from another row's place)");
    const int T = h * w;
    const long rows = (long)B * T;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(rows, 4));
    if (E <= PN_SMALL_E)
        hipLaunchKernelGGL((k_lattice_gather_ln<PN_SMALL_E / 256>), grid, dim3(256), 0, st, x, gamma, beta, y, rows, T, w, E, sy, sx, s0, ns, eps);
    else
        hipLaunchKernelGGL((k_lattice_gather_ln<PN_MAX_E / 256>), grid, dim3(256), 0, st, x, gamma, beta, y, rows, T, w, E, sy, sx, s0, ns, eps);
    VQW_LAUNCH_CHECK("vqw_lattice_gather_ln");
    return VQW_OK;
}
