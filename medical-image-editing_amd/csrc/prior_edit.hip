// The composite of an edit with the code prior (trainers/prior.py PriorTrainer.edit): the pixels of the selected latent cells come
// from the edited picture, the others from the original.  NHWC, fp32, one streaming kernel: every output element is written once,
// and only the picture it comes from is read.
#include "common.h"
#include "../../include/vqwnet_hip.h"

// a thread per unit of VEC ? 4 floats : 1 float; VEC: a cell's row of fx C floats is a multiple of 4, so a unit lies in one cell
template <bool VEC>
__global__ void __launch_bounds__(256) k_paste_cells(const float* __restrict__ image, const float* __restrict__ edit,
                                                     const uint8_t* __restrict__ cellmask, float* __restrict__ out, long units, int H, int W,
                                                     int C, int h, int w, int fy, int fx) {
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += gstride) {
        const long e = VEC ? 4 * i : i, p = e / C;
        const int x = (int)(p % W), y = (int)((p / W) % H);
        const long b = p / ((long)W * H);
        const float* src = cellmask[(b * h + y / fy) * w + x / fx] ? edit : image;
        if (VEC) *(float4*)(out + e) = *(const float4*)(src + e);
        else out[e] = src[e];
    }
}

extern "C" int vqw_paste_cells(const float* image, const float* edit, const uint8_t* cellmask, float* out, int N, int H, int W, int C, int h,
                               int w, void* stream) {
    VQW_CHECK(image && edit && cellmask && out, "vqw_paste_cells: null pointer");
    VQW_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 1, "vqw_paste_cells: N=%d, H=%d, W=%d, C=%d must be positive", N, H, W, C);
    VQW_CHECK(h >= 1 && w >= 1 && H % h == 0 && W % w == 0, "vqw_paste_cells: H=%d, W=%d must be multiples of the cell grid h=%d, w=%d", H, W, h, w);
    long total = (long)N * H;                       // factor by factor: the product of four ints can leave a long
    if (total < (1L << 31)) total *= W;
    if (total < (1L << 31)) total *= C;
    VQW_CHECK(total < (1L << 31), "vqw_paste_cells: N * H * W * C = %d * %d * %d * %d elements need 32-bit indices", N, H, W, C);
    const int fy = H / h, fx = W / w;
    hipStream_t st = (hipStream_t)stream;
    if (((long)fx * C) % 4 == 0 && al16(image) && al16(edit) && al16(out))
        hipLaunchKernelGGL(k_paste_cells<true>, dim3(stream_grid(total / 4, 256)), dim3(256), 0, st, image, edit, cellmask, out, total / 4, H, W, C, h, w, fy, fx);
    else
        hipLaunchKernelGGL(k_paste_cells<false>, dim3(stream_grid(total, 256)), dim3(256), 0, st, image, edit, cellmask, out, total, H, W, C, h, w, fy, fx);
    VQW_LAUNCH_CHECK("vqw_paste_cells");
    return VQW_OK;
}
