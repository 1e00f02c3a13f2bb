"""Restatements of the seamless composite of an edit (csrc/blend.hip, ops.blend_cells): Burt-Adelson multi-band blending of the
difference picture under the Gaussian pyramid of the cell mask.

    REDUCE(x)[i, j] = sum_m sum_n w[m] w[n] x[clamp(2i+m), clamp(2j+n)], m, n = -2..2, w = [1, 4, 6, 4, 1] / 16
    EXPAND(x), along each axis in turn: [2k] = (x[k-1] + 6 x[k] + x[k+1]) / 8, [2k+1] = (x[k] + x[k+1]) / 2, indices clamped
    M_0 = the cell mask at pixels, M_{l+1} = REDUCE(M_l); G_0 = d = edit - image (or edit - recon), G_{l+1} = REDUCE(G_l)
    R_L = M_L G_L; R_l = M_l (G_l - EXPAND(G_{l+1})) + EXPAND(R_{l+1}); out = image + R_0

blend_ref follows the kernel's order operation by operation - row pass (along x), then column pass, taps ascending and accumulated
from the left, one rounding per operation - so that with dtype=torch.float32 it is the kernel's arithmetic and with torch.float64
the truth.  blend_brute is the same definition with explicit loops over the taps in numpy float64 (2-D sums, no separable passes).
"""
import numpy as np
import torch

TAPS = (0.0625, 0.25, 0.375, 0.25, 0.0625)          # exact in fp32


def _reduce_axis(x, dim):
    n = x.shape[dim]
    i = torch.arange(n // 2)
    acc = None
    for m in range(5):
        term = TAPS[m] * x.index_select(dim, (2 * i + m - 2).clamp(0, n - 1))
        acc = term if acc is None else acc + term
    return acc


def reduce(x):
    """REDUCE over the last two dimensions (..., H, W) -> (..., H/2, W/2): rows (along W) first, then columns."""
    return _reduce_axis(_reduce_axis(x, x.dim() - 1), x.dim() - 2)


def _expand_axis(x, dim):
    n = x.shape[dim]
    k = torch.arange(n)
    a, c = x.index_select(dim, (k - 1).clamp(0, n - 1)), x.index_select(dim, (k + 1).clamp(0, n - 1))
    even = ((a + 6.0 * x) + c) * 0.125
    odd = (x + c) * 0.5
    shape = list(x.shape)
    shape[dim] = 2 * n
    return torch.stack((even, odd), dim=dim + 1).reshape(shape)


def expand(x):
    """EXPAND over the last two dimensions (..., H, W) -> (..., 2H, 2W): rows (along W) first, then columns."""
    return _expand_axis(_expand_axis(x, x.dim() - 1), x.dim() - 2)


def mask_pixels(cellmask, H, W, dtype):
    """M_0 (B, 1, H, W): the cell mask (B, h, w) up-sampled by nearest neighbour, 0 / 1."""
    B, h, w = cellmask.shape
    m = (cellmask != 0).to(dtype)
    return m.repeat_interleave(H // h, dim=1).repeat_interleave(W // w, dim=2).reshape(B, 1, H, W)


def correction_ref(d, m0, levels):
    """R_0 (B, C, H, W) from the difference picture d (B, C, H, W) and M_0 (B, 1, H, W), in their dtype."""
    G, M = [d], [m0]
    for _ in range(levels):
        G.append(reduce(G[-1]))
        M.append(reduce(M[-1]))
    R = M[levels] * G[levels]
    for l in range(levels - 1, -1, -1):
        R = M[l] * (G[l] - expand(G[l + 1])) + expand(R)
    return R


def blend_ref(image, edit, cellmask, levels, recon=None, dtype=torch.float64, return_correction=False):
    """out = image + R_0 for image, edit, recon (B, C, H, W) and cellmask (B, h, w) uint8, computed in `dtype` on the host."""
    image, edit = image.detach().cpu().contiguous().to(dtype), edit.detach().cpu().contiguous().to(dtype)
    base = image if recon is None else recon.detach().cpu().contiguous().to(dtype)
    H, W = image.shape[-2:]
    if levels < 1 or H % (1 << levels) or W % (1 << levels):
        raise ValueError("blend_ref: 2^levels = 2^%d must divide %d x %d" % (levels, H, W))
    R = correction_ref(edit - base, mask_pixels(cellmask.cpu(), H, W, dtype), levels)
    out = image + R
    return (out, R) if return_correction else out


# ------------------------------------------------------------------------------------------------ brute force
def _c(v, n):
    return min(max(v, 0), n - 1)


def reduce_brute(x):
    H, W = x.shape
    w = [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16]
    out = np.zeros((H // 2, W // 2))
    for i in range(H // 2):
        for j in range(W // 2):
            s = 0.0
            for m in range(-2, 3):
                for n in range(-2, 3):
                    s += w[m + 2] * w[n + 2] * x[_c(2 * i + m, H), _c(2 * j + n, W)]
            out[i, j] = s
    return out


def expand_brute(x):
    H, W = x.shape
    rows = np.zeros((H, 2 * W))
    for i in range(H):
        for k in range(W):
            rows[i, 2 * k] = (x[i, _c(k - 1, W)] + 6 * x[i, k] + x[i, _c(k + 1, W)]) / 8
            rows[i, 2 * k + 1] = (x[i, k] + x[i, _c(k + 1, W)]) / 2
    out = np.zeros((2 * H, 2 * W))
    for k in range(H):
        for j in range(2 * W):
            out[2 * k, j] = (rows[_c(k - 1, H), j] + 6 * rows[k, j] + rows[_c(k + 1, H), j]) / 8
            out[2 * k + 1, j] = (rows[k, j] + rows[_c(k + 1, H), j]) / 2
    return out


def blend_brute(image, edit, cellmask, levels, recon=None):
    """numpy float64 (B, C, H, W), explicit loops over taps, pixels and planes."""
    image, edit = np.asarray(image, dtype=np.float64), np.asarray(edit, dtype=np.float64)
    base = image if recon is None else np.asarray(recon, dtype=np.float64)
    cellmask = np.asarray(cellmask)
    B, C, H, W = image.shape
    h, w = cellmask.shape[1:]
    out = np.zeros_like(image)
    for b in range(B):
        M = [np.zeros((H, W))]
        for y in range(H):
            for x in range(W):
                M[0][y, x] = 1.0 if cellmask[b, y // (H // h), x // (W // w)] else 0.0
        for _ in range(levels):
            M.append(reduce_brute(M[-1]))
        for c in range(C):
            G = [edit[b, c] - base[b, c]]
            for _ in range(levels):
                G.append(reduce_brute(G[-1]))
            R = M[levels] * G[levels]
            for l in range(levels - 1, -1, -1):
                R = M[l] * (G[l] - expand_brute(G[l + 1])) + expand_brute(R)
            out[b, c] = image[b, c] + R
    return out


def boundary_jump(picture, cellmask):
    """The largest |difference| between horizontally or vertically neighbouring pixels that lie in cells of different mask value:
    the step a composite carries along the boundary of the edited region.  picture (B, C, H, W), cellmask (B, h, w)."""
    B, C, H, W = picture.shape
    m = mask_pixels(cellmask.cpu(), H, W, torch.float64)
    p = picture.detach().cpu().double()
    dx, dy = (p[..., :, 1:] - p[..., :, :-1]).abs(), (p[..., 1:, :] - p[..., :-1, :]).abs()
    ex, ey = (m[..., :, 1:] != m[..., :, :-1]).expand_as(dx), (m[..., 1:, :] != m[..., :-1, :]).expand_as(dy)
    vals = [float(v[e].max()) for v, e in ((dx, ex), (dy, ey)) if bool(e.any())]
    return max(vals) if vals else 0.0
