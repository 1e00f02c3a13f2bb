"""Restatement of the test-mode metrics for the tests (not imported by the product package).

The SSIM / PSNR / MSE definitions restate torchmetrics 0.6.2 as the reference calls them (`metric(recon, image)` with
default arguments, trainers/base.py:75-77); the package is not installed, so this is written from its documented
arithmetic:
- _gaussian: dist = arange((1 - k) / 2, (1 + k) / 2), g = exp(-(dist / sigma)^2 / 2), g / sum(g); the 2-D window is the
  outer product, applied per channel (grouped conv).
- _ssim_compute: R = max(range preds, range target) unless data_range is given, C1 = (k1 R)^2, C2 = (k2 R)^2, reflect pad
  by (k - 1) / 2, conv of (p, t, p p, t t, p t), sigma = E[x y] - mu_x mu_y, the SSIM map cropped by (k - 1) / 2, mean.
- PSNR with data_range=None: min_target / max_target states seeded with tensor(0.0), so R = max(max t, 0) - min(min t, 0);
  psnr = (2 ln R - ln mse) * 10 / ln 10.
- Entropy: scipy.stats.entropy(bincount(ids, minlength=K + 1)[1:], base=2).

`package_form(..., dtype=torch.float32)` is the package's own fp32 arithmetic; the GPU tests bound the kernels' distance
from the float64 value by twice that form's distance from it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def gaussian(kernel_size, sigma, dtype=torch.float64):
    dist = torch.arange((1 - kernel_size) / 2, (1 + kernel_size) / 2, 1.0, dtype=dtype)
    g = torch.exp(-torch.pow(dist / sigma, 2) / 2)
    return g / g.sum()


def _window(channels, kernel_size, sigma, dtype):
    g = gaussian(kernel_size, sigma, dtype).unsqueeze(0)
    return torch.matmul(g.t(), g).expand(channels, 1, kernel_size, kernel_size)


def ssim_range(p, t, data_range=None):
    if data_range is not None:
        return torch.tensor(float(data_range), dtype=p.dtype)
    return torch.max(p.max() - p.min(), t.max() - t.min())


def _ssim_map(mom, c1, c2, B):
    mu_p, mu_t, e_pp, e_tt, e_pt = (mom[i * B:(i + 1) * B] for i in range(5))
    mu_pp, mu_tt, mu_pt = mu_p.pow(2), mu_t.pow(2), mu_p * mu_t
    upper = 2 * (e_pt - mu_pt) + c2
    lower = (e_pp - mu_pp) + (e_tt - mu_tt) + c2
    return ((2 * mu_pt + c1) * upper) / ((mu_pp + mu_tt + c1) * lower)


def ssim_padded(p, t, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, data_range=None):
    """The package's form: reflect pad, grouped conv of the five maps, crop."""
    R = ssim_range(p, t, data_range)
    c1, c2 = (k1 * R) ** 2, (k2 * R) ** 2
    B, C = p.shape[:2]
    pad = (kernel_size - 1) // 2
    pp = F.pad(p, (pad, pad, pad, pad), mode="reflect")
    tt = F.pad(t, (pad, pad, pad, pad), mode="reflect")
    mom = F.conv2d(torch.cat((pp, tt, pp * pp, tt * tt, pp * tt)), _window(C, kernel_size, sigma, p.dtype), groups=C)
    m = _ssim_map(mom, c1, c2, B)
    m = m[..., pad:-pad, pad:-pad] if pad else m
    return m.mean()


def ssim_valid(p, t, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, data_range=None):
    """The same over the valid windows only (no padding, no crop)."""
    R = ssim_range(p, t, data_range)
    c1, c2 = (k1 * R) ** 2, (k2 * R) ** 2
    B, C = p.shape[:2]
    mom = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), _window(C, kernel_size, sigma, p.dtype), groups=C)
    return _ssim_map(mom, c1, c2, B).mean()


def psnr_range(t, data_range=None):
    if data_range is not None:
        return torch.tensor(float(data_range), dtype=t.dtype)
    zero = torch.tensor(0.0, dtype=t.dtype)
    return torch.maximum(t.max(), zero) - torch.minimum(t.min(), zero)


def psnr(p, t, data_range=None):
    mse = ((p - t) ** 2).sum() / p.numel()
    R = psnr_range(t, data_range)
    return (2 * torch.log(R) - torch.log(mse)) * (10 / torch.log(torch.tensor(10.0, dtype=p.dtype)))


def mse(p, t):
    return ((p - t) ** 2).sum() / p.numel()


def package_form(pred, target, data_range=None, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, dtype=torch.float64):
    """{'mse', 'ssim', 'psnr'} on the CPU in `dtype` (float64: the reference values; float32: the package's arithmetic)."""
    p = pred.detach().cpu().to(dtype)
    t = target.detach().cpu().to(dtype)
    return dict(mse=float(mse(p, t)), ssim=float(ssim_padded(p, t, kernel_size, sigma, k1, k2, data_range)),
                psnr=float(psnr(p, t, data_range)))


def entropy(ids, dict_size):
    """-> (entropy in bits, counts of 0..K): the numpy formula of scipy.stats.entropy(counts[1:], base=2)."""
    a = ids.detach().cpu().reshape(-1).numpy() if torch.is_tensor(ids) else np.asarray(ids).reshape(-1)
    counts = np.bincount(a, minlength=dict_size + 1)
    c = counts[1:].astype(np.float64)
    s = c.sum()
    if s == 0:
        return math.nan, counts
    pk = c[c > 0] / s
    return float(-(pk * np.log(pk)).sum() / np.log(2.0)), counts


def close(a, b, tol):
    """|a - b| <= tol, with nan == nan and equal infinities equal."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol
