"""fp64 restatement of the reference's VGGLoss(conv_index='22') (functions/perceptual_loss.py; trainers/base.py:271-275):

    vgg = vgg19.features[:8] = conv1_1, ReLU, conv1_2, ReLU, MaxPool2d(2), conv2_1, ReLU, conv2_2   (output before ReLU)
    loss = F.mse_loss(vgg(sr.expand(B, 3, H, W)), vgg(hr.expand(B, 3, H, W)))            gradient to sr only

Every convolution is accumulated tap by tap and input channel by input channel with element-wise fp64 multiply-adds, not
through a GEMM: each output element sees the same operations in the same order wherever it sits, so equal input windows
give bit-equal outputs and the max-pool's ties are exact.  Ties go to the first maximum in row-major window order (ATen's
rule).  The backward pass is written out (transposed convolutions the same way, the pool routed by the forward's arg-max).
`window` = (alpha, beta, lo, hi): both images go through clamp(alpha x + beta, lo, hi) first; its derivative is alpha
strictly inside (lo, hi), else 0.
"""
import torch
import torch.nn.functional as F

LAYERS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128))


def he_weights(seed=0, layout="torchvision"):
    """He-normal VGG slice weights (small random biases), keyed as torchvision's vgg19 state dict (`features.N.*`) or as
    VGGLoss's own (`vgg.N.*`)."""
    g = torch.Generator().manual_seed(seed)
    pre = "features." if layout == "torchvision" else "vgg."
    sd = {}
    for idx, cin, cout in LAYERS:
        sd["%s%d.weight" % (pre, idx)] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd["%s%d.bias" % (pre, idx)] = torch.randn(cout, generator=g) * 0.05
    return sd


def conv3x3(x, w, b=None):
    """'same' 3x3 convolution, element-wise accumulation in a fixed (ky, kx, c) order."""
    N, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros(N, w.shape[0], H, W, dtype=x.dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            for c in range(C):
                y.addcmul_(xp[:, c:c + 1, ky:ky + H, kx:kx + W], w[:, c, ky, kx].reshape(1, -1, 1, 1))
    if b is not None:
        y += b.reshape(1, -1, 1, 1)
    return y


def conv3x3_t(g, w):
    """Input gradient of conv3x3 (the transposed convolution) from the output gradient g."""
    return conv3x3(g, w.flip(2, 3).transpose(0, 1))


def maxpool2(r):
    """-> (pooled, arg-max index 0..3 in row-major window order, top-1 minus top-2 of each window)."""
    H2, W2 = r.shape[2] // 2 * 2, r.shape[3] // 2 * 2
    c = [r[:, :, dy:H2:2, dx:W2:2] for dy in (0, 1) for dx in (0, 1)]
    m, idx = c[0].clone(), torch.zeros(c[0].shape, dtype=torch.int64, device=r.device)
    for k in (1, 2, 3):
        upd = c[k] > m
        m = torch.where(upd, c[k], m)
        idx = torch.where(upd, torch.full_like(idx, k), idx)
    s = torch.stack(c).sort(dim=0, descending=True).values
    return m, idx, s[0] - s[1]


def unpool2(g, idx, H, W):
    out = torch.zeros(g.shape[0], g.shape[1], H, W, dtype=g.dtype, device=g.device)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, dy:H // 2 * 2:2, dx:W // 2 * 2:2] = torch.where(idx == k, g, torch.zeros_like(g))
    return out


def _win(x, window):
    if window is None:
        return x
    a, b, lo, hi = window
    return (a * x + b).clamp(lo, hi)


def features(x, sd, window=None, keep=False):
    """vgg(x) in fp64 for x (N, 1 or 3, H, W); sd: {'vgg.N.weight' ...} fp64 on x's device."""
    x = _win(x, window).expand(x.shape[0], 3, x.shape[2], x.shape[3])
    z1 = conv3x3(x, sd["vgg.0.weight"], sd["vgg.0.bias"])
    a1 = z1.clamp_min(0)
    z12 = conv3x3(a1, sd["vgg.2.weight"], sd["vgg.2.bias"])
    p1, idx, gap = maxpool2(z12.clamp_min(0))
    z21 = conv3x3(p1, sd["vgg.5.weight"], sd["vgg.5.bias"])
    y = conv3x3(z21.clamp_min(0), sd["vgg.7.weight"], sd["vgg.7.bias"])
    return (y, dict(z1=z1, z12=z12, idx=idx, gap=gap, p1=p1, z21=z21)) if keep else y


def _sd64(sd, device):
    out = {}
    for k, v in sd.items():
        k = "vgg." + k.split(".", 1)[1] if k.startswith("features.") else k
        out[k] = v.detach().to(device=device, dtype=torch.float64)
    return out


def vgg_loss_ref(sr, hr, sd, window=None, device=None, dtype=torch.float64):
    """-> (loss, dloss/dsr, per-window top-1 minus top-2 gap of the sr half's pool [N, 64, H/2, W/2]), all fp64 (dtype =
    torch.float32: the same operations in fp32, one rendering of the reference's fp32 arithmetic)."""
    device = device or sr.device
    sd = {k: v.to(dtype) for k, v in _sd64(sd, device).items()}
    sr = sr.detach().to(device=device, dtype=dtype)
    hr = hr.detach().to(device=device, dtype=dtype)
    ys, t = features(sr, sd, window, keep=True)
    yh = features(hr, sd, window)
    diff = ys - yh
    loss = (diff * diff).mean()
    g = diff * (2.0 / diff.numel())
    g = conv3x3_t(g, sd["vgg.7.weight"]) * (t["z21"] > 0)
    g = conv3x3_t(g, sd["vgg.5.weight"]) * (t["p1"] > 0)
    g = unpool2(g, t["idx"], sr.shape[2], sr.shape[3])
    g = conv3x3_t(g, sd["vgg.2.weight"]) * (t["z1"] > 0)
    g = conv3x3_t(g, sd["vgg.0.weight"])                       # d/d expanded input, 3 channels
    if sr.shape[1] == 1:
        g = g.sum(dim=1, keepdim=True)                           # expand's backward
    if window is not None:
        a, b, lo, hi = window
        z = a * sr + b
        g = g * a * ((z > lo) & (z < hi))
    return loss, g, t["gap"]


def sequential_ref(sd):
    """The 8 modules as a plain nn.Sequential (the reference's self.vgg), fp64."""
    import torch.nn as nn
    mods = []
    for i in range(8):
        spec = next((s for s in LAYERS if s[0] == i), None)
        if spec:
            c = nn.Conv2d(spec[1], spec[2], 3, padding=1).double()
            c.weight.data.copy_(sd["vgg.%d.weight" % i])
            c.bias.data.copy_(sd["vgg.%d.bias" % i])
            mods.append(c)
        else:
            mods.append(nn.MaxPool2d(2) if i == 4 else nn.ReLU())
    return nn.Sequential(*mods)
