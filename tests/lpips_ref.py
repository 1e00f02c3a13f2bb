"""fp64 restatement of the reference's LPIPSLoss (functions/lpips_loss.py; trainers/base.py:271-275), i.e. of
lpips.LPIPS(net='alex') version 0.1 with its defaults (linear layers on, spatial=False, eval mode, normalize=False):

    x -> (x - shift) / scale -> conv 11x11 / 4, pad 2 (3 -> 64), ReLU [tap 0] -> max-pool 3 / 2 -> conv 5x5, pad 2 (-> 192),
    ReLU [tap 1] -> max-pool 3 / 2 -> conv 3x3 (-> 384), ReLU [tap 2] -> conv 3x3 (-> 256), ReLU [tap 3] -> conv 3x3 (-> 256),
    ReLU [tap 4];  per tap a = f / (|f| + 1e-10) over channels, d = sum_c w_c (a_c - b_c)^2, mean over pixels; taps summed
    per image; loss = mean over the batch; gradient to sr only

Every convolution is accumulated tap by tap and input channel by input channel with element-wise multiply-adds, not through
a GEMM: each output element sees the same operations in the same order wherever it sits, so equal input windows give
bit-equal outputs and the max-pools' ties are exact.  Ties go to the first maximum in row-major window order (ATen's rule).
The backward pass is written out.  Where a pixel's tap features are all zero the normalisation contributes zero gradient
(autograd through sqrt gives NaN there, discarded again by the select in the ReLU's backward).  `window` = (alpha, beta,
lo, hi): both images go through clamp(alpha x + beta, lo, hi) first; its derivative is alpha strictly inside (lo, hi),
else 0.
"""
import torch
import torch.nn.functional as F

# (slice, features index, in, out, kernel, stride, padding)
LAYERS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
          (5, 10, 256, 256, 3, 1, 1))
CHANNELS = (64, 192, 384, 256, 256)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10


def he_weights(seed=0, layout="lpips", bias0=None, gain0=1.0):
    """He-normal AlexNet front-end weights with small positive biases and non-negative lin weights.  layout 'lpips': one
    dict keyed as the LPIPS module's state dict (`loss_func.net.slice1.0.weight`, `loss_func.lin0.model.1.weight`, ...);
    'pair': (alexnet, lins) keyed as torchvision's alexnet (`features.N.*`) and the package's alex.pth
    (`lin{i}.model.1.weight`).  bias0: a constant for the first layer's bias (strongly negative: whole pixels go to zero);
    gain0: a factor on the first layer's weight."""
    g = torch.Generator().manual_seed(seed)
    alex, lins = {}, {}
    for s, idx, cin, cout, k, _, _ in LAYERS:
        alex["features.%d.weight" % idx] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        alex["features.%d.bias" % idx] = torch.rand(cout, generator=g) * 0.05 + 0.01
    if bias0 is not None:
        alex["features.0.bias"] = torch.full((64,), float(bias0))
    alex["features.0.weight"] = alex["features.0.weight"] * gain0
    for i, c in enumerate(CHANNELS):
        lins["lin%d.model.1.weight" % i] = torch.rand(1, c, 1, 1, generator=g)
    if layout == "pair":
        return alex, lins
    sd = {}
    for s, idx, *_ in LAYERS:
        for kind in ("weight", "bias"):
            sd["loss_func.net.slice%d.%d.%s" % (s, idx, kind)] = alex["features.%d.%s" % (idx, kind)]
    for i in range(5):
        sd["loss_func.lin%d.model.1.weight" % i] = lins["lin%d.model.1.weight" % i]
    return sd


def params_of(sd, device, dtype=torch.float64):
    """{'w': [5 conv weights], 'b': [5 biases], 'lin': [5 x (C,)], 'shift', 'scale'} from a state dict in the module's own
    layout (scaling buffers optional)."""
    sd = {k[len("perceptual_loss."):] if k.startswith("perceptual_loss.") else k: v for k, v in sd.items()}
    t = lambda v: v.detach().to(device=device, dtype=dtype)        # noqa: E731
    w = [t(sd["loss_func.net.slice%d.%d.weight" % (s, idx)]) for s, idx, *_ in LAYERS]
    b = [t(sd["loss_func.net.slice%d.%d.bias" % (s, idx)]) for s, idx, *_ in LAYERS]
    lin = [t(sd["loss_func.lin%d.model.1.weight" % i]).reshape(-1) for i in range(5)]
    shift = t(sd["loss_func.scaling_layer.shift"]) if "loss_func.scaling_layer.shift" in sd else torch.tensor(SHIFT, device=device, dtype=dtype)
    scale = t(sd["loss_func.scaling_layer.scale"]) if "loss_func.scaling_layer.scale" in sd else torch.tensor(SCALE, device=device, dtype=dtype)
    return dict(w=w, b=b, lin=lin, shift=shift.reshape(1, 3, 1, 1), scale=scale.reshape(1, 3, 1, 1))


def conv(x, w, b=None, stride=1, pad=0):
    """k x k convolution, element-wise accumulation in a fixed (ky, kx, c) order."""
    N, C, H, W = x.shape
    k = w.shape[2]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    y = torch.zeros(N, w.shape[0], Ho, Wo, dtype=x.dtype, device=x.device)
    for ky in range(k):
        for kx in range(k):
            for c in range(C):
                y.addcmul_(xp[:, c:c + 1, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride],
                           w[:, c, ky, kx].reshape(1, -1, 1, 1))
    if b is not None:
        y += b.reshape(1, -1, 1, 1)
    return y


def conv_t(g, w, H, W, stride=1, pad=0):
    """Input gradient (N, Cin, H, W) of conv from the output gradient g."""
    if stride == 1:
        return conv(g, w.flip(2, 3).transpose(0, 1), None, 1, w.shape[2] - 1 - pad)
    N, _, Ho, Wo = g.shape
    k = w.shape[2]
    out = torch.zeros(N, w.shape[1], H + 2 * pad, W + 2 * pad, dtype=g.dtype, device=g.device)
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += torch.einsum(
                "nohw,oc->nchw", g, w[:, :, ky, kx])
    return out[:, :, pad:pad + H, pad:pad + W]


def maxpool3(r):
    """MaxPool2d(3, 2), floor mode -> (pooled, arg-max index 0..8 in row-major window order, top-1 minus top-2 per window)."""
    Ho, Wo = (r.shape[2] - 3) // 2 + 1, (r.shape[3] - 3) // 2 + 1
    c = [r[:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2] for dy in range(3) for dx in range(3)]
    m, idx = c[0].clone(), torch.zeros(c[0].shape, dtype=torch.int64, device=r.device)
    for k in range(1, 9):
        upd = c[k] > m
        m = torch.where(upd, c[k], m)
        idx = torch.where(upd, torch.full_like(idx, k), idx)
    s = torch.stack(c).topk(2, dim=0).values
    return m, idx, s[0] - s[1]


def unpool3(g, idx, H, W):
    out = torch.zeros(g.shape[0], g.shape[1], H, W, dtype=g.dtype, device=g.device)
    Ho, Wo = g.shape[2], g.shape[3]
    for k in range(9):
        dy, dx = divmod(k, 3)
        out[:, :, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2] += torch.where(idx == k, g, torch.zeros_like(g))
    return out


def _win(x, window):
    if window is None:
        return x
    a, b, lo, hi = window
    return (a * x + b).clamp(lo, hi)


def features(x, p, window=None):
    """-> ([f0 .. f4] the five taps, dict of what the backward needs) for x (N, 1 or 3, H, W)."""
    x = _win(x, window).expand(x.shape[0], 3, x.shape[2], x.shape[3])
    x = (x - p["shift"]) / p["scale"]
    f0 = conv(x, p["w"][0], p["b"][0], 4, 2).clamp_min(0)
    p0, i0, gap0 = maxpool3(f0)
    f1 = conv(p0, p["w"][1], p["b"][1], 1, 2).clamp_min(0)
    p1, i1, gap1 = maxpool3(f1)
    f2 = conv(p1, p["w"][2], p["b"][2], 1, 1).clamp_min(0)
    f3 = conv(f2, p["w"][3], p["b"][3], 1, 1).clamp_min(0)
    f4 = conv(f3, p["w"][4], p["b"][4], 1, 1).clamp_min(0)
    return [f0, f1, f2, f3, f4], dict(i0=i0, i1=i1, gap0=gap0, gap1=gap1, top0=p0, top1=p1)


def distance(fs, fh, w):
    """-> (d per image (N,), d(mean d)/dfs under the zero-norm convention, the number of all-zero pixels of fs, the smallest
    non-zero norm of either half) of one tap."""
    r = (fs * fs).sum(1, keepdim=True).sqrt()
    a = fs / (r + EPS)
    rh = (fh * fh).sum(1, keepdim=True).sqrt()
    b = fh / (rh + EPS)
    wv = w.reshape(1, -1, 1, 1)
    delta = a - b
    hw = fs.shape[2] * fs.shape[3]
    d = (wv * delta * delta).sum(1).sum((1, 2)) / hw
    S = (wv * delta * fs).sum(1, keepdim=True)
    safe = torch.where(r > 0, r, torch.ones_like(r))
    g = (2.0 / (r + EPS)) * (wv * delta - a * S / safe)
    g = torch.where(r > 0, g, torch.zeros_like(g)) / hw
    rmin = min(float(v[v > 0].min()) if bool((v > 0).any()) else float("inf") for v in (r, rh))
    return d, g, int((r == 0).sum()), rmin


def lpips_loss_ref(sr, hr, sd, window=None, device=None, dtype=torch.float64, allow_zero_norm=False):
    """-> (loss, dloss/dsr, info) in fp64 (dtype = torch.float32: the same operations in fp32, one rendering of the
    reference's fp32 arithmetic).  info: gap0 / gap1 = top-1 minus top-2 of the sr half's pool windows, top0 / top1 = their
    maxima, zero_norm = the number of (pixel, tap) pairs of the sr half with all-zero features (asserted 0 unless allowed),
    rmin = the smallest non-zero feature norm of any pixel of either half at any tap."""
    device = device or sr.device
    p = params_of(sd, device, dtype)
    sr = sr.detach().to(device=device, dtype=dtype)
    hr = hr.detach().to(device=device, dtype=dtype)
    N, C, H, W = sr.shape
    fs, t = features(sr, p, window)
    fh, _ = features(hr, p, window)
    loss = torch.zeros((), dtype=dtype, device=device)
    gd, zero_norm, rmin = [], 0, float("inf")
    for i in range(5):
        d, g, z, rm = distance(fs[i], fh[i], p["lin"][i])
        rmin = min(rmin, rm)
        loss = loss + d.sum() / N
        gd.append(g / N)
        zero_norm += z
    assert allow_zero_norm or zero_norm == 0, "lpips_ref: %d all-zero feature pixels" % zero_norm
    g = gd[4] * (fs[4] > 0)
    g = (conv_t(g, p["w"][4], 0, 0, 1, 1) + gd[3]) * (fs[3] > 0)
    g = (conv_t(g, p["w"][3], 0, 0, 1, 1) + gd[2]) * (fs[2] > 0)
    g = conv_t(g, p["w"][2], 0, 0, 1, 1)
    g = (unpool3(g, t["i1"], fs[1].shape[2], fs[1].shape[3]) + gd[1]) * (fs[1] > 0)
    g = conv_t(g, p["w"][1], 0, 0, 1, 2)
    g = (unpool3(g, t["i0"], fs[0].shape[2], fs[0].shape[3]) + gd[0]) * (fs[0] > 0)
    g = conv_t(g, p["w"][0], H, W, 4, 2) / p["scale"]          # d/d expanded input, 3 channels
    if C == 1:
        g = g.sum(dim=1, keepdim=True)                           # expand's backward
    if window is not None:
        a, b, lo, hi = window
        z = a * sr + b
        g = g * a * ((z > lo) & (z < hi))
    info = dict(gap0=t["gap0"], gap1=t["gap1"], top0=t["top0"], top1=t["top1"], zero_norm=zero_norm, rmin=rmin)
    return loss, g, info


def reach(mask, stride, kernel, offset, H, W):
    """Input pixels (N, 1, H, W) reached by the marked windows of a map whose window (oy, ox) covers the input rows
    stride * oy - offset .. + kernel - 1 (and columns likewise)."""
    m = F.conv_transpose2d(mask.double(), torch.ones(1, 1, kernel, kernel, dtype=torch.float64, device=mask.device), stride=stride)
    m = F.pad(m, (0, max(0, W + offset - m.shape[3]), 0, max(0, H + offset - m.shape[2])))
    return m[:, :, offset:offset + H, offset:offset + W] > 0


def unclear_pixels(info, H, W, rel=1e-5):
    """Input pixels reached by a pool window whose top-2 gap is positive and <= rel * (1 + |top|).  A window of the first
    pool covers 19 x 19 input pixels (rows 8 oy - 2 ..), one of the second pool 67 x 67 (rows 16 oy - 18 ..)."""
    out, n = None, 0
    for gap, top, stride, kernel, offset in ((info["gap0"], info["top0"], 8, 19, 2), (info["gap1"], info["top1"], 16, 67, 18)):
        u = ((gap > 0) & (gap <= rel * (1 + top.abs())))
        n += int(u.sum())
        r = reach(u.any(dim=1, keepdim=True), stride, kernel, offset, H, W)
        out = r if out is None else (out | r)
    return out, n


def module_ref(sd, dtype=torch.float64, device="cpu"):
    """The same network as plain torch modules and functions (F.conv2d, F.max_pool2d, autograd): f(sr, hr) -> loss."""
    p = params_of(sd, device, dtype)

    def feats(x):
        x = (x.expand(x.shape[0], 3, x.shape[2], x.shape[3]) - p["shift"]) / p["scale"]
        out = []
        for i, (_, _, _, _, _, stride, pad) in enumerate(LAYERS):
            if i in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, p["w"][i], p["b"][i], stride=stride, padding=pad))
            out.append(x)
        return out

    def f(sr, hr, window=None):
        fs, fh = feats(_win(sr, window)), feats(_win(hr, window))
        total = 0
        for i in range(5):
            a = fs[i] / (fs[i].pow(2).sum(1, keepdim=True).sqrt() + EPS)
            b = fh[i] / (fh[i].pow(2).sum(1, keepdim=True).sqrt() + EPS)
            total = total + F.conv2d((a - b) ** 2, p["lin"][i].reshape(1, -1, 1, 1)).mean((2, 3), keepdim=True)
        return total.mean()
    return f
