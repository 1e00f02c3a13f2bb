"""Plain-torch restatement of the VQGAN decoder's blocks (GroupNorm(32, eps 1e-6)(+swish), single-head self-attention over a
feature map, ResnetBlock, AttnBlock, Upsample, Decoder), written from the formulas and evaluated from a state dict in any dtype:
the float64 truth of tests/test_gpu_vqgan_blocks.py and the check of tests/golden/vqgan_blocks*.npz in
tests/test_vqgan_blocks_host.py.

    GroupNorm   y = act(gamma_c (x - mean_{n,g}) / sqrt(var_{n,g} + eps) + beta_c), statistics over H W (C / 32) values,
                biased variance; act = identity or u * sigmoid(u)
    attention   o_i = sum_j softmax_j(scale <q_i, k_j>) v_j over the N = H W positions; lse_i = log sum_j exp(scale <q_i, k_j>)
"""
import torch
import torch.nn.functional as F

GROUPS = 32
EPS = 1e-6


def swish(u):
    return u * torch.sigmoid(u)


def group_norm_ref(x, gamma, beta, eps=EPS, act=False):
    N, C, H, W = x.shape
    xg = x.reshape(N, GROUPS, -1)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2, keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(N, C, H, W)
    u = xh * gamma[None, :, None, None] + beta[None, :, None, None]
    return swish(u) if act else u


def attention_ref(q, k, v, scale):
    """q, k, v (B, C, H, W) -> (o (B, C, H, W), lse (B, H W))"""
    B, C, H, W = q.shape
    qf, kf, vf = (t.reshape(B, C, H * W).transpose(1, 2) for t in (q, k, v))          # (B, N, C)
    s = torch.bmm(qf, kf.transpose(1, 2)) * scale
    lse = torch.logsumexp(s, dim=2)
    o = torch.bmm(torch.exp(s - lse[:, :, None]), vf)
    return o.transpose(1, 2).reshape(B, C, H, W), lse


def _conv(x, st, pre, pad):
    return F.conv2d(x, st[pre + "weight"], st[pre + "bias"], padding=pad)


def resnet_block_ref(x, st, pre):
    h = group_norm_ref(x, st[pre + "norm1.weight"], st[pre + "norm1.bias"], act=True)
    h = _conv(h, st, pre + "conv1.", 1)
    h = group_norm_ref(h, st[pre + "norm2.weight"], st[pre + "norm2.bias"], act=True)
    h = _conv(h, st, pre + "conv2.", 1)
    if pre + "conv_shortcut.weight" in st:
        x = _conv(x, st, pre + "conv_shortcut.", 1)
    elif pre + "nin_shortcut.weight" in st:
        x = _conv(x, st, pre + "nin_shortcut.", 0)
    return x + h


def attn_block_ref(x, st, pre):
    h = group_norm_ref(x, st[pre + "norm.weight"], st[pre + "norm.bias"])
    q, k, v = (_conv(h, st, pre + n + ".", 0) for n in "qkv")
    o, _ = attention_ref(q, k, v, int(x.shape[1]) ** (-0.5))
    return x + _conv(o, st, pre + "proj_out.", 0)


def upsample_ref(x, st, pre):
    return _conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), st, pre + "conv.", 1)


def decoder_ref(z, st, pre=""):
    """The decoder's forward from its state dict alone: the levels, blocks per level and attention blocks are read off the keys."""
    h = _conv(z, st, pre + "conv_in.", 1)
    h = resnet_block_ref(h, st, pre + "mid.block_1.")
    h = attn_block_ref(h, st, pre + "mid.attn_1.")
    h = resnet_block_ref(h, st, pre + "mid.block_2.")
    levels = 1 + max(int(k[len(pre) + 3:].split(".")[0]) for k in st if k.startswith(pre + "up."))
    for lv in reversed(range(levels)):
        b = 0
        while "%sup.%d.block.%d.norm1.weight" % (pre, lv, b) in st:
            h = resnet_block_ref(h, st, "%sup.%d.block.%d." % (pre, lv, b))
            if "%sup.%d.attn.%d.norm.weight" % (pre, lv, b) in st:
                h = attn_block_ref(h, st, "%sup.%d.attn.%d." % (pre, lv, b))
            b += 1
        if lv != 0:
            h = upsample_ref(h, st, "%sup.%d.upsample." % (pre, lv))
    h = group_norm_ref(h, st[pre + "norm_out.weight"], st[pre + "norm_out.bias"], act=True)
    return _conv(h, st, pre + "conv_out.", 1)


# the fixture cases of tests/golden/make_golden_vqgan_blocks.py: name -> (constructor name, kwargs, input shape, restatement)
CASES = {
    "res64": ("ResnetBlock", dict(in_channels=64), (2, 64, 16, 16), resnet_block_ref),
    "res32_64_nin": ("ResnetBlock", dict(in_channels=32, out_channels=64), (2, 32, 16, 16), resnet_block_ref),
    "res32_64_conv": ("ResnetBlock", dict(in_channels=32, out_channels=64, use_conv_shortcut=True), (2, 32, 16, 16), resnet_block_ref),
    "attn64": ("AttnBlock", dict(in_channels=64), (2, 64, 16, 16), attn_block_ref),
    "decoder": ("Decoder", dict(in_channels=8, mid_channels=32, out_channels=1, ch_multiplier=(1, 2), num_res_blocks=1,
                                attn_resolutions=[16], resolution=32, p_dropout=0.0, resamp_with_conv=True), (2, 8, 16, 16), decoder_ref),
}
SEEDS = {"res64": 71, "res32_64_nin": 72, "res32_64_conv": 73, "attn64": 74, "decoder": 75}


def case_ref(name, x, st):
    fn = CASES[name][3]
    return fn(x, st) if fn is decoder_ref else fn(x, st, "")


def round64(t):
    return torch.round(t * 64) / 64


def init_case_(module, seed):
    """The fixture's initial state of a freshly constructed module (reference or this project's): convolution weights rounded to
    multiples of 1/64, GroupNorm weight / bias drawn from a generator seeded with seed + 1000 - weight = 1 + N(0, 1) / 4,
    bias = N(0, 1) / 4, rounded likewise - so that dgamma, dbeta and the gamma factor of dx are exercised (the default 1 / 0 hides
    them).  The module must have been built under torch.manual_seed(seed)."""
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(round64(m.weight))
                m.bias.copy_(round64(m.bias))
            elif isinstance(m, torch.nn.GroupNorm):
                m.weight.copy_(round64(1 + torch.randn(m.weight.shape, generator=g) / 4))
                m.bias.copy_(round64(torch.randn(m.bias.shape, generator=g) / 4))
    return module


def case_input(name, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    return round64(torch.randn(*CASES[name][2], generator=g))


def grads_ref(name, state, x, dtype, fmt=None):
    """(output, {parameter name / "input": gradient}) of sum <output, weight_pattern> through the restatement."""
    from unet_dis_ref import weight_pattern
    st = {}
    for k, v in state.items():
        v = v.detach().clone().to(dtype)
        if fmt is not None and v.dim() == 4:
            v = v.contiguous(memory_format=fmt)
        st[k] = v.requires_grad_(True)
    xin = x.detach().clone().to(dtype)
    if fmt is not None:
        xin = xin.contiguous(memory_format=fmt)
    xin.requires_grad_(True)
    out = case_ref(name, xin, st)
    (out * weight_pattern(out.shape, dtype)).sum().backward()
    grads = {k: v.grad for k, v in st.items()}
    grads["input"] = xin.grad
    return out.detach(), grads
