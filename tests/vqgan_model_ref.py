"""Plain-torch restatement of the rest of the VQGAN (Downsample, Encoder, the EMA vector quantiser, VQGAN itself) on the blocks of
tests/vqgan_ref.py, evaluated from a state dict alone in any dtype: the float64 truth of tests/test_gpu_vqgan_model.py and the check
of tests/golden/vqgan_model_*.npz in tests/test_vqgan_model_host.py.

    Downsample  y[yo, xo] = bias + sum_{ky, kx < 3} w[ky, kx] x[2 yo + ky, 2 xo + kx], x zero beyond its bottom / right edge
    VQ          id = argmin_k |x - e_k|^2 per pixel, q = e_id (forward) with the gradient passed to x, commit = mean (x - q)^2;
                training: cluster_size <- m cluster_size + (1 - m) counts, embed_avg <- m embed_avg + (1 - m) sum_{id = k} x,
                embed_k <- embed_avg_k / (n (cluster_size_k + eps) / (n + K eps)), n = sum cluster_size
"""
import torch
import torch.nn.functional as F

import vqgan_ref as V

VQ_MOMENTUM = 0.99
VQ_EPS = 1e-5


def down2_ref(x, w, b=None):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def embed4(w):
    """The 3x3 kernel at [:, :, 1:, 1:] of a zero 4x4 kernel: conv(x, embed4(w), stride 2, padding 1) = down2_ref(x, w) for even H, W."""
    w4 = w.new_zeros(w.shape[0], w.shape[1], 4, 4)
    w4[:, :, 1:, 1:] = w
    return w4


def downsample_ref(x, st, pre):
    return down2_ref(x, st[pre + "conv.weight"], st[pre + "conv.bias"])


def encoder_ref(x, st, pre=""):
    """The encoder's forward from its state dict alone: levels, blocks per level and attention blocks are read off the keys."""
    h = V._conv(x, st, pre + "conv_in.", 1)
    levels = 1 + max(int(k[len(pre) + 5:].split(".")[0]) for k in st if k.startswith(pre + "down."))
    for lv in range(levels):
        b = 0
        while "%sdown.%d.block.%d.norm1.weight" % (pre, lv, b) in st:
            h = V.resnet_block_ref(h, st, "%sdown.%d.block.%d." % (pre, lv, b))
            if "%sdown.%d.attn.%d.norm.weight" % (pre, lv, b) in st:
                h = V.attn_block_ref(h, st, "%sdown.%d.attn.%d." % (pre, lv, b))
            b += 1
        if lv != levels - 1:
            h = downsample_ref(h, st, "%sdown.%d.downsample." % (pre, lv))
    h = V.resnet_block_ref(h, st, pre + "mid.block_1.")
    h = V.attn_block_ref(h, st, pre + "mid.attn_1.")
    h = V.resnet_block_ref(h, st, pre + "mid.block_2.")
    h = V.group_norm_ref(h, st[pre + "norm_out.weight"], st[pre + "norm_out.bias"], act=True)
    return V._conv(h, st, pre + "conv_out.", 1)


def vq_ref(x, st, pre, training):
    """-> (q with the straight-through gradient, commit, ids (B, H, W) of pixel (h, w), relative top-1 / top-2 distance gap
    (B, H, W), the three buffers after the step: they are returned, st is left alone)."""
    embed = st[pre + "embed"].detach()
    B, D, H, W = x.shape
    flat = x.detach().permute(0, 2, 3, 1).reshape(-1, D)
    d = ((flat[:, None, :] - embed[None]) ** 2).sum(-1)                      # (N, K)
    two = d.topk(2, dim=1, largest=False)
    ids = two.indices[:, 0]
    gap = (two.values[:, 1] - two.values[:, 0]) / two.values[:, 0]
    quant = embed[ids].reshape(B, H, W, D).permute(0, 3, 1, 2)
    commit = F.mse_loss(x, quant)
    q = quant + (x - x.detach())
    buf = {k: st[pre + k].detach().clone() for k in ("embed", "cluster_size", "embed_avg")}
    if training:
        K = embed.shape[0]
        counts = torch.bincount(ids, minlength=K).to(flat.dtype)
        esum = torch.zeros(K, D, dtype=flat.dtype).index_add_(0, ids, flat).t()
        buf["cluster_size"] = VQ_MOMENTUM * buf["cluster_size"] + (1 - VQ_MOMENTUM) * counts
        buf["embed_avg"] = VQ_MOMENTUM * buf["embed_avg"] + (1 - VQ_MOMENTUM) * esum
        n = buf["cluster_size"].sum()
        cs = n * (buf["cluster_size"] + VQ_EPS) / (n + K * VQ_EPS)
        buf["embed"] = buf["embed_avg"].t() / cs[:, None]
    return q, commit, ids.reshape(B, H, W), gap.reshape(B, H, W), buf


def vqgan_forward_ref(x, st, training=True):
    """-> dict(recon, commit, ids, gap, emb, buffers).  ids and gap come in the modules' layout: entry [b, i, j] belongs to pixel
    (h = j, w = i) - the reference flattens in (B, W, H) order and views the result as (b, h, w), vq_module.py:172-180."""
    z = encoder_ref(x, st, "encoder.")
    q, commit, ids, gap, buf = vq_ref(z, st, "vq.", training)
    recon = V.decoder_ref(q, st, "decoder.")
    return dict(recon=recon, commit=commit, ids=ids.transpose(1, 2), gap=gap.transpose(1, 2), emb=q, buffers=buf)


def generate_ref(ids, st):
    """VQGAN.generate_image_from_ids on ids in the modules' layout."""
    x = st["vq.embed"][ids]                                                  # (B, A, C, D)
    return V.decoder_ref(x.transpose(3, 1), st, "decoder.")


def codebook(seed, K=8, D=32):
    g = torch.Generator().manual_seed(seed + 3000)
    return V.round64(torch.randn(K, D, generator=g) / 4)


# the fixture cases of tests/golden/make_golden_vqgan_model.py: name -> (constructor name, positional arguments, input shape)
CASES = {
    "down64": ("Downsample", (64, True), (2, 64, 16, 16)),
    "encoder": ("Encoder", (1, 32, 32, (1, 2), 1, [16], 32, 0.0, True), (2, 1, 32, 32)),
    "vqgan": ("VQGAN", (1, 32, 1, 32, 8, (1, 2), (1, 2), 1, [16], [16], 32, 0.0, True, "torch"), (2, 1, 32, 32)),
}
SEEDS = {"down64": 76, "encoder": 77, "vqgan": 80}


def case_input(name, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    return V.round64(torch.randn(*CASES[name][2], generator=g))


def init_case_(module, name, seed):
    """vqgan_ref.init_case_ plus, for the VQGAN, the fixture's codebook: embed = codebook(seed), embed_avg = its transpose."""
    V.init_case_(module, seed)
    if name == "vqgan":
        with torch.no_grad():
            module.vq.embed.copy_(codebook(seed))
            module.vq.embed_avg.copy_(module.vq.embed.t())
    return module


def is_param(k):
    return not k.startswith("vq.")


def grads_ref(name, state, x, dtype, fmt=None):
    """(outputs dict, {parameter name / "input": gradient}) through the restatement.  Loss: sum <output, weight_pattern>, for the
    VQGAN sum <recon, weight_pattern> + commit_loss."""
    from unet_dis_ref import weight_pattern
    st = {}
    for k, v in state.items():
        v = v.detach().clone().to(dtype)
        if fmt is not None and v.dim() == 4:
            v = v.contiguous(memory_format=fmt)
        st[k] = v.requires_grad_(True) if is_param(k) else v
    xin = x.detach().clone().to(dtype)
    if fmt is not None:
        xin = xin.contiguous(memory_format=fmt)
    xin.requires_grad_(True)
    if name == "vqgan":
        res = vqgan_forward_ref(xin, st, training=True)
        out = res["recon"]
        loss = (out * weight_pattern(out.shape, dtype)).sum() + res["commit"]
    else:
        out = downsample_ref(xin, st, "") if name == "down64" else encoder_ref(xin, st)
        res = dict(out=out)
        loss = (out * weight_pattern(out.shape, dtype)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in st.items() if is_param(k)}
    grads["input"] = xin.grad
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in res.items()}, grads
