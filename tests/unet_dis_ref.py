"""Plain-torch restatement (any dtype, meant for float64; autograd does the backward) of the U-Net discriminator, BigGAN's
spectral normalisation and the losses of the second training step that uses them.

    spectral norm     W = weight as a rows x K matrix of the logical tensor, u0 a (1, rows) buffer.  EVERY forward:
                      v = normalize(u0 W), u' = normalize(v W^T), sv = v W^T u'^T with u', v constants, weight / sv;
                      normalize(x) = x / max(|x|, eps).  Training mode stores u0 <- u', sv0 <- sv; eval stores nothing.
    down block i      h = conv2(relu(conv1(relu(x) if i > 0 else x))); out = avgpool2(h) + shortcut, shortcut =
                      avgpool2(conv_sc(x)) for i > 0 and conv_sc(avgpool2(x)) for i = 0
    up block          out = conv2(relu(conv1(up2x(relu(x))))) + conv_sc(up2x(x)), nearest up-sampling
    network (512)     7 down blocks, in -> ch * [1, 2, 4, 8, 8, 8, 16]; bottleneck = linear_middle(sum(relu(h), [2, 3])) after block
                      6; 7 up blocks, ch * [16, 16, 16, 16, 8, 4, 2] -> ch * [8, 8, 8, 4, 2, 1, 1], block 8 + k reading
                      cat(h, output of down block 5 - k); a plain 1x1 convolution -> 1 channel.  `linear` is never used.
                      -> (out, bottleneck, the 7 up-block outputs)
    losses            see dis_losses_ref / gen_loss_ref / unet_perceptual_ref
`state` is a dict with the module's state_dict keys; buffers in it are updated in place.
"""
import numpy as np
import torch
import torch.nn.functional as F


def sn_weight_ref(weight, u0, sv0, training, eps=1e-12):
    W = weight.reshape(weight.shape[0], -1)
    with torch.no_grad():
        Wd = W.detach()
        v = u0 @ Wd
        v = v / v.norm().clamp_min(eps)
        u = v @ Wd.t()
        u = u / u.norm().clamp_min(eps)
    sv = (v @ W.t() @ u.t()).squeeze()
    if training:
        with torch.no_grad():
            u0.copy_(u)
            sv0.copy_(sv.detach().reshape(1))
    return weight / sv


def _conv(x, state, pre, training, padding):
    w = sn_weight_ref(state[pre + "weight"], state[pre + "u0"], state[pre + "sv0"], training)
    return F.conv2d(x, w, state[pre + "bias"], padding=padding)


def dblock_ref(x, state, pre, training, preactivation):
    h = F.relu(x) if preactivation else x
    h = _conv(h, state, pre + "conv1.", training, 1)
    h = _conv(F.relu(h), state, pre + "conv2.", training, 1)
    h = F.avg_pool2d(h, 2)
    if preactivation:
        s = F.avg_pool2d(_conv(x, state, pre + "conv_sc.", training, 0), 2)
    else:
        s = _conv(F.avg_pool2d(x, 2), state, pre + "conv_sc.", training, 0)
    return h + s


def gblock_ref(x, state, pre, training):
    h = F.interpolate(F.relu(x), scale_factor=2, mode="nearest")
    xu = F.interpolate(x, scale_factor=2, mode="nearest")
    h = _conv(h, state, pre + "conv1.", training, 1)
    h = _conv(F.relu(h), state, pre + "conv2.", training, 1)
    return h + _conv(xu, state, pre + "conv_sc.", training, 0)


def unet_discriminator_ref(x, state, training=True):
    """Forward over `state`.  The spectral-norm layers run in the module's order within a block (conv1, conv2, conv_sc): each
    layer has buffers of its own, so the order does not matter to the result."""
    h = x
    down = []
    for i in range(7):
        h = dblock_ref(h, state, "blocks.%d.0." % i, training, i > 0)
        if i < 6:
            down.append(h)
    w = sn_weight_ref(state["linear_middle.weight"], state["linear_middle.u0"], state["linear_middle.sv0"], training)
    bottleneck = F.linear(F.relu(h).sum((2, 3)), w, state["linear_middle.bias"])
    feats = []
    for j in range(7, 14):
        if j >= 8:
            h = torch.cat((h, down[13 - j]), dim=1)
        h = gblock_ref(h, state, "blocks.%d.0." % j, training)
        feats.append(h)
    out = F.conv2d(h, state["blocks.14.weight"], state["blocks.14.bias"])
    return out, bottleneck, feats


def cutmix_box_ref(height, width):
    """One rectangle from numpy's global generator: lam = beta(1, 1), then the centre (x = uniform(0, width), y = uniform(0,
    height)); both sides scaled by sqrt(1 - lam), clipped to the image, rounded half to even.  -> ((y0, y1), (x0, x1))"""
    lam = np.random.beta(1.0, 1.0)
    cx = np.random.uniform(0, width)
    cy = np.random.uniform(0, height)
    size = np.array([height, width], dtype=np.float64)
    half = size * np.sqrt(1 - lam) / 2
    centre = np.array([cy, cx])
    lo = np.rint(np.clip(centre - half, 0, None)).astype(int)
    hi = np.rint(np.minimum(centre + half, size)).astype(int)
    return (int(lo[0]), int(hi[0])), (int(lo[1]), int(hi[1]))


def cutmix_mask_ref(like, box, flip):
    """1 outside the rectangle, 0 inside; 1 - mask when flip."""
    (y0, y1), (x0, x1) = box
    mask = torch.ones_like(like)
    mask[:, :, y0:y1, x0:x1] = 0
    return 1 - mask if flip else mask


def cutmix_images_ref(image, recon, box, flip):
    mask = cutmix_mask_ref(image, box, flip)
    return image * mask + (1 - mask) * recon


def hinge_d_loss_ref(real, fake):
    return 0.5 * (F.relu(1.0 - real).mean() + F.relu(1.0 + fake).mean())


def dis_losses_ref(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, box, flip):
    """-> (l_dis, l_cutmix, l_consistency)"""
    mask = cutmix_mask_ref(r_map, box, flip)
    l_dis = hinge_d_loss_ref(r_map, f_map) + hinge_d_loss_ref(r_bottle, f_bottle)
    l_cutmix = F.relu(1.0 + c_bottle).mean() + F.relu(1.0 - (mask * 2 - 1) * c_map).mean()
    l_cons = F.mse_loss(c_map, r_map * mask + (1 - mask) * f_map)
    return l_dis, l_cutmix, l_cons


def gen_loss_ref(f_map, f_bottle):
    return -(f_map.mean() + f_bottle.mean())


def unet_perceptual_ref(f_feats, r_feats):
    return torch.stack([F.mse_loss(f, r.detach()) for f, r in zip(f_feats, r_feats)]).sum()


LOSS_NAMES = ("gen_total", "recon", "gen", "freq", "perceptual", "unet_perceptual", "dis_total", "dis", "cutmix", "consistency")


def weight_pattern(shape, dtype=torch.float64):
    """A closed-form cotangent for a tensor of `shape` (2-D or 4-D): cos(0.37 y + 0.91 x + 1.7 c + 0.3 n + 0.3), so that a
    fixture's backward needs no stored 512 x 512 weights."""
    idx = [torch.arange(n, dtype=torch.float64) for n in shape]
    if len(shape) == 4:
        n, c, y, x = idx
        ph = 0.3 * n[:, None, None, None] + 1.7 * c[None, :, None, None] + 0.37 * y[None, None, :, None] + 0.91 * x[None, None, None, :]
    else:
        n, c = idx
        ph = 0.3 * n[:, None] + 1.7 * c[None, :]
    return torch.cos(ph + 0.3).to(dtype)


def subset_index(size):
    """Whole below 64; from there every 8th index plus the two outermost on each side."""
    if size < 64:
        return torch.arange(size)
    return torch.tensor(sorted(set(range(0, size, 8)) | {0, 1, size - 2, size - 1}))


def subset(t):
    """The stored part of a (N, C, H, W) fixture tensor."""
    return t[:, :, subset_index(t.shape[2])][:, :, :, subset_index(t.shape[3])]
