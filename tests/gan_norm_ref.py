"""Plain-torch restatement (any dtype, meant for float64; autograd does the backward) of the discriminator configurations
of the second training step: the PatchGAN with BatchNorm or ActNorm, with or without spectral normalisation.

    ActNorm           y = scale * (x + loc); the first training-mode forward with initialized == 0 sets, per channel over
                      (N, H, W), loc = -mean and scale = 1 / (std + 1e-6) with the unbiased std, then initialized = 1
    spectral norm     W = weight_orig as a Cout x (Cin k k) matrix of the logical (O, I, H, W) tensor; training mode:
                      v <- normalize(W^T u), u <- normalize(W v), normalize(x) = x / max(|x|, eps), buffers updated in place
                      without gradient; sigma = u^T W v with u, v constants; weight = weight_orig / sigma
    discriminator     conv 4x4 / 2 pad 1 (in -> f), LeakyReLU 0.2; n_layers - 1 times conv 4x4 / 2 (-> f * min(2^n, 8)), norm,
                      LeakyReLU; conv 4x4 / 1, norm, LeakyReLU; conv 4x4 / 1 (-> out).  Convolutions next to a BatchNorm have no
                      bias.  `state` is a dict with the module's state_dict keys (main.N.*); buffers in it are updated in place.
"""
import torch
import torch.nn.functional as F


def actnorm_ref(x, state, pre, training):
    loc, scale, init = state[pre + "loc"], state[pre + "scale"], state[pre + "initialized"]
    if training and int(init) == 0:
        with torch.no_grad():
            flat = x.transpose(0, 1).reshape(x.shape[1], -1)
            loc.copy_(-flat.mean(1).view(1, -1, 1, 1))
            scale.copy_((1.0 / (flat.std(1, unbiased=True) + 1e-6)).view(1, -1, 1, 1))
            init.fill_(1)
    return scale * (x + loc)


def spectral_weight_ref(weight_orig, u, v, training, eps=1e-12):
    """-> weight_orig / sigma; u, v (1-d, v in the logical (Cin, k, k) order) are updated in place in training mode."""
    W = weight_orig.reshape(weight_orig.shape[0], -1)
    if training:
        with torch.no_grad():
            Wd = W.detach()
            t = Wd.t() @ u
            v.copy_(t / t.norm().clamp_min(eps))
            s = Wd @ v
            u.copy_(s / s.norm().clamp_min(eps))
    uc, vc = u.detach().clone(), v.detach().clone()
    sigma = torch.dot(uc, W @ vc)
    return weight_orig / sigma


def batchnorm_ref(x, state, pre, training, momentum=0.1, eps=1e-5):
    w, b, rm, rv = (state[pre + k] for k in ("weight", "bias", "running_mean", "running_var"))
    if not training:
        return (x - rm.view(1, -1, 1, 1)) / torch.sqrt(rv.view(1, -1, 1, 1) + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    mean = x.mean((0, 2, 3))
    var = x.var((0, 2, 3), unbiased=False)
    with torch.no_grad():
        n = x.numel() / x.shape[1]
        rm.mul_(1 - momentum).add_(momentum * mean)
        rv.mul_(1 - momentum).add_(momentum * var * n / (n - 1))
        if pre + "num_batches_tracked" in state:
            state[pre + "num_batches_tracked"].add_(1)
    return (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def layout(n_layers):
    """[(Sequential index of the conv, stride, index of its norm or None, LeakyReLU after it)]"""
    out, i = [(0, 2, None, True)], 2
    for _ in range(1, n_layers):
        out.append((i, 2, i + 1, True))
        i += 3
    out.append((i, 1, i + 1, True))
    out.append((i + 3, 1, None, False))
    return out


def discriminator_ref(x, state, n_layers, training, slope=0.2):
    """Forward of the PatchGAN over `state` (tensors of one dtype; parameters may require grad).  The configuration is read
    from the keys: `main.N.weight_orig` = spectral norm, `main.N.loc` = ActNorm, `main.N.running_mean` = BatchNorm."""
    for ci, stride, ni, act in layout(n_layers):
        pre = "main.%d." % ci
        if pre + "weight_orig" in state:
            w = spectral_weight_ref(state[pre + "weight_orig"], state[pre + "weight_u"], state[pre + "weight_v"], training)
        else:
            w = state[pre + "weight"]
        x = F.conv2d(x, w, state.get(pre + "bias"), stride=stride, padding=1)
        if ni is not None:
            npre = "main.%d." % ni
            x = actnorm_ref(x, state, npre, training) if npre + "loc" in state else batchnorm_ref(x, state, npre, training)
        if act:
            x = F.leaky_relu(x, slope)
    return x


def hinge_d_loss_ref(real, fake):
    return 0.5 * (F.relu(1.0 - real).mean() + F.relu(1.0 + fake).mean())


def adam_ref(params, grads, moments, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam update (no weight decay, no amsgrad) in place; moments: {name: [exp_avg, exp_avg_sq]}."""
    b1, b2 = betas
    for k, p in params.items():
        g = grads[k]
        m, v = moments[k]
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / (1 - b2 ** step) ** 0.5).add_(eps)
        p.data.addcdiv_(m, denom, value=-lr / (1 - b1 ** step))
