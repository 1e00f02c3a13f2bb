"""PatchGAN discriminator of the second training step (reference: networks/discriminator.py:18-87) on the HIP kernels.

Same constructor, `self.main` Sequential layout and state_dict keys (`main.0.weight`, `main.3.running_mean`, ...) and the
reference's `weights_init` (:9-15).  Convolutions are 4x4, padding 1, stride 2 (last two: stride 1); BatchNorm2d +
LeakyReLU(0.2) run as one kernel, the first layer's LeakyReLU in the conv epilogue.  normalization='actnorm' puts
networks.actnorm.ActNorm (+ LeakyReLU, one kernel) in BatchNorm's place and gives the neighbouring convolutions a bias.

Spectral normalisation (utils.apply_spectral_norm, the reference's config.model.dis.apply_spectral_norm) is installed per
SConv2d by `install_spectral_norm`: parameter `weight_orig`, buffers `weight_u`, `weight_v` and no parameter `weight`, the
state_dict layout of torch.nn.utils.spectral_norm.  The discriminator's forward normalises the weights of all its
convolutions in one multi-layer call (ops.spectral_norm_weights) before the first convolution runs.
"""
import torch
import torch.nn as nn

from hipops import ops

from .actnorm import ActNorm


class SConv2d(nn.Conv2d):
    """nn.Conv2d holder (weight kept channels_last = OHWI) evaluated by the strided direct-conv kernels."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)

    spectral_eps = None               # set by install_spectral_norm

    def forward(self, x, slope=1.0, weight=None):
        """weight: this forward's spectrally normalised weight when the caller computed it with other layers'."""
        if weight is None:
            weight = self.weight if self.spectral_eps is None else \
                ops.spectral_norm_weight(self.weight_orig, self.weight_u, self.weight_v, self.training, self.spectral_eps)
        return ops.sconv2d(x, weight, self.bias, self.stride[0], self.padding[0], slope)


def install_spectral_norm(m, eps=1e-12):
    """torch.nn.utils.spectral_norm(m) with its defaults (name='weight', n_power_iterations=1, dim=0) for an SConv2d:
    `weight` becomes `weight_orig`; `weight_u` (Cout) and `weight_v` (Cin * k * k, in the logical (Cin, k, k) order) start as
    normalised standard-normal draws with no warm-up iteration.  The arithmetic of a forward is ops.spectral_norm_weight."""
    if not isinstance(m, SConv2d):
        raise NotImplementedError("spectral normalisation is built for networks.discriminator.SConv2d only (got %s)"
                                  % m.__class__.__name__)
    if m.spectral_eps is not None:
        raise RuntimeError("Cannot register two spectral_norm hooks on the same parameter weight")
    w = m.weight
    del m._parameters['weight']
    m.register_parameter('weight_orig', w)
    with torch.no_grad():
        u = nn.functional.normalize(w.new_empty(w.shape[0]).normal_(0, 1), dim=0, eps=eps)
        v = nn.functional.normalize(w.new_empty(w[0].numel()).normal_(0, 1), dim=0, eps=eps)
    m.register_buffer('weight_u', u)
    m.register_buffer('weight_v', v)
    m.spectral_eps = float(eps)
    return m


class FusedLeakyReLU(nn.Identity):
    """Placeholder keeping the reference's Sequential indices: the activation is fused into the previous kernel."""

    def __init__(self, negative_slope=0.2, inplace=True):
        super().__init__()
        self.negative_slope = negative_slope


def weights_init(m):
    classname = m.__class__.__name__
    if classname.find('Conv') != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find('BatchNorm') != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class NLayerDiscriminator(nn.Module):
    def __init__(self, in_channels=1, out_channels=1, n_filters=64, n_layers=3, normalization='batchnorm'):
        super().__init__()
        assert normalization in {'instancenorm', 'batchnorm', 'actnorm'}
        if normalization == 'instancenorm':
            raise NotImplementedError("normalization='instancenorm' is not built ('batchnorm' and 'actnorm' are)")
        norm_layer = nn.BatchNorm2d if normalization == 'batchnorm' else ActNorm
        use_bias = norm_layer is not nn.BatchNorm2d      # BatchNorm2d has affine parameters (reference :49-52)
        kw, padw = 4, 1
        sequence = [SConv2d(in_channels, n_filters, kw, stride=2, padding=padw), FusedLeakyReLU(0.2)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev, nf_mult = nf_mult, min(2 ** n, 8)
            sequence += [SConv2d(n_filters * nf_mult_prev, n_filters * nf_mult, kw, stride=2, padding=padw, bias=use_bias),
                         norm_layer(n_filters * nf_mult), FusedLeakyReLU(0.2)]
        nf_mult_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        sequence += [SConv2d(n_filters * nf_mult_prev, n_filters * nf_mult, kw, stride=1, padding=padw, bias=use_bias),
                     norm_layer(n_filters * nf_mult), FusedLeakyReLU(0.2)]
        sequence += [SConv2d(n_filters * nf_mult, out_channels, kw, stride=1, padding=padw)]
        self.main = nn.Sequential(*sequence)
        self.apply(weights_init)
        for m in self.modules():              # init rewrote the conv weights: keep them channels_last
            if isinstance(m, SConv2d):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)

    def forward(self, input):
        x = input
        layers = list(self.main)
        sn = [m for m in layers if isinstance(m, SConv2d) and m.spectral_eps is not None]
        sn_weight = {}
        if sn:                                # all spectrally normalised weights of this forward in one multi-layer call
            ws = ops.spectral_norm_weights([m.weight_orig for m in sn], [m.weight_u for m in sn], [m.weight_v for m in sn],
                                           self.training, sn[0].spectral_eps)
            sn_weight = {id(m): w for m, w in zip(sn, ws)}
        i = 0
        while i < len(layers):
            m = layers[i]
            if isinstance(m, SConv2d):
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                if isinstance(nxt, FusedLeakyReLU):
                    x = m(x, slope=nxt.negative_slope, weight=sn_weight.get(id(m)))
                    i += 2
                    continue
                x = m(x, weight=sn_weight.get(id(m)))
            elif isinstance(m, ActNorm):
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                slope = nxt.negative_slope if isinstance(nxt, FusedLeakyReLU) else 1.0
                x = m(x, slope=slope)
                if slope != 1.0:
                    i += 2
                    continue
            elif isinstance(m, nn.BatchNorm2d):
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                slope = nxt.negative_slope if isinstance(nxt, FusedLeakyReLU) else 1.0
                x = ops.batch_norm_lrelu(x, m.weight, m.bias, m.running_mean, m.running_var, self.training,
                                         momentum=m.momentum, eps=m.eps, slope=slope,
                                         num_batches_tracked=m.num_batches_tracked if self.training else None)
                if slope != 1.0:
                    i += 2
                    continue
            i += 1
        return x
