"""U-Net discriminator of the second training step (reference: networks/unet_discriminator.py:386-627, `Unet_Discriminator`, with
the BigGAN blocks of networks/biggan/layers.py) on the HIP kernels.

Same constructor, module tree and state_dict keys in the same order (`blocks.0.0.conv1.{weight,bias,u0,sv0}`, ...,
`blocks.14.{weight,bias}`, `linear.*`, `linear_middle.*`), the same parameter-creation order (a seed gives the reference's
initial values) and `D_init='ortho'`.  Only the 512 architecture runs in the reference (its forward needs `output_features`,
which `__init__` sets for resolution 512 alone), so only that one is built: 7 DBlocks (AvgPool2d(2) each, block 0 without
pre-activation), 7 GBlock2s (nearest x2, learnable 1x1 shortcut, input = cat(h, residual) from the second on), a plain 1x1
output convolution and the bottleneck head `linear_middle(sum(relu(h), [2, 3]))` after block 6.  `linear` exists and is never
used, as in the reference.

How a forward runs:
  * the 43 spectrally normalised weights in use (`linear`, the 44th, is not) in one multi-layer call (BigGAN's SN: buffers u0 / sv0, every forward iterates,
    training stores);
  * 3x3 convolutions with the ReLU between conv1 and conv2 in conv1's epilogue; conv1 of an up block reads the rectified
    concat buffer as one up-sampled source (the collapsed form where the shape is served);
  * 1x1 shortcuts on the pooled (down) / low-resolution (up) input - they commute with the average pool and with nearest
    up-sampling - the up blocks' over the virtual concat (h | residual), never materialised;
  * block tails, head: csrc/unet_dis.hip (ops.unet_down_tail / unet_up_tail / unet_bottleneck_head).
Weights are kept channels_last (OHWI) like SConv2d's.
"""
import torch
import torch.nn as nn
from torch.nn import init

from hipops import ops


def D_unet_arch_512(in_channels, ch):
    """unet_discriminator.py:375-381"""
    return dict(in_channels=[in_channels] + [ch * k for k in [1, 2, 4, 8, 8, 8, 16, 8 * 2, 8 * 2, 8 * 2, 4 * 2, 2 * 2, 1 * 2]],
                out_channels=[ch * k for k in [1, 2, 4, 8, 8, 8, 16, 8, 8, 8, 4, 2, 1, 1]],
                downsample=[True] * 7 + [False] * 7,
                resolution=[256, 128, 64, 32, 16, 8, 4, 8, 16, 32, 64, 128, 256, 512])


class SNConv2d(nn.Conv2d):
    """biggan/layers.py:97-109: nn.Conv2d parameters, then the buffers u0 (1, Cout) ~ N(0, 1) and sv0 = 1."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, eps=1e-12):
        super().__init__(in_channels, out_channels, kernel_size, padding=padding)
        self.register_buffer('u0', torch.randn(1, out_channels))
        self.register_buffer('sv0', torch.ones(1))
        self.eps = eps


class SNLinear(nn.Linear):
    """biggan/layers.py:113-119"""

    def __init__(self, in_features, out_features, eps=1e-12):
        super().__init__(in_features, out_features)
        self.register_buffer('u0', torch.randn(1, out_features))
        self.register_buffer('sv0', torch.ones(1))
        self.eps = eps


class DBlock(nn.Module):
    """biggan/layers.py:461-506 (downsample = AvgPool2d(2)): parameter holder, evaluated by UNetDiscriminator.forward."""

    def __init__(self, in_channels, out_channels, wide=True, preactivation=False, eps=1e-12):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.hidden_channels = out_channels if wide else in_channels
        self.preactivation = preactivation
        self.conv1 = SNConv2d(in_channels, self.hidden_channels, eps=eps)
        self.conv2 = SNConv2d(self.hidden_channels, out_channels, eps=eps)
        self.conv_sc = SNConv2d(in_channels, out_channels, kernel_size=1, padding=0, eps=eps)


class GBlock2(nn.Module):
    """biggan/layers.py:416-457 (upsample = nearest x2, skip_connection=True): parameter holder."""

    def __init__(self, in_channels, out_channels, eps=1e-12):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv1 = SNConv2d(in_channels, out_channels, eps=eps)
        self.conv2 = SNConv2d(out_channels, out_channels, eps=eps)
        self.conv_sc = SNConv2d(in_channels, out_channels, kernel_size=1, padding=0, eps=eps)


def _channels_last_(module):
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)


def sn_weights(layers, training, eps=1e-12):
    """{id(layer): this forward's spectrally normalised weight} for SNConv2d / SNLinear layers, one multi-layer call."""
    ws = ops.spectral_norm_weights([m.weight for m in layers], [m.u0 for m in layers], None, training, eps,
                                   svs=[m.sv0 for m in layers], biggan=True)
    return {id(m): w for m, w in zip(layers, ws)}


def down_block(b, W, raw, rect):
    """DBlock.forward on (x, relu(x)) = (raw, rect) -> (out, relu(out)); rect is not read without pre-activation."""
    h = ops.conv2d(rect if b.preactivation else raw, W[id(b.conv1)], b.conv1.bias, relu=True)
    h = ops.conv2d(h, W[id(b.conv2)], b.conv2.bias)
    pooled, _ = ops.unet_down_tail(raw, want_relu=False)
    return ops.unet_down_tail(h, s_low=ops.conv2d(pooled, W[id(b.conv_sc)], b.conv_sc.bias))


def up_block(b, W, raw, rect, res, nxt, want_cat=True):
    """GBlock2.forward on x = cat(raw, res) (res may be None) with rect = relu(x) as one tensor -> (out, [relu(out) | relu(nxt)]):
    the second is the next up block's `rect` for its input cat(out, nxt)."""
    h = ops.conv2d(rect, W[id(b.conv1)], b.conv1.bias, up2x=True, relu=True)
    h = ops.conv2d(h, W[id(b.conv2)], b.conv2.bias)
    s = ops.conv2d(raw, W[id(b.conv_sc)], b.conv_sc.bias, skip=res)
    return ops.unet_up_tail(h, s, res=nxt, want_cat=want_cat)


class UNetDiscriminator(nn.Module):
    def __init__(self, in_channels=9, D_ch=64, D_wide=True, resolution=128, D_kernel_size=3, D_attn='64', n_classes=1000,
                 num_D_SVs=1, num_D_SV_itrs=1, D_activation=None, D_lr=2e-4, D_B1=0.0, D_B2=0.999, adam_eps=1e-8,
                 SN_eps=1e-12, output_dim=1, D_mixed_precision=False, D_fp16=False, D_init='ortho', skip_init=False,
                 D_param='SN', decoder_skip_connection=True, unconditional=True, **kwargs):
        super().__init__()
        if resolution != 512:
            raise NotImplementedError("UNetDiscriminator: resolution %r is not built - only the 512 arch runs in the reference "
                                      "(its forward raises AttributeError for 128 and 256)" % (resolution,))
        attn = [int(a) for a in str(D_attn).split('_')]
        if any(a in (256, 128, 64, 32, 16) for a in attn):
            raise NotImplementedError("UNetDiscriminator: D_attn=%r would place an Attention layer, which is not built" % (D_attn,))
        if not unconditional:
            raise NotImplementedError("UNetDiscriminator: the class-conditional projection (unconditional=False) is not built")
        if D_param != 'SN' or num_D_SVs != 1 or num_D_SV_itrs != 1 or D_kernel_size != 3 or output_dim != 1 or D_fp16 \
                or D_mixed_precision:
            raise NotImplementedError("UNetDiscriminator: only D_param='SN' with one singular value and one power iteration, "
                                      "3x3 kernels, output_dim=1 and fp32 are built")
        if D_activation is not None and not isinstance(D_activation, nn.ReLU):
            raise NotImplementedError("UNetDiscriminator: only the ReLU activation is built")
        if D_init not in ('ortho', 'N02', 'glorot', 'xavier'):
            raise ValueError("UNetDiscriminator: unknown D_init %r" % (D_init,))
        self.ch, self.D_wide, self.resolution, self.attention, self.init, self.SN_eps = D_ch, D_wide, resolution, D_attn, D_init, SN_eps
        self.unconditional = True
        self.arch = D_unet_arch_512(in_channels, D_ch)
        blocks = []
        for i, (cin, cout, down) in enumerate(zip(self.arch['in_channels'], self.arch['out_channels'], self.arch['downsample'])):
            blocks.append(nn.ModuleList([DBlock(cin, cout, wide=D_wide, preactivation=i > 0, eps=SN_eps) if down
                                         else GBlock2(cin, cout, eps=SN_eps)]))
        self.blocks = nn.ModuleList(blocks)
        self.blocks.append(nn.Conv2d(D_ch, 1, kernel_size=1))
        self.linear = SNLinear(self.arch['out_channels'][-1], output_dim, eps=SN_eps)        # constructed, never used (as the reference)
        self.linear_middle = SNLinear(16 * D_ch, output_dim, eps=SN_eps)
        if not skip_init:
            self.init_weights()
        _channels_last_(self)

    def init_weights(self):
        """`D_init` on every convolution and linear weight, in module order (the order the reference draws them in)."""
        fill = {'ortho': init.orthogonal_, 'N02': lambda w: init.normal_(w, 0, 0.02), 'glorot': init.xavier_uniform_,
                'xavier': init.xavier_uniform_}[self.init]
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fill(m.weight)

    def sn_layers(self):
        """The spectrally normalised layers that a forward uses, in forward order (`linear` is not among them)."""
        ls = []
        for b in list(self.blocks)[:-1]:
            ls += [b[0].conv1, b[0].conv2, b[0].conv_sc]
        return ls + [self.linear_middle]

    def forward(self, x):
        sn = self.sn_layers()
        W = sn_weights(sn, self.training, self.SN_eps)
        raw, rect = x, None               # a block's input and its ReLU
        down = []                         # outputs of blocks 0..5: the residual features
        for i in range(7):
            raw, rect = down_block(self.blocks[i][0], W, raw, rect)
            if i < 6:
                down.append(raw)
        bottleneck_out = ops.unet_bottleneck_head(raw, W[id(self.linear_middle)], self.linear_middle.bias)
        features_out = []
        res = None                        # the residual feature concatenated to this block's input
        for j in range(7, 14):
            nxt = down[12 - j] if j < 13 else None
            raw, rect = up_block(self.blocks[j][0], W, raw, rect, res, nxt, want_cat=j < 13)
            res = nxt
            features_out.append(raw)
        last = self.blocks[-1]
        out = ops.conv2d(raw, last.weight, last.bias)
        return out.view(out.size(0), 1, self.resolution, self.resolution), bottleneck_out, features_out
