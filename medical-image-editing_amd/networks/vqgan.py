"""The VQGAN decoder's blocks on the MI355X HIP kernels.

Same classes, constructor signatures, module tree, state_dict keys and parameter-creation order as the reference's
networks/vqgan.py (Normalize :15-19, Upsample :22-37, ResnetBlock :61-122, AttnBlock :125-180, Decoder :284-380), so a seed
gives the reference's initial values and a reference checkpoint loads with strict=True.  The forward passes call hipops.ops:
GroupNorm(+swish) is one pass of its own (ops.group_norm), the attention is ops.self_attention (the HW x HW score matrix is
never materialised), the convolutions are ops.conv2d - Upsample's with up2x=True, so the up-sampled tensor is never written.

The reference's Encoder, Downsample (a stride-2 convolution behind an asymmetric pad) and VQGAN are in networks/vqgan_model.py.
"""
import torch.nn as nn

from hipops import ops
from .blocks import Conv2d


def nonlinearity(x):
    """swish, x * sigmoid(x) (vqgan.py:10-12).  The blocks below do not call it: they evaluate norm -> swish as one
    ops.group_norm(..., swish=True)."""
    return ops.swish(x)


def Normalize(in_channels):
    """nn.GroupNorm(32, in_channels, eps=1e-6, affine=True) as the parameter holder (keys `weight`, `bias`); evaluate it with
    normalize(module, x)."""
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


def normalize(norm, x, swish=False):
    return ops.group_norm(x, norm.weight, norm.bias, eps=norm.eps, swish=swish)


class Upsample(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if self.with_conv:
            self.conv = Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        if self.with_conv:
            return self.conv(x, up2x=True)              # nearest x2 folded into the convolution's loader
        raise NotImplementedError("Upsample(with_conv=False): a bare nearest up-sampling has no kernel here")


class ResnetBlock(nn.Module):
    def __init__(self, in_channels, out_channels=None, use_conv_shortcut=False, p_dropout=0.0):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = use_conv_shortcut

        self.norm1 = Normalize(in_channels)
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(p_dropout)
        self.conv2 = Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        h = normalize(self.norm1, x, swish=True)
        h = self.conv1(h)
        h = normalize(self.norm2, h, swish=True)
        h = self.dropout(h)                              # torch's own module; the identity at the reference's p_dropout = 0
        h = self.conv2(h)
        if self.in_channels != self.out_channels:
            x = self.conv_shortcut(x) if self.use_conv_shortcut else self.nin_shortcut(x)
        return ops.add(x, h)


class AttnBlock(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        h = normalize(self.norm, x)
        q, k, v = self.q(h), self.k(h), self.v(h)
        h = ops.self_attention(q, k, v, int(self.in_channels) ** (-0.5))
        return ops.add(x, self.proj_out(h))


class Decoder(nn.Module):
    def __init__(self, in_channels, mid_channels, out_channels, ch_multiplier, num_res_blocks, attn_resolutions, resolution,
                 p_dropout, resamp_with_conv):
        super().__init__()
        self.in_channels = in_channels
        self.mid_channels = mid_channels
        self.out_channels = out_channels
        self.num_resolutions = len(ch_multiplier)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution

        curr_res = resolution // 2 ** (self.num_resolutions - 1)
        block_in = mid_channels * ch_multiplier[-1]

        self.conv_in = Conv2d(in_channels, block_in, kernel_size=3, stride=1, padding=1)

        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, p_dropout=p_dropout)
        self.mid.attn_1 = AttnBlock(in_channels=block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, p_dropout=p_dropout)

        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_out = mid_channels * ch_multiplier[i_level]
            for _ in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, p_dropout=p_dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(AttnBlock(in_channels=block_in))
            up = nn.Module()
            up.block = block
            up.attn = attn
            if i_level != 0:
                up.upsample = Upsample(in_channels=block_in, with_conv=resamp_with_conv)
                curr_res = curr_res * 2
            self.up.insert(0, up)

        self.norm_out = Normalize(block_in)
        self.conv_out = Conv2d(block_in, out_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, z):
        h = self.conv_in(z)
        h = self.mid.block_1(h)
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h)
        for i_level in reversed(range(self.num_resolutions)):
            for i_block in range(self.num_res_blocks):
                h = self.up[i_level].block[i_block](h)
                if len(self.up[i_level].attn) > 0:
                    h = self.up[i_level].attn[i_block](h)
            if i_level != 0:
                h = self.up[i_level].upsample(h)
        h = normalize(self.norm_out, h, swish=True)
        return self.conv_out(h)
