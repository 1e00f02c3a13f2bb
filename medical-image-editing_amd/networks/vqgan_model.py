"""The VQGAN autoencoder on the MI355X HIP kernels: Downsample, Encoder and VQGAN itself, on the blocks of networks/vqgan.py.

Same classes, constructor signatures, module tree, state_dict keys and parameter-creation order as the reference's
networks/vqgan.py (Downsample :40-58, Encoder :183-281, VQGAN :383-446), so a seed gives the reference's initial values and a
reference checkpoint loads with strict=True.  Downsample's convolution - 3x3, stride 2, behind F.pad(x, (0, 1, 0, 1)) - is
ops.conv2d_down2 (the pad is index arithmetic in the kernel's loader, the padded tensor is never written); the quantiser is
networks.vq.VQ.
"""
import torch
import torch.nn as nn

from .blocks import Conv2d
from .vq import VQ
from .vqgan import AttnBlock, Decoder, Normalize, ResnetBlock, normalize


class Downsample(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if self.with_conv:
            self.conv = Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def forward(self, x):
        if self.with_conv:
            return self.conv(x)                          # ops.conv2d_down2: the bottom / right zero pad is in the loader
        raise NotImplementedError("Downsample(with_conv=False): the 2x2 average pooling has no kernel here")


class Encoder(nn.Module):
    def __init__(self, in_channels, mid_channels, out_channels, ch_multiplier, num_res_blocks, attn_resolutions, resolution,
                 p_dropout, resamp_with_conv):
        super().__init__()
        self.in_channels = in_channels
        self.mid_channels = mid_channels
        self.out_channels = out_channels
        self.num_resolutions = len(ch_multiplier)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution

        self.conv_in = Conv2d(in_channels, mid_channels, kernel_size=3, stride=1, padding=1)

        curr_res = resolution
        in_ch_multiplier = (1,) + tuple(ch_multiplier)
        self.down = nn.ModuleList()
        for i_level in range(self.num_resolutions):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_in = mid_channels * in_ch_multiplier[i_level]
            block_out = mid_channels * ch_multiplier[i_level]
            for _ in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, p_dropout=p_dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(AttnBlock(in_channels=block_in))
            down = nn.Module()
            down.block = block
            down.attn = attn
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(in_channels=block_in, with_conv=resamp_with_conv)
                curr_res = curr_res // 2
            self.down.append(down)

        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, p_dropout=p_dropout)
        self.mid.attn_1 = AttnBlock(in_channels=block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, p_dropout=p_dropout)

        self.norm_out = Normalize(block_in)
        self.conv_out = Conv2d(block_in, out_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        h = self.conv_in(x)
        for i_level in range(self.num_resolutions):
            for i_block in range(self.num_res_blocks):
                h = self.down[i_level].block[i_block](h)
                if len(self.down[i_level].attn) > 0:
                    h = self.down[i_level].attn[i_block](h)
            if i_level != self.num_resolutions - 1:
                h = self.down[i_level].downsample(h)
        h = self.mid.block_1(h)
        h = self.mid.attn_1(h)
        h = self.mid.block_2(h)
        h = normalize(self.norm_out, h, swish=True)
        return self.conv_out(h)


class VQGAN(nn.Module):
    def __init__(self, in_channels: int = 1, mid_channels: int = 32, out_channels: int = 9, emb_dim: int = 512,
                 dict_size: int = 64, enc_ch_multiplier: tuple = (1, 2, 4, 8, 16, 32), dec_ch_multiplier: tuple = (1, 1, 2, 4, 8, 16),
                 num_res_blocks: int = 2, enc_attn_resolutions: list = [], dec_attn_resolutions: list = [16],
                 resolution: int = 512, p_dropout: float = 0.0, resamp_with_conv: bool = True, knn_backend: str = 'torch'):
        super().__init__()
        self.encoder = Encoder(in_channels=in_channels, mid_channels=mid_channels, out_channels=emb_dim,
                               ch_multiplier=enc_ch_multiplier, num_res_blocks=num_res_blocks,
                               attn_resolutions=enc_attn_resolutions, resolution=resolution, p_dropout=p_dropout,
                               resamp_with_conv=resamp_with_conv)
        self.decoder = Decoder(in_channels=emb_dim, mid_channels=mid_channels, out_channels=out_channels,
                               ch_multiplier=dec_ch_multiplier, num_res_blocks=num_res_blocks,
                               attn_resolutions=dec_attn_resolutions, resolution=resolution, p_dropout=p_dropout,
                               resamp_with_conv=resamp_with_conv)
        self.vq = VQ(emb_dim=emb_dim, dict_size=dict_size, momentum=0.99, eps=1e-5, knn_backend=knn_backend)
        self.vq.torch_ema_weight = True                  # the codebook update follows torch's add_(update, alpha=1 - momentum)

    def forward(self, x):
        x = self.encoder(x)
        emb, commit_loss, ids = self.vq(x)
        recon = self.decoder(emb)
        return recon, commit_loss, ids, emb

    def generate_image_from_ids(self, ids):
        x = self.vq.lookup(ids)
        x = x.transpose(3, 1)                            # (B, A, C, D) -> (B, D, C, A): the reference's layout, vqgan.py:441-446
        return self.decoder(x)

    # ---- the code side: what the GPT prior trains on and samples into (trainers/prior.py).  Raster order - row-major over the
    # latent's h, then w, the order taming-transformers trains its prior in - while VQ.forward's ids and generate_image_from_ids
    # use the reference's transposed (B, W, H) view; the two methods below are the only place that converts.
    @staticmethod
    def raster_from_vq_ids(ids):
        """VQ.forward's ids (B, W, H) -> (B, h * w) in raster order: out[b, r * w + c] is the code of latent pixel (r, c)."""
        return ids.transpose(1, 2).reshape(ids.shape[0], -1)

    @staticmethod
    def vq_ids_from_raster(seq, h, w):
        """(B, h * w) in raster order -> the (B, W, H) view generate_image_from_ids takes."""
        if seq.dim() != 2 or seq.shape[1] != h * w:
            raise ValueError("decode_from_ids: seq of shape (B, h * w) = (B, %d) expected, got %s" % (h * w, tuple(seq.shape)))
        return seq.reshape(seq.shape[0], h, w).transpose(1, 2)

    def _eval_only(self):
        if self.training:
            raise RuntimeError("encode_to_ids: eval mode only")

    @torch.no_grad()
    def encode_to_ids(self, x):
        """x (B, C, H, W) -> (B, h * w) torch.long, the codes of the latent in raster order.  Eval mode only (no EMA update of the
        codebook), no gradients."""
        self._eval_only()
        _, _, ids = self.vq(self.encoder(x))
        return self.raster_from_vq_ids(ids).contiguous()

    @torch.no_grad()
    def decode_from_ids(self, seq, h, w):
        """seq (B, h * w) torch.long in raster order -> the decoder's picture of those codes.  Eval mode only, no gradients."""
        self._eval_only()
        return self.generate_image_from_ids(self.vq_ids_from_raster(seq, h, w))
