"""Second training step with the U-Net discriminator: reference trainers/single_window_trainer.py:264-432
(`_train_second_step_unet_dis`), optimisers per trainers/base.py:165-181.

The encoder is frozen (eval mode, no_grad).  Generator half: the decoder is trained on
    w.recon * MSE + w.freq * FFL + w.perceptual * VGG/LPIPS + w.gen * l_gen + w.unet_perceptual * l_unet_perceptual
with l_gen = -(mean(f_map) + mean(f_bottle)) on D(recon) and, with use_unet_perceptual_loss, the sum over the seven up-block
outputs of mse(D(recon) feature, D(image) feature) (base.py:284-288).  Discriminator half, n_inner_loops times: D(image),
D(recon), one CutMix rectangle, D(cutmix_images) and
    w.dis * l_dis + w.cutmix * l_cutmix + w.consistency * l_consistency                  (ops.unet_dis_losses, one kernel pass).
The discriminator stays in train mode throughout: every forward advances every u0 (BigGAN's spectral norm), also those of the
generator half, where its parameters are frozen and the D(image) pass runs without a tape.

The rectangle is `draw_cutmix_box(H, W)` (the draws of utils/__init__.py:192-205: np.random.beta, np.random.uniform twice) and the flip
`random() > 0.5`, drawn in the reference's order from the generators a run's state already saves; `cutmix_box` - a callable
-> (((y0, y1), (x0, x1)), flip) or one such fixed pair - overrides the draw.
"""
from collections import namedtuple
import random

import numpy as np
import torch

from hipops import ops
from networks.unet_discriminator import UNetDiscriminator
from .second_step import SecondStepBase

UNetGanLossWeights = namedtuple("UNetGanLossWeights", "recon gen dis freq perceptual unet_perceptual cutmix consistency",
                                defaults=(1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0))


def draw_cutmix_box(height, width):
    """One CutMix rectangle ((y0, y1), (x0, x1)) from numpy's global generator, drawn as the reference draws it
    (utils/__init__.py:192-205 with alpha = 1): lam ~ Beta(1, 1), then the centre's x ~ U(0, width) and y ~ U(0, height), in
    that order.  The rectangle covers the fraction 1 - lam of the area: each side is sqrt(1 - lam) of the image's, centred
    there, clipped to the image and rounded to pixels."""
    lam = np.random.beta(1.0, 1.0)
    centre = {"x": np.random.uniform(0, width), "y": np.random.uniform(0, height)}
    fraction = np.sqrt(1 - lam)

    def span(c, size):
        half = size * fraction / 2
        return int(np.round(max(c - half, 0))), int(np.round(min(c + half, size)))
    return span(centre["y"], height), span(centre["x"], width)


class UNetDisHalves:
    """What training against the U-Net discriminator adds to SecondStepBase, whatever the generator is: the generator pass on
    D(recon) (and D(image)), the three discriminator passes with their CutMix draw, the discriminator's update.  Mixed in in
    front of SecondStepBase by UNetSecondStepTrainer and VQGANUNetDisTrainer; it reads self.dis, self.w, self.dis_optim,
    self.dis_reducer, self.use_unet_perceptual_loss and self.cutmix_box."""
    dis_keys = ("dis_total", "dis", "cutmix", "consistency")

    def reduced_dis_params(self):
        unused = {id(p) for p in self.dis.linear.parameters()}       # `linear` is never used: it never has a gradient
        return [p for p in super().reduced_dis_params() if id(p) not in unused]

    def _draw_box(self, H, W):
        if self.cutmix_box is not None:
            return self.cutmix_box() if callable(self.cutmix_box) else self.cutmix_box
        return draw_cutmix_box(H, W), random.random() > 0.5

    def generator_pass(self, image, recon):
        """D(recon) with a tape, then, with use_unet_perceptual_loss, D(image) without one -> (l_gen, l_unet_perceptual or None)"""
        f_map, f_bottle, f_feat = self.dis(recon)
        l_gen = ops.weighted_sum([ops.neg_mean(f_map), ops.neg_mean(f_bottle)], [1.0, 1.0])
        l_unet = None
        if self.use_unet_perceptual_loss:
            with torch.no_grad():
                _, _, r_feat = self.dis(image.detach())
            l_unet = ops.weighted_sum([ops.mse_loss(f, r) for f, r in zip(f_feat, r_feat)], [1.0] * len(f_feat))
        return l_gen, l_unet

    def discriminator_pass(self, image, recon):
        """D(image), D(recon), one CutMix draw, D(cutmix_images) (single_window_trainer.py:319-349) -> (l_dis, l_cutmix, l_consistency)"""
        r_map, r_bottle, _ = self.dis(image.detach())
        f_map, f_bottle, _ = self.dis(recon.detach())
        box, flip = self._draw_box(image.shape[2], image.shape[3])
        cutmix_images = ops.cutmix_select(image, recon, box, flip)
        c_map, c_bottle, _ = self.dis(cutmix_images)
        return ops.unet_dis_losses(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, box, flip)

    def discriminator_step(self, l_dis, l_cutmix, l_cons):
        """The weighted total of the three losses and one Adam step -> (l_dis_total, l_dis, l_cutmix, l_consistency)"""
        w = self.w
        l_dis_total = ops.weighted_sum([l_dis, l_cutmix, l_cons], [w.dis, w.cutmix, w.consistency])
        self.update(l_dis_total, [self.dis_optim], self.dis_reducer)
        return l_dis_total, l_dis, l_cutmix, l_cons

    def discriminator_update(self, image, recon):
        """One inner loop of the discriminator half (single_window_trainer.py:319-357): the three passes and their losses, one
        Adam step.  -> (l_dis_total, l_dis, l_cutmix, l_consistency)"""
        return self.discriminator_step(*self.discriminator_pass(image, recon))


class UNetSecondStepTrainer(UNetDisHalves, SecondStepBase):
    Weights = UNetGanLossWeights

    def __init__(self, encoder, decoder, dis, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999), weight_decay=0.0,
                 device="cuda", data_parallel=False, frequency_loss=None, perceptual_loss=None, dec_optim=None, dis_optim=None,
                 use_recon_loss=True, use_unet_perceptual_loss=False, use_l1_loss=False, cutmix_box=None):
        if use_l1_loss:
            raise NotImplementedError("loss.use_l1_loss: the L1 reconstruction loss is not built (MSE is)")
        if not isinstance(dis, UNetDiscriminator):
            raise TypeError("UNetSecondStepTrainer trains a networks.UNetDiscriminator (SecondStepTrainer the PatchGAN)")
        super().__init__(encoder, decoder, dis, loss_weight, n_inner_loops, lr, betas, weight_decay, device, data_parallel,
                         frequency_loss, perceptual_loss, dec_optim, dis_optim, use_recon_loss)
        self.use_unet_perceptual_loss = bool(use_unet_perceptual_loss)
        self.cutmix_box = cutmix_box

    def generator_terms(self, image, recon, shared):
        l_gen, l_unet = self.generator_pass(image, recon)
        return [("gen", l_gen, self.w.gen), *shared, ("unet_perceptual", l_unet, self.w.unet_perceptual)]
