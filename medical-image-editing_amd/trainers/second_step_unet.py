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

from hipops import ops, Adam
from networks.unet_discriminator import UNetDiscriminator

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


class UNetSecondStepTrainer:
    def __init__(self, encoder, decoder, dis, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999), weight_decay=0.0,
                 device="cuda", data_parallel=False, frequency_loss=None, perceptual_loss=None, dec_optim=None, dis_optim=None,
                 use_recon_loss=True, use_unet_perceptual_loss=False, use_l1_loss=False, cutmix_box=None):
        if use_l1_loss:
            raise NotImplementedError("loss.use_l1_loss: the L1 reconstruction loss is not built (MSE is)")
        if not isinstance(dis, UNetDiscriminator):
            raise TypeError("UNetSecondStepTrainer trains a networks.UNetDiscriminator (SecondStepTrainer the PatchGAN)")
        self.device = torch.device(device)
        from .first_step import StepThrottle
        self.throttle = StepThrottle(self.device)      # at most two steps enqueued ahead of the GPU
        self.encoder = encoder.to(self.device)
        self.decoder = decoder.to(self.device).train()
        self.dis = dis.to(self.device).train()
        self.w = loss_weight if loss_weight is not None else UNetGanLossWeights()
        self.n_inner_loops = int(n_inner_loops)
        self.frequency_loss = frequency_loss
        self.perceptual_loss = perceptual_loss.to(self.device) if perceptual_loss is not None else None
        self.use_recon_loss = bool(use_recon_loss)
        self.use_unet_perceptual_loss = bool(use_unet_perceptual_loss)
        self.cutmix_box = cutmix_box
        shared = dict(lr=lr, betas=betas, weight_decay=weight_decay)
        self.dec_optim = Adam([p for p in self.decoder.parameters() if p.requires_grad], **(dec_optim or shared))
        self.dis_optim = Adam([p for p in self.dis.parameters() if p.requires_grad], **(dis_optim or shared))
        self.dec_reducer = self.dis_reducer = None
        if data_parallel:
            from .data_parallel import GradientAllReducer
            unused = {id(p) for p in self.dis.linear.parameters()}       # `linear` is never used: it never has a gradient
            self.dec_reducer = GradientAllReducer(list(reversed([p for p in self.decoder.parameters() if p.requires_grad])))
            self.dis_reducer = GradientAllReducer(list(reversed([p for p in self.dis.parameters()
                                                                 if p.requires_grad and id(p) not in unused])))

    def modules(self):
        return {"encoder": self.encoder, "decoder": self.decoder, "dis": self.dis}

    def optimizers(self):
        return {"dec": self.dec_optim, "dis": self.dis_optim}

    def state_dict(self):
        from .first_step import trainer_state_dict
        return trainer_state_dict(self)

    def load_state_dict(self, state):
        from .first_step import load_trainer_state_dict
        load_trainer_state_dict(self, state)

    def test_step(self, batch):
        from .evaluation import Evaluator
        return Evaluator(self.encoder, self.decoder, self.encoder.dict_size).test_step(batch)

    def _draw_box(self, H, W):
        if self.cutmix_box is not None:
            return self.cutmix_box() if callable(self.cutmix_box) else self.cutmix_box
        return draw_cutmix_box(H, W), random.random() > 0.5

    def discriminator_update(self, image, recon):
        """One inner loop of the discriminator half (single_window_trainer.py:319-357): D(image), D(recon), one CutMix draw,
        D(cutmix_images), the three losses, one Adam step.  -> (l_dis_total, l_dis, l_cutmix, l_consistency)"""
        w = self.w
        r_map, r_bottle, _ = self.dis(image.detach())
        f_map, f_bottle, _ = self.dis(recon.detach())
        box, flip = self._draw_box(image.shape[2], image.shape[3])
        cutmix_images = ops.cutmix_select(image, recon, box, flip)
        c_map, c_bottle, _ = self.dis(cutmix_images)
        l_dis, l_cutmix, l_cons = ops.unet_dis_losses(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, box, flip)
        l_dis_total = ops.weighted_sum([l_dis, l_cutmix, l_cons], [w.dis, w.cutmix, w.consistency])
        self.dis_optim.zero_grad()
        if self.dis_reducer is not None:
            self.dis_reducer.prepare()
        l_dis_total.backward()
        if self.dis_reducer is not None:
            self.dis_reducer.finish()
        self.dis_optim.step()
        return l_dis_total, l_dis, l_cutmix, l_cons

    def training_step(self, batch):
        image = batch['image'] if isinstance(batch, dict) else batch
        w = self.w
        self.throttle.begin()
        ops.begin_step()
        if self.dec_reducer is not None:
            ops.reset_pending(self.dec_optim.param_groups[0]["params"])
        self.encoder.eval()
        with torch.no_grad():
            embed, _, ids = self.encoder(image)
        recon = self.decoder(embed.detach())
        l_recon = ops.mse_loss(recon, image) if self.use_recon_loss else None
        l_freq = self.frequency_loss(recon, image) if self.frequency_loss is not None else None
        l_percep = self.perceptual_loss(recon, image) if self.perceptual_loss is not None else None
        # the discriminator's parameter gradients of this pass are discarded by the reference (dis_optim.zero_grad() below):
        # they are not computed; its buffers advance as in the reference
        dis_params = [p for p in self.dis.parameters() if p.requires_grad]
        for p in dis_params:
            p.requires_grad_(False)
        try:
            f_map, f_bottle, f_feat = self.dis(recon)
            l_gen = ops.weighted_sum([ops.neg_mean(f_map), ops.neg_mean(f_bottle)], [1.0, 1.0])
            l_unet = None
            if self.use_unet_perceptual_loss:
                with torch.no_grad():
                    _, _, r_feat = self.dis(image.detach())
                l_unet = ops.weighted_sum([ops.mse_loss(f, r) for f, r in zip(f_feat, r_feat)], [1.0] * len(f_feat))
            terms, weights = [l_gen], [w.gen]
            for t, wt in ((l_recon, w.recon), (l_freq, w.freq), (l_percep, w.perceptual), (l_unet, w.unet_perceptual)):
                if t is not None:
                    terms.append(t)
                    weights.append(wt)
            l_gen_total = ops.weighted_sum(terms, weights)
            self.dec_optim.zero_grad()
            if self.dec_reducer is not None:
                self.dec_reducer.prepare()
            l_gen_total.backward()
        finally:
            for p in dis_params:
                p.requires_grad_(True)
        ops.join_streams()
        if self.dec_reducer is not None:
            self.dec_reducer.finish()
        self.dec_optim.step()
        l_dis_total = l_dis = l_cutmix = l_cons = None
        for _ in range(self.n_inner_loops):
            l_dis_total, l_dis, l_cutmix, l_cons = self.discriminator_update(image, recon)
        self.throttle.end()
        out = dict(gen_total=l_gen_total, recon=l_recon, gen=l_gen, freq=l_freq, perceptual=l_percep, unet_perceptual=l_unet,
                   dis_total=l_dis_total, dis=l_dis, cutmix=l_cutmix, consistency=l_cons, ids=ids, recon_image=recon)
        return {k: v for k, v in out.items() if v is not None}
