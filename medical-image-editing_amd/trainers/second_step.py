"""Second training step (generator + PatchGAN discriminator) of the VQ-W-Net: reference
trainers/single_window_trainer.py:434-488 (`_train_second_step_nl_dis`), optimisers per trainers/base.py:165-181.

The encoder is frozen (eval mode, no_grad); the decoder is trained on  w.recon * MSE(recon, image) + w.gen * (-mean(D(recon)))
(+ w.freq * FFL(recon, image) with a frequency_loss, + w.perceptual * VGGLoss(recon, image) with a perceptual_loss,
:453-467); then the discriminator on  w.dis * hinge_d_loss(D(image), D(recon.detach()))  for n_inner_loops.  `dec_optim` / `dis_optim`
(dicts lr / betas / weight_decay, the reference's config.dec_optim / config.dis_optim, base.py:171-181) override the shared
lr / betas / weight_decay per optimiser; use_recon_loss=False drops the reconstruction term (:448-451).
trainers.build_second_step_trainer builds one from a config.

SecondStepBase is the step itself; a discriminator's trainer (here the PatchGAN's, second_step_unet.py the U-Net's) adds what
depends on the discriminator: its generator terms, its update and its loss-weight namedtuple.
"""
from collections import namedtuple

import torch

from hipops import ops, Adam
from networks.discriminator import NLayerDiscriminator
from functions.gan_loss import hinge_d_loss, generator_loss
from . import data_parallel as dp
from .base import TrainerBase

GanLossWeights = namedtuple("GanLossWeights", "recon gen dis freq perceptual", defaults=(1.0, 1.0, 1.0, 0.0, 0.0))


class SecondStepBase(TrainerBase):
    """A subclass sets `Weights` (its loss-weight namedtuple) and `dis_keys` (the names of what discriminator_update returns)
    and supplies generator_terms() and discriminator_update(); a multi-window step also overrides shared_terms() and
    discriminator_inputs().  reconstruct() is the generator itself: the frozen encoder and the trained decoder here; a trainer
    whose generator is one module (the VQGAN's) passes encoder=None and overrides it.  training_step is the one step body of
    all of them."""

    def __init__(self, encoder, decoder, dis=None, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999),
                 weight_decay=0.0, device="cuda", data_parallel=False, frequency_loss=None,
                 perceptual_loss=None, dec_optim=None, dis_optim=None, use_recon_loss=True):
        super().__init__(device)
        if encoder is not None:
            self.encoder = encoder.to(self.device)
        self.decoder = decoder.to(self.device).train()
        self.dis = (dis if dis is not None else NLayerDiscriminator()).to(self.device).train()
        if encoder is not None:
            self.dict_size = encoder.dict_size
        self.w = loss_weight if loss_weight is not None else self.Weights()
        self.n_inner_loops = int(n_inner_loops)
        self.frequency_loss = frequency_loss          # functions.FocalFrequencyLoss or None (use_frequency_loss)
        # functions.VGGLoss or None (use_perceptual_loss); no trainable parameters, so nothing to all-reduce
        self.perceptual_loss = perceptual_loss.to(self.device) if perceptual_loss is not None else None
        self.use_recon_loss = bool(use_recon_loss)
        shared = dict(lr=lr, betas=betas, weight_decay=weight_decay)
        self.dec_optim = Adam([p for p in self.decoder.parameters() if p.requires_grad], **(dec_optim or shared))
        self.dis_optim = Adam([p for p in self.dis.parameters() if p.requires_grad], **(dis_optim or shared))
        # one process per GPU (run_vqwnet.py:112-121): bucketed gradient all-reduce per optimiser, overlapped with
        # the rest of its backward pass; BatchNorm statistics (StyledDenorm and the discriminator's) are synchronised
        # inside their kernels' host code when a process group is up
        self.dec_reducer = self.dis_reducer = None
        if data_parallel:
            self.dec_reducer = dp.GradientAllReducer(list(reversed([p for p in self.decoder.parameters() if p.requires_grad])))
            self.dis_reducer = dp.GradientAllReducer(list(reversed(self.reduced_dis_params())))

    # `modules` / `optimizers` are in the reference's order
    def modules(self):
        return {"encoder": self.encoder, "decoder": self.decoder, "dis": self.dis}

    def optimizers(self):
        return {"dec": self.dec_optim, "dis": self.dis_optim}

    def reduced_dis_params(self):
        """The discriminator's parameters whose gradients a data-parallel run all-reduces."""
        return [p for p in self.dis.parameters() if p.requires_grad]

    def reconstruct(self, image):
        """image -> (recon with the generator's tape, ids, [(name, term, weight)] further entries of the generator total that
        come out of the generator's own forward).  Here: the frozen encoder (eval mode, no tape), then the decoder."""
        self.encoder.eval()
        with torch.no_grad():
            embed, _, ids = self.encoder(image)
        return self.decoder(embed.detach()), ids, []

    def shared_terms(self, image, recon):
        """-> the ("recon", "freq", "perceptual") entries (name, term or None, weight) of the generator total: the terms that
        do not depend on the discriminator."""
        w = self.w
        return [("recon", ops.mse_loss(recon, image) if self.use_recon_loss else None, w.recon),
                ("freq", self.frequency_loss(recon, image) if self.frequency_loss is not None else None, w.freq),
                ("perceptual", self.perceptual_loss(recon, image) if self.perceptual_loss is not None else None, w.perceptual)]

    def discriminator_inputs(self, image, recon):
        """-> (image, recon) as generator_terms and discriminator_update get them, made once per step: the tensors
        themselves here, one view per window in a multi-window step."""
        return image, recon

    def generator_terms(self, image, recon, shared):
        """-> [(name, term or None, weight)] of the generator total in the order ops.weighted_sum adds them (the order is
        part of the total's bits), the discriminator's forward on `recon` included; `shared`: the (recon, freq, perceptual)
        entries, followed by reconstruct()'s own.  Runs with the discriminator's parameters frozen."""
        raise NotImplementedError

    def discriminator_update(self, image, recon):
        """One inner loop of the discriminator half, its Adam step included -> the tensors `dis_keys` names."""
        raise NotImplementedError

    def training_step(self, batch):
        image = batch['image'] if isinstance(batch, dict) else batch
        self.throttle.begin()
        ops.begin_step()
        if self.dec_reducer is not None:
            ops.reset_pending(self.dec_optim.param_groups[0]["params"])
        recon, ids, own = self.reconstruct(image)
        shared = self.shared_terms(image, recon) + own
        d_image, d_recon = self.discriminator_inputs(image, recon)
        # The reference lets autograd fill the discriminator's parameter gradients in this pass and discards them
        # (dis_optim.zero_grad() in the discriminator half); they are not computed here.  Same decoder gradients, same
        # update; the discriminator's buffers advance as in the reference.
        dis_params = [p for p in self.dis.parameters() if p.requires_grad]

        def thaw():
            for p in dis_params:
                p.requires_grad_(True)

        def thaw_and_join():
            thaw()
            ops.join_streams()

        for p in dis_params:
            p.requires_grad_(False)
        try:
            terms = [t for t in self.generator_terms(d_image, d_recon, shared) if t[1] is not None]
            l_gen_total = ops.weighted_sum([t for _, t, _ in terms], [c for _, _, c in terms])
            self.update(l_gen_total, [self.dec_optim], self.dec_reducer, thaw_and_join)
        finally:
            thaw()
        last = ()
        for _ in range(self.n_inner_loops):
            last = self.discriminator_update(d_image, d_recon)
        self.throttle.end()
        out = dict(gen_total=l_gen_total)
        out.update((name, t) for name, t, _ in terms)
        out.update(zip(self.dis_keys, last), ids=ids, recon_image=recon)
        return out


class SecondStepTrainer(SecondStepBase):
    Weights = GanLossWeights
    dis_keys = ("dis_total",)

    def generator_terms(self, image, recon, shared):
        l_recon, l_freq, l_percep = shared
        return [l_recon, ("gen", generator_loss(self.dis(recon)), self.w.gen), l_freq, l_percep]

    def discriminator_update(self, image, recon):
        """-> (l_dis_total,): hinge loss on D(image), D(recon), one Adam step (single_window_trainer.py:472-486)."""
        l_dis = hinge_d_loss(self.dis(image.detach()), self.dis(recon.detach()))
        l_dis_total = ops.weighted_sum([l_dis], [self.w.dis])
        self.update(l_dis_total, [self.dis_optim], self.dis_reducer)
        return (l_dis_total,)
