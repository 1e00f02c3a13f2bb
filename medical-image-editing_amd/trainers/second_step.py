"""Second training step (generator + PatchGAN discriminator) of the VQ-W-Net: reference
trainers/single_window_trainer.py:434-488 (`_train_second_step_nl_dis`), optimisers per trainers/base.py:165-181.

The encoder is frozen (eval mode, no_grad); the decoder is trained on  w.recon * MSE(recon, image) + w.gen * (-mean(D(recon)))
(+ w.freq * FFL(recon, image) with a frequency_loss, + w.perceptual * VGGLoss(recon, image) with a perceptual_loss,
:453-467); then the discriminator on  w.dis * hinge_d_loss(D(image), D(recon.detach()))  for n_inner_loops.  `dec_optim` / `dis_optim`
(dicts lr / betas / weight_decay, the reference's config.dec_optim / config.dis_optim, base.py:171-181) override the shared
lr / betas / weight_decay per optimiser; use_recon_loss=False drops the reconstruction term (:448-451).
trainers.build_second_step_trainer builds one from a config.
"""
from collections import namedtuple

import torch

from hipops import ops, Adam
from networks.discriminator import NLayerDiscriminator
from functions.gan_loss import hinge_d_loss, generator_loss

GanLossWeights = namedtuple("GanLossWeights", "recon gen dis freq perceptual", defaults=(1.0, 1.0, 1.0, 0.0, 0.0))


class SecondStepTrainer:
    def __init__(self, encoder, decoder, dis=None, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999),
                 weight_decay=0.0, device="cuda", data_parallel=False, frequency_loss=None,
                 perceptual_loss=None, dec_optim=None, dis_optim=None, use_recon_loss=True):
        self.device = torch.device(device)
        from .first_step import StepThrottle
        self.throttle = StepThrottle(self.device)      # at most two steps enqueued ahead of the GPU
        self.encoder = encoder.to(self.device)
        self.decoder = decoder.to(self.device).train()
        self.dis = (dis if dis is not None else NLayerDiscriminator()).to(self.device).train()
        self.w = loss_weight if loss_weight is not None else GanLossWeights()
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
            from .data_parallel import GradientAllReducer
            self.dec_reducer = GradientAllReducer(list(reversed([p for p in self.decoder.parameters() if p.requires_grad])))
            self.dis_reducer = GradientAllReducer(list(reversed([p for p in self.dis.parameters() if p.requires_grad])))

    # -- what a run saves and restores (trainers/fit.py); `modules` / `optimizers` are in the reference's order
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
        """{'NMSE', 'SSIM', 'PSNR', 'Entropy'} of one batch through trainers.evaluation.Evaluator (eval mode, no gradients;
        training state untouched)."""
        from .evaluation import Evaluator
        return Evaluator(self.encoder, self.decoder, self.encoder.dict_size).test_step(batch)

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
        # The reference lets autograd fill the discriminator's parameter gradients in this pass and discards them
        # (dis_optim.zero_grad() below); they are not computed here.  Same decoder gradients, same update.
        dis_params = [p for p in self.dis.parameters() if p.requires_grad]
        for p in dis_params:
            p.requires_grad_(False)
        try:
            l_gen = generator_loss(self.dis(recon))
            terms, weights = ([l_recon, l_gen], [w.recon, w.gen]) if l_recon is not None else ([l_gen], [w.gen])
            if l_freq is not None:
                terms.append(l_freq)
                weights.append(w.freq)
            if l_percep is not None:
                terms.append(l_percep)
                weights.append(w.perceptual)
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
        l_dis_total = None
        for _ in range(self.n_inner_loops):
            l_real = self.dis(image.detach())
            l_fake = self.dis(recon.detach())
            l_dis = hinge_d_loss(l_real, l_fake)
            l_dis_total = ops.weighted_sum([l_dis], [w.dis])
            self.dis_optim.zero_grad()
            if self.dis_reducer is not None:
                self.dis_reducer.prepare()
            l_dis_total.backward()
            if self.dis_reducer is not None:
                self.dis_reducer.finish()
            self.dis_optim.step()
        self.throttle.end()
        out = dict(gen_total=l_gen_total, recon=l_recon, gen=l_gen, dis_total=l_dis_total, ids=ids, recon_image=recon)
        if l_recon is None:
            del out["recon"]
        if l_freq is not None:
            out["freq"] = l_freq
        if l_percep is not None:
            out["perceptual"] = l_percep
        return out
