"""The VQGAN trained against the U-Net discriminator: reference trainers/vqgan_unet_dis.py:36-136 (`VQGAN_UNetDis_Trainer`, the
launcher's -v), optimisers per trainers/base.py:165-181.

Generator half: recon, l_commit, ids, _ = VQGAN(image) in train mode (the quantiser's EMA update runs once per step), then
    w.recon * MSE + w.freq * FFL + w.perceptual * P + w.commit * l_commit + w.gen * l_gen + w.unet_perceptual * l_unet_perceptual
in that order, with l_gen and l_unet_perceptual as in second_step_unet.py, and one Adam step of dec_optim over ALL parameters
of the VQGAN (the reference's `decoder` is the whole autoencoder).  Discriminator half, n_inner_loops times: exactly
UNetSecondStepTrainer's (D(image), D(recon.detach()), one CutMix rectangle and flip, D(cutmix_images), the three losses, one Adam
step of dis_optim).

The step body is SecondStepBase.training_step and the two halves are second_step_unet.UNetDisHalves: this file is the
generator (reconstruct) and the order of the generator total.  The reference also builds a U-Net encoder that this step never
uses; it is not built here, so `modules()` is {'decoder': vqgan, 'dis': dis} and a checkpoint's keys read
decoder.encoder.conv_in.weight, decoder.vq.embed, dis.* as a reference checkpoint's do.  The reference has no test step for this
trainer, and neither has this one.
"""
from collections import namedtuple

from networks.unet_discriminator import UNetDiscriminator
from networks.vqgan_model import VQGAN
from .second_step import SecondStepBase
from .second_step_unet import UNetDisHalves

VQGANLossWeights = namedtuple("VQGANLossWeights", "recon freq perceptual commit gen unet_perceptual dis cutmix consistency",
                              defaults=(1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0))


class VQGANUNetDisTrainer(UNetDisHalves, SecondStepBase):
    Weights = VQGANLossWeights

    def __init__(self, vqgan, dis, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999), weight_decay=0.0, device="cuda",
                 data_parallel=False, frequency_loss=None, perceptual_loss=None, dec_optim=None, dis_optim=None,
                 use_recon_loss=True, use_unet_perceptual_loss=False, cutmix_box=None):
        if not isinstance(vqgan, VQGAN):
            raise TypeError("VQGANUNetDisTrainer trains a networks.VQGAN")
        if not isinstance(dis, UNetDiscriminator):
            raise TypeError("VQGANUNetDisTrainer trains against a networks.UNetDiscriminator")
        # the generator is one module: `decoder`, as the reference names it; there is no frozen encoder.  dec_optim and the
        # gradient all-reduce run over all of its parameters; the quantiser's collectives are networks.vq.VQ's own.
        super().__init__(None, vqgan, dis, loss_weight, n_inner_loops, lr, betas, weight_decay, device, data_parallel,
                         frequency_loss, perceptual_loss, dec_optim, dis_optim, use_recon_loss)
        self.vqgan = self.decoder
        self.dict_size = self.vqgan.vq.dict_size
        self.use_unet_perceptual_loss = bool(use_unet_perceptual_loss)
        self.cutmix_box = cutmix_box

    def modules(self):
        return {"decoder": self.vqgan, "dis": self.dis}

    def reconstruct(self, image):
        recon, l_commit, ids, _ = self.vqgan(image)
        return recon, ids, [("commit", l_commit, self.w.commit)]

    def generator_terms(self, image, recon, shared):
        """recon, freq, perceptual, commit, gen, unet_perceptual: the reference's order (vqgan_unet_dis.py:70-75)"""
        l_gen, l_unet = self.generator_pass(image, recon)
        return [*shared, ("gen", l_gen, self.w.gen), ("unet_perceptual", l_unet, self.w.unet_perceptual)]
