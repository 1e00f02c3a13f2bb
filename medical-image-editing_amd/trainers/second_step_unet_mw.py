"""Multi-window second training step with the U-Net discriminator: reference trainers/multi_window_trainer.py:208-321
(`_train_second_step`, the launcher's -w with training_mode second_step).

The decoder and the discriminator are trained on three views of every slice, in this order: the full dataset window (the
image as it is), the lung window and the mediastinal window.  `ops.window_stack` makes the three views of the reconstruction
(with a tape: one gradient back into the decoder's output, from one kernel) and of the image (without) once per step; both
halves use them.

Generator half, per window i in order: D(recons[i]) with a tape, then, with use_unet_perceptual_loss, D(images[i]) without
one - every forward advances every u0, so the order is part of the result.
    l_gen = mean_i -(mean f_map_i + mean f_bottle_i),   l_unet_perceptual = mean_i sum_feat mse,
    recon / freq / perceptual = mean_i recon_weights[i] * MSE_i, freq_weights[i] * FFL_i, percep_weights[i] * percep_i
(trainers.window_terms, as the first step assembles them).  Discriminator half, n_inner_loops times (the reference ignores
n_inner_loops; 1 is its behaviour), per window i in order: D(images[i]), D(recons[i]), one CutMix rectangle and flip,
D(cutmix_images), the three losses; the means over the windows of the three loss kinds, then ONE backward and one Adam step.
Every mean over windows is ops.weighted_sum with the weights w_i / 3.

clamp_windows: True re-windows with the clamp of ops.window_map, the convention this project's multi-window first step trains
the decoder under; False is the reference trainer's literal arithmetic - its to_lung / to_mediastinal call `t_normalize`
(utils/__init__.py:30-40), whose clamp is commented out, so the reference re-windows by a pure affine map.
"""
from hipops import ops
from . import window_terms
from .second_step_unet import UNetSecondStepTrainer


def _window_mean(terms):
    """mean over the windows of 0-dim terms; None when there are none"""
    return ops.weighted_sum(terms, [1.0 / len(terms)] * len(terms)) if terms else None


def _weighted(pairs):
    """[(term, weight)] -> their weighted sum; None when there are none"""
    return ops.weighted_sum([t for t, _ in pairs], [c for _, c in pairs]) if pairs else None


class UNetMultiWindowSecondStepTrainer(UNetSecondStepTrainer):
    def __init__(self, encoder, decoder, dis, loss_weight=None, n_inner_loops=1, lr=1e-4, betas=(0.5, 0.999), weight_decay=0.0,
                 device="cuda", data_parallel=False, frequency_loss=None, perceptual_loss=None, dec_optim=None, dis_optim=None,
                 use_recon_loss=True, use_unet_perceptual_loss=False, use_l1_loss=False, cutmix_box=None, multi_window=None,
                 freq_weights=None, percep_weights=None, clamp_windows=True):
        if multi_window is None or len(tuple(multi_window["recon_weights"])) != 3:
            raise ValueError("UNetMultiWindowSecondStepTrainer needs multi_window=dict(dataset_window=(width, center, scale), "
                             "recon_weights=(w_full, w_lung, w_mediastinal))")
        if frequency_loss is not None and freq_weights is None:
            raise ValueError("multi-window training with the frequency loss needs freq_weights (config.loss.freq_weights)")
        if perceptual_loss is not None and percep_weights is None:
            raise ValueError("multi-window training with the perceptual loss needs percep_weights (config.loss.percep_weights)")
        super().__init__(encoder, decoder, dis, loss_weight, n_inner_loops, lr, betas, weight_decay, device, data_parallel,
                         frequency_loss, perceptual_loss, dec_optim, dis_optim, use_recon_loss, use_unet_perceptual_loss,
                         use_l1_loss, cutmix_box)
        self.multi_window = dict(dataset_window=tuple(multi_window["dataset_window"]),
                                 recon_weights=tuple(multi_window["recon_weights"]))
        self.freq_weights = tuple(freq_weights) if freq_weights is not None else None
        self.percep_weights = tuple(percep_weights) if percep_weights is not None else None
        self.clamp_windows = bool(clamp_windows)
        self.windows = window_terms.window_maps(self.multi_window["dataset_window"], clamp=self.clamp_windows)

    def shared_terms(self, image, recon):
        w, mw, clamp = self.w, self.multi_window, self.clamp_windows
        rec = window_terms.recon_terms(recon, image, mw, 1.0, clamp) if self.use_recon_loss else []
        frq = window_terms.freq_terms(self.frequency_loss, recon, image, mw, self.freq_weights, 1.0, clamp)
        pcp = window_terms.percep_terms(self.perceptual_loss, recon, image, mw, self.percep_weights, 1.0, clamp)
        return [("recon", _weighted(rec), w.recon), ("freq", _weighted(frq), w.freq), ("perceptual", _weighted(pcp), w.perceptual)]

    def discriminator_inputs(self, image, recon):
        return ops.window_stack(image.detach(), self.windows), ops.window_stack(recon, self.windows)

    def generator_terms(self, images, recons, shared):
        passes = [self.generator_pass(image, recon) for image, recon in zip(images, recons)]
        l_gen = _window_mean([g for g, _ in passes])
        l_unet = _window_mean([u for _, u in passes if u is not None])
        return [("gen", l_gen, self.w.gen), *shared, ("unet_perceptual", l_unet, self.w.unet_perceptual)]

    def discriminator_update(self, images, recons):
        """One inner loop (multi_window_trainer.py:275-319): the three passes of every window, the window means of the three
        loss kinds, one Adam step.  -> (l_dis_total, l_dis, l_cutmix, l_consistency)"""
        passes = [self.discriminator_pass(image, recon) for image, recon in zip(images, recons)]
        return self.discriminator_step(*(_window_mean([p[k] for p in passes]) for k in range(3)))
