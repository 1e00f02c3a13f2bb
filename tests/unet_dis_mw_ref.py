"""Plain-torch restatement (any dtype, meant for float64) of the multi-window second training step with the U-Net
discriminator, over tests/unet_dis_ref.py: the three views of a slice (the full dataset window, the lung window, the
mediastinal window), the generator half's losses and the discriminator half's, each the mean over the windows.

    to_window(x)      hu = (x / s0 + 0.5) * (vmax0 - vmin0) + vmin0 (the dataset window back to CT values), then
                      ((clip(hu, vmin1, vmax1) - vmin1) / (vmax1 - vmin1) - 0.5) * s1 with clamp, the same without the clip
                      otherwise (the affine map the upstream trainers apply)
    generator half    per window i in order: D(recons[i]), then D(images[i]); recon = mean_i recon_weights[i] * mse_i,
                      gen = mean_i -(mean f_map + mean f_bottle), unet_perceptual = mean_i sum_feat mse
    discriminator     per window i in order: D(images[i]), D(recons[i]), D(cutmix_i) with the window's own rectangle and flip;
                      dis / cutmix / consistency = the means over the windows
Every forward advances every u0 of `state` (training mode), so the order above is part of the result.
"""
import torch
import torch.nn.functional as F

import unet_dis_ref as U

LUNG_WINDOW = (1500, -550, 2.0)
MEDIASTINAL_WINDOW = (400, 20, 2.0)


def to_window(x, dataset_window, target_window, clamp):
    w0, c0, s0 = dataset_window
    w1, c1, s1 = target_window
    vmax0, vmin0 = c0 + w0 // 2, c0 - w0 // 2
    vmax1, vmin1 = c1 + w1 // 2, c1 - w1 // 2
    hu = (x / s0 + 0.5) * (vmax0 - vmin0) + vmin0
    if clamp:
        hu = hu.clamp(vmin1, vmax1)
    return ((hu - vmin1) / (vmax1 - vmin1) - 0.5) * s1


def window_views(x, dataset_window, clamp):
    return [x, to_window(x, dataset_window, LUNG_WINDOW, clamp), to_window(x, dataset_window, MEDIASTINAL_WINDOW, clamp)]


def step_losses_ref(image, recon, state, boxes, flips, w, dataset_window, recon_weights, clamp):
    """The ten logged values (U.LOSS_NAMES order, un-weighted window means; freq and perceptual are 0: those losses are off)
    of one step on `image` and its reconstruction `recon`; `state` (the discriminator's, buffers advanced in place) is the
    one BEFORE the step: no optimiser runs here - the decoder's update does not touch `recon`, and the discriminator steps
    after its last forward.  boxes / flips: one rectangle and flip per window; w: the loss weights of the two totals."""
    with torch.no_grad():
        images = window_views(image, dataset_window, clamp)
        recons = window_views(recon, dataset_window, clamp)
        v = {k: [] for k in ("recon", "gen", "unet_perceptual", "dis", "cutmix", "consistency")}
        for i, (r, x) in enumerate(zip(recons, images)):
            v["recon"].append(recon_weights[i] * F.mse_loss(r, x))
            f_map, f_bottle, f_feat = U.unet_discriminator_ref(r, state, True)
            v["gen"].append(U.gen_loss_ref(f_map, f_bottle))
            v["unet_perceptual"].append(U.unet_perceptual_ref(f_feat, U.unet_discriminator_ref(x, state, True)[2]))
        for i, (r, x) in enumerate(zip(recons, images)):
            r_map, r_bottle, _ = U.unet_discriminator_ref(x, state, True)
            f_map, f_bottle, _ = U.unet_discriminator_ref(r, state, True)
            c_map, c_bottle, _ = U.unet_discriminator_ref(U.cutmix_images_ref(x, r, boxes[i], flips[i]), state, True)
            d, c, s = U.dis_losses_ref(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, boxes[i], flips[i])
            v["dis"].append(d), v["cutmix"].append(c), v["consistency"].append(s)
        v = {k: torch.stack(t).mean() for k, t in v.items()}
        v["gen_total"] = w["recon"] * v["recon"] + w["gen"] * v["gen"] + w["unet_perceptual"] * v["unet_perceptual"]
        v["dis_total"] = w["dis"] * v["dis"] + w["cutmix"] * v["cutmix"] + w["consistency"] * v["consistency"]
    zero = torch.zeros((), dtype=image.dtype)
    return torch.stack([v.get(k, zero).to(image.dtype) for k in U.LOSS_NAMES])
