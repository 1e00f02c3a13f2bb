#!/usr/bin/env python3
"""Generate the golden vectors of the multi-window second training step with the U-Net discriminator from the upstream
reference's own modules: ONE step of trainers/multi_window_trainer.py `_train_second_step` (:208-321) restated around the
reference's UNetEncoder / UNetDecoder / Unet_Discriminator, its re-windowing arithmetic (utils.denormalize followed by
utils.t_normalize, which is what trainers/base.py imports as `normalize` for to_lung / to_mediastinal: a pure affine map, the
clamp is commented out upstream), hinge_d_loss, utils.cutmix and utils.mask_src_tgt.

Runs ONLY in the build container (needs the reference sources); the loading is make_golden_unet_dis.py's.  Output, tensors only:

    tests/golden/unet_dis_mw_step.npz        step/  image, box{i}, flip{i} (one rectangle and flip per window), loss (the ten
                                                    logged values, un-weighted window means, in LOSS_NAMES order), P.* (the
                                                    discriminator before), init_sum/* (encoder / decoder checksums), cfg/*,
                                                    spread.loss, spread.update_{dec,dis} (as make_golden_unet_dis.py)
    tests/golden/unet_dis_mw_step_after.npz  step/after.dis.*  the discriminator's state after the step
    tests/golden/unet_dis_mw_step_dec.npz    step/after.dec.*  the decoder's

512 x 512, batch 1, D_ch = 4, dataset window (2000, 0, 2.0), recon_weights (1.0, 0.5, 0.25), use_unet_perceptual_loss on, the
frequency and perceptual losses off (weights 0), Adam at lr 1e-6 for the reason make_golden_unet_dis.py documents.  The image's
pixels are multiples of 1/64 in [-1, 1]: none lies on a window bound (x = 0.2 for the lung window, -0.18 and 0.22 for the
mediastinal one), and at least 5 % of them lie outside each window's bounds (asserted), so whether a trainer clamps matters on
this image.  Storage (rounding, subsets, the 1 MiB limit) as in make_golden_unet_dis.py.

    python tests/golden/make_golden_unet_dis_mw.py
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_unet_dis import R, npy, save, spread, build, load_unet_discriminator, refutils  # noqa: E402
from unet_dis_ref import LOSS_NAMES  # noqa: E402

DATASET_WINDOW = dict(width=2000, center=0, scale=2.0)
WINDOWS = (None, dict(width=1500, center=-550, scale=2.0), dict(width=400, center=20, scale=2.0))     # trainers/base.py:33-43
STEP = dict(enc_filters=[4, 4, 8, 8, 16], dec_filters=[8, 8, 16, 16, 32], K=10, momentum=0.999, seed=66, dis_seed=67, lr=1e-6,
            betas=(0.5, 0.999), recon_weights=(1.0, 0.5, 0.25),
            boxes=[((100, 300), (64, 200)), ((0, 256), (300, 512)), ((200, 470), (10, 330))], flips=[False, True, False],
            w=dict(recon=1.0, freq=0.0, perceptual=0.0, gen=0.5, unet_perceptual=0.25, dis=1.0, cutmix=0.75, consistency=2.0))


def to_window(x, window):
    """trainers/base.py:290-314 with its `normalize` = utils.t_normalize"""
    if window is None:
        return x
    return refutils.t_normalize(refutils.denormalize(x, **DATASET_WINDOW).clone(), **window)


def one_step(enc, dec, dis, dopt, sopt, image, boxes, flips, w, rw):
    """multi_window_trainer.py:208-321 without the frequency / perceptual terms (weights 0 here)."""
    enc.eval()
    with torch.no_grad():
        embed, _, ids = enc(image, rank=0)
    o_recon = dec(embed.detach())
    images = [to_window(image, win) for win in WINDOWS]
    recons = [to_window(o_recon, win) for win in WINDOWS]
    l_recon, l_gen, l_unet = [], [], []
    for i, (recon, img) in enumerate(zip(recons, images)):
        l_recon.append(rw[i] * F.mse_loss(recon, img, reduction='mean'))
        f_map, f_bottle, f_feat = dis(recon)
        l_gen.append(-(torch.mean(f_map) + torch.mean(f_bottle)))
        _, _, r_feat = dis(img.detach())
        l_unet.append(torch.sum(torch.stack([F.mse_loss(o, t.detach(), reduction='mean') for o, t in zip(f_feat, r_feat)])))
    l_recon, l_gen, l_unet = (torch.mean(torch.stack(t)) for t in (l_recon, l_gen, l_unet))
    l_gen_total = w["recon"] * l_recon + w["gen"] * l_gen + w["unet_perceptual"] * l_unet
    dopt.zero_grad()
    l_gen_total.backward()
    dopt.step()
    l_dis, l_cutmix, l_cons = [], [], []
    for i, (recon, img) in enumerate(zip(recons, images)):
        r_map, r_bottle, _ = dis(img.detach())
        f_map, f_bottle, _ = dis(recon.detach())
        l_dis.append(R.hinge_d_loss(r_map, f_map) + R.hinge_d_loss(r_bottle, f_bottle))
        mask = refutils.cutmix(torch.ones_like(r_map), torch.zeros_like(r_map), (boxes[i], None))
        if flips[i]:
            mask = 1 - mask
        cutmix_images = refutils.mask_src_tgt(img, recon, mask)
        c_map, c_bottle, _ = dis(cutmix_images.detach())
        l_cutmix.append(torch.mean(F.relu(1. + c_bottle)) + torch.mean(F.relu(1. - (mask * 2 - 1) * c_map)))
        l_cons.append(F.mse_loss(c_map, refutils.mask_src_tgt(r_map, f_map, mask)))
    l_dis, l_cutmix, l_cons = (torch.mean(torch.stack(t)) for t in (l_dis, l_cutmix, l_cons))
    l_dis_total = w["dis"] * l_dis + w["cutmix"] * l_cutmix + w["consistency"] * l_cons
    sopt.zero_grad()
    l_dis_total.backward()
    sopt.step()
    vals = dict(gen_total=l_gen_total, recon=l_recon, gen=l_gen, unet_perceptual=l_unet, dis_total=l_dis_total, dis=l_dis,
                cutmix=l_cutmix, consistency=l_cons)
    zero = torch.zeros((), dtype=image.dtype)
    return torch.stack([vals.get(k, zero).detach() for k in LOSS_NAMES])


def make_image(seed):
    """Smooth structure (codes form regions, not noise) on the 1/64 grid: a bicubic 16 x 16 field in [-0.6, 0.6] plus 5 x 5
    box-filtered uniform noise.  A field over the whole of [-1.5, 1.5] was tried first: the reference's own fp32 run then lies
    4e-1 (decoder) and 5e-2 (discriminator) from its fp64 run in the updates and 2e-4 in the losses - chance events of that
    image (sign decisions within rounding of zero), which would make this fixture's bounds, taken from those distances, hold
    nothing.  With this image they are 6e-2, 1.5e-3 and 3e-7, the figures of make_golden_unet_dis.py's fixture."""
    g = torch.Generator().manual_seed(seed)
    coarse = F.interpolate(torch.rand(1, 1, 16, 16, generator=g) * 1.2 - 0.6, size=(512, 512), mode="bicubic", align_corners=False)
    fine = F.avg_pool2d(F.pad(torch.rand(1, 1, 512, 512, generator=g) * 2 - 1, (2, 2, 2, 2), mode="reflect"), 5, 1)
    return (torch.round((coarse + fine).clamp_(-1, 1) * 64) / 64).clamp_(-1, 1)


def step_case(Unet, d, da, dd):
    from helpers import checksum
    c = STEP
    torch.manual_seed(c["seed"])
    enc = R.UNetEncoder(1, c["enc_filters"], c["K"], c["momentum"], "torch", False, 4, True)
    dec = R.UNetDecoder(c["enc_filters"][0], 1, c["dec_filters"], use_dropblock=False, dropped_skip_layers=[],
                        use_styled_up_block=True, use_pixel_shuffle=False)
    for pre, m in (("enc", enc), ("dec", dec)):
        for k, v in m.state_dict().items():
            d["step/init_sum/%s.%s" % (pre, k)] = checksum(v.float())
    with torch.no_grad():                    # checkpoint-like VQ state, as the warm step fixtures and smoke() use
        enc.vq.embed.mul_(0.7)
        enc.vq.cluster_size.fill_(512 * 512 / c["K"])
        enc.vq.embed_avg.copy_(enc.vq.embed.t() * enc.vq.cluster_size[None, :])
    dec.train()
    dis = build(Unet, 4, c["dis_seed"]).train()
    for k, v in dis.state_dict().items():
        d["step/P." + k] = npy(v).copy()
    for k in ("enc_filters", "dec_filters", "K", "momentum", "seed", "lr", "betas", "recon_weights"):
        d["step/cfg/" + k] = np.array(c[k])
    d["step/cfg/dataset_window"] = np.array([DATASET_WINDOW[k] for k in ("width", "center", "scale")], dtype=np.float64)
    for k, v in c["w"].items():
        d["step/cfg/w." + k] = np.array(v)
    image = make_image(c["seed"])
    flat = image.reshape(-1)
    assert bool((flat * 64 == torch.round(flat * 64)).all()) and float(flat.abs().max()) <= 1.0
    # the windows' bounds in the dataset's units: lung (-1300, 200) HU -> x in (-1.3, 0.2); mediastinal (-180, 220) HU
    outside = {"lung": float((flat > 0.2).float().mean()), "mediastinal": float(((flat < -0.18) | (flat > 0.22)).float().mean())}
    print("  pixels outside the window: lung %.1f %%, mediastinal %.1f %%" % (100 * outside["lung"], 100 * outside["mediastinal"]))
    assert min(outside.values()) >= 0.05, outside
    for win in WINDOWS[1:]:                  # no pixel lands on a bound
        hu = refutils.denormalize(flat.double(), **DATASET_WINDOW)
        assert not bool(((hu == win["center"] + win["width"] // 2) | (hu == win["center"] - win["width"] // 2)).any())
    mods = (enc, dec, dis)
    mods64 = tuple(copy.deepcopy(m).double() for m in mods)
    before = [{k: v.detach().clone() for k, v in m.named_parameters()} for m in (dec, dis)]
    opts = [[torch.optim.Adam(m.parameters(), lr=c["lr"], betas=c["betas"]) for m in ms[1:]] for ms in (mods, mods64)]
    l32 = one_step(*mods, *opts[0], image, c["boxes"], c["flips"], c["w"], c["recon_weights"])
    l64 = one_step(*mods64, *opts[1], image.double(), c["boxes"], c["flips"], c["w"], c["recon_weights"])
    d["step/image"], d["step/loss"] = npy(image), npy(l32)
    for i, (box, flip) in enumerate(zip(c["boxes"], c["flips"])):
        d["step/box%d" % i] = np.array([box[0][0], box[0][1], box[1][0], box[1][1]])
        d["step/flip%d" % i] = np.array(int(flip))
    print("  losses " + " ".join("%s %.6g" % kv for kv in zip(LOSS_NAMES, l32.tolist())))
    for pre, m in (("dec", dec), ("dis", dis)):
        for k, v in m.state_dict().items():
            (da if pre == "dis" else dd)["step/after.%s.%s" % (pre, k)] = npy(v).copy()
    d["step/spread.loss"] = np.float64(spread(l32, l64))
    # the UPDATE of each network (after - before, all parameters as one vector): the fp32 run's distance from the fp64 run's
    for name, m, m64, b in (("dec", dec, mods64[1], before[0]), ("dis", dis, mods64[2], before[1])):
        p64 = dict(m64.named_parameters())
        u32 = torch.cat([(p.detach().double() - b[k].double()).reshape(-1) for k, p in m.named_parameters()])
        u64 = torch.cat([(p64[k].detach() - b[k].double()).reshape(-1) for k, p in m.named_parameters()])
        d["step/spread.update_" + name] = np.float64((u32 - u64).norm() / u64.norm())
        print("  %s update: norm %.3e, fp32 run %.3e from the fp64 run's" % (name, float(u64.norm()), float(d["step/spread.update_" + name])))
    print("  spread loss %.1e" % d["step/spread.loss"])


def main():
    Unet = load_unet_discriminator()
    d, da, dd = {}, {}, {}
    step_case(Unet, d, da, dd)
    files = {"unet_dis_mw_step.npz": d, "unet_dis_mw_step_after.npz": da, "unet_dis_mw_step_dec.npz": dd}
    for f, arrays in files.items():
        save(f, arrays)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
