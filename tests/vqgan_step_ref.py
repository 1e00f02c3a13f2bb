"""Plain-torch restatement (any dtype, meant for float64; autograd does the backward, torch.optim.Adam the update) of one
training step of the VQGAN against the U-Net discriminator, on top of vqgan_model_ref.py and unet_dis_ref.py: reference
trainers/vqgan_unet_dis.py:36-136 without the frequency and perceptual terms.

    generator half      recon, commit, ids = VQGAN(image) in train mode (the quantiser's EMA update runs once);
                        gen_total = w.recon MSE + w.commit commit + w.gen l_gen + w.unet_perceptual l_unet, one Adam step of `gopt`
    discriminator half  n_inner times: D(image), D(recon), the CutMix rectangle, D(cutmix images);
                        dis_total = w.dis l_dis + w.cutmix l_cutmix + w.consistency l_consistency, one Adam step of `dopt`
    logged              LOGGED, each term times its weight, total = gen_total + dis_total

`gen` / `dis` are state dicts whose parameters are leaf tensors with requires_grad (make_states); buffers in them are updated
in place.  The case of tests/golden/make_golden_vqgan_step.py is CASE.
"""
import torch
import torch.nn.functional as F

import unet_dis_ref as U
import vqgan_model_ref as M

LOGGED = ("total", "gen_total", "recon", "freq", "perceptual", "commit", "gen", "unet_perceptual", "dis_total", "dis", "cutmix",
          "consistency")
VQ_BUFFERS = ("embed", "cluster_size", "embed_avg")

CASE = dict(vqgan=(1, 32, 1, 32, 8, (1, 1, 1, 1), (1, 1, 1, 1), 1, [], [], 512, 0.0, True, "torch"), seed=95, dis_seed=63, lr=1e-6,
            betas=(0.5, 0.999), boxes=[((100, 300), (64, 200)), ((0, 256), (300, 512))], flips=[False, True],
            w=dict(recon=1.0, freq=0.0, perceptual=0.0, commit=0.6, gen=0.5, unet_perceptual=0.25, dis=1.25, cutmix=0.75,
                   consistency=2.0))


def step_image(generator):
    """One smooth 512 x 512 image in [-1, 1] on multiples of 1/256 (make_golden_unet_dis.py's: codes form regions, not noise)."""
    image = (torch.round((torch.rand(1, 1, 512, 512, generator=generator) * 2 - 1) * 64) / 64).clamp_(-1, 1)
    image = F.avg_pool2d(F.pad(image, (2, 2, 2, 2), mode="reflect"), 5, 1)
    return torch.round(image * 256) / 256


def make_states(gen_state, dis_state, dtype=torch.float64):
    """-> (gen, dis) state dicts in `dtype`: parameters as leaves with requires_grad, buffers plain."""
    def leaf(k, v, is_param):
        v = v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()
        return v.requires_grad_(True) if is_param else v
    gen = {k: leaf(k, v, M.is_param(k)) for k, v in gen_state.items()}
    dis = {k: leaf(k, v, not k.endswith(("u0", "sv0"))) for k, v in dis_state.items()}
    return gen, dis


def params(state):
    return [v for v in state.values() if v.requires_grad]


def step_ref(gen, dis, gopt, dopt, image, box, flip, w, use_recon=True, use_unet_perceptual=True, n_inner=1):
    """-> (the LOGGED values as one tensor, ids in the modules' layout)."""
    res = M.vqgan_forward_ref(image, gen, training=True)
    recon = res["recon"]
    zero = torch.zeros((), dtype=image.dtype)
    l_recon = F.mse_loss(recon, image) if use_recon else zero
    f_map, f_bottle, f_feat = U.unet_discriminator_ref(recon, dis, training=True)
    l_gen = U.gen_loss_ref(f_map, f_bottle)
    l_unet = zero
    if use_unet_perceptual:
        _, _, r_feat = U.unet_discriminator_ref(image, dis, training=True)
        l_unet = U.unet_perceptual_ref(f_feat, r_feat)
    gen_total = w["recon"] * l_recon + w["commit"] * res["commit"] + w["gen"] * l_gen + w["unet_perceptual"] * l_unet
    gopt.zero_grad()
    gen_total.backward()
    gopt.step()
    with torch.no_grad():
        for k in VQ_BUFFERS:
            gen["vq." + k].copy_(res["buffers"][k])
    recon = recon.detach()
    for _ in range(n_inner):
        r_map, r_bottle, _ = U.unet_discriminator_ref(image, dis, training=True)
        f_map, f_bottle, _ = U.unet_discriminator_ref(recon, dis, training=True)
        c_map, c_bottle, _ = U.unet_discriminator_ref(U.cutmix_images_ref(image, recon, box, flip), dis, training=True)
        l_dis, l_cutmix, l_cons = U.dis_losses_ref(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, box, flip)
        dis_total = w["dis"] * l_dis + w["cutmix"] * l_cutmix + w["consistency"] * l_cons
        dopt.zero_grad()
        dis_total.backward()
        dopt.step()
    vals = dict(total=gen_total + dis_total, gen_total=gen_total, recon=w["recon"] * l_recon, freq=zero, perceptual=zero,
                commit=w["commit"] * res["commit"], gen=w["gen"] * l_gen, unet_perceptual=w["unet_perceptual"] * l_unet,
                dis_total=dis_total, dis=w["dis"] * l_dis, cutmix=w["cutmix"] * l_cutmix, consistency=w["consistency"] * l_cons)
    return torch.stack([vals[k].detach() for k in LOGGED]), res["ids"]


def logged_of(out, w):
    """The LOGGED values, in float64, of a trainer's training_step output `out` under the weight namedtuple `w`."""
    term = lambda k: float(getattr(w, k)) * float(out[k].double()) if k in out else 0.0  # noqa: E731
    vals = {k: term(k) for k in ("recon", "freq", "perceptual", "commit", "gen", "unet_perceptual", "dis", "cutmix", "consistency")}
    vals["gen_total"], vals["dis_total"] = float(out["gen_total"].double()), float(out["dis_total"].double())
    vals["total"] = vals["gen_total"] + vals["dis_total"]
    return torch.tensor([vals[k] for k in LOGGED], dtype=torch.float64)


VQGAN_KEYS = ("in_channels", "mid_channels", "out_channels", "emb_dim", "dict_size", "enc_ch_multiplier", "dec_ch_multiplier",
              "num_res_blocks", "enc_attn_resolutions", "dec_attn_resolutions", "resolution", "p_dropout", "resamp_with_conv", "knn_backend")
UNET_DIS = dict(model_name="UNetDiscriminator", D_ch=4, D_wide=True, D_attn="0", resolution=512, normalization="batchnorm")


def run_sections(**run):
    """Config sections (for run_helpers.raw_config) of a small run of the VQGAN trainer: CASE's VQGAN and D_ch = 4 on 512 x 512
    synthetic slices, batch 1, two training samples."""
    vqgan = {k: (list(v) if isinstance(v, tuple) else v) for k, v in zip(VQGAN_KEYS, CASE["vqgan"])}
    return dict(run=dict(run), dataset=dict(dataset_name="synthetic", image_size=512, batch_size=1, n_samples_train=2, n_samples_val=1),
                model=dict(dis=dict(UNET_DIS), vqgan=vqgan, vqmodel=dict(model_name="VQGAN")),
                loss=dict(use_unet_perceptual_loss=True, n_inner_loops=1, dis_loss_type="hinge_d_loss", loss_weight=dict(CASE["w"])),
                save=dict(n_save_images=1))
