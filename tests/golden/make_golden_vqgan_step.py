#!/usr/bin/env python3
"""Generate the golden vectors of the VQGAN trainer's step (reference trainers/vqgan_unet_dis.py:36-136) from the upstream
reference's own modules and functions: networks/vqgan.py `VQGAN`, networks/unet_discriminator.py `Unet_Discriminator`,
hinge_d_loss, utils.cutmix / mask_src_tgt, F.mse_loss and torch.optim.Adam, with the step's lines in the reference's order -
by the method of make_golden_unet_dis.py::step_case.

Runs ONLY in the build container (needs the reference sources).  Output, tensors only (vqgan_step_ref.CASE is the case):

    tests/golden/vqgan_step.npz            step/  two steps of VQGAN(1, 32, 1, 32, 8, (1,1,1,1), (1,1,1,1), 1, [], [], 512, 0.0, True,
                                                  'torch') (latent 64 x 64: the mid attention sees N = 4096) against
                                                  Unet_Discriminator(1, D_ch=4, D_wide=True, D_attn='0', 512), one 512 x 512 image
                                                  per step, use_unet_perceptual_loss on, no frequency / perceptual loss,
                                                  n_inner_loops 1: cfg/* (seed, dis_seed, lr, betas, w.*), init_sum/* (checksums of
                                                  the VQGAN's initial state: the seed reproduces it; the codebook is
                                                  vqgan_model_ref.codebook(seed), embed_avg its transpose), P.* (the discriminator
                                                  before), image{s}, box{s}, flip{s}, loss{s} (the twelve logged values in
                                                  vqgan_step_ref.LOGGED order, fp64), ids{s} (fp64 run), buf{s}.* (the VQ buffers
                                                  after step s, fp32 run), min_gap (the smallest relative top-1 / top-2 distance
                                                  gap of both steps, fp64), spread.loss, spread.after, spread.buf, spread.update_{vqgan,dis}
    tests/golden/vqgan_step_after_enc.npz  step/after.vqgan.{encoder,vq}.*   the fp32 run's state after the two steps
    tests/golden/vqgan_step_after_dec.npz  step/after.vqgan.decoder.*
    tests/golden/vqgan_step_after_dis.npz  step/after.dis.*

Adam runs at lr 1e-6 for the reason make_golden_unet_dis.py gives.  The spreads are over THREE mathematically identical fp32 runs
of the two steps (eight threads, one thread, the VQGAN in channels_last) against the fp64 run: spread.loss = max |fp32 - fp64| over the largest
|fp64| logged value of the step; spread.after = the same per state tensor, the worst; spread.buf = the same
over the three VQ buffers after each step; spread.update_* = the relative L2 distance
of the fp32 run's update (after - before, all parameters as one vector) from the fp64 run's, the worst of the three.

Asserted here: every fp32 run gives the fp64 ids on every latent pixel in both steps and all 8 codes are in use in both; the seed
is searched from vqgan_step_ref.CASE["seed"] upwards until that holds, and the one found must be the one recorded there.

The smallest relative top-1 / top-2 gap is recorded, not bounded: with 4096 latent pixels per step none of the seeds 95 ... 134
reaches make_golden_vqgan_model.py's 1e-4 (the best, seed 121, has 9.7e-5 in step 0); seed 95 has 4.9e-5, and what the fixture
asserts instead is the thing itself - three fp32 evaluations of the reference agree with fp64 on every pixel.

    python tests/golden/make_golden_vqgan_step.py
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

import _refshim  # noqa: E402
from make_golden_dis import R, npy, save, spread  # noqa: E402  (loads the reference's generator side and its utils once)
from make_golden_unet_dis import load_unet_discriminator, build  # noqa: E402
from helpers import checksum  # noqa: E402
import vqgan_model_ref as M  # noqa: E402
import vqgan_step_ref as S  # noqa: E402

refutils = sys.modules["refutils"]
torch.set_num_threads(8)
REF = _refshim._load("networks.vqgan", "networks/vqgan.py")
FILES = ("vqgan_step.npz", "vqgan_step_after_enc.npz", "vqgan_step_after_dec.npz", "vqgan_step_after_dis.npz")


def one_step(vqgan, dis, gopt, dopt, image, box, flip, w):
    """vqgan_unet_dis.py:36-136 without the frequency / perceptual terms (weights 0 there) -> (the logged values, ids)."""
    recon, l_commit, ids, _ = vqgan(image)
    l_recon = F.mse_loss(recon, image, reduction='mean')
    f_map, f_bottle, f_perceptual = dis(recon)
    l_gen = -(torch.mean(f_map) + torch.mean(f_bottle))
    _, _, r_perceptual = dis(image.detach())
    l_unet = torch.sum(torch.stack([F.mse_loss(o, t.detach(), reduction='mean') for o, t in zip(f_perceptual, r_perceptual)]))
    l_gen_total = w["recon"] * l_recon + w["commit"] * l_commit + w["gen"] * l_gen + w["unet_perceptual"] * l_unet
    gopt.zero_grad()
    l_gen_total.backward()
    gopt.step()
    r_map, r_bottle, _ = dis(image.detach())
    f_map, f_bottle, _ = dis(recon.detach())
    l_dis = R.hinge_d_loss(r_map, f_map) + R.hinge_d_loss(r_bottle, f_bottle)
    mask = refutils.cutmix(torch.ones_like(r_map), torch.zeros_like(r_map), (box, None))
    if flip:
        mask = 1 - mask
    cutmix_images = refutils.mask_src_tgt(image, recon, mask)
    c_map, c_bottle, _ = dis(cutmix_images.detach())
    l_cutmix = torch.mean(F.relu(1. + c_bottle)) + torch.mean(F.relu(1. - (mask * 2 - 1) * c_map))
    l_cons = F.mse_loss(c_map, refutils.mask_src_tgt(r_map, f_map, mask))
    l_dis_total = w["dis"] * l_dis + w["cutmix"] * l_cutmix + w["consistency"] * l_cons
    dopt.zero_grad()
    l_dis_total.backward()
    dopt.step()
    zero = torch.zeros((), dtype=image.dtype)
    vals = dict(total=l_gen_total + l_dis_total, gen_total=l_gen_total, recon=w["recon"] * l_recon, freq=zero, perceptual=zero,
                commit=w["commit"] * l_commit, gen=w["gen"] * l_gen, unet_perceptual=w["unet_perceptual"] * l_unet,
                dis_total=l_dis_total, dis=w["dis"] * l_dis, cutmix=w["cutmix"] * l_cutmix, consistency=w["consistency"] * l_cons)
    return torch.stack([vals[k].detach() for k in S.LOGGED]), ids.detach().clone()


def build_vqgan(seed):
    torch.manual_seed(seed)
    vqgan = REF.VQGAN(*S.CASE["vqgan"])
    sums = {k: checksum(v.float()) for k, v in vqgan.state_dict().items()}
    with torch.no_grad():
        vqgan.vq.embed.copy_(M.codebook(seed))
        vqgan.vq.embed_avg.copy_(vqgan.vq.embed.t())
    return vqgan.train(), sums


def images(seed):
    g = torch.Generator().manual_seed(seed)
    return [S.step_image(g) for _ in range(2)]


def run_two(vqgan, dis, imgs, dtype, fmt=None):
    """Two steps on copies of the modules -> (vqgan, dis, [logged], [ids], [VQ buffers after each step])"""
    c = S.CASE
    vqgan, dis = copy.deepcopy(vqgan).to(dtype).train(), copy.deepcopy(dis).to(dtype).train()
    if fmt is not None:                      # the VQGAN only: the reference's discriminator views its weights as matrices
        vqgan = vqgan.to(memory_format=fmt)
    gopt = torch.optim.Adam(vqgan.parameters(), lr=c["lr"], betas=c["betas"])
    dopt = torch.optim.Adam(dis.parameters(), lr=c["lr"], betas=c["betas"])
    logged, ids, bufs, gaps = [], [], [], []

    def gap_hook(mod, inputs):                # the relative top-1 / top-2 distance gap of the quantiser's input, per pixel
        x = inputs[0].detach()
        flat = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        two = ((flat[:, None, :] - mod.embed.detach()[None]) ** 2).sum(-1).topk(2, dim=1, largest=False).values
        gaps.append(float(((two[:, 1] - two[:, 0]) / two[:, 0]).min()))
    hook = vqgan.vq.register_forward_pre_hook(gap_hook) if dtype == torch.float64 else None
    for s, image in enumerate(imgs):
        image = image.to(dtype)
        if fmt is not None:
            image = image.contiguous(memory_format=fmt)
        lg, i = one_step(vqgan, dis, gopt, dopt, image, c["boxes"][s], c["flips"][s], c["w"])
        logged.append(lg)
        ids.append(i)
        bufs.append({k: getattr(vqgan.vq, k).detach().clone() for k in S.VQ_BUFFERS})
    if hook is not None:
        hook.remove()
    return vqgan, dis, logged, ids, bufs, gaps


def fp64_conditions(vqgan, truth):
    for s in range(2):
        used = len(torch.unique(truth[3][s]))
        if used != vqgan.vq.dict_size:
            return "step %d: %d of %d codes in use" % (s, used, vqgan.vq.dict_size)
    return None


def evaluate(Unet, seed):
    vqgan, sums = build_vqgan(seed)
    dis = build(Unet, 4, S.CASE["dis_seed"]).train()
    imgs = images(seed)
    truth = run_two(vqgan, dis, imgs, torch.float64)
    if fp64_conditions(vqgan, truth) is not None:          # no need for the fp32 runs
        return vqgan, dis, sums, imgs, truth, []
    runs = [run_two(vqgan, dis, imgs, torch.float32)]
    torch.set_num_threads(1)
    try:
        runs.append(run_two(vqgan, dis, imgs, torch.float32))
    finally:
        torch.set_num_threads(8)
    runs.append(run_two(vqgan, dis, imgs, torch.float32, torch.channels_last))
    return vqgan, dis, sums, imgs, truth, runs


def conditions(vqgan, truth, runs):
    why = fp64_conditions(vqgan, truth)
    if why is not None:
        return why
    for s in range(2):
        for i, r in enumerate(runs):
            bad = int((r[3][s] != truth[3][s]).sum())
            if bad:
                return "step %d: fp32 run %d differs from the fp64 ids on %d pixels" % (s, i, bad)
    return None


def update_of(module, before):
    return torch.cat([(p.detach().double() - before[k].double()).reshape(-1) for k, p in module.named_parameters()])


def main():
    Unet = load_unet_discriminator()
    c = S.CASE
    for seed in range(c["seed"], c["seed"] + 40):
        vqgan, dis, sums, imgs, truth, runs = evaluate(Unet, seed)
        why = conditions(vqgan, truth, runs)
        if why is None:
            break
        print("  seed %d: %s" % (seed, why))
    assert why is None and seed == c["seed"], "vqgan_step_ref.CASE['seed'] must be %d" % seed
    d, de, dd, ds = {}, {}, {}, {}
    for k, v in sums.items():
        d["step/init_sum/" + k] = v
    for k, v in dis.state_dict().items():
        d["step/P." + k] = npy(v).copy()
    for k in ("seed", "dis_seed", "lr", "betas"):
        d["step/cfg/" + k] = np.array(c[k])
    for k, v in c["w"].items():
        d["step/cfg/w." + k] = np.array(v)
    # the restatement is the same mathematics: its fp64 gap is the recorded one
    gen_st, dis_st = S.make_states(vqgan.state_dict(), dis.state_dict())
    gopt, dopt = (torch.optim.Adam(S.params(st), lr=c["lr"], betas=c["betas"]) for st in (gen_st, dis_st))
    min_gap = np.inf
    sp_loss = sp_buf = 0.0
    for s in range(2):
        with torch.no_grad():
            min_gap = min(min_gap, float(M.vqgan_forward_ref(imgs[s].double(), gen_st, training=False)["gap"].min()))
        assert abs(min_gap - min(truth[5][:s + 1])) <= 1e-9 * min_gap
        lg, ids = S.step_ref(gen_st, dis_st, gopt, dopt, imgs[s].double(), c["boxes"][s], c["flips"][s], c["w"])
        assert torch.equal(ids, truth[3][s]) and spread(lg, truth[2][s]) < 1e-9, "the restatement differs from the reference in fp64"
        sp_loss = max(sp_loss, max(spread(r[2][s], truth[2][s]) for r in runs))
        d["step/image%d" % s], d["step/loss%d" % s], d["step/ids%d" % s] = npy(imgs[s]), npy(truth[2][s]), npy(truth[3][s])
        (y0, y1), (x0, x1) = c["boxes"][s]
        d["step/box%d" % s], d["step/flip%d" % s] = np.array([y0, y1, x0, x1]), np.array(int(c["flips"][s]))
        for k in S.VQ_BUFFERS:
            d["step/buf%d.%s" % (s, k)] = npy(runs[0][4][s][k])
            sp_buf = max(sp_buf, max(spread(r[4][s][k], truth[4][s][k]) for r in runs))
        print("  step %d logged " % s + " ".join("%s %.6g" % kv for kv in zip(S.LOGGED, truth[2][s].tolist())))
    d["step/min_gap"], d["step/spread.buf"] = np.float64(min_gap), np.float64(sp_buf)
    sp_after = 0.0
    for i, (pre, m64) in enumerate((("vqgan", truth[0]), ("dis", truth[1]))):
        sd64 = m64.state_dict()
        for r in runs:
            for k, v in r[i].state_dict().items():
                if v.is_floating_point():
                    sp_after = max(sp_after, spread(v, sd64[k]))
        for k, v in runs[0][i].state_dict().items():
            out = ds if pre == "dis" else (dd if k.startswith("decoder.") else de)
            out["step/after.%s.%s" % (pre, k)] = npy(v).copy()
        before = {k: v.detach().clone() for k, v in (vqgan, dis)[i].named_parameters()}
        u64 = update_of(m64, before)
        worst = max(float((update_of(r[i], before) - u64).norm() / u64.norm()) for r in runs)
        d["step/spread.update_" + pre] = np.float64(worst)
        print("  %s update: norm %.3e, the fp32 runs within %.3e of the fp64 run's" % (pre, float(u64.norm()), worst))
    d["step/spread.loss"], d["step/spread.after"] = np.float64(sp_loss), np.float64(sp_after)
    print("  seed %d, smallest gap %.2e, spread loss %.1e after %.1e buf %.1e" % (seed, min_gap, sp_loss, sp_after, sp_buf))
    for f, x in zip(FILES, (d, de, dd, ds)):
        save(f, x)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
