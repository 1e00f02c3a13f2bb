#!/usr/bin/env python3
"""Generate the golden vectors of the U-Net discriminator and of the second training step that uses it from the upstream
reference's own modules (networks/unet_discriminator.py `Unet_Discriminator` over networks/biggan/layers.py, UNetEncoder /
UNetDecoder, hinge_d_loss, utils.cutmix / cutmix_coordinates / mask_src_tgt).

Runs ONLY in the build container (needs the reference sources).  _refshim.py loads the generator side; the two BigGAN files
are loaded here under the stand-in packages it registers, with a stub `utils` and matplotlib (neither is used by the
discriminator).  Output, tensors only:

    tests/golden/unet_dis_ch4.npz         mod/   D_ch=4, in_channels=1, D_attn='0', 512^2, batch 1, train mode: P.* (state dict),
                                                 in.0, out.0, bottleneck, feat.0..6, gin.0, after.* (u0 / sv0 after the forward),
                                                 spread.{out,bottleneck,feat,gin,gP,after}
                                          eval/  one eval-mode forward of the same state: out.0, bottleneck (u0 / sv0 unchanged:
                                                 asserted here)
                                          draws/ cutmix_coordinates under np.random.seed(1234): 8 rectangles for 512 x 512
    tests/golden/unet_dis_ch4_grads.npz   mod/gP.*  every parameter gradient of that case (`linear.*` has none)
    tests/golden/unet_dis_step.npz        step/  two full steps of _train_second_step_unet_dis (use_unet_perceptual_loss on, all
                                                 weights 1 but the ones in cfg/) restated from the reference's modules: image{s},
                                                 box{s}, flip{s}, loss{s} (the ten logged values, un-weighted, in LOSS_NAMES
                                                 order), P.* (discriminator before), init_sum/* (encoder / decoder checksums),
                                                 spread.loss, spread.after, spread.update_{dec,dis} (relative L2 distance of the
                                                 fp32 run's update, after - before over all parameters, from the fp64 run's)
    tests/golden/unet_dis_step_after.npz  step/after.dis.* the discriminator's state after the two steps
    tests/golden/unet_dis_step_dec.npz    step/after.dec.* the decoder's

The step case runs Adam at lr 1e-6, as step_rcfg64_warm_lr1e-6.npz does: Adam's first updates are lr * g / (|g| + eps), about
lr * sign(g) for every element, so a gradient entry whose sign is within rounding of zero moves its weight by 2 lr between two
correct fp32 evaluations; at a training lr those chance events, not the arithmetic, decide how far step 1 of any fp32 run lies
from the fp64 one (one fp32-against-fp64 pair, which is what `spread` is, samples them once).  At 1e-6 they stay below fp32
rounding of the losses, so that spread.loss measures rounding; the updates themselves are still resolved by fp32 weights.

The backward of the module case is of  sum_i <output_i, weight_pattern(shape_i)>  over (out, bottleneck, feat.0..6) with
unet_dis_ref.weight_pattern - a closed form, so that no 512^2 cotangent has to be stored.

Every committed file stays below the repository's 1 MiB limit: conv weights are rounded to multiples of 1/64 (as
make_golden_dis.py does) and so are the inputs; a tensor with a side of 64 or more is stored on a fixed subset of its rows
and columns - every 8th plus the two outermost on each side (unet_dis_ref.subset_index) - whole otherwise.  The spreads are
make_golden_dis.py's: max |fp32 - fp64| over the largest |fp64| element, the worst tensor of the kind, taken on whole tensors.

    python tests/golden/make_golden_unet_dis.py
"""
import copy
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refshim  # noqa: E402
from make_golden_dis import R, npy, save, spread  # noqa: E402  (loads the reference's generator side and its utils once)
from unet_dis_ref import weight_pattern, subset, LOSS_NAMES  # noqa: E402

refutils = sys.modules["refutils"]
torch.set_num_threads(8)


def load_unet_discriminator():
    """networks.biggan and networks.unet_discriminator of the reference under the stand-in `networks` package."""
    stub = sys.modules["utils"]                      # _refshim's stub serves `import utils` (never used by the discriminator)
    assert isinstance(stub, types.ModuleType)
    import matplotlib
    matplotlib.use("Agg")
    bg = _refshim._pkg("networks.biggan", os.path.join(_refshim.REF_SRC, "networks", "biggan"))
    layers = _refshim._load("networks.biggan.layers", "networks/biggan/layers.py")
    for k, v in vars(layers).items():
        if not k.startswith("_"):
            setattr(bg, k, v)
    sys.modules["networks"].biggan = bg
    return _refshim._load("networks.unet_discriminator", "networks/unet_discriminator.py").Unet_Discriminator


def build(Unet, D_ch, seed):
    import contextlib
    import io
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):          # the constructor prints every parameter
        dis = Unet(in_channels=1, D_ch=D_ch, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    with torch.no_grad():
        for m in dis.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.round(m.weight * 64) / 64)
    return dis


def run(dis, x, train):
    dis.train(train)
    xin = x.clone().requires_grad_(True)
    out, bottle, feats = dis(xin)
    outs = [out, bottle] + list(feats)
    sum((o * weight_pattern(o.shape, o.dtype)).sum() for o in outs).backward()
    gP = {k: p.grad for k, p in dis.named_parameters() if p.grad is not None}
    after = {k: v.clone() for k, v in dis.state_dict().items() if k.endswith(("u0", "sv0"))}
    return outs, xin.grad, gP, after


TIE_MARGIN = 2e-6


def relu_margin(dis64, x64):
    """The smallest |input| of any ReLU that acts on a map of 128 x 128 or coarser (block outputs and conv1 outputs), in fp64."""
    seen = []
    hooks = [m.register_forward_hook(lambda mod, i, o: seen.append(float(o.detach().abs().min())) if o.shape[-1] <= 128 else None)
             for name, m in dis64.named_modules() if name.endswith(".conv1") or (name.startswith("blocks.") and name.endswith(".0"))]
    with torch.no_grad():
        state = copy.deepcopy(dis64.state_dict())
        dis64.train()
        dis64(x64)
        dis64.load_state_dict(state)
    for h in hooks:
        h.remove()
    return min(seen)


def module_case(Unet, d, dg):
    # Some 4.5 M values pass a ReLU in one forward, so a handful lie within fp32 rounding of zero and ANY two fp32 evaluations
    # take a few of those decisions differently.  On the fine maps one pixel's decision moves a gradient by 1e-5 or less; on a
    # map of 128 x 128 or coarser it moves every upstream gradient by 1e-3 ... 1e-2 (seed 61: |out of block 11| = 4.8e-8 at
    # one entry), which is luck, not arithmetic.  The seed is therefore the first from 61 on whose fp64 forward keeps every
    # such ReLU input at least TIE_MARGIN (about 8 fp32 ulps of a value of 2) away from zero.
    for seed in range(61, 81):
        dis = build(Unet, 4, seed)
        x = torch.round(torch.randn(1, 1, 512, 512) * 64) / 64
        margin = relu_margin(copy.deepcopy(dis).double(), x.double())
        print("  seed %d: smallest coarse-map ReLU input %.2e" % (seed, margin))
        if margin >= TIE_MARGIN:
            break
    else:
        raise RuntimeError("no seed with a ReLU margin of %g" % TIE_MARGIN)
    d["mod/seed"], d["mod/relu_margin"] = np.array(seed), np.float64(margin)
    dis64 = copy.deepcopy(dis).double()
    for k, v in dis.state_dict().items():
        d["mod/P." + k] = npy(v).copy()
    assert len(dis.state_dict()) == 178 and sum(p.numel() for p in dis.parameters()) == 222295
    disE = copy.deepcopy(dis).eval()
    with torch.no_grad():
        oe, be, _ = disE(x)
    for k, v in disE.state_dict().items():
        assert torch.equal(v, dis.state_dict()[k]), "eval forward changed " + k
    d["eval/out.0"], d["eval/bottleneck"] = npy(subset(oe)), npy(be)
    outs, gin, gP, after = run(dis, x, True)
    outs64, gin64, gP64, after64 = run(dis64, x.double(), True)
    assert "linear.weight" not in gP and len(gP) == 2 * 43 + 2          # 43 normalised layers in use + blocks.14
    d["mod/in.0"], d["mod/gin.0"] = npy(x), npy(subset(gin))
    d["mod/out.0"], d["mod/bottleneck"] = npy(subset(outs[0])), npy(outs[1])
    for i, f in enumerate(outs[2:]):
        d["mod/feat.%d" % i] = npy(subset(f))
    for k, g in gP.items():
        dg["mod/gP." + k] = npy(g)
    for k, v in after.items():
        d["mod/after." + k] = npy(v).copy()
    d["mod/spread.out"] = np.float64(spread(outs[0], outs64[0]))
    d["mod/spread.bottleneck"] = np.float64(spread(outs[1], outs64[1]))
    d["mod/spread.feat"] = np.float64(max(spread(a, b) for a, b in zip(outs[2:], outs64[2:])))
    d["mod/spread.gin"] = np.float64(spread(gin, gin64))
    d["mod/spread.gP"] = np.float64(max(spread(g, gP64[k]) for k, g in gP.items()))
    d["mod/spread.after"] = np.float64(max(spread(v, after64[k]) for k, v in after.items()))
    print("  mod   spread " + " ".join("%s %.1e" % (k, d["mod/spread." + k]) for k in ("out", "bottleneck", "feat", "gin", "gP", "after")))


def draws_case(d):
    np.random.seed(1234)
    rows = []
    for _ in range(8):
        ((y0, y1), (x0, x1)), lam = refutils.cutmix_coordinates(512, 512)
        rows.append([y0, y1, x0, x1])
    d["draws/seed"], d["draws/boxes"] = np.array(1234), np.array(rows, dtype=np.int64)


STEP = dict(enc_filters=[4, 4, 8, 8, 16], dec_filters=[8, 8, 16, 16, 32], K=10, momentum=0.999, seed=62, dis_seed=63, lr=1e-6,
            betas=(0.5, 0.999), boxes=[((100, 300), (64, 200)), ((0, 256), (300, 512))], flips=[False, True],
            w=dict(recon=1.0, freq=0.0, perceptual=0.0, gen=0.5, unet_perceptual=0.25, dis=1.0, cutmix=0.75, consistency=2.0))


def one_step(enc, dec, dis, dopt, sopt, image, box, flip, w):
    """single_window_trainer.py:264-374 without the frequency / perceptual terms (weights 0 there)."""
    enc.eval()
    with torch.no_grad():
        embed, _, ids = enc(image, rank=0)
    recon = dec(embed.detach())
    l_recon = F.mse_loss(recon, image, reduction='mean')
    f_map, f_bottle, f_feat = dis(recon)
    l_gen = -(torch.mean(f_map) + torch.mean(f_bottle))
    _, _, r_feat = dis(image.detach())
    l_unet = torch.sum(torch.stack([F.mse_loss(o, t.detach(), reduction='mean') for o, t in zip(f_feat, r_feat)]))
    l_gen_total = w["recon"] * l_recon + w["gen"] * l_gen + w["unet_perceptual"] * l_unet
    dopt.zero_grad()
    l_gen_total.backward()
    dopt.step()
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
    sopt.zero_grad()
    l_dis_total.backward()
    sopt.step()
    vals = dict(gen_total=l_gen_total, recon=l_recon, gen=l_gen, unet_perceptual=l_unet, dis_total=l_dis_total, dis=l_dis,
                cutmix=l_cutmix, consistency=l_cons)
    zero = torch.zeros((), dtype=image.dtype)
    return torch.stack([vals.get(k, zero).detach() for k in LOSS_NAMES])


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
    for k in ("enc_filters", "dec_filters", "K", "momentum", "seed", "lr", "betas"):
        d["step/cfg/" + k] = np.array(c[k])
    for k, v in c["w"].items():
        d["step/cfg/w." + k] = np.array(v)
    mods = (enc, dec, dis)
    mods64 = tuple(copy.deepcopy(m).double() for m in mods)
    before = [{k: v.detach().clone() for k, v in m.named_parameters()} for m in (dec, dis)]
    opts = [[torch.optim.Adam(m.parameters(), lr=c["lr"], betas=c["betas"]) for m in ms[1:]] for ms in (mods, mods64)]
    sp = 0.0
    g = torch.Generator().manual_seed(c["seed"])
    for s in range(2):
        image = (torch.round((torch.rand(1, 1, 512, 512, generator=g) * 2 - 1) * 64) / 64).clamp_(-1, 1)
        image = F.avg_pool2d(F.pad(image, (2, 2, 2, 2), mode="reflect"), 5, 1)        # smooth: codes form regions, not noise
        image = torch.round(image * 256) / 256
        l32 = one_step(*mods, *opts[0], image, c["boxes"][s], c["flips"][s], c["w"])
        l64 = one_step(*mods64, *opts[1], image.double(), c["boxes"][s], c["flips"][s], c["w"])
        sp = max(sp, spread(l32, l64))
        d["step/image%d" % s], d["step/loss%d" % s] = npy(image), npy(l32)
        d["step/box%d" % s] = np.array([c["boxes"][s][0][0], c["boxes"][s][0][1], c["boxes"][s][1][0], c["boxes"][s][1][1]])
        d["step/flip%d" % s] = np.array(int(c["flips"][s]))
        print("  step %d losses " % s + " ".join("%s %.6g" % kv for kv in zip(LOSS_NAMES, l32.tolist())))
    spa = 0.0
    for pre, m, m64 in (("dec", dec, mods64[1]), ("dis", dis, mods64[2])):
        sd64 = m64.state_dict()
        for k, v in m.state_dict().items():
            (da if pre == "dis" else dd)["step/after.%s.%s" % (pre, k)] = npy(v).copy()
            if v.is_floating_point():
                spa = max(spa, spread(v, sd64[k]))
    d["step/spread.loss"], d["step/spread.after"] = np.float64(sp), np.float64(spa)
    # the UPDATE of each network (after - before, all parameters as one vector): the fp32 run's distance from the fp64 run's
    for name, m, m64, b in (("dec", dec, mods64[1], before[0]), ("dis", dis, mods64[2], before[1])):
        p64 = dict(m64.named_parameters())
        u32 = torch.cat([(p.detach().double() - b[k].double()).reshape(-1) for k, p in m.named_parameters()])
        u64 = torch.cat([(p64[k].detach() - b[k].double()).reshape(-1) for k, p in m.named_parameters()])
        d["step/spread.update_" + name] = np.float64((u32 - u64).norm() / u64.norm())
        print("  step  %s update: norm %.3e, fp32 run %.3e from the fp64 run's" % (name, float(u64.norm()), float(d["step/spread.update_" + name])))
    print("  step  spread loss %.1e after %.1e" % (sp, spa))


def main():
    Unet = load_unet_discriminator()
    random.seed(0)
    d, dg = {}, {}
    module_case(Unet, d, dg)
    draws_case(d)
    save("unet_dis_ch4.npz", d)
    save("unet_dis_ch4_grads.npz", dg)
    d, da, dd = {}, {}, {}
    step_case(Unet, d, da, dd)
    save("unet_dis_step.npz", d)
    save("unet_dis_step_after.npz", da)
    save("unet_dis_step_dec.npz", dd)
    for f in ("unet_dis_ch4.npz", "unet_dis_ch4_grads.npz", "unet_dis_step.npz", "unet_dis_step_after.npz", "unet_dis_step_dec.npz"):
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
