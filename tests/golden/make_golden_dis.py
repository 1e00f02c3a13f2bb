#!/usr/bin/env python3
"""Generate the golden vectors of the discriminator's ActNorm / spectral-norm configurations from the upstream
reference's own modules (its NLayerDiscriminator, ActNorm, hinge_d_loss and utils.apply_spectral_norm).

Runs ONLY in the build container (needs the reference sources; see _refshim.py).  Output, tensors only, in the
`tag/P.*`, `in.*`, `out.*`, `R.*`, `gin.*`, `gP.*`, `after.*` layout of make_golden.module_case:

    tests/golden/gan_norms.npz              act_f8_eval, act_uninit_eval, sn_act_f8, sn_bn_f8_eval, gen_pass_sn, dstep_sn_act
    tests/golden/gan_norms_act_f16.npz      act_f16
    tests/golden/gan_norms_sn_bn_f16.npz    sn_bn_f16

(the two 16-filter cases carry 174 k parameters and as many gradients each, so each has a file of its own to stay below the
repository's 1 MiB limit for a committed file).  Every case also stores the reference's own fp32-against-fp64 spread - the
same module deep-copied to double on the same inputs - as `tag/spread.{out,gin,gP,after}` (dstep: `spread.loss`,
`spread.after`): max |fp32 - fp64| over the largest |fp64| element, the worst tensor of the kind.

Conv weights are drawn from normal(0, 0.2) rounded to multiples of 1/64 (outputs are then not dominated by the biases, and
the stored parameters compress); everything else keeps full fp32 entropy.

    python tests/golden/make_golden_dis.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refshim  # noqa: E402

R = _refshim.load_reference()
ref_apply_spectral_norm = _refshim.load_reference_utils().apply_spectral_norm
torch.set_num_threads(8)

STATE = ("running_", "num_batches", "loc", "scale", "initialized", "weight_u", "weight_v")


def npy(t):
    return t.detach().cpu().numpy()


def save(name, d):
    path = os.path.join(os.environ.get("GOLDEN_OUT", HERE), name)
    np.savez_compressed(path, **d)
    print("wrote %-28s %8.1f KB  (%d arrays)" % (name, os.path.getsize(path) / 1024, len(d)))


def spread(a, b):
    """max |fp32 - fp64| relative to the largest fp64 element"""
    b = b.detach().double()
    return float((a.detach().double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def build(normalization, n_filters, n_layers, spectral, seed):
    torch.manual_seed(seed)
    dis = R.NLayerDiscriminator(in_channels=1, out_channels=1, n_filters=n_filters, n_layers=n_layers,
                                normalization=normalization)
    with torch.no_grad():
        for m in dis.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.round(torch.randn_like(m.weight) * 0.2 * 64) / 64)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.1)
                m.bias.normal_(0.0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    if spectral:
        ref_apply_spectral_norm(dis)
    return dis


def run(mod, x, rnd, train, param_grads):
    mod.train(train)
    xin = x.clone().requires_grad_(True)
    out = mod(xin)
    (out * rnd.to(out.dtype)).sum().backward()
    gP = {k: p.grad for k, p in mod.named_parameters()} if param_grads else {}
    after = {k: v.clone() for k, v in mod.state_dict().items() if any(s in k for s in STATE)}
    return out, xin.grad, gP, after


def module_case(tag, mod, x, d, train=True, param_grads=True):
    """make_golden.module_case plus `after.*` for ActNorm / spectral-norm state and the fp32-against-fp64 spreads."""
    if not param_grads:
        for p in mod.parameters():
            p.requires_grad_(False)
    mod64 = copy.deepcopy(mod).double()
    for k, v in mod.state_dict().items():
        d["%s/P.%s" % (tag, k)] = npy(v).copy()
    mod.train(train)
    with torch.no_grad():
        shape = copy.deepcopy(mod).eval()(x).shape
    rnd = torch.randn(shape)
    out, gin, gP, after = run(mod, x, rnd, train, param_grads)
    out64, gin64, gP64, after64 = run(mod64, x.double(), rnd.double(), train, param_grads)
    d["%s/in.0" % tag], d["%s/gin.0" % tag] = npy(x), npy(gin)
    d["%s/out.0" % tag], d["%s/R.0" % tag] = npy(out), npy(rnd)
    for k, g in gP.items():
        d["%s/gP.%s" % (tag, k)] = npy(g)
    for k, v in after.items():
        d["%s/after.%s" % (tag, k)] = npy(v).copy()
    d["%s/spread.out" % tag] = np.float64(spread(out, out64))
    d["%s/spread.gin" % tag] = np.float64(spread(gin, gin64))
    d["%s/spread.gP" % tag] = np.float64(max([spread(g, gP64[k]) for k, g in gP.items()] or [0.0]))
    d["%s/spread.after" % tag] = np.float64(max([spread(v, after64[k]) for k, v in after.items() if v.is_floating_point()] or [0.0]))
    print("  %-16s spread out %.1e gin %.1e gP %.1e after %.1e" % (tag, d[tag + "/spread.out"], d[tag + "/spread.gin"],
                                                                     d[tag + "/spread.gP"], d[tag + "/spread.after"]))


def dstep_case(tag, dis, d, shape=(3, 1, 64, 64)):
    """The discriminator half of _train_second_step_nl_dis for two Adam steps, as make_golden's `dstep` group."""
    dis.train()
    dis64 = copy.deepcopy(dis).double()
    for k, v in dis.state_dict().items():
        d["%s/P.%s" % (tag, k)] = npy(v).copy()
    opt = torch.optim.Adam(dis.parameters(), lr=1e-3, betas=(0.5, 0.999))
    opt64 = torch.optim.Adam(dis64.parameters(), lr=1e-3, betas=(0.5, 0.999))
    sp = 0.0
    for s in range(2):
        real, fake = torch.randn(*shape).clamp_(-1, 1), torch.randn(*shape).clamp_(-1, 1)
        l_dis = R.hinge_d_loss(dis(real), dis(fake))
        opt.zero_grad()
        (0.8 * l_dis).backward()
        opt.step()
        l64 = R.hinge_d_loss(dis64(real.double()), dis64(fake.double()))
        opt64.zero_grad()
        (0.8 * l64).backward()
        opt64.step()
        sp = max(sp, spread(l_dis, l64))
        d["%s/real%d" % (tag, s)], d["%s/fake%d" % (tag, s)], d["%s/loss%d" % (tag, s)] = npy(real), npy(fake), npy(l_dis)
    sd64 = dis64.state_dict()
    for k, v in dis.state_dict().items():
        d["%s/after.%s" % (tag, k)] = npy(v).copy()
    d["%s/spread.loss" % tag] = np.float64(sp)
    d["%s/spread.after" % tag] = np.float64(max(spread(v, sd64[k]) for k, v in dis.state_dict().items() if v.is_floating_point()))
    print("  %-16s spread loss %.1e after %.1e" % (tag, d[tag + "/spread.loss"], d[tag + "/spread.after"]))


def main():
    d = {}
    module_case("act_f16", build("actnorm", 16, 3, False, 51), torch.randn(3, 1, 64, 64), d)
    save("gan_norms_act_f16.npz", d)
    d = {}
    module_case("sn_bn_f16", build("batchnorm", 16, 3, True, 54), torch.randn(3, 1, 64, 64), d)
    save("gan_norms_sn_bn_f16.npz", d)

    d = {}
    dis = build("actnorm", 8, 2, False, 52)
    with torch.no_grad():
        for m in dis.modules():
            if hasattr(m, "initialized"):
                m.loc.normal_(0, 0.3)
                m.scale.uniform_(0.5, 1.5)
                m.initialized.fill_(1)
    module_case("act_f8_eval", dis, torch.randn(2, 1, 40, 48), d, train=False)
    module_case("act_uninit_eval", build("actnorm", 8, 2, False, 53), torch.randn(2, 1, 24, 24), d, train=False)
    module_case("sn_act_f8", build("actnorm", 8, 2, True, 55), torch.randn(2, 1, 40, 48), d)
    module_case("sn_bn_f8_eval", build("batchnorm", 8, 2, True, 56), torch.randn(2, 1, 40, 48), d, train=False)
    module_case("gen_pass_sn", build("batchnorm", 8, 2, True, 58), torch.randn(2, 1, 24, 24), d, param_grads=False)
    torch.manual_seed(57)
    dstep_case("dstep_sn_act", build("actnorm", 8, 3, True, 57), d)
    save("gan_norms.npz", d)


if __name__ == "__main__":
    main()
