#!/usr/bin/env python3
"""Generate the golden vectors of the VQGAN decoder's blocks from the upstream reference's own modules (networks/vqgan.py:
ResnetBlock, AttnBlock, Decoder).

Runs ONLY in the build container (needs the reference sources); _refshim.py loads the reference as make_golden_unet_dis.py
loads its files.  Output, tensors only:

    tests/golden/vqgan_blocks_<case>.npz    <case>/   for the five cases of vqgan_ref.CASES: res64 = ResnetBlock(64),
                                            res32_64_nin = ResnetBlock(32, 64), res32_64_conv = the same with use_conv_shortcut,
                                            attn64 = AttnBlock(64), all on 2 x C x 16 x 16; decoder = Decoder(8, 32, 1, (1, 2), 1,
                                            [16], 32, 0.0, True) on 2 x 8 x 16 x 16

Each case, in train mode, forward plus backward of sum <output, weight_pattern(shape)> (unet_dis_ref.weight_pattern), once in
fp64 - the truth - and in three mathematically identical fp32 evaluations (eight threads, one thread, channels_last):

    seed, keys (state_dict order), nparams, in, P.* (the state), out, gin (fp32, as launched), eval_out (decoder: eval mode),
    g64.* (the fp64 gradient of every parameter and of `input` at helpers.sample_idx(numel, 256, seed=1)), gnorm64.* (its norm),
    gerr32.* (the three fp32 evaluations' relative L2 distance from it: all that helpers.grad_gate takes from a variant),
    spread.{out,gin,gP} (make_golden_dis.spread: max |fp32 - fp64| over the largest |fp64| element; gP: the worst parameter
    among `live`, the names whose gradient is not analytically zero, as helpers.grad_gate tells them)

Every file stays below the repository's 1 MiB limit: convolution weights, biases and inputs are multiples of 1/64 (they
compress), gradients are stored as samples.  The GroupNorm weight / bias are non-trivial (vqgan_ref.init_case_).  The fp32
evaluations alone must pass helpers.grad_gate at its defaults against the fp64 truth - asserted here, a fixture for which the
reference itself does not stay within the cap is not written.  Swish and softmax are smooth: no seed search for ReLU ties; the
seeds are vqgan_ref.SEEDS as first chosen.

    python tests/golden/make_golden_vqgan_blocks.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _refshim  # noqa: E402
from make_golden_dis import npy, save, spread  # noqa: E402  (loads the reference's generator side once)
from unet_dis_ref import weight_pattern  # noqa: E402
from helpers import grad_gate, sample_idx  # noqa: E402
import vqgan_ref as V  # noqa: E402

torch.set_num_threads(8)
REF = _refshim._load("networks.vqgan", "networks/vqgan.py")


def run(module, x, fmt=None):
    m = copy.deepcopy(module).to(x.dtype).train()
    if fmt is not None:
        m = m.to(memory_format=fmt)
        x = x.contiguous(memory_format=fmt)
    xin = x.clone().requires_grad_(True)
    out = m(xin)
    (out * weight_pattern(out.shape, x.dtype)).sum().backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = xin.grad
    return out.detach(), grads


def case(name, d):
    cls, kw, shape, _ = V.CASES[name]
    seed = V.SEEDS[name]
    torch.manual_seed(seed)
    module = V.init_case_(getattr(REF, cls)(**kw), seed)
    x = V.case_input(name, seed)
    out64, truth = run(module, x.double())
    out32, v0 = run(module, x)
    torch.set_num_threads(1)
    try:
        _, v1 = run(module, x)
    finally:
        torch.set_num_threads(8)
    _, v2 = run(module, x, torch.channels_last)
    variants = [v0, v1, v2]
    for i, v in enumerate(variants):          # the reference's own fp32 evaluations stay within the cap
        grad_gate(truth, variants, v, what="%s variant %d" % (name, i))
    # the restatement is the same mathematics
    # (live: not analytically zero - the gradient of AttnBlock's k.bias is rounding noise, a softmax ignores a row constant)
    gmax = max(float(g.norm()) for g in truth.values())
    live = [k for k, g in truth.items() if float(g.norm()) >= 1e-6 * gmax]
    r64, rg = V.grads_ref(name, module.state_dict(), x, torch.float64)
    assert spread(r64, out64) < 1e-12 and max(spread(rg[k], truth[k]) for k in live) < 1e-10, name
    p = name + "/"
    sd = module.state_dict()
    d[p + "seed"], d[p + "keys"] = np.array(seed), np.array(list(sd))
    d[p + "nparams"] = np.array(sum(q.numel() for q in module.parameters()))
    d[p + "in"], d[p + "out"], d[p + "gin"] = npy(x), npy(out32), npy(v0["input"])
    for k, t in sd.items():
        d[p + "P." + k] = npy(t).copy()
    for k, g in truth.items():
        idx = sample_idx(g.numel(), 256, seed=1)
        d[p + "g64." + k] = npy(g.reshape(-1)[idx])
        d[p + "gnorm64." + k] = np.float64(g.norm())
        d[p + "gerr32." + k] = np.array([float((v[k].double() - g).norm() / g.norm()) for v in variants])
    d[p + "live"] = np.array(live)
    d[p + "spread.out"] = np.float64(spread(out32, out64))
    d[p + "spread.gin"] = np.float64(spread(v0["input"], truth["input"]))
    d[p + "spread.gP"] = np.float64(max(spread(v0[k], truth[k]) for k in live if k != "input"))
    if name == "decoder":
        with torch.no_grad():
            e32, e64 = copy.deepcopy(module).eval()(x), copy.deepcopy(module).double().eval()(x.double())
        d[p + "eval_out"], d[p + "spread.eval_out"] = npy(e32), np.float64(spread(e32, e64))
    print("  %-14s %d parameters, spread out %.1e gin %.1e gP %.1e" % (name, int(d[p + "nparams"]), d[p + "spread.out"],
                                                                    d[p + "spread.gin"], d[p + "spread.gP"]))


def main():
    for name in V.CASES:
        d = {}
        case(name, d)
        f = "vqgan_blocks_%s.npz" % name
        save(f, d)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
