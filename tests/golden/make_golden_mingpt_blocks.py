#!/usr/bin/env python3
"""Generate the golden vectors of the minGPT blocks from the upstream reference's own modules (networks/mingpt.py:
CausalSelfAttention, Block).

Runs ONLY in the build container (needs the reference sources); _refshim.py loads the reference as make_golden_vqgan_blocks.py
loads its files.  Output, tensors only:

    tests/golden/mingpt_blocks_<case>.npz    <case>/   for the four cases of mingpt_ref.CASES, (E, n_head, T, n_unmasked, B):
                                             att64 = CausalSelfAttention (64, 2, 40, 5, 2), block64 = Block (64, 2, 40, 5, 2),
                                             block96 = Block (96, 3, 70, 0, 2), block128 = Block (128, 4, 129, 40, 1)

Each case, in train mode with all dropout probabilities 0, forward plus backward of sum <output, mingpt_ref.cotangent(shape)>,
once in fp64 - the truth - and in three mathematically identical fp32 evaluations (eight threads, one thread, batch reversed):

    seed, keys (state_dict order, the mask buffer included), nparams, in, P.* (the state), out, gin (fp32, as launched),
    present (att64: the stacked key / value projections), g64.* (the fp64 gradient of every parameter and of `input` at
    helpers.sample_idx(numel, 256, seed=1)), gnorm64.* (its norm), gerr32.* (the three fp32 evaluations' relative L2 distance
    from it), spread.{out,gin,gP,present} (make_golden_dis.spread; gP: the worst parameter among `live`, the names whose gradient
    is not analytically zero - att.k.bias is: a constant added to every key shifts each row's scores by a constant),
    past, past_in, past_out, past_present, spread.past_out, spread.past_present (mingpt_ref.PAST_CASES: the eval-mode forward
    of mingpt_ref.PAST_NEW new tokens behind a layer_past of mingpt_ref.PAST_LEN tokens)

Every file stays below the repository's 1 MiB limit: weights, biases and inputs are multiples of 1/64 (they compress), gradients
are stored as samples.  The fp32 evaluations alone must pass helpers.grad_gate at its defaults against the fp64 truth - asserted
here, a fixture for which the reference itself does not stay within the cap is not written.

    python tests/golden/make_golden_mingpt_blocks.py
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
from helpers import grad_gate, sample_idx  # noqa: E402
import mingpt_ref as M  # noqa: E402

torch.set_num_threads(8)
REF = _refshim._load("networks.mingpt", "networks/mingpt.py")


def run(module, x, threads=8, rev=False):
    m = copy.deepcopy(module).to(x.dtype).train()
    xin = (x.flip(0) if rev else x).clone().requires_grad_(True)
    torch.set_num_threads(threads)
    try:
        out = m(xin)
        out, present = out if isinstance(out, tuple) else (out, None)
        cot = M.cotangent(out.shape, x.dtype)
        (out * (cot.flip(0) if rev else cot)).sum().backward()
    finally:
        torch.set_num_threads(8)
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = xin.grad.flip(0) if rev else xin.grad
    return out.detach(), None if present is None else present.detach(), grads


def case(name, d):
    cls = M.CASES[name][0]
    seed = M.SEEDS[name]
    torch.manual_seed(seed)
    module = M.init_case_(getattr(REF, cls)(REF.GPTConfig(**M.config_kwargs(name))), seed)
    x = M.case_input(name, seed)
    out64, pres64, truth = run(module, x.double())
    out32, pres32, v0 = run(module, x)
    variants = [v0, run(module, x, threads=1)[2], run(module, x, rev=True)[2]]
    for i, v in enumerate(variants):          # the reference's own fp32 evaluations stay within the cap
        grad_gate(truth, variants, v, what="%s variant %d" % (name, i))
    gmax = max(float(g.norm()) for g in truth.values())
    live = [k for k, g in truth.items() if float(g.norm()) >= 1e-6 * gmax]
    assert ("att.k.bias" if cls == "Block" else "k.bias") not in live
    # the restatement is the same mathematics
    sd = module.state_dict()
    r64, rp64, rg = M.grads_ref(name, sd, x, torch.float64)
    assert spread(r64, out64) < 1e-12 and max(spread(rg[k], truth[k]) for k in live) < 1e-10, name
    p = name + "/"
    d[p + "seed"], d[p + "keys"] = np.array(seed), np.array(list(sd))
    d[p + "nparams"] = np.array(sum(q.numel() for q in module.parameters()))
    d[p + "in"], d[p + "out"], d[p + "gin"] = npy(x), npy(out32), npy(v0["input"])
    for k, t in sd.items():
        d[p + "P." + k] = npy(t).copy()
    for k, g in truth.items():
        idx = sample_idx(g.numel(), 256, seed=1)
        d[p + "g64." + k] = npy(g.reshape(-1)[idx])
        d[p + "gnorm64." + k] = np.float64(g.norm())
        d[p + "gerr32." + k] = np.array([float((v[k].double() - g).norm() / g.norm()) if float(g.norm()) > 0 else 0.0 for v in variants])
    d[p + "live"] = np.array(live)
    d[p + "spread.out"] = np.float64(spread(out32, out64))
    d[p + "spread.gin"] = np.float64(spread(v0["input"], truth["input"]))
    d[p + "spread.gP"] = np.float64(max(spread(v0[k], truth[k]) for k in live if k != "input"))
    if pres32 is not None:
        assert spread(rp64, pres64) < 1e-12
        d[p + "present"], d[p + "spread.present"] = npy(pres32), np.float64(spread(pres32, pres64))
    if name in M.PAST_CASES:
        past, xn = M.case_past(name, seed)
        with torch.no_grad():
            o32, p32 = copy.deepcopy(module).eval()(xn, layer_past=past)
            o64, p64 = copy.deepcopy(module).double().eval()(xn.double(), layer_past=past.double())
            ro, rp = M.case_ref(name, xn.double(), {k: (v if k.endswith("mask") else v.double()) for k, v in sd.items()}, past.double())
        assert spread(ro, o64) < 1e-12 and spread(rp, p64) < 1e-12
        d[p + "past"], d[p + "past_in"], d[p + "past_out"], d[p + "past_present"] = npy(past), npy(xn), npy(o32), npy(p32)
        d[p + "spread.past_out"], d[p + "spread.past_present"] = np.float64(spread(o32, o64)), np.float64(spread(p32, p64))
    print("  %-10s %d parameters, spread out %.1e gin %.1e gP %.1e" % (name, int(d[p + "nparams"]), d[p + "spread.out"],
                                                                    d[p + "spread.gin"], d[p + "spread.gP"]))


def main():
    for name in M.CASES:
        d = {}
        case(name, d)
        f = "mingpt_blocks_%s.npz" % name
        save(f, d)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
