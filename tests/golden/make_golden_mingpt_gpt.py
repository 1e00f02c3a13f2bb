#!/usr/bin/env python3
"""Generate the golden vectors of the GPT code prior from the upstream reference's own model (networks/mingpt.py: GPT).

Runs ONLY in the build container (needs the reference sources); _refshim.py loads the reference as make_golden_mingpt_blocks.py
loads it.  Output, tensors only:

    tests/golden/mingpt_gpt_<case>.npz    <case>/   for the two cases of gpt_ref.CASES,
                                          (V, block_size, n_layer, n_head, E, n_unmasked, B, Ti, Te):
                                          gpt64 = (100, 40, 2, 2, 64, 5, 2, 40, 0), gpt96p = (257, 70, 1, 3, 96, 0, 2, 37, 3) - the
                                          latter with 3 rows of `embeddings` in front of its 37 tokens

Each case, in train mode with all dropout probabilities 0, forward plus backward of F.cross_entropy(logits.view(-1, V),
target.view(-1)), once in fp64 - the truth - and in three mathematically identical fp32 evaluations (eight threads, one thread,
batch reversed):

    seed, keys (state_dict order, the mask buffers included), nparams, init.* (helpers.checksum of every entry of the state as
    seeded, before gpt_ref.init_gpt_), P.* (the state: multiples of 1/64, pos_embed non-zero), in (idx), target, prefix (gpt96p),
    out (the fp32 logits as launched), logits (the fp64 logits), loss64, loss32 (the three evaluations'), g64.* (the fp64
    gradient of every parameter and - gpt96p - of `input`, the prefix, at helpers.sample_idx(numel, 256, seed=1)), gnorm64.*,
    gerr32.* (the three fp32 evaluations' relative L2 distance from it), live (the names whose gradient is not analytically zero:
    every blocks.N.att.k.bias is), spread.{out,gP}; gpt96p also eval_logits / spread.eval_logits: the full-sequence logits of
    forward() in eval mode, fp64 - the truth of the cached route - and the fp32 evaluation's spread from them

Every file stays below the repository's 1 MiB limit.  The reference's fp32 evaluations alone must pass helpers.grad_gate at its
defaults against the fp64 truth, and gpt_ref.gpt_ref must equal the reference in fp64 (1e-12 on outputs, 1e-10 on gradients) -
both asserted here before anything is written.

    python tests/golden/make_golden_mingpt_gpt.py
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
from make_golden_dis import npy, save, spread  # noqa: E402  (loads the reference's generator side once)
from helpers import checksum, grad_gate, sample_idx  # noqa: E402
import gpt_ref as G  # noqa: E402

torch.set_num_threads(8)
REF = _refshim._load("networks.mingpt", "networks/mingpt.py")


def run(model, idx, target, prefix, dtype, threads=8, rev=False):
    m = copy.deepcopy(model).to(dtype).train()
    flip = (lambda t: t.flip(0)) if rev else (lambda t: t)
    pin = None if prefix is None else flip(prefix).to(dtype).clone().requires_grad_(True)
    torch.set_num_threads(threads)
    try:
        logits = m(flip(idx), embeddings=pin)
        loss = F.cross_entropy(logits.view(-1, logits.shape[-1]), flip(target).reshape(-1))
        loss.backward()
    finally:
        torch.set_num_threads(8)
    grads = {k: p.grad for k, p in m.named_parameters()}
    if pin is not None:
        grads["input"] = flip(pin.grad)
    return flip(logits.detach()), loss.detach(), grads


def case(name, d):
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    seed = G.SEEDS[name]
    torch.manual_seed(seed)
    model = REF.GPT(**G.gpt_kwargs(name))
    init = {k: checksum(v) for k, v in model.state_dict().items()}
    G.init_gpt_(model, seed)
    idx, target, prefix = G.case_inputs(name, seed)
    out64, loss64, truth = run(model, idx, target, prefix, torch.float64)
    out32, l0, v0 = run(model, idx, target, prefix, torch.float32)
    _, l1, v1 = run(model, idx, target, prefix, torch.float32, threads=1)
    _, l2, v2 = run(model, idx, target, prefix, torch.float32, rev=True)
    variants = [v0, v1, v2]
    for i, v in enumerate(variants):          # the reference's own fp32 evaluations stay within the cap
        grad_gate(truth, variants, v, what="%s variant %d" % (name, i))
    gmax = max(float(g.norm()) for g in truth.values())
    live = [k for k, g in truth.items() if float(g.norm()) >= 1e-6 * gmax]
    assert [k for k in truth if k not in live] == ["blocks.%d.att.k.bias" % i for i in range(nl)]
    # the restatement is the same mathematics
    sd = model.state_dict()
    r64, rl64, rg = G.grads_ref(name, sd, idx, target, prefix, torch.float64)
    assert set(rg) == set(truth)
    assert spread(r64, out64) < 1e-12 and abs(float(rl64) - float(loss64)) < 1e-12 * abs(float(loss64)), name
    assert max(spread(rg[k], truth[k]) for k in live) < 1e-10, name
    p = name + "/"
    d[p + "seed"], d[p + "keys"] = np.array(seed), np.array(list(sd))
    d[p + "nparams"] = np.array(sum(q.numel() for q in model.parameters()))
    d[p + "in"], d[p + "target"], d[p + "out"], d[p + "logits"] = npy(idx), npy(target), npy(out32), npy(out64)
    if prefix is not None:
        d[p + "prefix"] = npy(prefix)
    d[p + "loss64"], d[p + "loss32"] = np.float64(loss64), np.array([float(l0), float(l1), float(l2)], dtype=np.float32)
    for k, t in sd.items():
        d[p + "P." + k] = npy(t).copy()
        d[p + "init." + k] = init[k]
    for k, g in truth.items():
        d[p + "g64." + k] = npy(g.reshape(-1)[sample_idx(g.numel(), 256, seed=1)])
        d[p + "gnorm64." + k] = np.float64(g.norm())
        d[p + "gerr32." + k] = np.array([float((v[k].double() - g).norm() / g.norm()) if float(g.norm()) > 0 else 0.0 for v in variants])
    d[p + "live"] = np.array(live)
    d[p + "spread.out"] = np.float64(spread(out32, out64))
    d[p + "spread.gP"] = np.float64(max(spread(v0[k], truth[k]) for k in live))
    if name == G.CACHED_CASE:
        with torch.no_grad():
            e32 = copy.deepcopy(model).eval()(idx, embeddings=prefix)
            e64 = copy.deepcopy(model).double().eval()(idx, embeddings=prefix.double())
            st = {k: (v if k.endswith("mask") else v.double()) for k, v in sd.items()}
            assert spread(G.gpt_ref(idx, st, nl, nh, prefix.double())[0], e64) < 1e-12
        d[p + "eval_logits"], d[p + "spread.eval_logits"] = npy(e64), np.float64(spread(e32, e64))
    print("  %-8s %d parameters, loss %.6f (fp32 %s), spread out %.1e gP %.1e" % (
        name, int(d[p + "nparams"]), float(loss64), d[p + "loss32"], d[p + "spread.out"], d[p + "spread.gP"]))


def main():
    for name in G.CASES:
        d = {}
        case(name, d)
        f = "mingpt_gpt_%s.npz" % name
        save(f, d)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
