#!/usr/bin/env python3
"""Generate the golden vectors of the VQGAN's Downsample, Encoder and VQGAN from the upstream reference's own modules
(networks/vqgan.py), by the method of make_golden_vqgan_blocks.py.

Runs ONLY in the build container (needs the reference sources).  Output, tensors only:

    tests/golden/vqgan_model_<case>.npz   <case>/  for the three cases of vqgan_model_ref.CASES: down64 = Downsample(64, True) on
                                          2 x 64 x 16 x 16; encoder = Encoder(1, 32, 32, (1, 2), 1, [16], 32, 0.0, True) and
                                          vqgan = VQGAN(1, 32, 1, 32, 8, (1, 2), (1, 2), 1, [16], [16], 32, 0.0, True, 'torch') on
                                          2 x 1 x 32 x 32

Each case, in train mode, forward plus backward of sum <output, weight_pattern(shape)> (the VQGAN: sum <recon, weight_pattern> +
commit_loss), once in fp64 - the truth - and in three mathematically identical fp32 evaluations (eight threads, one thread,
channels_last).  Keys as in vqgan_blocks_*.npz:

    seed, keys (state_dict order), nparams, in, P.* (the state before the step), out, gin, g64.* / gnorm64.* / gerr32.* (gradient
    samples at helpers.sample_idx(numel, 256, seed=1), norms, the fp32 evaluations' distances), live, spread.{out,gin,gP}

and for the VQGAN: out is recon; commit, ids, emb, gap (the fp64 relative top-1 / top-2 distance gap (d2 - d1) / d1 per pixel, in
the layout of ids), buf.{embed,cluster_size,embed_avg} (the three VQ buffers after the step), gen_out (generate_image_from_ids(ids)
in eval mode on the state before the step), spread.{commit,emb,buf.*,gen_out}, nparams_default (the default VQGAN()'s count).

Parameters as vqgan_ref.init_case_ leaves them (multiples of 1/64); the codebook is round64(randn(8, 32) / 4) from a generator
seeded with seed + 3000, embed_avg its transpose.  Asserted here: the reference's fp32 evaluations alone pass helpers.grad_gate;
for the VQGAN all 8 codes are in use, the smallest relative gap is at least 1e-4 and all three fp32 evaluations give the fp64 ids
on every pixel - the seed is searched from vqgan_model_ref.SEEDS["vqgan"] upwards until that holds, and the one found must be the
one recorded there.

    python tests/golden/make_golden_vqgan_model.py
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
import vqgan_model_ref as M  # noqa: E402

torch.set_num_threads(8)
REF = _refshim._load("networks.vqgan", "networks/vqgan.py")
MIN_GAP = 1e-4


def run(name, module, x, fmt=None):
    m = copy.deepcopy(module).to(x.dtype).train()
    if fmt is not None:
        m = m.to(memory_format=fmt)
        x = x.contiguous(memory_format=fmt)
    xin = x.clone().requires_grad_(True)
    if name == "vqgan":
        recon, commit, ids, emb = m(xin)
        res = dict(out=recon.detach(), commit=commit.detach(), ids=ids, emb=emb.detach(),
                   buf={k: getattr(m.vq, k).detach().clone() for k in ("embed", "cluster_size", "embed_avg")})
        loss = (recon * weight_pattern(recon.shape, x.dtype)).sum() + commit
    else:
        out = m(xin)
        res = dict(out=out.detach())
        loss = (out * weight_pattern(out.shape, x.dtype)).sum()
    loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = xin.grad
    return res, grads


def evaluate(name, seed):
    cls, args, _ = M.CASES[name]
    torch.manual_seed(seed)
    module = M.init_case_(getattr(REF, cls)(*args), name, seed)
    x = M.case_input(name, seed)
    r64, truth = run(name, module, x.double())
    r32, v0 = run(name, module, x)
    torch.set_num_threads(1)
    try:
        r1, v1 = run(name, module, x)
    finally:
        torch.set_num_threads(8)
    r2, v2 = run(name, module, x, torch.channels_last)
    return module, x, r64, truth, [r32, r1, r2], [v0, v1, v2]


def vqgan_conditions(module, x, r64, runs):
    """None if the draw is usable, else the reason it is not."""
    with torch.no_grad():
        ref = M.vqgan_forward_ref(x.double(), {k: v.double() for k, v in module.state_dict().items()}, training=True)
    assert torch.equal(ref["ids"], r64["ids"]), "the restatement's ids differ from the reference's in fp64"
    if len(torch.unique(r64["ids"])) != module.vq.dict_size:
        return "%d of %d codes in use" % (len(torch.unique(r64["ids"])), module.vq.dict_size)
    if float(ref["gap"].min()) < MIN_GAP:
        return "smallest relative gap %.2e" % float(ref["gap"].min())
    if not all(torch.equal(r["ids"], r64["ids"]) for r in runs):
        return "an fp32 evaluation's ids differ from the fp64 ids"
    return None


def case(name, d):
    seed = M.SEEDS[name]
    if name == "vqgan":                      # the first seed from the recorded one on that meets the conditions
        for s in range(seed, seed + 40):
            module, x, r64, truth, runs, variants = evaluate(name, s)
            why = vqgan_conditions(module, x, r64, runs)
            if why is None:
                break
            print("  vqgan seed %d: %s" % (s, why))
        assert why is None and s == seed, "vqgan_model_ref.SEEDS['vqgan'] must be %d" % s
    else:
        module, x, r64, truth, runs, variants = evaluate(name, seed)
    for i, v in enumerate(variants):          # the reference's own fp32 evaluations stay within the cap
        grad_gate(truth, variants, v, what="%s variant %d" % (name, i))
    gmax = max(float(g.norm()) for g in truth.values())
    live = [k for k, g in truth.items() if float(g.norm()) >= 1e-6 * gmax]
    # the restatement is the same mathematics
    q64, rg = M.grads_ref(name, module.state_dict(), x, torch.float64)
    assert spread(q64["recon" if name == "vqgan" else "out"], r64["out"]) < 1e-12, name
    assert max(spread(rg[k], truth[k]) for k in live) < 1e-10, name
    r32, v0 = runs[0], variants[0]
    p = name + "/"
    sd = module.state_dict()
    d[p + "seed"], d[p + "keys"] = np.array(seed), np.array(list(sd))
    d[p + "nparams"] = np.array(sum(q.numel() for q in module.parameters()))
    d[p + "in"], d[p + "out"], d[p + "gin"] = npy(x), npy(r32["out"]), npy(v0["input"])
    for k, t in sd.items():
        d[p + "P." + k] = npy(t).copy()
    for k, g in truth.items():
        idx = sample_idx(g.numel(), 256, seed=1)
        d[p + "g64." + k] = npy(g.reshape(-1)[idx])
        d[p + "gnorm64." + k] = np.float64(g.norm())
        d[p + "gerr32." + k] = np.array([float((v[k].double() - g).norm() / g.norm()) for v in variants])
    d[p + "live"] = np.array(live)
    d[p + "spread.out"] = np.float64(spread(r32["out"], r64["out"]))
    d[p + "spread.gin"] = np.float64(spread(v0["input"], truth["input"]))
    d[p + "spread.gP"] = np.float64(max(spread(v0[k], truth[k]) for k in live if k != "input"))
    msg = ""
    if name == "vqgan":
        d[p + "commit"], d[p + "ids"], d[p + "emb"] = npy(r32["commit"]), npy(r64["ids"]), npy(r32["emb"])
        d[p + "gap"] = npy(q64["gap"])
        d[p + "spread.commit"] = np.float64(spread(r32["commit"], r64["commit"]))
        d[p + "spread.emb"] = np.float64(spread(r32["emb"], r64["emb"]))
        for k in ("embed", "cluster_size", "embed_avg"):
            d[p + "buf." + k] = npy(r32["buf"][k])
            d[p + "spread.buf." + k] = np.float64(spread(r32["buf"][k], r64["buf"][k]))
            assert spread(q64["buffers"][k], r64["buf"][k]) < 1e-12, k
        with torch.no_grad():
            g32 = copy.deepcopy(module).eval().generate_image_from_ids(r64["ids"])
            g64 = copy.deepcopy(module).double().eval().generate_image_from_ids(r64["ids"])
            assert spread(M.generate_ref(r64["ids"], {k: v.double() for k, v in sd.items()}), g64) < 1e-12
        d[p + "gen_out"], d[p + "spread.gen_out"] = npy(g32), np.float64(spread(g32, g64))
        torch.manual_seed(0)
        d[p + "nparams_default"] = np.array(sum(q.numel() for q in REF.VQGAN().parameters()))
        msg = ", smallest gap %.1e, default VQGAN %d parameters" % (float(q64["gap"].min()), int(d[p + "nparams_default"]))
    print("  %-8s %d parameters, spread out %.1e gin %.1e gP %.1e%s" % (name, int(d[p + "nparams"]), d[p + "spread.out"],
                                                                       d[p + "spread.gin"], d[p + "spread.gP"], msg))


def main():
    for name in M.CASES:
        d = {}
        case(name, d)
        f = "vqgan_model_%s.npz" % name
        save(f, d)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
