#!/usr/bin/env python3
"""Generate the golden vectors of the GPT code prior's training step from the upstream reference's own model (networks/mingpt.py:
GPT) under stock torch.optim.AdamW, on minGPT's two parameter groups, and torch.nn.utils.clip_grad_norm_.

Runs ONLY in the build container (needs the reference sources); _refshim.py loads the reference as make_golden_mingpt_gpt.py loads
it.  Output, tensors only:

    tests/golden/prior_step_<case>.npz    <case>/   for the two cases of prior_ref.CASES, (V, block_size, n_layer, n_head, E,
                                          n_unmasked, B, T): p64 = (64, 16, 2, 2, 64, 0, 2, 16), p96 = (64, 16, 2, 3, 96, 3, 2, 16)

Each case: the model built under torch.manual_seed(seed) and brought to gpt_ref.init_gpt_'s state, fixed ids, then
prior_ref.STEPS = 3 steps in train mode with all dropout probabilities 0 - input = the start token in front of ids shifted right,
F.cross_entropy against ids, backward, clip_grad_norm_(model.parameters(), prior_ref.GRAD_NORM_CLIP[case]), AdamW(prior_ref.OPTIM)
- once in fp64, the truth, and in three mathematically identical fp32 evaluations (eight threads, one thread, batch reversed):

    seed, keys (the parameters' names), nparams, init.* (helpers.checksum of every parameter of the state the steps start from -
    the test rebuilds it from the seed), ids, clip, loss64 / norm64 / coef64 [3] (per step: the loss, the pre-clip global gradient
    norm, the clip coefficient), loss32 / norm32 / coef32 [3 variants][3], and per parameter at helpers.sample_idx(numel, 256,
    seed=1): g64.* / g32.* [3 variants] (the UNCLIPPED gradient of step 0), p64.* / p32.* (the parameter after step 3), plus
    gnorm64.* and pnorm64.* (whole-tensor norms); live (the names whose step-0 gradient is not analytically zero)

Asserted here before anything is written: the clip lies between the smallest and the largest of the three fp64 norms; every fp32
evaluation passes helpers.grad_gate at its defaults against the fp64 truth and the three evaluations, on the sampled gradients and
on the sampled parameters; prior_ref.steps_ref equals the reference in fp64 (1e-12 on losses, norms and coefficients, 1e-10 on
gradients, 1e-11 on parameters - 1e-8 on those whose gradient is analytically zero); every file stays below the repository's 1 MiB limit.

    python tests/golden/make_golden_prior_step.py
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
import prior_ref as P  # noqa: E402

torch.set_num_threads(8)
REF = _refshim._load("networks.mingpt", "networks/mingpt.py")


def groups(model, weight_decay):
    """minGPT's configure_optimizers: by module type, not by name"""
    decay, no_decay = set(), set()
    for mn, m in model.named_modules():
        for pn, _ in m.named_parameters(recurse=False):
            fpn = "%s.%s" % (mn, pn) if mn else pn
            if pn.endswith("bias"):
                no_decay.add(fpn)
            elif pn.endswith("weight") and isinstance(m, torch.nn.Linear):
                decay.add(fpn)
            elif pn.endswith("weight") and isinstance(m, (torch.nn.LayerNorm, torch.nn.Embedding)):
                no_decay.add(fpn)
    no_decay.add("pos_embed")
    params = dict(model.named_parameters())
    assert not (decay & no_decay) and (decay | no_decay) == set(params)
    return [{"params": [params[k] for k in sorted(decay)], "weight_decay": weight_decay},
            {"params": [params[k] for k in sorted(no_decay)], "weight_decay": 0.0}], decay


def run(model, ids, dtype, clip, threads=8, rev=False):
    m = copy.deepcopy(model).to(dtype).train()
    if rev:
        ids = ids.flip(0)
    o = P.OPTIM
    gr, decay = groups(m, o["weight_decay"])
    opt = torch.optim.AdamW(gr, lr=o["lr"], betas=o["betas"], eps=o["eps"])
    out = dict(loss=[], norm=[], coef=[], decay=decay)
    torch.set_num_threads(threads)
    try:
        for s in range(P.STEPS):
            inp = torch.cat((torch.full_like(ids[:, :1], P.SOS), ids[:, :-1]), dim=1)
            logits = m(inp)
            loss = F.cross_entropy(logits.view(-1, logits.shape[-1]), ids.reshape(-1))
            opt.zero_grad()
            loss.backward()
            if s == 0:
                out["g0"] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
            norm = torch.nn.utils.clip_grad_norm_(m.parameters(), clip)
            opt.step()
            out["loss"].append(float(loss.detach()))
            out["norm"].append(float(norm))
            out["coef"].append(float(torch.clamp(clip / (norm + 1e-6), max=1.0)))
    finally:
        torch.set_num_threads(8)
    out["P"] = {k: p.detach().clone() for k, p in m.named_parameters()}
    return out


def sampled(d):
    return {k: t.reshape(-1)[sample_idx(t.numel(), 256, seed=1)] for k, t in d.items()}


def case(name, d):
    seed, clip = P.SEEDS[name], P.GRAD_NORM_CLIP[name]
    torch.manual_seed(seed)
    model = REF.GPT(**P.gpt_kwargs(name))
    G.init_gpt_(model, seed)
    ids = P.case_ids(name, seed)
    truth = run(model, ids, torch.float64, clip)
    variants = [run(model, ids, torch.float32, clip), run(model, ids, torch.float32, clip, threads=1),
                run(model, ids, torch.float32, clip, rev=True)]
    assert min(truth["norm"]) < clip < max(truth["norm"]), (name, truth["norm"], clip)
    assert sorted(k for k in truth["P"] if P.decays(k)) == sorted(truth["decay"]), "prior_ref.decays differs from minGPT's rule"
    assert all([c < 1 for c in v["coef"]] == [c < 1 for c in truth["coef"]] for v in variants)
    for what in ("g0", "P"):          # the reference's own fp32 evaluations stay within the gate, on what the test will see
        t64, v32 = sampled(truth[what]), [sampled(v[what]) for v in variants]
        for i, v in enumerate(v32):
            grad_gate(t64, v32, v, what="%s %s variant %d" % (name, what, i))
    # the restatement is the same mathematics
    r = P.steps_ref(name, model.state_dict(), ids, torch.float64, clip)
    for q in ("loss", "norm", "coef"):
        assert max(abs(a - b) / abs(b) for a, b in zip(r[q], truth[q])) < 1e-12, (name, q)
    gmax = max(float(g.norm()) for g in truth["g0"].values())
    live = [k for k, g in truth["g0"].items() if float(g.norm()) >= 1e-6 * gmax]
    assert max(spread(r["g0"][k], truth["g0"][k]) for k in live) < 1e-10, name
    # (a parameter whose gradient is analytically zero - every att.k.bias - moves by Adam's m / (sqrt(v) + eps) of rounding noise:
    # 1e-17 / 1e-8 in fp64, and the two evaluations' noise differs)
    for k in truth["P"]:
        assert spread(r["P"][k], truth["P"][k]) < (1e-11 if k in live else 1e-8), (name, k, spread(r["P"][k], truth["P"][k]))
    p = name + "/"
    keys = list(truth["P"])
    d[p + "seed"], d[p + "keys"], d[p + "live"] = np.array(seed), np.array(keys), np.array(live)
    d[p + "nparams"] = np.array(sum(q.numel() for q in model.parameters()))
    d[p + "ids"], d[p + "clip"] = npy(ids), np.float64(clip)
    for q in ("loss", "norm", "coef"):
        d[p + q + "64"] = np.array(truth[q], dtype=np.float64)
        d[p + q + "32"] = np.array([v[q] for v in variants], dtype=np.float64)
    for k, t in model.named_parameters():
        d[p + "init." + k] = checksum(t)
    for what, tag in (("g0", "g"), ("P", "p")):
        t64, v32 = sampled(truth[what]), [sampled(v[what]) for v in variants]
        for k in keys:
            d[p + tag + "64." + k] = npy(t64[k])
            d[p + tag + "32." + k] = np.stack([npy(v[k]) for v in v32])
            d[p + tag + "norm64." + k] = np.float64(truth[what][k].norm())
    print("  %-4s %d parameters, loss %s, norm %s, coef %s" % (name, int(d[p + "nparams"]), truth["loss"], truth["norm"], truth["coef"]))
    for q in ("loss", "norm", "coef"):
        print("       %s: fp32 - fp64 relative %s" % (q, np.abs(d[p + q + "32"] - d[p + q + "64"]).max(axis=0) / np.abs(d[p + q + "64"])))


def main():
    for name in P.CASES:
        d = {}
        case(name, d)
        f = "prior_step_%s.npz" % name
        save(f, d)
        assert os.path.getsize(os.path.join(os.environ.get("GOLDEN_OUT", HERE), f)) <= 1 << 20, f + " exceeds 1 MiB"


if __name__ == "__main__":
    main()
