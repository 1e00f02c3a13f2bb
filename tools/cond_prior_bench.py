#!/usr/bin/env python3
"""The conditional code prior (trainers/cond_prior.py, csrc/cond.hip) on one GPU, one JSON line per measurement, device events
around windows of calls, every side warmed up, the sides of a comparison alternating window by window, medians over --windows:

  step        ConditionalPriorTrainer.training_step({'ids', 'cond'}) of the default model (12 layers, 8 heads, 256 wide), B = 32,
              T = Tc = 256 (block size 512, n_unmasked 256), V = 1024, L = 2, pkeep 0.9, AdamW with the clip, beside
              full_head    the same step with ln_f, the head and the logits on all 512 positions (GPT.forward and a slice) in place
                           of GPT.forward_tail: what the tail saves
              uncond       PriorTrainer.training_step({'ids'}) of the unconditional default model (block size 256): the step without
                           the prefix
              torch        the conditional step in plain torch on the same GPU: the test restatement's model
                           (tests/cond_prior_ref.py) under torch.optim.AdamW and clip_grad_norm_
  cell_labels ops.cell_labels at 4 x 512 x 512 onto a 16 x 16 latent, L = 2, in torch.uint8 and torch.long: microseconds per call
              beside the byte floor - the bytes of the map over the HBM rate --hbm-tbs (TB/s)
  synthesize  ConditionalPriorTrainer.synthesize of ONE slice, 8 candidates, top-k 32, top-p 0.95 on the 16 x 16 latent (V = 1024;
              a small VQGAN decodes): ms per call

  --guidance  classifier-free guidance, in place of the measurements above: synthesize as above on a model with the null embedding
              at guidance scale 1 (the unguided route: the code the model without a null embedding runs, measured beside it as
              `plain`) and at scale 3 (one cache of 16 rows, one sampler launch and one decode step per position), with the
              per-position time = ms / 256; and the two sampler launches alone at B = 8, V = 1024, top-k 32, top-p 0.95:
              ops.sample_filtered on 8 rows against ops.sample_guided on 8 pairs of rows, microseconds per launch

    python tools/cond_prior_bench.py [--steps 10] [--warmup 3] [--windows 5] [--batch 32] [--hbm-tbs 8.0] [--guidance] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

V, T, L, N_LAYER, N_HEAD, N_EMBED = 1024, 256, 2, 12, 8, 256
OPTIM = dict(lr=4.5e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
CLIP, PKEEP = 1.0, 0.9


def window(fn, steps):
    """ms per call of `steps` calls between two device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(sides, args, what, steps=None):
    steps = steps or args.steps
    for fn in sides.values():
        window(fn, args.warmup)
    times = {n: [] for n in sides}
    for _ in range(args.windows):
        for n, fn in sides.items():
            times[n].append(window(fn, steps))
    rec = dict(what=what, steps=steps, windows=args.windows)
    for n, ts in times.items():
        rec[n + "_ms"] = round(statistics.median(ts), 5)
        rec[n + "_ms_windows"] = [round(t, 5) for t in ts]
    return rec


def small_vqgan():
    from networks import VQGAN
    return VQGAN(1, 32, 1, 32, V, (1, 2), (1, 2), 1, [], [], 32, 0.0, True, "torch")          # 32 x 32 pictures, a 16 x 16 latent


def build_trainers(batch):
    import torch
    from networks import GPT, LabelCondition
    from trainers import ConditionalPriorTrainer, PriorTrainer
    kw = dict(pkeep=PKEEP, lr=OPTIM["lr"], betas=OPTIM["betas"], weight_decay=OPTIM["weight_decay"], grad_norm_clip=CLIP, device="cuda")
    torch.manual_seed(0)
    gpt = GPT(V, 2 * T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED, n_unmasked=T)
    cond_tr = ConditionalPriorTrainer(small_vqgan(), gpt, LabelCondition(L, N_EMBED, 16, 16), **kw)
    state = {k: v.detach().clone() for k, v in gpt.state_dict().items()}
    state["cond.embed.weight"] = cond_tr.cond.embed.weight.detach().clone()
    torch.manual_seed(0)
    full = ConditionalPriorTrainer(small_vqgan(), GPT(V, 2 * T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED, n_unmasked=T),
                                   LabelCondition(L, N_EMBED, 16, 16), **kw)
    full._logits = lambda inp, prefix: full.gpt(inp, embeddings=prefix)[:, prefix.shape[1]:]          # the head on all 512 positions
    torch.manual_seed(0)
    plain = PriorTrainer(small_vqgan(), GPT(V, T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED), **kw)
    ids = torch.randint(0, V, (batch, T), device="cuda")
    cond = torch.randint(0, L, (batch, T), device="cuda")
    both = {"ids": ids, "cond": cond}
    return {"cond": lambda: cond_tr.training_step(both), "full_head": lambda: full.training_step(both),
            "uncond": lambda: plain.training_step({"ids": ids})}, state, ids, cond, cond_tr


def build_torch(state, ids, cond):
    import torch
    import cond_prior_ref as C
    import prior_ref as P
    st = {k: (v.detach().clone().cuda() if k.endswith("mask") else v.detach().clone().cuda().requires_grad_(True)) for k, v in state.items()}
    names = [k for k in st if not k.endswith("mask")]
    params = [st[k] for k in names]
    decayed = [k for k in names if k != C.TABLE and P.decays(k)]
    opt = torch.optim.AdamW([{"params": [st[k] for k in decayed], "weight_decay": OPTIM["weight_decay"]},
                             {"params": [st[k] for k in names if k not in decayed], "weight_decay": 0.0}],
                            lr=OPTIM["lr"], betas=OPTIM["betas"], eps=OPTIM["eps"])
    gen = torch.Generator(device="cuda").manual_seed(0)

    def step():
        u_keep, u_rand = torch.rand(ids.shape, generator=gen, device="cuda"), torch.rand(ids.shape, generator=gen, device="cuda")
        inp = P.tokens_ref(ids, 0, PKEEP, V, u_keep, u_rand)
        logits = C.cond_logits(st, inp, cond, N_LAYER, N_HEAD)
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), ids.reshape(-1))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
    return step


def guidance_lines(args):
    import torch
    from hipops import ops
    from networks import GPT, LabelCondition
    from trainers import ConditionalPriorTrainer
    trainers = {}
    for name, null in (("plain", False), ("null", True)):
        torch.manual_seed(0)
        gpt = GPT(V, 2 * T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED, n_unmasked=T)
        trainers[name] = ConditionalPriorTrainer(small_vqgan(), gpt, LabelCondition(L, N_EMBED, 16, 16, null_token=null), device="cuda")
    one = torch.randint(0, L, (1, T), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    kw = dict(cond=one, n_candidates=8, top_k=32, top_p=0.95, generator=gen)
    sides = {"plain": lambda: trainers["plain"].synthesize(**kw),
             "scale1": lambda: trainers["null"].synthesize(guidance_scale=1.0, **kw),
             "scale3": lambda: trainers["null"].synthesize(guidance_scale=3.0, **kw)}
    rec = measure(sides, args, "synthesize one slice, 8 candidates, top-k 32, top-p 0.95, 16 x 16 latent: no null row / scale 1 / scale 3", steps=2)
    for n in sides:
        rec[n + "_per_position_us"] = round(1e3 * rec[n + "_ms"] / T, 3)
    rec["scale1_over_plain"] = round(rec["scale1_ms"] / rec["plain_ms"], 4)
    rec["scale3_over_scale1"] = round(rec["scale3_ms"] / rec["scale1_ms"], 4)
    lines = [rec]
    B = 8
    z = torch.randn(2 * B, V, device="cuda")
    zc = z[:B].contiguous()
    u = torch.rand(B, device="cuda")
    launches = {"sample_filtered": lambda: ops.sample_filtered(zc, u, None, 1.0, 32, 0.95),
                "sample_guided": lambda: ops.sample_guided(z, u, 3.0, None, 1.0, 32, 0.95)}
    rec = measure(launches, args, "one sampler launch, B=%d V=%d, top-k 32, top-p 0.95: 8 rows against 8 guided pairs" % (B, V), steps=200)
    for n in launches:
        rec[n + "_us"] = round(1e3 * rec[n + "_ms"], 3)
    lines.append(rec)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--guidance", action="store_true", help="measure classifier-free guidance in place of the default measurements")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from hipops import ops
    if not torch.cuda.is_available():
        raise SystemExit("cond_prior_bench.py measures on a GPU; none is available")
    if args.guidance:
        lines = guidance_lines(args)
        for rec in lines:
            print(json.dumps(rec))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")
        return
    lines = []
    sides, state, ids, cond, cond_tr = build_trainers(args.batch)
    sides["torch"] = build_torch(state, ids, cond)
    rec = measure(sides, args, "training step B=%d T=Tc=%d V=%d L=%d, %d layers %d wide" % (args.batch, T, V, L, N_LAYER, N_EMBED))
    rec["tail_saves_ms"] = round(rec["full_head_ms"] - rec["cond_ms"], 5)
    rec["cond_over_uncond"] = round(rec["cond_ms"] / rec["uncond_ms"], 4)
    rec["torch_over_cond"] = round(rec["torch_ms"] / rec["cond_ms"], 4)
    lines.append(rec)

    maps = {}
    for name, dtype in (("uint8", torch.uint8), ("long", torch.long)):
        lab = (torch.rand(4, 512, 512, device="cuda") < 0.1).to(dtype)
        maps[name] = (lambda lab=lab: ops.cell_labels(lab, 16, 16, L))
    rec = measure(maps, args, "cell_labels 4 x 512 x 512 -> 16 x 16, L=%d" % L, steps=200)
    for name, nbytes in (("uint8", 4 * 512 * 512), ("long", 8 * 4 * 512 * 512)):
        rec[name + "_us"] = round(1e3 * rec[name + "_ms"], 3)
        rec[name + "_floor_us"] = round(nbytes / (args.hbm_tbs * 1e12) * 1e6, 3)
    lines.append(rec)

    one = cond[:1].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(0)
    syn = {"synthesize": lambda: cond_tr.synthesize(cond=one, n_candidates=8, top_k=32, top_p=0.95, generator=gen)}
    lines.append(measure(syn, args, "synthesize one slice, 8 candidates, top-k 32, top-p 0.95, 16 x 16 latent", steps=2))
    for rec in lines:
        print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
