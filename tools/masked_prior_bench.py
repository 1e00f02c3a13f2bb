#!/usr/bin/env python3
"""The bidirectional masked code prior (trainers/masked_prior.py, csrc/masked_prior.hip) on one GPU, one JSON line per measurement,
device events around windows of calls, every side warmed up, the sides of a comparison alternating window by window, medians over
--windows:

  launches    ops.mask_tokens and ops.unmask_step (gamma 0.5, tau 2.25, half of every row masked) at B x T = 32 x 256 and
              64 x 4096: microseconds per launch
  step        MaskedPriorTrainer.training_step({'ids'}) of the default model (12 layers, 8 heads, 256 wide), B = 32, T = 256,
              V = 1024, AdamW with the clip, beside PriorTrainer.training_step of the autoregressive model of the same size (pkeep
              0.9) in the same session
  edit        MaskedPriorTrainer.edit of ONE slice, 8 candidates, top-k 32, top-p 0.95 on the 16 x 16 latent (V = 64, the vocabulary
              of tools/prior_edit_bench.py's figures; a small VQGAN decodes) with n_steps in {8, 12, 16}, beside PriorTrainer.edit (one
              cached decode step per position from the first redrawn one) on the same region, for three regions: the central
              quarter, the whole latent, the last two rows: ms per call

    python tools/masked_prior_bench.py [--steps 10] [--warmup 3] [--windows 5] [--batch 32] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

V, V_EDIT, T, N_LAYER, N_HEAD, N_EMBED = 1024, 64, 256, 12, 8, 256
OPTIM = dict(lr=4.5e-4, betas=(0.9, 0.95), weight_decay=0.01)
CLIP, PKEEP = 1.0, 0.9
N_STEPS = (8, 12, 16)
REGIONS = {"central_quarter": (8, 24, 8, 24), "whole_latent": (0, 32, 0, 32), "last_two_rows": (28, 32, 0, 32)}      # pixel boxes, 2 x 2 cells


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


def small_vqgan(vocab):
    from networks import VQGAN
    return VQGAN(1, 32, 1, 32, vocab, (1, 2), (1, 2), 1, [], [], 32, 0.0, True, "torch")          # 32 x 32 pictures, a 16 x 16 latent


def build_trainers(vocab):
    import torch
    from networks import GPT, MaskedGPT
    from trainers import MaskedPriorTrainer, PriorTrainer
    kw = dict(lr=OPTIM["lr"], betas=OPTIM["betas"], weight_decay=OPTIM["weight_decay"], grad_norm_clip=CLIP, device="cuda")
    torch.manual_seed(0)
    masked = MaskedPriorTrainer(small_vqgan(vocab), MaskedGPT(vocab, T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED), **kw)
    torch.manual_seed(0)
    plain = PriorTrainer(small_vqgan(vocab), GPT(vocab, T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED), pkeep=PKEEP, **kw)
    return masked, plain


def launch_lines(args):
    import torch
    from hipops import ops
    lines = []
    for B, Tn in ((32, 256), (64, 4096)):
        ids = torch.randint(0, V, (B, Tn), device="cuda")
        logp = -torch.rand(B, Tn, device="cuda") * 5
        u = torch.rand(B, Tn, device="cuda")
        masked = ops.mask_tokens(ids, V, 0, 0, ratio=0.5)[1]
        m0 = torch.full((B,), Tn, dtype=torch.int32, device="cuda")
        fixed = torch.zeros(B, Tn, device="cuda")
        sides = {"mask_tokens": lambda ids=ids: ops.mask_tokens(ids, V, 0, 1),
                 "unmask_step": lambda ids=ids, logp=logp, masked=masked, m0=m0, u=u, fixed=fixed:
                     ops.unmask_step(ids, logp, masked, m0, 0.5, 2.25, V, u=u, fixed_logp=fixed)}
        rec = measure(sides, args, "one launch, B x T = %d x %d (with the operator's allocations)" % (B, Tn), steps=200)
        for n in sides:
            rec[n + "_us"] = round(1e3 * rec[n + "_ms"], 3)
        lines.append(rec)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("masked_prior_bench.py measures on a GPU; none is available")
    lines = launch_lines(args)
    masked, plain = build_trainers(V)
    ids = torch.randint(0, V, (args.batch, T), device="cuda")
    sides = {"masked": lambda: masked.training_step({"ids": ids}), "autoregressive": lambda: plain.training_step({"ids": ids})}
    rec = measure(sides, args, "training step B=%d T=%d V=%d, %d layers %d wide: masked beside autoregressive" % (args.batch, T, V, N_LAYER, N_EMBED))
    rec["masked_over_autoregressive"] = round(rec["masked_ms"] / rec["autoregressive_ms"], 4)
    lines.append(rec)

    del masked, plain, sides
    masked, plain = build_trainers(V_EDIT)
    one = torch.randint(0, V_EDIT, (1, T), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    kw = dict(n_candidates=8, top_k=32, top_p=0.95, generator=gen)
    for region, box in REGIONS.items():
        sides = {"autoregressive": lambda box=box: plain.edit({"ids": one}, box=box, **kw)}
        for n in N_STEPS:
            sides["masked_%d" % n] = lambda box=box, n=n: masked.edit({"ids": one}, box=box, n_steps=n, **kw)
        y0, y1, x0, x1 = box
        cells = (y1 - y0) // 2 * ((x1 - x0) // 2)
        rec = measure(sides, args, "edit one slice, %s (%d of %d codes), V=%d, 8 candidates, top-k 32, top-p 0.95" % (region, cells, T, V_EDIT), steps=2)
        rec["cells"] = cells
        for n in N_STEPS:
            rec["masked_%d_over_autoregressive" % n] = round(rec["masked_%d_ms" % n] / rec["autoregressive_ms"], 4)
        lines.append(rec)
    for rec in lines:
        print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
