#!/usr/bin/env python3
"""The label-conditioned masked code prior (trainers/masked_cond_prior.py, csrc/cond.hip vqw_embed_cond_fwd) on one GPU, one JSON
line per measurement, device events around windows of calls, every side warmed up, the sides of a comparison alternating window by
window, medians over --windows, one process:

  embedding   ops.embedding_cond at B x T x E = 32 x 256 x 256 (V = 1024 + the mask token, 2 labels + the null row) beside the
              three launches it replaces, ops.embedding + ops.embedding_lookup and the ATen add: microseconds per forward
  step        ConditionalMaskedPriorTrainer.training_step({'ids', 'cond'}) of the default model (12 layers, 8 heads, 256 wide),
              B = 32, T = 256, V = 1024, p_uncond 0.1, beside MaskedPriorTrainer.training_step (unconditional) and
              ConditionalPriorTrainer.training_step (autoregressive, the condition as a prefix of 256 tokens, p_uncond 0.1) in the
              same session
  synthesize  ONE slice from its label map, 8 candidates, top-k 32, top-p 0.95 on the 16 x 16 latent (V = 64; a small VQGAN decodes):
              the masked prior in 8 passes at guidance scale 1 and 3 beside the autoregressive conditional prior at the same scales
  edit        edit(new_label=...) of ONE slice for a disc in the central quarter of the label map, 8 candidates, both priors, at
              scale 1 and 3

    python tools/masked_cond_bench.py [--steps 10] [--warmup 3] [--windows 5] [--batch 32] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from masked_prior_bench import CLIP, N_EMBED, N_HEAD, N_LAYER, OPTIM, PKEEP, T, V, V_EDIT, measure, small_vqgan      # noqa: E402

N_LABELS, P_UNCOND, N_PASSES, SIDE = 2, 0.1, 8, 16


def build_trainers(vocab):
    """(conditional masked, unconditional masked, autoregressive conditional) trainers of the default size over `vocab` codes"""
    import torch
    from networks import GPT, LabelCondition, MaskedGPT
    from trainers import ConditionalMaskedPriorTrainer, ConditionalPriorTrainer, MaskedPriorTrainer
    kw = dict(lr=OPTIM["lr"], betas=OPTIM["betas"], weight_decay=OPTIM["weight_decay"], grad_norm_clip=CLIP, device="cuda")
    size = dict(n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED)
    drop = dict(p_uncond=P_UNCOND, cond_drop_seed=0)
    cond = lambda: LabelCondition(N_LABELS, N_EMBED, SIDE, SIDE, null_token=True)          # noqa: E731
    torch.manual_seed(0)
    masked_cond = ConditionalMaskedPriorTrainer(small_vqgan(vocab), MaskedGPT(vocab, T, **size), cond(), n_steps=N_PASSES, **drop, **kw)
    torch.manual_seed(0)
    masked = MaskedPriorTrainer(small_vqgan(vocab), MaskedGPT(vocab, T, **size), n_steps=N_PASSES, **kw)
    torch.manual_seed(0)
    ar_cond = ConditionalPriorTrainer(small_vqgan(vocab), GPT(vocab, 2 * T, n_unmasked=T, **size), cond(), pkeep=PKEEP, **drop, **kw)
    return masked_cond, masked, ar_cond


def embedding_line(args):
    import torch
    from hipops import ops
    B = args.batch
    idx = torch.randint(0, V + 1, (B, T), device="cuda")
    cidx = torch.randint(0, N_LABELS, (B, T), device="cuda")
    tok, pos, ctab = torch.randn(V + 1, N_EMBED, device="cuda"), torch.randn(1, T, N_EMBED, device="cuda"), torch.randn(N_LABELS + 1, N_EMBED, device="cuda")
    sides = {"embedding_cond": lambda: ops.embedding_cond(idx, tok, pos, cidx, ctab),
             "three_launches": lambda: ops.embedding(idx, tok, pos) + ops.embedding_lookup(cidx, ctab)}
    rec = measure(sides, args, "conditioned embedding forward, B x T x E = %d x %d x %d (with the operators' allocations)" % (B, T, N_EMBED), steps=200)
    for n in sides:
        rec[n + "_us"] = round(1e3 * rec[n + "_ms"], 3)
    rec["embedding_cond_over_three_launches"] = round(rec["embedding_cond_ms"] / rec["three_launches_ms"], 4)
    return rec


def disc(label, cy, cx, radius, value):
    import torch
    yy, xx = torch.meshgrid(torch.arange(label.shape[-2], device=label.device), torch.arange(label.shape[-1], device=label.device), indexing="ij")
    new = label.clone()
    new[:, (yy - cy) ** 2 + (xx - cx) ** 2 <= radius ** 2] = value
    return new


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
        raise SystemExit("masked_cond_bench.py measures on a GPU; none is available")
    lines = [embedding_line(args)]
    masked_cond, masked, ar_cond = build_trainers(V)
    batch = {"ids": torch.randint(0, V, (args.batch, T), device="cuda"), "cond": torch.randint(0, N_LABELS, (args.batch, T), device="cuda")}
    sides = {"masked_cond": lambda: masked_cond.training_step(batch), "masked": lambda: masked.training_step(batch),
             "autoregressive_cond": lambda: ar_cond.training_step(batch)}
    rec = measure(sides, args, "training step B=%d T=%d V=%d, %d layers %d wide, p_uncond %.1f: conditional masked beside unconditional "
                  "masked and autoregressive conditional" % (args.batch, T, V, N_LAYER, N_EMBED, P_UNCOND))
    rec["masked_cond_over_masked"] = round(rec["masked_cond_ms"] / rec["masked_ms"], 4)
    rec["masked_cond_over_autoregressive_cond"] = round(rec["masked_cond_ms"] / rec["autoregressive_cond_ms"], 4)
    lines.append(rec)

    del masked_cond, masked, ar_cond, sides
    masked_cond, _, ar_cond = build_trainers(V_EDIT)
    label = torch.zeros(1, 2 * SIDE, 2 * SIDE, dtype=torch.long, device="cuda")          # 32 x 32 pixels, cells of 2 x 2
    label = disc(label, 8, 8, 5, 1)
    new = disc(label, SIDE, SIDE, SIDE // 2, 1)          # a disc of radius 8 pixels in the central quarter
    one = {"ids": torch.randint(0, V_EDIT, (1, T), device="cuda"), "label": label}
    gen = torch.Generator(device="cuda").manual_seed(0)
    kw = dict(n_candidates=8, top_k=32, top_p=0.95, generator=gen)
    sides = {}
    for scale in (1.0, 3.0):
        sides["masked_scale%d" % scale] = lambda scale=scale: masked_cond.synthesize(label=label, n_steps=N_PASSES, guidance_scale=scale, **kw)
        sides["autoregressive_scale%d" % scale] = lambda scale=scale: ar_cond.synthesize(label=label, guidance_scale=scale, **kw)
    rec = measure(sides, args, "synthesize one slice from its label map, V=%d, 8 candidates, top-k 32, top-p 0.95, masked in %d passes" % (V_EDIT, N_PASSES),
                  steps=2)
    for scale in (1, 3):
        rec["masked_over_autoregressive_scale%d" % scale] = round(rec["masked_scale%d_ms" % scale] / rec["autoregressive_scale%d_ms" % scale], 4)
    lines.append(rec)
    cells = int(masked_cond.edit(one, new_label=new, n_candidates=1)["cellmask"].sum())
    sides = {}
    for scale in (1.0, 3.0):
        sides["masked_scale%d" % scale] = lambda scale=scale: masked_cond.edit(one, new_label=new, n_steps=N_PASSES, guidance_scale=scale, **kw)
        sides["autoregressive_scale%d" % scale] = lambda scale=scale: ar_cond.edit(one, new_label=new, guidance_scale=scale, **kw)
    rec = measure(sides, args, "edit(new_label) one slice, a disc in the central quarter (%d of %d codes), V=%d, 8 candidates, masked in %d passes" % (
        cells, T, V_EDIT, N_PASSES), steps=2)
    rec["cells"] = cells
    for scale in (1, 3):
        rec["masked_over_autoregressive_scale%d" % scale] = round(rec["masked_scale%d_ms" % scale] / rec["autoregressive_scale%d_ms" % scale], 4)
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
