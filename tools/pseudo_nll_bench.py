#!/usr/bin/env python3
"""The pseudo-likelihood map of the masked code prior (MaskedGPT.pseudo_nll, csrc/pseudo_nll.hip) on one GPU, one JSON line per
measurement, device events around windows of calls, every side warmed up, the sides of a comparison alternating window by window,
medians over --windows, one process:

  kernels     ops.lattice_inputs and ops.lattice_gather_ln alone at the default model's chunk: B = 4, a 16 x 16 latent, stride (4, 4),
              the 16 passes of a sample side by side (64 rows x 256 positions x 256 wide), microseconds per call; beside the gather,
              ops.layer_norm over all 64 x 256 rows, which it keeps the head from needing
  map         MaskedGPT.pseudo_nll of the default model (12 layers, 8 heads, 256 wide, V = 1024), B = 4, at the strides (2, 2),
              (4, 4) and (16, 16), max_rows 64, beside the same map composed from the existing operators - per chunk
              ops.lattice_inputs, a full forward with the head over every row, ops.cross_entropy and torch indexing - and beside the
              autoregressive PriorTrainer.token_nll of the same batch
  detect      MaskedPriorTrainer.detect_pseudo of ONE slice (V = 64, a small VQGAN decodes; 8 candidates, 8 passes, top-k 32, top-p
              0.95, stride (2, 2)) beside the autoregressive PriorTrainer.detect, the thresholds at the median of each map

    python tools/pseudo_nll_bench.py [--steps 10] [--warmup 3] [--windows 5] [--batch 4] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from masked_prior_bench import N_EMBED, T, V, V_EDIT, build_trainers, measure      # noqa: E402

SIDE, MAX_ROWS = 16, 64
STRIDES = ((2, 2), (4, 4), (16, 16))


def kernel_line(args):
    import torch
    from hipops import ops
    B, stride, ns = args.batch, (4, 4), 16
    ids = torch.randint(0, V, (B, T), device="cuda")
    x = torch.randn(B * ns, T, N_EMBED, device="cuda")
    gamma, beta, y = torch.ones(N_EMBED, device="cuda"), torch.zeros(N_EMBED, device="cuda"), torch.empty(B, T, N_EMBED, device="cuda")
    with torch.no_grad():
        sides = {"lattice_inputs": lambda: ops.lattice_inputs(ids, (SIDE, SIDE), stride, 0, ns, V),
                 "lattice_gather_ln": lambda: ops.lattice_gather_ln(x, gamma, beta, y, (SIDE, SIDE), stride, 0, ns),
                 "layer_norm_all_rows": lambda: ops.layer_norm(x, gamma, beta)}
        rec = measure(sides, args, "the two kernels alone, B=%d, %d x %d latent, stride %s, %d passes side by side (%d x %d x %d), with the "
                      "operators' allocations" % (B, SIDE, SIDE, stride, ns, B * ns, T, N_EMBED), steps=200)
    for n in sides:
        rec[n + "_us"] = round(1e3 * rec[n + "_ms"], 3)
    return rec


def composed_map(gpt, ids, stride, max_rows):
    """pseudo_nll from the existing operators: per chunk a full forward with the head over all rows, the cross-entropy of all rows
    and torch indexing"""
    import torch
    from hipops import ops
    B = ids.shape[0]
    sy, sx = stride
    S, per = sy * sx, max(1, max_rows // B)
    t = torch.arange(T, device=ids.device)
    grp = ((t // SIDE) % sy) * sx + (t % SIDE) % sx
    out = torch.empty(B, T, device=ids.device)
    with torch.no_grad():
        for s0 in range(0, S, per):
            ns = min(per, S - s0)
            inp = ops.lattice_inputs(ids, (SIDE, SIDE), stride, s0, ns, gpt.mask_token)
            nll = ops.cross_entropy(gpt(inp), ids.repeat_interleave(ns, dim=0), reduction="none").view(B, ns, T)
            mine = (grp >= s0) & (grp < s0 + ns)
            out[:, mine] = nll[:, grp[mine] - s0, t[mine]]
    return out.view(B, SIDE, SIDE)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_nll_bench.py measures on a GPU; none is available")
    lines = [kernel_line(args)]

    masked, plain = build_trainers(V)
    masked.gpt.eval()
    ids = torch.randint(0, V, (args.batch, T), device="cuda")
    batch = {"ids": ids}
    for stride in STRIDES:
        S = stride[0] * stride[1]
        a, b = masked.gpt.pseudo_nll(ids, (SIDE, SIDE), stride=stride, max_rows=MAX_ROWS), composed_map(masked.gpt, ids, stride, MAX_ROWS)
        sides = {"pseudo_nll": lambda stride=stride: masked.gpt.pseudo_nll(ids, (SIDE, SIDE), stride=stride, max_rows=MAX_ROWS),
                 "composed": lambda stride=stride: composed_map(masked.gpt, ids, stride, MAX_ROWS),
                 "autoregressive_token_nll": lambda: plain.token_nll(batch)}
        rec = measure(sides, args, "pseudo_nll B=%d T=%d V=%d stride %s (%d passes, max_rows %d) beside the map composed from forward + "
                      "cross_entropy + indexing and the autoregressive token_nll" % (args.batch, T, V, stride, S, MAX_ROWS),
                      steps=max(2, args.steps // (1 + S // 16)))
        rec["stride"], rec["passes"] = list(stride), S
        rec["max_abs_difference_to_composed"] = float((a - b).abs().max())
        rec["logit_bytes_pseudo_nll"], rec["logit_bytes_composed_per_chunk"] = 4 * args.batch * T * V, 4 * min(S, MAX_ROWS // args.batch) * args.batch * T * V
        rec["pseudo_nll_over_composed"] = round(rec["pseudo_nll_ms"] / rec["composed_ms"], 4)
        rec["pseudo_nll_over_autoregressive_token_nll"] = round(rec["pseudo_nll_ms"] / rec["autoregressive_token_nll_ms"], 4)
        lines.append(rec)

    del masked, plain, sides
    masked, plain = build_trainers(V_EDIT)
    image = torch.randn(1, 1, 2 * SIDE, 2 * SIDE, device="cuda")
    one = {"image": image}
    tau_m, tau_a = float(masked.pseudo_nll(one).median()), float(plain.token_nll(one).median())
    gen = torch.Generator(device="cuda").manual_seed(0)
    kw = dict(n_candidates=8, top_k=32, top_p=0.95, generator=gen)
    sides = {"detect_pseudo": lambda: masked.detect_pseudo(one, tau_m, stride=(2, 2), n_steps=8, **kw),
             "autoregressive_detect": lambda: plain.detect(one, tau_a, **kw)}
    rec = measure(sides, args, "detect one slice, V=%d, 8 candidates, top-k 32, top-p 0.95, half of the %d codes restored: detect_pseudo "
                  "(stride (2, 2), 8 passes) beside the autoregressive detect" % (V_EDIT, T), steps=2)
    rec["detect_pseudo_over_autoregressive_detect"] = round(rec["detect_pseudo_ms"] / rec["autoregressive_detect_ms"], 4)
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
