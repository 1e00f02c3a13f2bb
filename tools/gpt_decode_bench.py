#!/usr/bin/env python3
"""GPT.sample (the cached route that concatenates the past per step) against GPT.generate (the preallocated KV cache, one host call per
token) on one GPU, DESIGN 6s's protocol: the default model (12 layers, 256 wide, 8 heads, V = 1024, block_size 256), B = 8,
top_k = 100, 255 tokens behind a one-token prompt; the host clock around the call, ending in a synchronise; warmed up; the two
alternating in one process, three windows each.  One JSON line per run is appended to profiles/gpt_decode_bench.jsonl.

    python tools/gpt_decode_bench.py                 # the measurement
    python tools/gpt_decode_bench.py --trace 32      # a short run for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...):
                                                     # one generate of that many tokens, no timing, nothing written
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=255)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0, help="generate this many tokens once (after one warm-up call) and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_decode_bench.jsonl"))
    args = ap.parse_args()

    import networks
    torch.manual_seed(0)
    m = networks.GPT(vocab_size=1024, block_size=256).cuda().eval()
    prompt = torch.zeros(args.batch, 1, dtype=torch.long, device="cuda")

    def run(fn, steps, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(prompt, steps, temperature=1.0, top_k=args.top_k, generator=gen)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if args.trace:
        run(m.generate, args.trace, 1)
        run(m.generate, args.trace, 2)
        return
    for fn in (m.sample, m.generate):          # warm-up: allocator, kernel modules, LDS opt-ins
        run(fn, args.steps, 1)
    ms = {"sample": [], "generate": []}
    same = True
    for w in range(args.windows):
        a, sa = run(m.sample, args.steps, 10 + w)
        b, sb = run(m.generate, args.steps, 10 + w)
        ms["sample"].append(a)
        ms["generate"].append(b)
        same = same and bool(torch.equal(sa, sb))          # informative: one seed, one stream of uniforms; unclear decisions may differ
    per = {k: [v / args.steps for v in vs] for k, vs in ms.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    n_layer = m.config.n_layer
    rec = {"tool": "gpt_decode_bench", "device": torch.cuda.get_device_name(0), "model": "12 x 256, 8 heads, V 1024, block_size 256",
           "batch": args.batch, "steps": args.steps, "top_k": args.top_k, "launches_per_decode_step": 2 + 5 * n_layer,
           "sample_ms_total": [round(v, 2) for v in ms["sample"]], "generate_ms_total": [round(v, 2) for v in ms["generate"]],
           "sample_ms_per_token": [round(v, 4) for v in per["sample"]], "generate_ms_per_token": [round(v, 4) for v in per["generate"]],
           "speedup_median": round(med["sample"] / med["generate"], 2), "tokens_equal_under_one_seed": same}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
