#!/usr/bin/env python3
"""PriorTrainer.edit on one GPU against the same loop in plain torch, DESIGN 6x's protocol.  The default prior (12 layers, 256 wide,
8 heads, V = 64, block_size 256 = the 16 x 16 latent) behind a small VQGAN (32 x 32 pictures: only its dictionary and latent size
matter here, the pictures' decoding is not the subject); one slice, 8 candidates, top-k 32, top-p 0.95.  Regions:

    quarter   the central 8 x 8 cells (64 codes redrawn; the prefill covers the 68 codes in front of the first, 187 decode steps)
    whole     every cell (256 codes redrawn, 255 decode steps)
    late      the last two latent rows (32 codes redrawn; the prefill covers 224 codes, 31 decode steps): the prefill shortcut

ours   tr.edit({'image'}, box=...): VQGAN.encode_to_ids, GPT.generate_masked (prefill, then ops.sample_filtered + decode_step per
       position), the ranking's host read, two decode_from_ids, ops.paste_cells
torch  the same route in plain torch: tests/gpt_ref.py's model on the GPU (its pieces for the step behind a past), the past
       concatenated per step, a torch top-k / top-p filter (sort, cumsum), log_softmax, an inverse CDF by cumsum and comparison
       (no multinomial), torch.where for the kept codes and the composite; the VQGAN calls are shared
Per region: ms per edit and ms per position behind the prefill (the median of --windows windows of one edit each, after a warm-up,
the two sides alternating).  Then the sampling launch alone at B = 8, V = 64, the step's shape: ops.sample_topk against
ops.sample_filtered at top_p = 1 (the pin's route, with the log-probability) and at top_p = 0.95, ms per launch over --launches
launches.  One JSON line per record is appended to profiles/prior_edit_bench.jsonl.

    python tools/prior_edit_bench.py [--windows 5] [--candidates 8] [--launches 2000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

V, T, SIDE, N_LAYER, N_HEAD, N_EMBED = 64, 256, 16, 12, 8, 256
TOP_K, TOP_P = 32, 0.95
REGIONS = {"quarter": (8, 24, 8, 24), "whole": (0, 32, 0, 32), "late": (28, 32, 0, 32)}          # pixel boxes: 2 pixels per cell


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def build():
    import torch
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    torch.manual_seed(0)
    vqgan = VQGAN(1, 32, 1, 32, V, (1, 2), (1, 2), 1, [], [], 32, 0.0, True, "torch")
    gpt = GPT(V, T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED)
    return PriorTrainer(vqgan, gpt, device="cuda")


def torch_filter(logits, top_k, top_p):
    """top_k_top_p_filtering in plain torch -> the kept mask (ties at the top-k threshold kept; an entry stays iff the mass
    strictly greater than it is <= top_p)"""
    import torch
    kept = logits >= torch.topk(logits, top_k, dim=-1).values[:, -1:]
    if top_p < 1:
        p = torch.softmax(logits.masked_fill(~kept, float("-inf")), dim=-1)
        ps, order = torch.sort(p, dim=-1, descending=True)
        excl = torch.cumsum(ps, dim=-1) - ps
        first = torch.searchsorted((-ps).contiguous(), (-ps).contiguous(), right=False)
        g = torch.empty_like(p).scatter_(1, order, excl.gather(1, first))
        kept = kept & (g <= top_p)
    return kept


def torch_decode_step(tok, st, past, pos, n_layer, n_head):
    """One token per row behind the concatenated past, in plain torch on tests/mingpt_ref.py's pieces: tok (B,), past (n_layer, 2,
    B, n_head, Tp, hs) -> (logits (B, V), the past with the new position appended).  No mask: every key is behind the query."""
    import math
    import torch
    import mingpt_ref as M
    x = st["tok_embed.weight"][tok][:, None] + st["pos_embed"][:, pos:pos + 1]
    B, _, E = x.shape
    hs = E // n_head
    presents = []
    for i in range(n_layer):
        pre = "blocks.%d." % i
        h = M.layer_norm_ref(x, st[pre + "ln1.weight"], st[pre + "ln1.bias"])
        k, q, v = (M.linear_ref(h, st, pre + "att." + name + ".").reshape(B, 1, n_head, hs).transpose(1, 2) for name in "kqv")
        k, v = torch.cat((past[i, 0], k), dim=-2), torch.cat((past[i, 1], v), dim=-2)
        presents.append(torch.stack((k, v)))
        att = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) * (1.0 / math.sqrt(hs)), dim=-1)
        x = x + M.linear_ref(torch.matmul(att, v).transpose(1, 2).reshape(B, 1, E), st, pre + "att.proj.")
        h = M.layer_norm_ref(x, st[pre + "ln2.weight"], st[pre + "ln2.bias"])
        x = x + M.linear_ref(M.gelu_ref(M.linear_ref(h, st, pre + "mlp.0.")), st, pre + "mlp.2.")
    x = M.layer_norm_ref(x, st["ln_f.weight"], st["ln_f.bias"])
    return torch.matmul(x[:, 0], st["head.weight"].t()), torch.stack(presents)


def build_torch_edit(tr, n):
    import torch
    import gpt_ref as G
    st = {k: v.detach().clone() for k, v in tr.gpt.state_dict().items()}
    h = w = SIDE

    def edit(image, box, gen):
        ids = tr.vqgan.encode_to_ids(image)
        B = ids.shape[0]
        cells = torch.from_numpy(tr.cell_mask(B, box=box, image_size=tuple(image.shape[-2:]))).cuda()
        resample = cells.reshape(B, T).repeat_interleave(n, dim=0)
        known = ids.repeat_interleave(n, dim=0)
        j0 = int(torch.nonzero(resample.any(dim=0))[0])
        start = torch.zeros(B * n, 1, dtype=torch.long, device="cuda")
        with torch.no_grad():
            logits, past = G.gpt_ref(torch.cat((start, known[:, :j0]), dim=1), st, N_LAYER, N_HEAD)
            lp = [torch.log_softmax(logits[:, :j0], dim=-1).gather(-1, known[:, :j0, None])[..., 0]]
            tokens, z = [known[:, :j0]], logits[:, -1]
            for k in range(j0, T):
                kept = torch_filter(z, TOP_K, TOP_P)
                p = torch.softmax(z.masked_fill(~kept, float("-inf")), dim=-1)
                u = torch.rand(B * n, 1, generator=gen, device="cuda")
                draw = torch.clamp((torch.cumsum(p, dim=-1) <= u).sum(dim=-1), max=V - 1)
                new = torch.where(resample[:, k], draw, known[:, k])
                tokens.append(new[:, None])
                lp.append(torch.log_softmax(z, dim=-1).gather(-1, new[:, None]))
                if k + 1 < T:
                    z, past = torch_decode_step(new, st, past, 1 + k, N_LAYER, N_HEAD)
        tokens, scores = torch.cat(tokens, dim=1), torch.cat(lp, dim=1).double().sum(1).reshape(B, n)
        best = scores.argmax(dim=1).cpu()          # the ranking's host read
        best_ids = tokens.reshape(B, n, T)[torch.arange(B, device="cuda"), best.cuda()]
        recon, edited = tr.vqgan.decode_from_ids(ids, h, w), tr.vqgan.decode_from_ids(best_ids, h, w)
        m = cells.repeat_interleave(image.shape[-2] // h, dim=1).repeat_interleave(image.shape[-1] // w, dim=2)
        return torch.where(m[:, None], edited, image), recon

    return edit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_edit_bench.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from hipops import ops
    tr = build()
    n = args.candidates
    image = torch.randn(1, 1, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
    torch_edit = build_torch_edit(tr, n)
    gen = lambda s: torch.Generator(device="cuda").manual_seed(s)  # noqa: E731
    ours = lambda box, s: tr.edit({"image": image}, box=box, n_candidates=n, top_k=TOP_K, top_p=TOP_P, generator=gen(s))  # noqa: E731
    records = []
    for name, box in REGIONS.items():
        cells = tr.cell_mask(1, box=box, image_size=(32, 32)).reshape(-1)
        j0 = int(np.flatnonzero(cells)[0])
        positions = T - j0
        timed(lambda: ours(box, 0))          # warm-up: allocator, kernel modules
        timed(lambda: torch_edit(image, box, gen(0)))
        ms = {"ours": [], "torch": []}
        for wdw in range(args.windows):
            ms["ours"].append(timed(lambda: ours(box, 10 + wdw))[0])
            ms["torch"].append(timed(lambda: torch_edit(image, box, gen(10 + wdw)))[0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        records.append(dict(tool="prior_edit_bench", what="edit", region=name, box=list(box), device=torch.cuda.get_device_name(0),
                            model="12 x 256, 8 heads, V 64, block_size 256", candidates=n, top_k=TOP_K, top_p=TOP_P,
                            codes_resampled=int(cells.sum()), prefill_tokens=1 + min(j0, T - 1), positions_behind_prefill=positions,
                            ours_ms_per_edit=round(med["ours"], 2), torch_ms_per_edit=round(med["torch"], 2),
                            ours_ms_per_position=round(med["ours"] / positions, 4), torch_ms_per_position=round(med["torch"] / positions, 4),
                            speedup_median=round(med["torch"] / med["ours"], 2),
                            ours_ms_windows=[round(v, 2) for v in ms["ours"]], torch_ms_windows=[round(v, 2) for v in ms["torch"]]))

    # the sampling launch alone at the step's shape
    B = n
    z = torch.randn(B, V, generator=torch.Generator().manual_seed(2)).cuda()
    u = torch.rand(B, generator=torch.Generator().manual_seed(3)).cuda()
    forced = torch.full((B,), -1, dtype=torch.long, device="cuda")
    sides = {"sample_topk": lambda: ops.sample_topk(z, u, 1.0, TOP_K),
             "sample_filtered_top_p_1": lambda: ops.sample_filtered(z, u, forced, 1.0, TOP_K, None),
             "sample_filtered_top_p_0.95": lambda: ops.sample_filtered(z, u, forced, 1.0, TOP_K, TOP_P)}

    def loop(fn):
        for _ in range(args.launches):
            fn()

    per = {k: [] for k in sides}
    for fn in sides.values():
        timed(lambda: loop(fn))
    for _ in range(args.windows):
        for k, fn in sides.items():
            per[k].append(timed(lambda: loop(fn))[0] / args.launches)
    rec = dict(tool="prior_edit_bench", what="sampling launch", device=torch.cuda.get_device_name(0), batch=B, V=V, top_k=TOP_K,
               launches=args.launches, windows=args.windows)
    for k, v in per.items():
        rec[k + "_us"] = round(statistics.median(v) * 1e3, 2)
        rec[k + "_us_windows"] = [round(t * 1e3, 2) for t in v]
    records.append(rec)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in records:
            line = json.dumps(rec)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
