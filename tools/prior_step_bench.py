#!/usr/bin/env python3
"""The GPT code prior's training step (trainers/prior.py, `run_vqwnet.py -p`) on one GPU, one JSON line per measurement:

  step      PriorTrainer.training_step({'ids'}) of the default model (12 layers, 8 heads, 256 wide, block size 256), B = 32,
            T = 256, V = 1024, pkeep 0.9, AdamW with the clip: ms per step - the median of --windows windows of --steps steps after
            --warmup steps, from a host clock around work that ends in a device synchronise - and its two parts, each timed alone
            the same way: fwd_bwd (tokens, forward, loss, backward) and optim (the gradient norm, the clip and the AdamW update)
  torch     the same model and recipe in plain torch on the same GPU: the test restatement's GPT (tests/gpt_ref.py) under
            torch.optim.AdamW on minGPT's two groups and torch.nn.utils.clip_grad_norm_, with the same split
  encode    VQGAN.encode_to_ids of the configs/prior_vqgan_512.json first stage on --encode-batch 512 x 512 slices: ms per batch,
            and the GPT step at that batch size next to it - what a cached-codes mode would save

  attention with --attention instead of the above: the causal attention kernels alone at B = --batch, T = 256, 8 heads of hs = 32 and
            of hs = 128 - the forward launch and the backward's three launches, each without and with the dropout policy at
            --pdrop (0.1 when --pdrop is 0)

--pdrop P (default 0) trains with dropout: our model with emb_pdrop = res_pdrop = att_pdrop = P and a seed (counter-based masks
inside the kernels), the plain-torch column with torch's dropout at the same three places (the embedding, the attention
probabilities, the two residual branches).

The windows of the two implementations alternate, so that what else runs on the machine touches both alike.

    python tools/prior_step_bench.py [--steps 20] [--warmup 5] [--windows 5] [--batch 32] [--encode-batch 4] [--pdrop 0]
                                     [--no-encode] [--attention] [--out FILE]
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

V, T, N_LAYER, N_HEAD, N_EMBED = 1024, 256, 12, 8, 256
OPTIM = dict(lr=4.5e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
CLIP = 1.0


def window(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def build_ours(batch, pkeep=0.9, pdrop=0.0):
    import torch
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    torch.manual_seed(0)
    # only its dict_size and latent size matter for a step from {'ids'}: 32 x 32 pictures, a 16 x 16 latent
    vqgan = VQGAN(1, 32, 1, 32, V, (1, 2), (1, 2), 1, [], [], 32, 0.0, True, "torch")
    gpt = GPT(V, T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=N_EMBED, emb_pdrop=pdrop, res_pdrop=pdrop, att_pdrop=pdrop)
    kw = dict(dropout_seed=0) if pdrop > 0 else {}
    tr = PriorTrainer(vqgan, gpt, pkeep=pkeep, lr=OPTIM["lr"], betas=OPTIM["betas"], weight_decay=OPTIM["weight_decay"],
                      grad_norm_clip=CLIP, device="cuda", **kw)
    ids = torch.randint(0, V, (batch, T), device="cuda")
    from hipops import ops

    def fwd_bwd():
        inp = tr._inputs(ids, tr.pkeep)
        loss = ops.cross_entropy(tr.gpt(inp), ids)
        tr.optim.zero_grad()
        loss.backward()

    return dict(step=lambda: tr.training_step({"ids": ids}), fwd_bwd=fwd_bwd, optim=tr.optim.step), tr


def gpt_torch_dropout(idx, st, p):
    """The restatement's GPT (tests/gpt_ref.py, tests/mingpt_ref.py) with torch's dropout where the reference has nn.Dropout: behind
    the embedding (mingpt.py:189), on the attention probabilities (:83), behind proj (:88) and behind the MLP (:104)."""
    import math
    import torch
    import mingpt_ref as M
    drop = lambda t: torch.nn.functional.dropout(t, p, training=True)
    B, Tn = idx.shape
    hs = N_EMBED // N_HEAD
    see = M.visible(Tn, Tn).to(idx.device)[None, None]
    x = drop(st["tok_embed.weight"][idx] + st["pos_embed"][:, :Tn])
    for i in range(N_LAYER):
        pre = "blocks.%d." % i
        h = M.layer_norm_ref(x, st[pre + "ln1.weight"], st[pre + "ln1.bias"])
        k, q, v = (M.linear_ref(h, st, pre + "att." + n + ".").reshape(B, Tn, N_HEAD, hs).transpose(1, 2) for n in "kqv")
        s = (torch.matmul(q, k.transpose(-2, -1)) * (1.0 / math.sqrt(hs))).masked_fill(~see, float("-inf"))
        o = torch.matmul(drop(torch.softmax(s, dim=-1)), v).transpose(1, 2).reshape(B, Tn, N_EMBED)
        x = x + drop(M.linear_ref(o, st, pre + "att.proj."))
        h = M.layer_norm_ref(x, st[pre + "ln2.weight"], st[pre + "ln2.bias"])
        x = x + drop(M.linear_ref(M.gelu_ref(M.linear_ref(h, st, pre + "mlp.0.")), st, pre + "mlp.2."))
    return torch.matmul(M.layer_norm_ref(x, st["ln_f.weight"], st["ln_f.bias"]), st["head.weight"].t())


def build_torch(batch, state, pkeep=0.9, pdrop=0.0):
    """The restatement's GPT on the GPU from `state` (a GPT state dict), stock AdamW and clip_grad_norm_."""
    import torch
    import gpt_ref as G
    import prior_ref as P
    st = {k: (v.detach().clone().cuda() if k.endswith("mask") else v.detach().clone().cuda().requires_grad_(True)) for k, v in state.items()}
    names = [k for k in st if not k.endswith("mask")]
    params = [st[k] for k in names]
    opt = torch.optim.AdamW([{"params": [st[k] for k in names if P.decays(k)], "weight_decay": OPTIM["weight_decay"]},
                             {"params": [st[k] for k in names if not P.decays(k)], "weight_decay": 0.0}],
                            lr=OPTIM["lr"], betas=OPTIM["betas"], eps=OPTIM["eps"])
    ids = torch.randint(0, V, (batch, T), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)

    def fwd_bwd():
        u_keep, u_rand = torch.rand(ids.shape, generator=gen, device="cuda"), torch.rand(ids.shape, generator=gen, device="cuda")
        inp = P.tokens_ref(ids, 0, pkeep, V, u_keep, u_rand)
        logits = gpt_torch_dropout(inp, st, pdrop) if pdrop > 0 else G.gpt_ref(inp, st, N_LAYER, N_HEAD)[0]
        loss = torch.nn.functional.cross_entropy(logits.view(-1, V), ids.view(-1))
        opt.zero_grad()
        loss.backward()

    def optim():
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()

    def step():
        fwd_bwd()
        optim()

    return dict(step=step, fwd_bwd=fwd_bwd, optim=optim)


def measure(sides, args, what):
    """sides {name: {part: callable}}: every part of every side warmed up, then --windows windows each, the sides alternating."""
    times = {n: {p: [] for p in parts} for n, parts in sides.items()}
    for parts in sides.values():
        for fn in parts.values():
            window(fn, args.warmup)
    for _ in range(args.windows):
        for part in ("step", "fwd_bwd", "optim"):
            for n, parts in sides.items():
                times[n][part].append(window(parts[part], args.steps))
    out = []
    for n in sides:
        rec = dict(what=what, impl=n, steps=args.steps, windows=args.windows)
        for part, ts in times[n].items():
            rec[part + "_ms"] = round(statistics.median(ts), 4)
            rec[part + "_ms_windows"] = [round(t, 4) for t in ts]
        out.append(rec)
    return out


def measure_attention(args):
    """The causal attention launches alone, without and with the dropout policy, the two alternating window by window."""
    import torch
    from hipops import ops
    L, p, key, out = ops._L(), args.pdrop if args.pdrop > 0 else 0.1, (0, 0, 1), []
    for hs in (32, 128):
        B, nh = args.batch, N_HEAD
        q, k, v, go = (torch.randn(B, T, nh * hs, device="cuda") for _ in range(4))
        o, gq, gk, gv = (torch.empty_like(q) for _ in range(4))
        lse, d = (torch.empty(B, nh, T, device="cuda") for _ in range(2))
        shape = (B, T, T, nh, hs, 1.0 / hs ** 0.5, 1, 0)
        fns = {
            "fwd": lambda: L.vqw_causal_attention_fwd(q, k, v, o, lse, *shape),
            "fwd_drop": lambda: L.vqw_causal_attention_drop_fwd(q, k, v, o, lse, *shape, p, *key),
            "bwd": lambda: L.vqw_causal_attention_bwd(q, k, v, o, lse, go, d, gq, gk, gv, *shape),
            "bwd_drop": lambda: L.vqw_causal_attention_drop_bwd(q, k, v, o, lse, go, d, gq, gk, gv, *shape, p, *key),
        }
        fns["fwd"]()
        times = {n: [] for n in fns}
        for fn in fns.values():
            window(fn, args.warmup)
        for _ in range(args.windows):
            for n, fn in fns.items():
                times[n].append(window(fn, args.steps))
        rec = dict(what="causal attention kernels alone B=%d T=%d nh=%d hs=%d, dropout p=%g" % (B, T, nh, hs, p), steps=args.steps, windows=args.windows)
        for n, ts in times.items():
            rec[n + "_ms"] = round(statistics.median(ts), 4)
            rec[n + "_ms_windows"] = [round(t, 4) for t in ts]
        rec["fwd_drop_over_fwd"] = round(rec["fwd_drop_ms"] / rec["fwd_ms"], 4)
        rec["bwd_drop_over_bwd"] = round(rec["bwd_drop_ms"] / rec["bwd_ms"], 4)
        out.append(rec)
    return out


def emit(lines, args):
    for rec in lines:
        print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--encode-batch", type=int, default=4)
    ap.add_argument("--pdrop", type=float, default=0.0, help="the three dropout probabilities of both columns (default 0: no dropout)")
    ap.add_argument("--no-encode", action="store_true", help="skip the encode measurement")
    ap.add_argument("--attention", action="store_true", help="measure the attention kernels alone, without and with dropout, and nothing else")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prior_step_bench: needs a GPU (a timing on the CPU says nothing)")
    if args.attention:
        return emit(measure_attention(args), args)
    lines = []
    ours, tr = build_ours(args.batch, pdrop=args.pdrop)
    state = {k: v.detach().cpu() for k, v in tr.gpt.state_dict().items()}
    lines += measure(dict(hip=ours, torch=build_torch(args.batch, state, pdrop=args.pdrop)), args,
                     "prior step B=%d T=%d V=%d, %d layers%s" % (args.batch, T, V, N_LAYER, ", dropout p=%g" % args.pdrop if args.pdrop > 0 else ""))
    if args.no_encode:
        return emit(lines, args)
    # the first stage's encoder next to the GPT step at the batch size a 512 x 512 run uses
    from utils import load_json
    from trainers.config import configure_vqgan
    vq = configure_vqgan(load_json(os.path.join(ROOT, "configs", "prior_vqgan_512.json"))).cuda().eval()
    x = torch.rand(args.encode_batch, 1, 512, 512, device="cuda") * 2 - 1
    small, _ = build_ours(args.encode_batch)
    for fn in (lambda: vq.encode_to_ids(x), small["step"]):
        window(fn, args.warmup)
    enc = [window(lambda: vq.encode_to_ids(x), args.steps) for _ in range(args.windows)]
    stp = [window(small["step"], args.steps) for _ in range(args.windows)]
    lines.append(dict(what="encode_to_ids of %d x 1 x 512 x 512 next to the GPT step at that batch" % args.encode_batch,
                      encode_ms=round(statistics.median(enc), 4), step_ms=round(statistics.median(stp), 4),
                      encode_over_step=round(statistics.median(enc) / statistics.median(stp), 3)))
    emit(lines, args)


if __name__ == "__main__":
    main()
