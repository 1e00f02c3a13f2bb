#!/usr/bin/env python3
"""The VQGAN trainer's step (configs/vqgan_unet_512.json, `run_vqwnet.py -v`) on one GPU, one JSON line per measurement:

  step      per batch size (--batches, default 1 and 4): ms per step - the median of --windows windows of --steps steps after
            --warmup steps - and its split into five phases, from HIP events on the launch stream:
              vqgan_fwd      VQGAN(image): encoder, quantiser (with its EMA update), decoder
              d_gen          the reconstruction loss, D(recon) with a tape and D(image) without one, the generator total
              gen_bwd_adam   the generator half's backward (through D and the VQGAN) and dec_optim's Adam step
              dis_passes     D(image), D(recon), CutMix, D(cutmix images) and the three losses
              dis_bwd_adam   the discriminator half's backward and dis_optim's Adam step
            every window (step and phases) is also appended to --out (profiles/vqgan_step_bench.jsonl)
  families  the same step once more under vqw_profile_begin / end, serialised (no side stream): launches, ms and share of the
            six kernel families that interface times (MFMA forward / input gradient, MFMA weight gradient, generic forward,
            generic weight gradient, Winograd forms, HBM-bound norm / element-wise) and `other_ms`, the rest of the step -
            GroupNorm-swish, attention, the stride-2 convolution, the quantiser, the U-Net discriminator's tails, heads and
            losses, spectral norm, Adam
  export    ops.export_grey_auto next to ops.export_grey (one window) on 4 x 1 x 512 x 512: ms, bytes/s and their ratio

    python tools/vqgan_step_bench.py [--steps 10] [--warmup 4] [--windows 5] [--reps 200] [--batches 1 4] [--out FILE]

The kernel families inside `other_ms` come from a kernel trace of the same step:

    rocprofv3 --kernel-trace --stats -d prof -o t -- python tools/vqgan_step_bench.py --only-step --windows 1 --batches 4
    python tools/vqgan_step_bench.py --stats prof/.../t_kernel_stats.csv
"""
import argparse, csv, ctypes, json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))

PHASES = ("vqgan_fwd", "d_gen", "gen_bwd_adam", "dis_passes", "dis_bwd_adam")
FAMILIES = ("mfma_fwd_dgrad", "mfma_wgrad", "generic_fwd", "generic_wgrad", "winograd", "norm_elementwise")
GROUPS = (("attention", r"k_attn|k_attention"), ("groupnorm_swish", r"k_gn_|k_groupnorm|k_swish"), ("conv_stride2", r"k_conv3s2|k_down2"),
          ("vq", r"k_vq_"), ("unet_dis_tails_heads_losses", r"k_dtail_|k_utail_|k_bottleneck_|k_cutmix_select|k_dis_losses_"),
          ("spectral_norm", r"k_sn_"), ("adam", r"k_adam"),
          ("convolution", r"k_conv_|k_pw_|k_stem_|k_head_|k_wino_|k_pack_|k_input_grad_gather|k_reduce_|k_fold_multi|k_collapse_up|k_bias_grad"))


def stats(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out, seen = {}, 0.0
    for name, pat in GROUPS:
        ns = sum(float(r["TotalDurationNs"]) for r in rows if re.search(pat, r["Name"]))
        out[name] = dict(ms=round(ns / 1e6, 2), share=round(ns / total, 4))
        seen += ns
    out["everything_else"] = dict(ms=round((total - seen) / 1e6, 2), share=round((total - seen) / total, 4))
    print(json.dumps(dict(what="kernel time of the traced run", total_ms=round(total / 1e6, 2), groups=out,
                          launches=sum(int(r["Calls"]) for r in rows))))


def build(batch):
    import torch
    from utils import load_json
    from trainers import build_vqgan_trainer
    c = load_json(os.path.join(ROOT, "configs", "vqgan_unet_512.json"))
    torch.manual_seed(0)
    tr = build_vqgan_trainer(c, device="cuda")
    S = c.dataset.image_size
    imgs = [torch.rand(batch, 1, S, S, device="cuda") * 2 - 1 for _ in range(4)]
    return tr, imgs


def mark_phases(tr, marks):
    """Record an event on the launch stream at the end of each phase: after reconstruct(), generator_pass(), dec_optim.step(),
    discriminator_pass(); the step's own end closes the last phase."""
    import torch

    def after(fn):
        def wrapped(*a, **k):
            r = fn(*a, **k)
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
            return r
        return wrapped
    tr.reconstruct = after(tr.reconstruct)
    tr.generator_pass = after(tr.generator_pass)
    tr.dec_optim.step = after(tr.dec_optim.step)
    tr.discriminator_pass = after(tr.discriminator_pass)


def step_rows(args, batch, sink):
    import torch
    tr, imgs = build(batch)
    marks = []
    mark_phases(tr, marks)
    for i in range(args.warmup):
        tr.training_step({"image": imgs[i % 4]})
    torch.cuda.synchronize()
    windows, phases = [], {p: [] for p in PHASES}
    for w in range(args.windows):
        del marks[:]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ends[0].record()
        for i in range(args.steps):
            tr.training_step({"image": imgs[i % 4]})
            ends[i + 1].record()
        torch.cuda.synchronize()
        assert len(marks) == 4 * args.steps, "one inner loop expected"
        ms = ends[0].elapsed_time(ends[-1]) / args.steps
        split = {}
        for j, p in enumerate(PHASES):
            tot = 0.0
            for i in range(args.steps):
                edge = [ends[i]] + marks[4 * i:4 * i + 4] + [ends[i + 1]]
                tot += edge[j].elapsed_time(edge[j + 1])
            split[p] = tot / args.steps
            phases[p].append(split[p])
        windows.append(ms)
        sink(dict(what="window", batch=batch, window=w, steps=args.steps, ms_per_step=round(ms, 3),
                  phases_ms={p: round(v, 3) for p, v in split.items()}))
    row = dict(what="step", config="vqgan_unet_512", batch=batch, steps=args.steps, ms_per_step=round(statistics.median(windows), 2),
               windows=[round(v, 2) for v in windows], phases_ms={p: round(statistics.median(v), 2) for p, v in phases.items()})
    print(json.dumps(row), flush=True)
    return tr, imgs, row


def family_row(args, tr, imgs, batch, sink):
    """The step under the profiling interface, serialised as bench.py's serialised pass is."""
    import torch
    from hipops import _lib, ops
    L = _lib.load()
    ops.WGRAD_ASYNC = False
    try:
        tr.training_step({"image": imgs[0]})
        torch.cuda.synchronize()
        L.vqw_profile_families(0x3F)
        _lib.check(L.vqw_profile_begin(), "vqw_profile_begin")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            tr.training_step({"image": imgs[i % 4]})
        e1.record()
        torch.cuda.synchronize()
        prof = (ctypes.c_double * 24)()
        _lib.check(L.vqw_profile_end(prof), "vqw_profile_end")
    finally:
        ops.WGRAD_ASYNC = True
    ms = e0.elapsed_time(e1) / args.steps
    fam = {}
    for f, name in enumerate(FAMILIES):
        launches, tot = prof[4 * f], prof[4 * f + 1]
        fam[name] = dict(launches_per_step=round(launches / args.steps, 1), ms=round(tot / args.steps, 3), share=round(tot / args.steps / ms, 4))
    other = ms - sum(v["ms"] for v in fam.values())
    row = dict(what="families", batch=batch, serialised_ms_per_step=round(ms, 2), families=fam, other_ms=round(other, 2),
               other_share=round(other / ms, 4))
    print(json.dumps(row), flush=True)
    sink(row)


def export_rows(args, sink):
    import torch
    from hipops import ops
    x = torch.randn(4, 1, 512, 512, device="cuda")
    n = x.numel()
    res = {}
    for name, fn, nbytes in (("export_grey", lambda: ops.export_grey(x), 5 * n), ("export_grey_auto", lambda: ops.export_grey_auto(x), 9 * n)):
        times = []
        for _ in range(args.windows):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.reps)
        ms = statistics.median(times)
        res[name] = ms
        row = dict(what="export", op=name, shape=[4, 1, 512, 512], ms=round(ms, 4), windows=[round(t, 4) for t in times],
                   mbytes=round(nbytes / 1e6, 2), gbytes_per_s=round(nbytes / ms / 1e6, 1))
        print(json.dumps(row), flush=True)
        sink(row)
    row = dict(what="export ratio", auto_over_fixed=round(res["export_grey_auto"] / res["export_grey"], 3))
    print(json.dumps(row), flush=True)
    sink(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vqgan_step_bench.jsonl"))
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--stats", help="a rocprofv3 --stats kernel CSV of a run with --only-step: print the kernel groups' shares")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def sink(row):
            f.write(json.dumps(row) + "\n")
            f.flush()
        for batch in args.batches:
            tr, imgs, row = step_rows(args, batch, sink)
            sink(row)
            if not args.only_step:
                family_row(args, tr, imgs, batch, sink)
            del tr, imgs
        if not args.only_step:
            export_rows(args, sink)


if __name__ == "__main__":
    main()
