#!/usr/bin/env python3
"""LPIPS perceptual loss (hipops.ops.lpips_loss / functions.LPIPSLoss): forward + backward timed with HIP events at
(64, 1, 256, 256) - both views of BASELINE config 2 (batch 32) - and at (4, 1, 512, 512), as ms and executed TFLOP/s, beside
the eager F.conv2d / F.max_pool2d stack under autograd as the reference's lpips package runs it (context only, not a
product path).  Then config 2's whole first step with the loss off and on (use_perceptual_loss, perceptual_loss_type
'lpips', loss_weight.perceptual = 1), alternating the trainers on one box, and one multi-window step (three windows of each
view in one batch).  Weights: He-normal (the timing does not depend on their values).  Prints one JSON line per
measurement.  --once N,C,H,W runs three forward + backward passes at one shape and nothing else: the program to put behind a
kernel tracer.

    python tools/lpips_bench.py [--reps 10] [--rounds 5] [--steps 10] [--no-step] [--once SHAPE]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))
import torch
import torch.nn.functional as F
import bench

PEAK_FP32 = 157.3e12             # MI355X_MICROARCH.md: fp32-input MFMA = vector fp32 peak
LAYERS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
          (5, 10, 256, 256, 3, 1, 1))
CHANNELS = (64, 192, 384, 256, 256)


def he_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for s, idx, cin, cout, k, _, _ in LAYERS:
        sd["loss_func.net.slice%d.%d.weight" % (s, idx)] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        sd["loss_func.net.slice%d.%d.bias" % (s, idx)] = torch.rand(cout, generator=g) * 0.05 + 0.01
    for i, c in enumerate(CHANNELS):
        sd["loss_func.lin%d.model.1.weight" % i] = torch.rand(1, c, 1, 1, generator=g)
    return sd


def layer_flop(N, C, H, W):
    """{layer: FLOP as launched} for N image pairs: forward on 2N images (recon and clear), backward on the N recon images.
    The stem counts its planes (2 for a 1-channel input: folded weights and the in-bounds constant; 3 otherwise); the 3x3
    layers are counted in direct form (the Winograd form, where the dispatch takes it, executes 4/9 of that)."""
    from hipops import ops
    (h0, w0), (h1, w1), (h2, w2) = ops.lpips_map_sizes(H, W)[:3]
    planes = 2 if C == 1 else 3
    out = {"stem fwd": 2.0 * 2 * N * h0 * w0 * 64 * 121 * planes, "stem bwd": 2.0 * N * h0 * w0 * 64 * 121 * C,
           "conv5 fwd": 2.0 * 2 * N * h1 * w1 * 25 * 64 * 192, "conv5 bwd": 2.0 * N * h1 * w1 * 25 * 64 * 192}
    for name, cin, cout in (("conv3a", 192, 384), ("conv3b", 384, 256), ("conv3c", 256, 256)):
        out[name + " fwd"] = 2.0 * 2 * N * h2 * w2 * 9 * cin * cout
        out[name + " bwd"] = 2.0 * N * h2 * w2 * 9 * cin * cout
    return out


def eager_lpips(sd):
    w = [sd["loss_func.net.slice%d.%d.weight" % (s, idx)].cuda() for s, idx, *_ in LAYERS]
    b = [sd["loss_func.net.slice%d.%d.bias" % (s, idx)].cuda() for s, idx, *_ in LAYERS]
    lin = [sd["loss_func.lin%d.model.1.weight" % i].cuda() for i in range(5)]
    shift = torch.tensor([-.030, -.088, -.188], device="cuda").view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device="cuda").view(1, 3, 1, 1)

    def feats(x):
        x = (x.expand(x.shape[0], 3, x.shape[2], x.shape[3]) - shift) / scale
        out = []
        for i, (_, _, _, _, _, stride, pad) in enumerate(LAYERS):
            if i in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w[i], b[i], stride=stride, padding=pad))
            out.append(x)
        return out

    def loss(x, t):
        with torch.no_grad():
            fh = feats(t)
        total = 0
        for i, f in enumerate(feats(x)):
            a = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            bb = fh[i] / (fh[i].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            total = total + F.conv2d((a - bb) ** 2, lin[i]).mean((2, 3), keepdim=True)
        return total.mean()
    return loss


def time_fwd_bwd(fn, pred, target, reps):
    def once():
        x = pred.detach().requires_grad_(True)
        fn(x, target).backward()
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _pair(shape):
    pred, noise = bench.synthetic_batch(shape[0], shape[2], 11, torch.device("cuda"))
    if shape[1] == 3:
        pred, noise = pred.expand(-1, 3, -1, -1).contiguous(), noise.expand(-1, 3, -1, -1).contiguous()
    return pred, (pred + noise).clamp(-1, 1)


def kernel_rows(reps):
    from functions import LPIPSLoss
    sd = he_weights()
    lp = LPIPSLoss(weights=sd).cuda()
    eager = eager_lpips(sd)
    for shape in ((64, 1, 256, 256), (4, 1, 512, 512)):
        pred, target = _pair(shape)
        ms = time_fwd_bwd(lp, pred, target, reps)
        ms_eager = time_fwd_bwd(eager, pred, target, reps)
        fl = sum(layer_flop(*shape).values())
        print(json.dumps(dict(what="lpips_loss fwd+bwd", shape=list(shape), ms=round(ms, 4), gflop_direct_form=round(fl / 1e9, 1),
                              tflops=round(fl / ms / 1e9, 1), share_of_fp32_peak=round(fl / ms / 1e9 / (PEAK_FP32 / 1e12), 3),
                              eager_aten_ms=round(ms_eager, 4))), flush=True)


def once(shape):
    """One warm forward + backward at `shape` between two synchronisations: the body of a kernel-trace run."""
    from functions import LPIPSLoss
    lp = LPIPSLoss(weights=he_weights()).cuda()
    pred, target = _pair(shape)
    for _ in range(3):
        x = pred.detach().requires_grad_(True)
        lp(x, target).backward()
    torch.cuda.synchronize()
    print(json.dumps(dict(what="lpips_loss fwd+bwd x 3 (trace body)", shape=list(shape),
                          layer_gflop={k: round(v / 1e9, 2) for k, v in layer_flop(*shape).items()})), flush=True)


def _trainers(variants, wpath):
    from trainers import build_first_step_trainer
    from utils import load_json
    raw0 = json.load(open(os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json")))
    out = {}
    for name in variants:
        raw = json.loads(json.dumps(raw0))
        if name != "off":
            raw["loss"].update(use_perceptual_loss=True, perceptual_loss_type="lpips", lpips_weights=wpath,
                               percep_weights=[1.0, 1.0, 1.0])
            raw["loss"]["loss_weight"]["perceptual"] = 1.0
        path = wpath + "." + name + ".json"
        with open(path, "w") as f:
            json.dump(raw, f)
        cfg = load_json(path)
        mw = dict(dataset_window=(2000, 0, 2.0), recon_weights=(1.0, 1.0, 1.0)) if name == "multi" else None
        torch.manual_seed(0)
        out[name] = build_first_step_trainer(cfg, device="cuda", data_parallel=False, multi_window=mw)
    return out, cfg


def step_rows(rounds, steps, wpath):
    variants = ("off", "on", "multi")
    trs, cfg = _trainers(variants, wpath)
    B, S = int(cfg.dataset.batch_size), int(cfg.dataset.image_size)
    pool = [bench.synthetic_batch(B, S, 1234 + s, torch.device("cuda")) for s in range(2)]
    for tr in trs.values():
        for i in range(3):
            tr.training_step({"image": pool[i % 2][0]}, noise=pool[i % 2][1])
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    outs = {}
    for _ in range(rounds):
        for k in variants:
            tr = trs[k]
            t0 = time.perf_counter()
            for i in range(steps):
                outs[k] = tr.training_step({"image": pool[i % 2][0]}, noise=pool[i % 2][1])
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(what="config-2 first step (B=32, 256x256)", ms_off=[round(v, 2) for v in ms["off"]],
                          ms_on=[round(v, 2) for v in ms["on"]], median_off=round(med["off"], 2), median_on=round(med["on"], 2),
                          added_ms=round(med["on"] - med["off"], 2),
                          perceptual_scalar=round(trs["on"].scalars(outs["on"])["perceptual"], 6))), flush=True)
    print(json.dumps(dict(what="config-2 first step, multi-window (recon + lpips on three windows per view)",
                          ms_multi=[round(v, 2) for v in ms["multi"]], median_multi=round(med["multi"], 2),
                          added_ms_vs_off=round(med["multi"] - med["off"], 2),
                          perceptual_scalar=round(trs["multi"].scalars(outs["multi"])["perceptual"], 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="kernel rows only")
    ap.add_argument("--once", default=None, help="N,C,H,W: three forward + backward passes at that shape and nothing else "
                                                 "(the program to put behind a kernel tracer)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)
    if a.once:
        once(tuple(int(v) for v in a.once.split(",")))
        return
    kernel_rows(a.reps)
    if not a.no_step:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            wpath = os.path.join(d, "lpips.pth")
            torch.save(he_weights(), wpath)
            step_rows(a.rounds, a.steps, wpath)


if __name__ == "__main__":
    main()
