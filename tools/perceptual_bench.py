#!/usr/bin/env python3
"""VGG perceptual loss (hipops.ops.perceptual_loss / functions.VGGLoss): forward + backward timed with HIP events at
(64, 1, 256, 256) - both views of BASELINE config 2 (batch 32) - and at (4, 1, 512, 512), as ms and executed TFLOP/s, beside
the eager F.conv2d module stack as the reference runs it (weight gradients included; context only, not a product path).
Then config 2's whole first step with the loss off and on (use_perceptual_loss, loss_weight.perceptual = 1), alternating
the two trainers on one box, and one multi-window step (three windows of each view in one batch).  Weights: He-normal
(the timing does not depend on their values).  Prints one JSON line per measurement.

    python tools/perceptual_bench.py [--reps 10] [--rounds 5] [--steps 10]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))
import torch
import torch.nn as nn
import torch.nn.functional as F
import bench

PEAK_FP32 = 157.3e12             # MI355X_MICROARCH.md: fp32-input MFMA = vector fp32 peak


def he_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128)):
        sd["vgg.%d.weight" % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd["vgg.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.05
    return sd


def executed_flop(N, C, H, W):
    """As launched for 2N images (recon and clear): stem 1 -> 64 direct on both halves, conv1_2 direct on both, conv2_1 and
    conv2_2 (once, on the difference) in Winograd form (4/9) where served; backward on the N recon images: conv2_2^T,
    conv2_1^T, conv1_2^T in Winograd form, the stem's 64 -> 1 input gradient direct."""
    P, p = H * W, (H // 2) * (W // 2)
    mac = 2 * N * P * 64 * 9 * C + 2 * N * P * 64 * 64 * 9 + (4 / 9) * (2 * N * p * 64 * 128 * 9 + N * p * 128 * 128 * 9)
    mac += (4 / 9) * (N * p * 128 * 128 * 9 + N * p * 128 * 64 * 9 + N * P * 64 * 64 * 9) + N * P * 64 * 9 * C
    return 2.0 * mac


def eager_vgg(sd):
    seq = nn.Sequential(nn.Conv2d(3, 64, 3, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
                        nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(), nn.Conv2d(128, 128, 3, padding=1))
    seq.load_state_dict({k[len("vgg."):]: v for k, v in sd.items()})
    seq = seq.cuda()

    def loss(x, t):
        B, _, H, W = x.shape
        with torch.no_grad():
            yh = seq(t.expand(B, 3, H, W))
        return F.mse_loss(seq(x.expand(B, 3, H, W)), yh)
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


def kernel_rows(reps):
    from functions import VGGLoss
    sd = he_weights()
    vgg = VGGLoss(weights=sd).cuda()
    eager = eager_vgg(sd)
    for shape in ((64, 1, 256, 256), (4, 1, 512, 512)):
        pred, noise = bench.synthetic_batch(shape[0], shape[2], 11, torch.device("cuda"))
        target = (pred + noise).clamp(-1, 1)
        ms = time_fwd_bwd(vgg, pred, target, reps)
        ms_eager = time_fwd_bwd(eager, pred, target, reps)
        fl = executed_flop(*shape)
        print(json.dumps(dict(what="perceptual_loss fwd+bwd", shape=list(shape), ms=round(ms, 4), gflop=round(fl / 1e9, 1),
                              tflops=round(fl / ms / 1e9, 1), share_of_fp32_peak=round(fl / ms / 1e9 / (PEAK_FP32 / 1e12), 3),
                              eager_f_conv2d_ms=round(ms_eager, 4))), flush=True)


def _trainers(variants, wpath):
    from trainers import build_first_step_trainer
    from utils import load_json
    raw0 = json.load(open(os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json")))
    out = {}
    for name in variants:
        raw = json.loads(json.dumps(raw0))
        if name != "off":
            raw["loss"].update(use_perceptual_loss=True, perceptual_loss_type="vgg", perceptual_weights=wpath,
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
    print(json.dumps(dict(what="config-2 first step, multi-window (recon + perceptual on three windows per view)",
                          ms_multi=[round(v, 2) for v in ms["multi"]], median_multi=round(med["multi"], 2),
                          added_ms_vs_off=round(med["multi"] - med["off"], 2),
                          perceptual_scalar=round(trs["multi"].scalars(outs["multi"])["perceptual"], 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_bench.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)
    kernel_rows(a.reps)
    if not a.no_step:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            wpath = os.path.join(d, "vgg.pth")
            torch.save(he_weights(), wpath)
            step_rows(a.rounds, a.steps, wpath)


if __name__ == "__main__":
    main()
