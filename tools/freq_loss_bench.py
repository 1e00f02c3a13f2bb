#!/usr/bin/env python3
"""Focal frequency loss (hipops.ops.frequency_loss): forward + backward timed with HIP events at (64, 1, 256, 256) - both
views of BASELINE config 2 (batch 32) - and at (4, 1, 512, 512), as ms and executed TFLOP/s, beside the eager torch.fft.fft2
composition of the same loss (context only, not a product path).  Then config 2's whole first step with the loss off and on
(use_frequency_loss, loss_weight.freq = 1), alternating the two trainers on one box.  Prints one JSON line per measurement.

    python tools/freq_loss_bench.py [--reps 20] [--rounds 5] [--steps 10]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))
import torch
import bench
from hipops import ops

PEAK_FP32 = 157.3e12             # MI355X_MICROARCH.md: fp32-input MFMA = vector fp32 peak


def executed_flop(N, C, H, W, pf=1):
    """The four GEMM passes per plane as launched: x W_w (real x complex, 2 h w^2 MAC), W_h Y and conj(W_h) G (complex,
    4 h^2 w MAC each), Re(Z conj(W_w)) (2 h w^2 MAC)."""
    h, w = H // pf, W // pf
    return 2.0 * N * pf * pf * C * (4 * h * w * w + 8 * h * h * w)


def eager_loss(pred, target):
    """The package's formulation in eager torch (fp32 torch.fft on the GPU): for context only."""
    D = torch.fft.fft2(pred - target, norm="ortho")
    m = D.abs()
    m = m / m.amax(dim=(-2, -1), keepdim=True)
    m = torch.nan_to_num(m, nan=0.0).clamp(0.0, 1.0).detach()
    return torch.mean(m * (D.real ** 2 + D.imag ** 2))


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
    for shape in ((64, 1, 256, 256), (4, 1, 512, 512)):
        pred, noise = bench.synthetic_batch(shape[0], shape[2], 11, torch.device("cuda"))
        target = (pred + noise).clamp(-1, 1)
        ms = time_fwd_bwd(ops.frequency_loss, pred, target, reps)
        ms_eager = time_fwd_bwd(eager_loss, pred, target, reps)
        fl = executed_flop(*shape)
        print(json.dumps(dict(what="frequency_loss fwd+bwd", shape=list(shape), ms=round(ms, 4), gflop=round(fl / 1e9, 2),
                              tflops=round(fl / ms / 1e9, 1), share_of_fp32_peak=round(fl / ms / 1e9 / (PEAK_FP32 / 1e12), 3),
                              eager_torch_fft_ms=round(ms_eager, 4))), flush=True)


def step_rows(rounds, steps):
    from trainers import build_first_step_trainer
    from utils import load_json
    cfg_path = os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json")
    trainers = {}
    for on in (False, True):
        cfg = load_json(cfg_path)
        if on:
            cfg = cfg._replace(loss=cfg.loss._replace(use_frequency_loss=True, loss_weight=cfg.loss.loss_weight._replace(freq=1.0)))
        torch.manual_seed(0)
        trainers[on] = build_first_step_trainer(cfg, device="cuda", data_parallel=False)
    B, S = int(cfg.dataset.batch_size), int(cfg.dataset.image_size)
    pool = [bench.synthetic_batch(B, S, 1234 + s, torch.device("cuda")) for s in range(2)]
    for tr in trainers.values():
        for i in range(3):
            tr.training_step({"image": pool[i % 2][0]}, noise=pool[i % 2][1])
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            tr = trainers[on]
            t0 = time.perf_counter()
            for i in range(steps):
                out = tr.training_step({"image": pool[i % 2][0]}, noise=pool[i % 2][1])
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    sc = trainers[True].scalars(out)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    print(json.dumps(dict(what="config-2 first step (B=32, 256x256)", ms_off=[round(v, 2) for v in ms[False]],
                          ms_on=[round(v, 2) for v in ms[True]], median_off=round(off, 2), median_on=round(on, 2),
                          added_ms=round(on - off, 2), freq_scalar=round(sc["freq"], 6))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="kernel rows only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freq_loss_bench.py needs a GPU")
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)
    kernel_rows(a.reps)
    if not a.no_step:
        step_rows(a.rounds, a.steps)


if __name__ == "__main__":
    main()
