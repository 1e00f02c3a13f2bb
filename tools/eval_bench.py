#!/usr/bin/env python3
"""Test-mode evaluation (hipops.ops.recon_metrics + trainers.Evaluator) timed with HIP events at config-5 size
(B = 64, 256 x 256, K = 10) and at 512 x 512 (B = 16): the metric call alone (device-only, no host read), the same
metrics restated in ATen on the GPU (the package's reflect pad / cat / grouped conv / elementwise form plus a bincount
entropy; context only, not a product path), and a whole test step (eval encoder + decoder + metrics + the one host read).
Prints one JSON line per measurement.

    python tools/eval_bench.py [--reps 50] [--steps 10]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))
import torch
import torch.nn.functional as F
from hipops import ops


def aten_metrics(p, t, ids, K, ks=11, sigma=1.5):
    """torchmetrics 0.6.2's arithmetic in fp32 ATen on the GPU (MSE, SSIM, PSNR) and the bincount entropy."""
    d = (p - t)
    mse = (d * d).sum() / p.numel()
    zero = torch.zeros((), device=p.device)
    rng_p = torch.maximum(t.max(), zero) - torch.minimum(t.min(), zero)
    psnr = (2 * torch.log(rng_p) - torch.log(mse)) * (10 / torch.log(torch.tensor(10.0, device=p.device)))
    R = torch.max(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    dist = torch.arange((1 - ks) / 2, (1 + ks) / 2, 1.0, device=p.device)
    g = torch.exp(-(dist / sigma) ** 2 / 2)
    g = (g / g.sum()).unsqueeze(0)
    w = torch.matmul(g.t(), g).expand(p.shape[1], 1, ks, ks)
    pad = (ks - 1) // 2
    pp = F.pad(p, (pad,) * 4, mode="reflect")
    tt = F.pad(t, (pad,) * 4, mode="reflect")
    o = F.conv2d(torch.cat((pp, tt, pp * pp, tt * tt, pp * tt)), w, groups=p.shape[1])
    B = p.shape[0]
    mp, mt, ep, et, ept = (o[i * B:(i + 1) * B] for i in range(5))
    s = ((2 * mp * mt + c1) * (2 * (ept - mp * mt) + c2)) / ((mp * mp + mt * mt + c1) * ((ep - mp * mp) + (et - mt * mt) + c2))
    ssim = s[..., pad:-pad, pad:-pad].mean()
    c = torch.bincount(ids.reshape(-1), minlength=K + 1)[1:].double()
    q = c / c.sum()
    ent = -(torch.where(q > 0, q * torch.log(q), torch.zeros_like(q))).sum() / torch.log(torch.tensor(2.0, dtype=torch.float64))
    return mse, ssim, psnr, ent


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    from networks import UNetEncoder, UNetDecoder
    from trainers import Evaluator
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    K = 10
    torch.manual_seed(0)
    enc = UNetEncoder(1, [16, 32, 64, 128, 256], K, 0.999, 'torch', False, 1, True).cuda().eval()
    dec = UNetDecoder(16, 1, [32, 64, 128, 256, 512], use_dropblock=False, dropped_skip_layers=[],
                      use_pixel_shuffle=False).cuda().eval()
    ev = Evaluator(enc, dec, K)
    for B, S in ((64, 256), (16, 512)):
        g = torch.Generator().manual_seed(S)
        t = torch.tanh(torch.randn(B, 1, S, S, generator=g)).cuda()
        p = torch.tanh(t + 0.1 * torch.randn(B, 1, S, S, generator=g).cuda())
        ids = torch.randint(1, K + 1, (B, S, S), generator=g).cuda().transpose(1, 2)
        n = B * S * S
        hbm_bytes = 2 * (2 * 4 * n) + 8 * n            # stats + SSIM passes read p and t; the histogram reads the ids
        ms, lo, hi = event_ms(lambda: ops._recon_metrics_out(p, t, ids, K, None, 11, 1.5, 0.01, 0.03), args.reps)
        print(json.dumps({"what": "recon_metrics (device only, 4 launches)", "shape": [B, 1, S, S], "K": K,
                          "ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "min_hbm_mb": round(hbm_bytes / 1e6, 1), "effective_tb_s": round(hbm_bytes / ms / 1e9, 2)}),
              flush=True)
        ms_a, lo_a, hi_a = event_ms(lambda: aten_metrics(p, t, ids, K), args.reps)
        print(json.dumps({"what": "ATen restatement (fp32, GPU)", "shape": [B, 1, S, S], "K": K, "ms": round(ms_a, 4),
                          "ms_min": round(lo_a, 4), "ms_max": round(hi_a, 4), "speedup": round(ms_a / ms, 1)}), flush=True)
        got = ops.recon_metrics_values(p, t, ids, K)
        ref = [float(v) for v in aten_metrics(p, t, ids, K)]
        print(json.dumps({"what": "values (kernel vs ATen fp32)", "shape": [B, 1, S, S],
                          "kernel": [got["mse"], got["ssim"], got["psnr"], got["entropy"]], "aten": ref}), flush=True)
        image = t
        batch = {"image": image}
        step_ms, step_lo, step_hi = event_ms(lambda: ev.test_step(batch), max(1, args.steps))
        print(json.dumps({"what": "Evaluator.test_step (eval forward + metrics + host read)", "shape": [B, 1, S, S],
                          "ms": round(step_ms, 3), "ms_min": round(step_lo, 3), "ms_max": round(step_hi, 3),
                          "metrics_share": round(ms / step_ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
