#!/usr/bin/env python3
"""The VQGAN's stride-2 convolution, its 1024-channel attention and the whole default model on one GPU, one JSON line per
measurement, by the method of tools/vqgan_blocks_bench.py: HIP events on the launch stream around --reps launches, the median of
--windows windows after --warmup launches, every window listed (their spread is the measurement's own noise).

  downsample      the five Downsample layers of the default VQGAN at batch 4 (C x H x W = 32 x 512^2, 64 x 256^2, 128 x 128^2,
                  256 x 64^2, 512 x 32^2), forward, input gradient and weight gradient (with dbias) separately, three routes:
                  new       vqw_conv3s2_fwd / _dgrad / _wgrad (nine taps)
                  embedded  the same layer as a 4x4 / stride 2 / pad 1 convolution of the 3x3 kernel embedded in a zero 4x4 one,
                            through vqw_sconv_fwd / _dgrad / _wgrad (sixteen taps): what the kernels could do before
                  torch     F.conv2d on the padded input, and its autograd gradients (for information)
                  `slower_than_embedded` is set when the new route's median exceeds the baseline's by more than the two rows' spread
  self_attention  forward and backward at (4, 16x16, 1024), beside torch's bmm / softmax / bmm composition
  model           one forward + backward of the default VQGAN() on 1 x 1 x 512 x 512: ms and peak memory

    python tools/vqgan_model_bench.py [--reps 20] [--warmup 5] [--windows 5] [--skip-model]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))

PEAK_FP32_MATRIX_TFLOPS = 157.3
LAYERS = ((32, 512), (64, 256), (128, 128), (256, 64), (512, 32))


def timed(fn, args, reps=None):
    import torch
    reps = reps or args.reps
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), ms


def downsample_rows(args):
    import torch
    import torch.nn.functional as F
    from hipops import ops
    L = ops._L()
    CL = torch.channels_last
    N = 4
    for C, S in LAYERS:
        H = W = S
        x = torch.randn(N, C, H, W, device="cuda").contiguous(memory_format=CL)
        w = (torch.randn(C, C, 3, 3, device="cuda") / (3 * C ** 0.5)).contiguous(memory_format=CL)
        w4 = torch.zeros(C, C, 4, 4, device="cuda")
        w4[:, :, 1:, 1:] = w
        w4 = w4.contiguous(memory_format=CL)
        b = torch.randn(C, device="cuda")
        y = torch.empty(N, C, H // 2, W // 2, device="cuda").contiguous(memory_format=CL)
        gy = torch.randn_like(y)
        gx, gw, gw4, gb = torch.empty_like(x), torch.empty_like(w), torch.empty_like(w4), torch.empty_like(b)

        def ws(n):
            return torch.empty(max(int(n), 16), dtype=torch.uint8, device="cuda")
        ws_d, ws_w = ws(L.vqw_conv3s2_dgrad_ws_bytes(C, C)), ws(L.vqw_conv3s2_wgrad_ws_bytes(N, H, W, C, C))
        es_f, es_d = ws(L.vqw_sconv_fwd_ws_bytes(N, H, W, C, C, 4, 2, 1)), ws(L.vqw_sconv_dgrad_ws_bytes(N, H, W, C, C, 4, 2, 1))
        es_w = ws(L.vqw_sconv_wgrad_ws_bytes(C, C, 4, N, H, W, 2, 1))
        xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        yt = F.conv2d(F.pad(xt, (0, 1, 0, 1)), wt, b, stride=2)

        def torch_fwd():
            with torch.no_grad():
                F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
        passes = {
            "forward": (lambda: L.vqw_conv3s2_fwd(x, w, b, y, N, H, W, C, C),
                        lambda: L.vqw_sconv_fwd(x, w4, b, y, es_f, es_f.numel(), N, H, W, C, C, 4, 2, 1, 1.0),
                        torch_fwd),
            "dgrad": (lambda: L.vqw_conv3s2_dgrad(gy, w, gx, ws_d, ws_d.numel(), N, H, W, C, C),
                      lambda: L.vqw_sconv_dgrad(gy, w4, gx, es_d, es_d.numel(), N, H, W, C, C, 4, 2, 1),
                      lambda: torch.autograd.grad(yt, xt, gy, retain_graph=True)),
            "wgrad": (lambda: L.vqw_conv3s2_wgrad(x, gy, gw, gb, ws_w, ws_w.numel(), N, H, W, C, C, 0),
                      lambda: L.vqw_sconv_wgrad(x, gy, gw4, gb, es_w, es_w.numel(), N, H, W, C, C, 4, 2, 1, 0),
                      lambda: torch.autograd.grad(yt, wt, gy, retain_graph=True)),
        }
        flops = 2.0 * N * (H // 2) * (W // 2) * C * C * 9
        for what, fns in passes.items():
            res = {}
            for route, fn in zip(("new", "embedded", "torch"), fns):
                med, ms = timed(fn, args)
                res[route] = (med, ms)
                print(json.dumps(dict(what="downsample " + what, route=route, shape=[N, C, H, W], ms=round(med, 4),
                                      windows_ms=[round(m, 4) for m in ms],
                                      tflops_9tap=round(flops / (med * 1e-3) / 1e12, 2))), flush=True)
            (mn, wn), (me, we) = res["new"], res["embedded"]
            spread = max(max(wn) - min(wn), max(we) - min(we))
            print(json.dumps(dict(what="downsample " + what, shape=[N, C, H, W], new_over_embedded=round(mn / me, 3),
                                  windows_spread_ms=round(spread, 4), slower_than_embedded=bool(mn > me + spread))), flush=True)


def torch_attention(q, k, v, scale):
    import torch
    return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale, dim=2), v)


def attention_rows(args):
    import torch
    from hipops import ops
    L = ops._L()
    B, H, W, C = 4, 16, 16, 1024
    N, scale = H * W, C ** -0.5
    q, k, v, go = (torch.randn(B, N, C, device="cuda") for _ in range(4))
    o, gq, gk, gv = (torch.empty_like(q) for _ in range(4))
    lse, d = torch.empty(B, N, device="cuda"), torch.empty(B, N, device="cuda")
    L.vqw_attention_fwd(q, k, v, o, lse, B, N, C, scale)
    qt, kt, vt = (t.clone().requires_grad_(True) for t in (q, k, v))

    def torch_fwd_bwd():
        torch_attention(qt, kt, vt, scale).backward(go)
        qt.grad = kt.grad = vt.grad = None

    def torch_fwd():
        with torch.no_grad():
            torch_attention(q, k, v, scale)
    f_fwd, f_bwd = 4.0 * B * N * N * C, 14.0 * B * N * N * C          # useful work: the halves' repeated score products not counted
    rows = (("self_attention forward", f_fwd, lambda: L.vqw_attention_fwd(q, k, v, o, lse, B, N, C, scale)),
            ("self_attention backward", f_bwd, lambda: L.vqw_attention_bwd(q, k, v, o, lse, go, d, gq, gk, gv, B, N, C, scale)),
            ("torch bmm/softmax forward", f_fwd, torch_fwd),
            ("torch bmm/softmax forward+backward", None, torch_fwd_bwd))
    for what, flops, fn in rows:
        med, ms = timed(fn, args)
        tf = round(flops / (med * 1e-3) / 1e12, 2) if flops else None
        print(json.dumps(dict(what=what, shape=[B, H, W, C], ms=round(med, 4), windows_ms=[round(m, 4) for m in ms], tflops=tf,
                              share_of_fp32_matrix_peak=round(tf / PEAK_FP32_MATRIX_TFLOPS, 4) if tf else None)), flush=True)


def model_row(args):
    import torch
    from networks import VQGAN
    torch.manual_seed(0)
    m = VQGAN().to("cuda").train()
    x = torch.randn(1, 1, 512, 512, device="cuda").contiguous(memory_format=torch.channels_last)

    def step():
        recon, commit, ids, emb = m(x)
        (recon.square().mean() + commit).backward()
        for p in m.parameters():
            p.grad = None
    torch.cuda.reset_peak_memory_stats()
    med, ms = timed(step, args, reps=max(1, args.reps // 10))
    print(json.dumps(dict(what="VQGAN() forward+backward", shape=[1, 1, 512, 512], parameters=sum(p.numel() for p in m.parameters()),
                          ms=round(med, 3), windows_ms=[round(v, 3) for v in ms],
                          peak_memory_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    downsample_rows(args)
    attention_rows(args)
    if not args.skip_model:
        model_row(args)


if __name__ == "__main__":
    main()
