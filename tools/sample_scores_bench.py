#!/usr/bin/env python3
"""The sample-score operators (hipops.ops.feature_moments, knn_radius, ball_counts) timed with HIP events at N = M in {2048, 16384},
D = 512, window by window in alternation with a plain-torch restatement on the same GPU (a double X^T X; cdist + kthvalue; cdist +
a comparison - context only, not a product path), with the peak memory of either side; then one PriorTrainer.score call at the
size of configs/prior_vqgan_512_score.json's models (random weights, fewer slices) split into sampling, decoding, encoding and
scoring.  One JSON line per measurement, appended to --out.

    python tools/sample_scores_bench.py [--out profiles/sample_scores_bench.jsonl] [--windows 5] [--no-score]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "medical-image-editing_amd"))
import torch
from hipops import ops


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stage_s(fn):
    """Seconds of one call between two synchronisations."""
    import time
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def alternate(ours, theirs, windows, reps):
    """Windows of `reps` calls, ours and theirs in turn -> (median ms ours, median ms theirs, all windows)."""
    for fn in (ours, theirs):
        fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(windows):
        a.append(window_ms(ours, reps))
        b.append(window_ms(theirs, reps))
    return statistics.median(a), statistics.median(b), a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_scores_bench.jsonl"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-score", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_scores_bench needs a GPU"
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    emit(device=torch.cuda.get_device_name(0))
    D, k = 512, 3
    for N in (2048, 16384):
        g = torch.Generator().manual_seed(N)
        real = (torch.randn(N, D, generator=g) + 5.0).cuda()
        fake = (1.1 * torch.randn(N, D, generator=g) + 5.1).cuda()
        shift = real[:64].mean(dim=0)
        reps = 4 if N <= 2048 else 1
        s, o = torch.zeros(D, dtype=torch.float64, device="cuda"), torch.zeros((D, D), dtype=torch.float64, device="cuda")

        def moments_torch():
            y = (real - shift).double()
            return y.sum(0), y.T @ y

        ms, ms_t, w, w_t = alternate(lambda: ops.feature_moments(real, s, o, shift), moments_torch, args.windows, reps)
        emit(what="feature_moments (plain double FMAs)", N=N, D=D, ms=round(ms, 4), torch_ms=round(ms_t, 4), windows=[round(v, 4) for v in w],
             torch_windows=[round(v, 4) for v in w_t], gflops_double=round(2.0 * N * D * D / ms / 1e6, 1),
             peak_mb=round(peak_mb(lambda: ops.feature_moments(real, s, o, shift)), 2), torch_peak_mb=round(peak_mb(moments_torch), 2),
             ws_mb=round(ops._L().vqw_feature_moments_ws_bytes(N, D) / 2 ** 20, 2))

        def knn_torch():
            y = real - shift
            d = torch.cdist(y, y).square_()
            d.fill_diagonal_(float("inf"))
            return d.kthvalue(k, dim=1).values

        ms, ms_t, w, w_t = alternate(lambda: ops.knn_radius(real, k, shift), knn_torch, args.windows, reps)
        emit(what="knn_radius", N=N, D=D, k=k, ms=round(ms, 4), torch_ms=round(ms_t, 4), windows=[round(v, 4) for v in w],
             torch_windows=[round(v, 4) for v in w_t], tflops_fp32=round(2.0 * N * N * D / ms / 1e9, 2),
             peak_mb=round(peak_mb(lambda: ops.knn_radius(real, k, shift)), 2), torch_peak_mb=round(peak_mb(knn_torch), 2),
             ws_mb=round(ops._L().vqw_knn_radius_ws_bytes(N) / 2 ** 20, 3), n_by_m_mb=round(4.0 * N * N / 2 ** 20, 1))
        r2 = ops.knn_radius(real, k, shift)

        def balls_torch():
            inside = torch.cdist(fake - shift, real - shift).square_() <= r2[None, :]
            return inside.sum(1, dtype=torch.int32), inside.sum(0, dtype=torch.int32)

        ms, ms_t, w, w_t = alternate(lambda: ops.ball_counts(fake, real, r2, shift), balls_torch, args.windows, reps)
        emit(what="ball_counts", N=N, M=N, D=D, ms=round(ms, 4), torch_ms=round(ms_t, 4), windows=[round(v, 4) for v in w],
             torch_windows=[round(v, 4) for v in w_t], tflops_fp32=round(2.0 * N * N * D / ms / 1e9, 2),
             peak_mb=round(peak_mb(lambda: ops.ball_counts(fake, real, r2, shift)), 2), torch_peak_mb=round(peak_mb(balls_torch), 2),
             ws_mb=round(ops._L().vqw_ball_counts_ws_bytes(N, N) / 2 ** 20, 3), n_by_m_mb=round(4.0 * N * N / 2 ** 20, 1))
        del real, fake, s, o, r2
    if not args.no_score:
        from utils import load_json
        from trainers import build_prior_trainer
        cfg = load_json(os.path.join(ROOT, "configs", "prior_vqgan_512_score.json"))
        torch.manual_seed(0)
        tr = build_prior_trainer(cfg, device="cuda:0")
        n = 64
        images = [torch.tanh(torch.randn(16, 1, 512, 512, generator=torch.Generator().manual_seed(i))) for i in range(n // 16)]
        kw = dict(n_samples=n, batch_size=16, k=3, top_k=32, top_p=0.95, against="recon")
        tr.score(images, generator=torch.Generator(device="cuda").manual_seed(0), **kw)          # warm-up
        total = stage_s(lambda: tr.score(images, generator=torch.Generator(device="cuda").manual_seed(0), **kw))
        # the stages of that call, each run on its own between two synchronisations (score() itself has no clock)
        from functions import FeatureStats, sample_scores
        gen = torch.Generator(device="cuda").manual_seed(0)
        dev = [im.cuda() for im in images]
        ids = []
        sampling = stage_s(lambda: ids.extend(tr._score_sample_ids(16, 1.0, 32, 0.95, gen) for _ in range(n // 16)))
        pics = []
        decoding = stage_s(lambda: pics.extend(tr.vqgan.decode_from_ids(i, tr.h, tr.w) for i in ids))
        feats = []
        encoding = stage_s(lambda: feats.extend(tr.features(p) for p in pics + dev))

        def scoring():
            fake, real = torch.cat(feats[:n // 16]), torch.cat(feats[n // 16:])
            shift = real[:16].mean(dim=0)
            stats = [FeatureStats(real.shape[1], shift, keep=n) for _ in range(4)]
            for st, x in zip(stats, (real, fake, real[0::2], real[1::2])):
                st.add(x)
            sample_scores(stats[0], stats[1], 3)
            sample_scores(stats[2], stats[3], 3)

        emit(what="PriorTrainer.score (random weights; models of configs/prior_vqgan_512_score.json)", n_slices=n, n_samples=n, batch_size=16,
             total_s=round(total, 4), stages_s=dict(sampling=round(sampling, 4), decoding=round(decoding, 4),
                                                    encoding_2n_pictures=round(encoding, 4), scoring=round(stage_s(scoring), 4)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
