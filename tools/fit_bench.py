"""ms per step of the trainers.Fit loop on a config (default: configs/baseline2, the benchmark's workload) with logging on
and validation / checkpoints off - the figure to hold against bench.py's ms_per_step on the same machine.

    python tools/fit_bench.py [--config configs/baseline2_256x256_b32_1gpu.json] [--steps 10] [--warmup 3] [--log-every 1]

One epoch of warmup + steps batches of the synthetic dataset; the clock (host, between two device synchronisations) starts
after the warm-up steps and stops when fit() returns.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-every", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fit_bench needs a GPU"
    from trainers import Fit, build_first_step_trainer
    from utils import load_json
    from utils.logger import Logger
    raw = json.load(open(args.config))
    tmp = tempfile.mkdtemp(prefix="fit_bench_")
    raw["run"].update(n_epochs=1, log_every_n_steps=args.log_every)
    raw["dataset"]["n_samples_train"] = raw["dataset"]["batch_size"] * (args.warmup + args.steps)
    raw["save"].update(save_dir=tmp, study_name="fit_bench")
    cfg_path = os.path.join(tmp, "config.json")
    with open(cfg_path, "w") as f:
        json.dump(raw, f)
    config = load_json(cfg_path)
    torch.manual_seed(0)
    trainer = build_first_step_trainer(config, device="cuda", multi_window=False)
    logger = Logger(tmp, config, config.run.monitoring_metrics, name="fit_bench")
    clock = {}

    class Timed(Fit):
        def _log_step(self, out):
            super()._log_step(out)
            if self.global_step + 1 == args.warmup:
                torch.cuda.synchronize()
                clock["t0"] = time.perf_counter()

    fit = Timed(config, trainer, logger, device="cuda", seed=0, validate=False, save_checkpoints=False)
    fit.fit()                      # ends with a device synchronise
    dt = time.perf_counter() - clock["t0"]
    rows = sum(1 for _ in open(os.path.join(logger.log_dir, "log.csv"))) - 1
    print(json.dumps(dict(metric="fit_loop_ms_per_step", ms_per_step=dt / args.steps * 1e3, steps=args.steps, warmup=args.warmup,
                          log_every_n_steps=args.log_every, log_rows=rows, batch=raw["dataset"]["batch_size"],
                          size=raw["dataset"].get("image_size"), num_workers=raw["dataset"].get("num_workers", 0))))


if __name__ == "__main__":
    main()
