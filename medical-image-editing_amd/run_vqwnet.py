"""Launcher: train, validate, test and export a VQ-W-Net from a config (the reference's run_vqwnet.py:61-155 command line).

    python run_vqwnet.py -c CONFIG [-m train|test] [-w] [-v | -p]
    python run_vqwnet.py -c CONFIG -p -m edit
    python run_vqwnet.py -c CONFIG -p -m detect
    python run_vqwnet.py -c CONFIG -p -m synth
    python run_vqwnet.py -c CONFIG -p -m score

run.training_mode picks the work: `first_step` / `second_step` train (-m train) or are scored (-m test: result.csv in the
run directory); `inference` (-m test only) exports PNG and NIfTI files per slice.  -w selects the multi-window step and
needs loss.recon_weights and dataset.window_width / window_center / window_scale.  -v trains the VQGAN of model.vqgan against
the U-Net discriminator (trainers/vqgan_unet_dis.py) whatever -w and run.training_mode say - the reference's step has no mode
dispatch - and needs model.vqmodel.model_name 'VQGAN' and the model.vqgan section; that trainer has no test step, so -v with
-m test or with training_mode 'inference' is refused.  -p trains the GPT code prior of model.prior on the codes of the frozen VQGAN
of model.vqgan (trainers/prior.py; run.first_stage_ckpt_path names the -v checkpoint the VQGAN's weights come from): it needs the
model.vqgan, model.prior and prior_optim sections, validates (cross-entropy and perplexity), writes a picture and a checkpoint per
epoch and resumes from run.resume_checkpoint.  -p is refused with -v, with -m test, with training_mode 'inference' and with
run.num_gpus > 1 (data-parallel prior training is not built).  -p -m edit edits slices with a trained prior (Fit.edit): the
prior of run.resume_checkpoint redraws the codes of the region the `edit` section selects (box, mask_path or nll_threshold) in the
first edit.n_slices test slices, edit.n_candidates times each, and keeps the likeliest; pictures, codes and scores go to
<run dir>/edit/.  The optional edit.{blend, blend_levels, blend_source} blend the composite tile over a pyramid in place of the hard
per-cell paste (ops.blend_cells; the same three keys under `synth` for its edit through the label map); absent, every file is what it
was.  -m edit without -p is refused.  -p -m detect localises anomalies with a trained prior (Fit.detect): the prior
of run.resume_checkpoint restores the codes whose token_nll exceeds detect.nll_threshold, the smoothed pixel residual is the
anomaly map of a slice (ops.anomaly_map), and with detect.labels the maps are scored against the lesion labels - AUROC, average
precision and the best Dice over all pixels (detect_result.csv beside detect.csv and the pictures in the run directory).  -m detect
without -p, or with -v, is refused.  With model.prior.cond the prior is conditioned on the label maps the loaders deliver
(trainers/cond_prior.py: one conditioning token per latent cell in front of the codes); -p -m synth (Fit.synth) then draws slices
from the label maps of the first synth.n_slices test slices and, with synth.discs, edits each slice through its label map -
pictures and synth.csv under <run dir>/synth/.  -m synth without -p, without model.prior.cond or without run.resume_checkpoint is
refused, and so is -m detect with model.prior.cond.  Classifier-free guidance is opt-in by keys: model.prior.cond.{null_token,
p_uncond, drop_seed} train the prior with the condition dropped onto a null embedding some of the time, and
synth.{guidance_scale, rank} (edit.{guidance_scale, rank}) draw from z_u + scale (z_c - z_u); absent keys mean off.
With model.prior.masked = {n_steps, choice_temperature, mask_seed} -p trains the bidirectional masked prior instead
(trainers/masked_prior.py: networks.MaskedGPT learns to fill in masked codes) and -p -m edit fills the region in again in
edit.n_steps (default: masked.n_steps) parallel passes that see the kept codes on both sides; edit.nll_threshold and
model.prior.cond are refused with it, and so is -m detect without detect.pseudo.  Absent or `false`, every mode is what it was.
The masked prior's own opinion of a slice is its pseudo-likelihood map (MaskedPriorTrainer.pseudo_nll: -log p(code | the codes
outside its lattice group), from both sides): edit.pnll_threshold, with the optional edit.stride = [sy, sx], is one more selector
of -p -m edit - the codes whose map exceeds it - and detect.pseudo = {threshold, stride} with detect.nll_threshold false runs
-p -m detect on the masked prior (MaskedPriorTrainer.detect_pseudo); detect.csv's mean_nll column then holds the mean pseudo-NLL.
With model.prior.masked.cond (model.prior.cond's keys) the masked prior is conditioned on the label maps
(trainers/masked_cond_prior.py: the label token of a latent cell is added to the embedding of its position, the sequence stays h w
long): -p trains p(codes | label map), -p -m synth decodes slices from label maps alone in synth.n_steps (default: masked.n_steps)
parallel passes and edits them through synth.discs, -p -m edit and -p -m score run under the slices' own label maps, and the guidance
keys work as for model.prior.cond; edit.pnll_threshold reads the map under the slice's own label; -m detect stays refused, with
detect.pseudo too.
-p -m score scores the samples of the prior of run.resume_checkpoint against the first score.n_slices test slices (Fit.score): the
Frechet distance, precision / recall and density / coverage in the frozen first stage's own feature space and the divergence of the
code histograms, each beside its floor - the same score between two halves of the real slices - in <run dir>/score/score.csv and
score.json.  -m score without -p, without run.resume_checkpoint or with score.n_samples < score.k + 1 is refused.

One process per GPU.  With run.num_gpus == 1 this process is the worker.  With more, this process never touches the GPU:
it starts num_gpus fresh interpreters of this file (`--rank r`, RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their
environment), waits for them, and when one fails it terminates the others and exits non-zero.  VQW_DP_ONE_DEVICE=1 puts
every rank on cuda:0 with the gloo backend (a rehearsal of the multi-process path on one card).
"""
import argparse
import os
import random
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

MAX_GPUS = 8
WINDOW_KEYS = ("loss.recon_weights", "dataset.window_width", "dataset.window_center", "dataset.window_scale")
TRAINING_MODES = ("first_step", "second_step", "inference")


def build_parser():
    parser = argparse.ArgumentParser(description="Train, score or export a VQ-W-Net from a JSON config")
    parser.add_argument("-c", "--config", required=True, help="path of the JSON config")
    parser.add_argument("-m", "--mode", default="train", help="train (default), test, or edit / detect / synth (with -p)")
    parser.add_argument("-w", "--multiwindow", action="store_true", help="multi-window training step")
    parser.add_argument("-v", "--vqgan", action="store_true", help="train the VQGAN (model.vqgan) with the U-Net discriminator; overrides -w")
    parser.add_argument("-p", "--prior", action="store_true", help="train the GPT code prior (model.prior) on the codes of the VQGAN (model.vqgan)")
    parser.add_argument('--rank', type=int, default=None, help='set by the launcher for its worker processes')
    parser.add_argument('--seed', type=int, default=None, help='set by the launcher: the seed all workers share')
    return parser


def _get(cfg, name, default=None):
    v = getattr(cfg, name, None) if cfg is not None else None
    return default if v is None else v


def _lookup(config, dotted):
    node = config
    for part in dotted.split("."):
        node = getattr(node, part, None)
        if node is None:
            return None
    return node


def check_arguments(config, args):
    """Everything that can be refused before a device is touched or a process started."""
    prior = bool(getattr(args, "prior", False))
    if prior and args.vqgan:
        raise ValueError("-p with -v: one run trains the VQGAN (-v) or the prior on its codes (-p), not both")
    if args.vqgan:
        from trainers.config import check_vqgan_config
        check_vqgan_config(config)              # NotImplementedError naming the VQGAN trainer and the missing keys
    if prior:
        from trainers.config import check_prior_config
        check_prior_config(config)              # NotImplementedError naming the prior trainer and the missing keys
    if args.mode == "edit":
        if not prior:
            raise ValueError("-m edit: editing redraws the codes of a region with the code prior and needs -p")
        from trainers.config import check_edit_config
        check_edit_config(config)               # NotImplementedError naming the missing keys of the `edit` section
    elif args.mode == "detect":
        if not prior:
            raise ValueError("-m detect: detection restores the unlikely codes with the code prior and needs -p")
        from trainers.config import check_detect_config
        check_detect_config(config)             # NotImplementedError naming the missing keys of the `detect` section
        from trainers.config import prior_condition
        if prior_condition(config) is not None:
            raise NotImplementedError("-m detect with model.prior.cond: a prior conditioned on the lesion labels is told where the lesion "
                                      "is; detection needs the unconditional prior")
        from trainers.config import detect_pseudo, prior_masked
        if prior_masked(config) is not None and detect_pseudo(config) is None:          # with detect.pseudo: MaskedPriorTrainer.detect_pseudo
            raise NotImplementedError("-m detect with model.prior.masked: detection selects the codes to restore by a raster-order "
                                      "likelihood, which the masked prior does not define; it needs the autoregressive prior")
    elif args.mode == "synth":
        if not prior:
            raise ValueError("-m synth: synthesis draws slices from label maps with the conditional code prior and needs -p")
        from trainers.config import check_synth_config
        check_synth_config(config)              # NotImplementedError naming the missing part
    elif args.mode == "score":
        if not prior:
            raise ValueError("-m score: scoring compares the code prior's samples with held-out slices and needs -p")
        from trainers.config import check_score_config
        check_score_config(config)              # NotImplementedError naming the missing part, ValueError for a value out of range
    elif args.mode not in ("train", "test"):
        raise ValueError("-m %r: the mode is 'train' or 'test' (or, with -p, 'edit', 'detect', 'synth' or 'score')" % (args.mode,))
    mode = _get(config.run, "training_mode", "first_step")
    if mode not in TRAINING_MODES:
        raise ValueError("run.training_mode %r: one of %s" % (mode, ", ".join(TRAINING_MODES)))
    if args.vqgan and (args.mode == "test" or mode == "inference"):
        raise ValueError("-v: the VQGAN trainer has no test step and no inference export (the reference defines neither); "
                         "it trains with -m train and run.training_mode first_step or second_step")
    if prior and (args.mode == "test" or mode == "inference"):
        raise ValueError("-p: the prior trainer has no test step and no inference export; it trains with -m train and "
                         "run.training_mode first_step or second_step")
    if prior and int(_get(config.run, "num_gpus", 1)) > 1:
        raise ValueError("-p with run.num_gpus = %d: data-parallel training of the prior is not built (out of scope); "
                         "set run.num_gpus to 1" % int(_get(config.run, "num_gpus", 1)))
    if mode == "inference" and args.mode != "test":
        raise ValueError("run.training_mode 'inference' exports with -m test; it cannot be trained (-m %s)" % args.mode)
    if args.multiwindow and not args.vqgan and not prior:         # -v and -p override -w
        missing = [k for k in WINDOW_KEYS if _lookup(config, k) is None]
        if missing:
            raise ValueError("-w (multi-window) needs the config keys %s; missing: %s" % (", ".join(WINDOW_KEYS), ", ".join(missing)))
    n = int(_get(config.run, "num_gpus", 1))
    if n < 1 or n > MAX_GPUS:
        raise ValueError("run.num_gpus = %d: one node of 1..%d GPUs" % (n, MAX_GPUS))
    return mode, n


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args, num_gpus, seed, child_command=None, poll_seconds=0.2, grace_seconds=10.0):
    """Start one worker per GPU and wait -> exit status (0, or the first failing worker's).  This process creates no GPU
    context.  child_command: the command line up to the per-rank arguments (default: this file under this interpreter)."""
    base = list(child_command) if child_command is not None else [sys.executable, os.path.abspath(__file__)]
    common = ["-c", args.config, "-m", args.mode, "--seed", str(seed)] + (["-w"] if args.multiwindow else []) + (["-v"] if args.vqgan else []) + (["-p"] if getattr(args, "prior", False) else [])
    env = dict(os.environ, WORLD_SIZE=str(num_gpus), MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"),
               MASTER_PORT=os.environ.get("MASTER_PORT") or str(_free_port()))
    procs = []
    for r in range(num_gpus):
        procs.append(subprocess.Popen(base + common + ["--rank", str(r)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r))))
    status = 0
    live = list(procs)
    while live and status == 0:
        time.sleep(poll_seconds)
        for p in list(live):
            rc = p.poll()
            if rc is None:
                continue
            live.remove(p)
            if rc != 0:
                status = rc if rc > 0 else 1
                print("run_vqwnet: worker %d exited with status %d; stopping the others" % (procs.index(p), rc), file=sys.stderr)
                break
    if status != 0:
        for p in live:
            p.terminate()
        deadline = time.time() + grace_seconds
        for p in live:
            try:
                p.wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return status


def seed_everything(seed):
    import numpy as np
    import torch
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)


def _digest(trainer, fit, path, rank):
    """Test aid (VQW_RUN_DIGEST=<path prefix>): a hash per module of this rank's parameters and buffers, and the sample
    indices its sampler handed out."""
    import hashlib
    import json
    import torch
    out = {"rank": rank, "modules": {}, "seen": fit.sampler.seen if fit.sampler is not None else []}
    for name, m in trainer.modules().items():
        h = hashlib.sha256()
        for k, v in m.state_dict().items():
            h.update(k.encode())
            h.update(v.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
        out["modules"][name] = h.hexdigest()
    with open("%s.rank%d.json" % (path, rank), "w") as f:
        json.dump(out, f)


def worker(config, args, training_mode, rank, world_size, seed):
    import torch
    import torch.distributed as dist
    from trainers import Fit, InferenceModels, build_first_step_trainer, build_second_step_trainer, build_vqgan_trainer, build_prior_trainer
    from utils.logger import Logger

    seed_everything(seed)                       # shared by all ranks: the replicas start from the same weights
    print('Seed: {}'.format(seed))
    if rank == 0:
        print('Config: ', config)
    distributed = world_size > 1
    device = "cuda:0"
    if distributed:
        one_device = os.environ.get("VQW_DP_ONE_DEVICE", "0") == "1"
        device = "cuda:0" if one_device else "cuda:%d" % rank
        torch.cuda.set_device(torch.device(device))
        dist.init_process_group("gloo" if one_device else "nccl", rank=rank, world_size=world_size)
    try:
        if getattr(args, "prior", False):
            trainer = build_prior_trainer(config, device=device)
        elif args.vqgan:
            trainer = build_vqgan_trainer(config, device=device, data_parallel=distributed)
        elif training_mode == "first_step":
            trainer = build_first_step_trainer(config, device=device, data_parallel=distributed,
                                               multi_window=None if args.multiwindow else False)
        elif training_mode == "second_step":
            trainer = build_second_step_trainer(config, device=device, data_parallel=distributed,
                                                multi_window=None if args.multiwindow else False)
        else:
            trainer = InferenceModels(config, device=device)
        # utils/init_seed.py:14-24: from here on every rank has its own seed; all of them are saved with the config
        seed_list = _get(config.run, "seed_list")
        rank_seed = int(seed_list[rank]) if seed_list else random.randint(1, 10000)
        seed_everything(rank_seed)
        print('Seed set to {} in gpu-rank: {}'.format(rank_seed, rank))
        seeds = [rank_seed]
        if distributed:
            seeds = [None] * world_size
            dist.all_gather_object(seeds, rank_seed)
        logger = None
        if rank == 0:
            logger = Logger(save_dir=config.save.save_dir, config=config, name=config.save.study_name,
                            monitoring_metrics=config.run.monitoring_metrics)
        fit = Fit(config, trainer, logger, device=device, rank=rank, world_size=world_size, seed=rank_seed, seeds=seeds,
                  data_seed=seed)
        if training_mode == "inference":
            fit.export()
        elif args.mode == "edit":
            fit.edit()
        elif args.mode == "detect":
            fit.detect()
        elif args.mode == "synth":
            fit.synth()
        elif args.mode == "score":
            fit.score()
        elif args.mode == "train":
            fit.fit()
        else:
            fit.test()
        if os.environ.get("VQW_RUN_DIGEST"):
            _digest(trainer, fit, os.environ["VQW_RUN_DIGEST"], rank)
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
    finally:
        if distributed and dist.is_initialized():
            dist.destroy_process_group()


def main(argv=None, child_command=None):
    args = build_parser().parse_args(argv)
    from utils import load_json
    config = load_json(args.config)
    training_mode, num_gpus = check_arguments(config, args)
    seed = args.seed if args.seed is not None else (_get(config.run, "seed") or random.randint(1, 10000))
    if num_gpus > 1 and args.rank is None:
        return launch(args, num_gpus, seed, child_command=child_command)
    rank = args.rank if args.rank is not None else 0
    worker(config, args, training_mode, rank, num_gpus, int(seed))
    return 0


if __name__ == '__main__':
    sys.exit(main())
