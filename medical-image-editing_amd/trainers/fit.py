"""The training run: epochs, logging, validation pictures, checkpoints, resume, test-mode scoring and the inference
export (reference: run_vqwnet.py:61-129, trainers/base.py:116-187, single_window_trainer.py:541-644, 716-779), as a plain
class over the trainers of this package - no PyTorch-Lightning.

    Fit(config, trainer, logger).fit()            train run.n_epochs epochs (from run.resume_checkpoint when set); with a
                                                  trainers.PriorTrainer (-p): the same loop, validate_prior per epoch
    Fit(config, trainer, logger).test()           result.csv of trainers.evaluation.Evaluator over the test loader
    Fit(config, trainer, logger).export()         training_mode 'inference': PNG + NIfTI of image, recon, label per slice
    Fit(config, trainer, logger).edit()           -p -m edit: PriorTrainer.edit over the first test slices -> pictures, codes, scores
    Fit(config, trainer, logger).detect()         -p -m detect: PriorTrainer.detect over the test slices -> anomaly maps, AUROC / AP / Dice
    Fit(config, trainer, logger).score()          -p -m score: PriorTrainer.score against the test slices -> score.csv, score.json

Nothing here reads a scalar from the device inside a step: the logged losses of a step go to the host in one small
copy that is looked at two steps later (after that step's StepThrottle event), so the loop adds host work only.
"""
import collections
import contextlib
import os
import random

import numpy as np
import torch
from torch.utils.data.distributed import DistributedSampler

from dataio import get_data_loader
from hipops import ops
from utils import checkpoint as ckpt_io
from utils import logger as run_logger
from utils import nifti, png

from .base import TrainerBase
from .config import configure_models
from .first_step import FlipViews, LUNG_WINDOW, MEDIASTINAL_WINDOW, LossWeights
from .evaluation import Evaluator
from .vqgan_unet_dis import VQGANUNetDisTrainer
from .prior import PriorTrainer
from .label_cond import LabelConditionMixin

LIMIT_VAL_BATCHES = 2              # run_vqwnet.py:127
SANITY_VAL_BATCHES = 2             # run_vqwnet.py:125
CKPT_LIMIT_NUM, CKPT_SAVE_INTERVAL = 10, 10        # run_vqwnet.py:72-74
DEFAULT_LOG_EVERY_N_STEPS = 50     # Lightning 1.5's Trainer default, which the reference does not override
DEFAULT_NOISE_STD = 0.02           # the second view's additive noise when there is no `augmentation` section


def _get(cfg, name, default=None):
    v = getattr(cfg, name, None) if cfg is not None else None
    return default if v is None else v


def dataset_window(config):
    d = config.dataset
    if all(_get(d, k) is not None for k in ("window_width", "window_center", "window_scale")):
        return (d.window_width, d.window_center, d.window_scale)
    return None


def build_loader(config, mode, seed=0, sampler=None, generator=None, label_modality=None, lesions=None):
    """The reference's train / val / test loader (base.py:116-162) from config.dataset.  The file datasets shuffle their
    file list once at construction with Python's `random`: it is seeded from (seed, mode) around the construction - and
    put back - so the list is the same in every process and run that names the same seed.  label_modality / lesions: the opt-in
    labels of get_data_loader (Fit.detect)."""
    d = config.dataset
    state = random.getstate()
    random.seed(int(seed) * 3 + ("train", "val", "test").index(mode))
    try:
        return get_data_loader(
            mode=mode, dataset_name=d.dataset_name, root_dir_path=_get(d, "root_dir_path"), batch_size=d.batch_size,
            num_workers=_get(d, "num_workers", 0), modality=_get(d, "modality"),
            augmentations=_get(d, "augmentations") if mode == "train" else None, drop_last=mode == "train",
            window_width=_get(d, "window_width"), window_center=_get(d, "window_center"), window_scale=_get(d, "window_scale"),
            sampler=sampler, generator=generator, image_size=_get(d, "image_size"), n_samples=_get(d, "n_samples_" + mode),
            seed=seed, label_modality=label_modality, lesions=lesions)
    finally:
        random.setstate(state)


# ----------------------------------------------------------------------------------------------------
# logged scalars: the reference's self.log keys and weighting (single_window_trainer.py:149-159, 490-499)
# ----------------------------------------------------------------------------------------------------
def _first_step_terms(out):
    names = ["total", "commit_1", "commit_2", "cross", "dist", "reg", "recon_l1", "recon_l2", "freq_1", "freq_2",
             "perceptual_1", "perceptual_2"]
    return [(n, out[n]) for n in names if n in out]


def _first_step_row(v, w):
    f = np.float32
    pair = lambda a, b: f(v.get(a, 0.0)) + f(v.get(b, 0.0))  # noqa: E731
    return {"total": v["total"], "gen_total": v["total"], "commit": f(w.commit) * pair("commit_1", "commit_2"),
            "cross": f(w.cross) * f(v["cross"]), "dist": f(w.dist) * f(v["dist"]), "reg": f(w.reg) * f(v["reg"]),
            "recon": f(w.recon) * pair("recon_l1", "recon_l2"), "freq": f(w.freq) * pair("freq_1", "freq_2"),
            "perceptual": f(w.perceptual) * pair("perceptual_1", "perceptual_2")}


def _second_step_terms(out):
    names = ("gen_total", "dis_total", "recon", "gen", "freq", "perceptual", "commit", "unet_perceptual", "dis", "cutmix", "consistency")
    return [(n, out[n]) for n in names if out.get(n) is not None]


_SWITCHED_OFF_IS_ZERO = ("recon", "freq", "perceptual", "unet_perceptual")      # terms a step leaves out when they are off


def _second_step_row(v, w):
    """The row of a second step or of the VQGAN step, from the fields its loss weights have (U-Net: single_window_trainer.py:361-374;
    VQGAN: vqgan_unet_dis.py:121-136, the only one with `commit`)."""
    f = np.float32
    term = lambda k: f(getattr(w, k)) * f(v.get(k, 0.0) if k in _SWITCHED_OFF_IS_ZERO else v[k])  # noqa: E731
    row = {"total": f(v["gen_total"]) + f(v["dis_total"]), "gen_total": v["gen_total"]}
    row.update((k, term(k)) for k in ("recon", "freq", "perceptual", "commit", "gen", "unet_perceptual") if k in w._fields)
    row["dis_total"] = v["dis_total"]
    if "cutmix" in w._fields:
        row.update((k, term(k)) for k in ("dis", "cutmix", "consistency"))
    else:                            # the PatchGAN step has one discriminator term: `dis` is its total
        row["dis"] = v["dis_total"]
    return row


class _ScalarQueue:
    """Logged scalars on their way to the host.  push() packs a step's 0-d device tensors into one small tensor and
    starts its copy into a pinned buffer; a row is handed to `emit` once `lag` later steps have been pushed (by then the
    throttle has waited for that step's event, so waiting for the copy's own event does not stall the GPU) or on flush()."""

    def __init__(self, emit, lag, cuda):
        self.emit, self.lag, self.cuda = emit, lag, cuda
        self.pending = collections.deque()
        self.age = 0

    def push(self, meta, named):
        names = [n for n, _ in named]
        tensors = [t.detach().reshape(()).float() if torch.is_tensor(t) else None for _, t in named]
        consts = {n: float(t) for (n, t), x in zip(named, tensors) if x is None}
        names = [n for n, x in zip(names, tensors) if x is not None]
        packed = torch.stack([x for x in tensors if x is not None])
        if self.cuda:
            host = torch.empty(packed.shape, dtype=torch.float32, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream())
        else:
            host, event = packed.clone(), None
        self.pending.append((self.age, meta, names, consts, host, event))

    def step(self):
        """One training step has been enqueued: emit what is `lag` steps old."""
        self.age += 1
        while self.pending and self.age - self.pending[0][0] > self.lag:
            self._pop()

    def flush(self):
        while self.pending:
            self._pop()

    def _pop(self):
        _, meta, names, consts, host, event = self.pending.popleft()
        if event is not None:
            event.synchronize()
        values = dict(consts)
        values.update({n: np.float32(x) for n, x in zip(names, host.numpy())})
        self.emit(meta, values)


def _rng_state(device):
    st = {"torch_cpu": torch.get_rng_state(), "python": list(_flatten_py(random.getstate())),
          "numpy": _numpy_state()}
    if device.type == "cuda":
        st["torch_device"] = torch.cuda.get_rng_state(device)
    return st


def _flatten_py(state):
    version, internal, gauss = state
    return [int(version), [int(x) for x in internal], gauss]


def _numpy_state():
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return {"name": name, "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
            "cached_gaussian": float(cached)}


def _set_rng_state(st, device):
    torch.set_rng_state(st["torch_cpu"])
    version, internal, gauss = st["python"]
    random.setstate((version, tuple(internal), gauss))
    n = st["numpy"]
    np.random.set_state((n["name"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    if device.type == "cuda" and "torch_device" in st:
        torch.cuda.set_rng_state(st["torch_device"], device)


class _RecordingSampler(DistributedSampler):
    """DistributedSampler that remembers what it handed out: `seen` = [(epoch, this rank's sample indices)]."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.seen = []

    def __iter__(self):
        indices = list(super().__iter__())
        self.seen.append((self.epoch, indices))
        return iter(indices)


class InferenceModels(TrainerBase):
    """Encoder and decoder alone, behind the part of the trainers' interface Fit.test() / Fit.export() use: what
    `training_mode: "inference"` needs (no optimisers, no losses)."""

    def __init__(self, config, device="cuda"):
        super().__init__(device)
        self.encoder, self.decoder = configure_models(config)
        self.encoder.to(self.device).eval()
        self.decoder.to(self.device).eval()
        self.dict_size = config.model.vqmodel.dict_size
        self.w = LossWeights()

    def modules(self):
        return {"encoder": self.encoder, "decoder": self.decoder}

    def optimizers(self):
        return {}


class Fit:
    """seed: this rank's seed (run.seed_list[rank]: the noise generator); data_seed: the seed every rank shares (run.seed:
    dataset file order, the distributed sampler's permutation, the loaders' generators); seeds: all ranks' seeds, saved
    with the hyper-parameters."""

    def __init__(self, config, trainer, logger=None, device="cuda", rank=0, world_size=1, seed=0, seeds=None,
                 data_seed=None, validate=True, save_checkpoints=True, log=print):
        self.config, self.trainer, self.logger = config, trainer, logger
        self.device = torch.device(device)
        self.rank, self.world_size = int(rank), int(world_size)
        self.seed = int(seed)
        self.data_seed = int(data_seed) if data_seed is not None else self.seed
        self.seeds = list(seeds) if seeds is not None else [self.seed]
        self.do_validate, self.do_save = validate, save_checkpoints
        self.print = log
        self.mode = _get(config.run, "training_mode", "first_step")
        # the VQGAN trainer (-v) has one step, a generator half and a discriminator half, whatever training_mode names
        # (vqgan_unet_dis.py has no mode dispatch): the loop and the log treat it as a second step
        self.vqgan = isinstance(trainer, VQGANUNetDisTrainer)
        if self.vqgan:
            self.mode = "second_step"
        # the prior trainer (-p) has a step, a validation and a picture of its own (PriorTrainer's methods); the loop, the
        # lagged log, the checkpoints and the resume are the ones of every run
        self.prior = isinstance(trainer, PriorTrainer)
        if self.prior:
            self.mode = "prior"
        # the conditional priors (model.prior.cond, model.prior.masked.cond): every loader delivers the label maps beside the slices
        self.cond = None
        if isinstance(trainer, LabelConditionMixin):
            from .config import prior_condition
            self.cond = prior_condition(config)
        self.dict_size = trainer.dict_size if self.vqgan or self.prior else config.model.vqmodel.dict_size
        self.n_epochs = int(_get(config.run, "n_epochs", 1))
        self.log_every = int(_get(config.run, "log_every_n_steps", DEFAULT_LOG_EVERY_N_STEPS))
        self.noise_std = float(_get(config.run, "noise_std", DEFAULT_NOISE_STD))
        self.epoch, self.global_step = 0, 0
        # generators the run owns, so that a checkpoint can hold them: the training shuffle (and workers' seeds), the
        # validation shuffle, the second view's additive noise
        self.train_gen = torch.Generator().manual_seed(self.data_seed)
        self.val_gen = torch.Generator().manual_seed(self.data_seed + 1)
        self.noise_gen = torch.Generator(device=self.device).manual_seed(self.seed)
        self.sampler = None
        self._loaders = {}
        throttle = getattr(trainer, "throttle", None)
        self.queue = _ScalarQueue(self._emit_row, lag=getattr(throttle, "max_inflight", 2), cuda=self.device.type == "cuda")

    # ---------------------------------------------------------------- data
    def loader(self, mode):
        if mode not in self._loaders:
            if self.cond is not None:
                self._loaders[mode] = build_loader(self.config, mode, self.data_seed, generator={"train": self.train_gen, "val": self.val_gen}.get(mode),
                                                   label_modality=self.cond["label_modality"], lesions=self.cond["lesions"])
            elif mode == "train":
                if self.world_size > 1:
                    probe = build_loader(self.config, "train", self.data_seed)
                    self.sampler = _RecordingSampler(probe.dataset, num_replicas=self.world_size, rank=self.rank,
                                                     shuffle=True, seed=self.data_seed, drop_last=False)
                    self.sampler.dataset = None
                    loader = build_loader(self.config, "train", self.data_seed, sampler=self.sampler, generator=self.train_gen)
                    self.sampler.dataset = loader.dataset
                    self._loaders[mode] = loader
                else:
                    self._loaders[mode] = build_loader(self.config, "train", self.data_seed, generator=self.train_gen)
            else:
                self._loaders[mode] = build_loader(self.config, mode, self.data_seed,
                                                   generator=self.val_gen if mode == "val" else None)
        return self._loaders[mode]

    def _to_device(self, batch):
        image = batch["image"] if isinstance(batch, dict) else batch
        return image.to(self.device, non_blocking=True)

    def _step_batch(self, batch, image, take=None):
        """What a step of the trainer takes: the slices and, for the conditional prior, their label maps."""
        if self.cond is None:
            return {"image": image}
        return {"image": image, "label": batch["label"][:take].to(self.device, non_blocking=True).contiguous()}

    # ---------------------------------------------------------------- state
    def run_state(self):
        st = {"rng": _rng_state(self.device), "train_generator": self.train_gen.get_state(),
              "val_generator": self.val_gen.get_state(), "noise_generator": self.noise_gen.get_state(),
              "sampler_epoch": int(self.sampler.epoch) if self.sampler is not None else -1, "seed": self.seed}
        return st

    def load_run_state(self, st):
        if not st:
            return
        _set_rng_state(st["rng"], self.device)
        self.train_gen.set_state(st["train_generator"])
        self.val_gen.set_state(st["val_generator"])
        self.noise_gen.set_state(st["noise_generator"])
        if self.sampler is not None and st.get("sampler_epoch", -1) >= 0:
            self.sampler.set_epoch(st["sampler_epoch"])

    def save_checkpoint(self, epoch):
        """rank 0: ckpt-epoch=<epoch:04d>-total_loss=0.00.ckpt in the run directory, then the reference's pruning rule."""
        os.makedirs(self.logger.log_dir, exist_ok=True)
        path = os.path.join(self.logger.log_dir, run_logger.checkpoint_name(epoch))
        ckpt_io.save_run_checkpoint(path, self.trainer.state_dict(), epoch, self.global_step, self.run_state())
        run_logger.prune_checkpoints(self.logger.log_dir, CKPT_LIMIT_NUM, CKPT_SAVE_INTERVAL)
        return path

    # ---------------------------------------------------------------- logging
    def _emit_row(self, meta, values):
        if self.prior:
            row = dict(values)            # loss, grad_norm, lr: logged as the step returns them
        else:
            w = self.trainer.w
            row = _first_step_row(values, w) if isinstance(w, LossWeights) else _second_step_row(values, w)
        row = {k: float(v) for k, v in row.items()}
        row.update(epoch=meta[0], iteration=meta[1])
        if self.rank == 0 and self.logger is not None:
            self.logger.log_metrics(row)

    def _log_step(self, out):
        if (self.global_step + 1) % self.log_every == 0:
            if self.prior:
                terms = [(n, out[n]) for n in ("loss", "grad_norm", "lr") if out.get(n) is not None]
            else:
                terms = _first_step_terms(out) if self.mode == "first_step" else _second_step_terms(out)
            self.queue.push((self.epoch, self.global_step), terms)
        self.queue.step()

    # ---------------------------------------------------------------- training
    def fit(self):
        cfg = self.config
        if self.mode not in ("first_step", "second_step", "prior"):
            raise ValueError("training_mode %r cannot be trained (inference runs with -m test)" % (self.mode,))
        start_epoch = 0
        resume = _get(cfg.run, "resume_checkpoint")
        run_state = None
        if resume:
            self.print("Loading model from {}".format(resume))
            state, last_epoch, self.global_step, run_state = ckpt_io.load_run_checkpoint(resume)
            self.trainer.load_state_dict(state)
            start_epoch = last_epoch + 1
        if self.rank == 0 and self.logger is not None:
            self.logger.log_hyperparams(self.seeds)
        train_loader = self.loader("train")
        if self.rank == 0 and self.do_validate and _get(cfg.run, "use_validation_sanity_check"):
            self.validate(start_epoch, limit=SANITY_VAL_BATCHES)
        if run_state:
            self.load_run_state(run_state)         # last: nothing between here and the first step draws a random number
        noise_views = self.mode == "first_step" and isinstance(self.trainer.views, FlipViews) and self.noise_std > 0
        use_dropblock = bool(_get(cfg.model.vqmodel, "use_dropblock"))
        # as in bench.py: the step's dependency chain runs on a high-priority stream, the off-chain weight gradients on the
        # normal-priority side stream of hipops, so the hardware dispatches chain kernels first (VQW_RUN_PRIORITY=0: off)
        chain = contextlib.nullcontext()
        if self.device.type == "cuda" and os.environ.get("VQW_RUN_PRIORITY", "1") != "0":
            stream = torch.cuda.Stream(device=self.device, priority=-1)
            stream.wait_stream(torch.cuda.current_stream(self.device))
            chain = torch.cuda.stream(stream)
        with chain:
            for epoch in range(start_epoch, self.n_epochs):
                self.epoch = epoch
                if self.sampler is not None:
                    self.sampler.set_epoch(epoch)
                for batch in train_loader:
                    image = self._to_device(batch)
                    if self.mode == "first_step":
                        noise = None
                        if noise_views:
                            noise = torch.randn(image.shape, device=self.device, dtype=torch.float32, generator=self.noise_gen)
                            noise = ops.affine_(noise, self.noise_std, 0.0)
                        out = self.trainer.training_step({"image": image}, noise=noise)
                    else:
                        out = self.trainer.training_step(self._step_batch(batch, image))
                    self._log_step(out)
                    self.global_step += 1
                self.queue.flush()
                if use_dropblock:
                    self.trainer.decoder.dropblock.step()          # base.py:185-187
                if self.rank == 0:
                    if self.do_validate:
                        self.validate(epoch)
                    if self.do_save and self.logger is not None:
                        self.save_checkpoint(epoch)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return self

    # ---------------------------------------------------------------- validation
    @torch.no_grad()
    def _eval_forward(self, image):
        enc, dec = self.trainer.encoder, self.trainer.decoder
        modes = (enc.training, dec.training)
        enc.eval()
        dec.eval()
        try:
            embed, _, ids = enc(image)
            recon = dec(embed)
        finally:
            enc.train(modes[0])
            dec.train(modes[1])
        return recon, ids

    def mosaic(self, image, recon, ids, n_rows):
        """-> ((n_rows * H, n_cols * W, 3) uint8 picture, (B, K + 1) counts) of one batch: one row per image; CRC (and any
        dataset without a CT window): image, recon, ids; otherwise lung image, lung recon, mediastinal image, mediastinal
        recon, ids (single_window_trainer.py:578-638 without the discriminator maps, which are all zero for the PatchGAN)."""
        dw = dataset_window(self.config)
        single = self.config.dataset.dataset_name == "CRCDataset" or dw is None
        labels = ops.export_labels(ids, self.dict_size, index=False)
        counts = labels.counts.cpu().numpy()
        if n_rows <= 0:
            return None, counts
        if single:
            grey = [ops.export_grey(image[:n_rows])[0], ops.export_grey(recon[:n_rows])[0]]
        else:
            wins = (ops.window_map(dw, LUNG_WINDOW), ops.window_map(dw, MEDIASTINAL_WINDOW))
            gi, gr = ops.export_grey(image[:n_rows], windows=wins), ops.export_grey(recon[:n_rows], windows=wins)
            grey = [gi[0], gr[0], gi[1], gr[1]]
        tiles = [np.repeat(g.cpu().numpy()[..., None], 3, axis=3) for g in grey] + [labels.rgb[:n_rows].cpu().numpy()]
        rows = [np.concatenate([t[i] for t in tiles], axis=1) for i in range(n_rows)]
        return np.concatenate(rows, axis=0), counts

    @torch.no_grad()
    def _vqgan_eval_forward(self, image):
        """-> (recon, r_map, f_map) of vqgan_unet_dis.py:191-196 with the VQGAN and the discriminator in eval mode (no EMA update
        of the codebook, no u0 step of the spectral norms); their training modes are put back."""
        vqgan, dis = self.trainer.vqgan, self.trainer.dis
        modes = (vqgan.training, dis.training)
        vqgan.eval()
        dis.eval()
        try:
            recon = vqgan(image)[0]
            r_map = dis(image)[0]
            f_map = dis(recon)[0]
        finally:
            vqgan.train(modes[0])
            dis.train(modes[1])
        return recon, r_map, f_map

    def vqgan_mosaic(self, image, recon, r_map, f_map, n_rows):
        """-> (n_rows * H, 4 * W, 3) uint8 picture: one row per image - image, recon (grey over [-1, 1]), r_map, f_map (each
        image's map over its own range, the reference's vmin = vmax = None; vqgan_unet_dis.py:212-221) - for every dataset."""
        if n_rows <= 0:
            return None
        grey = [ops.export_grey(image[:n_rows])[0], ops.export_grey(recon[:n_rows])[0],
                ops.export_grey_auto(r_map[:n_rows]), ops.export_grey_auto(f_map[:n_rows])]
        tiles = [np.repeat(g.cpu().numpy()[..., None], 3, axis=3) for g in grey]
        return np.concatenate([np.concatenate([t[i] for t in tiles], axis=1) for i in range(n_rows)], axis=0)

    def validate(self, epoch, limit=LIMIT_VAL_BATCHES):
        """At most `limit` validation batches in eval mode without gradients (rank 0): prints every batch's id histogram and
        writes <run dir>/<epoch:06d>.png from the last one (the reference saves each batch's figure to the same path).  The
        VQGAN trainer's picture has the discriminator's maps in place of the ids, and no histogram is printed."""
        if self.rank != 0:
            return None
        if self.prior:
            return self.validate_prior(epoch, limit)
        n_save = int(_get(self.config.save, "n_save_images", 0) or 0)
        picture = None
        for i, batch in enumerate(self.loader("val")):
            if i >= limit:
                break
            image = self._to_device(batch)
            if self.vqgan:
                recon, r_map, f_map = self._vqgan_eval_forward(image)
                picture = self.vqgan_mosaic(image, recon, r_map, f_map, min(n_save, image.shape[0]))
                continue
            recon, ids = self._eval_forward(image)
            picture, counts = self.mosaic(image, recon, ids, min(n_save, image.shape[0]))
            self.print("IDs: ", counts.sum(axis=0))
        if picture is not None and self.logger is not None:
            os.makedirs(self.logger.log_dir, exist_ok=True)
            path = os.path.join(self.logger.log_dir, "%06d.png" % epoch)
            png.save(path, picture)
            return path
        return None

    def validate_prior(self, epoch, limit=LIMIT_VAL_BATCHES):
        """The prior's validation: the mean cross-entropy of at most `limit` validation batches (PriorTrainer.validation_step:
        no corruption, eval mode) and its exponential, printed and logged as `val_loss` and `ppl`; and <run dir>/<epoch:06d>.png
        from the last batch: top row the slices, middle row their reconstructions from their own codes, bottom row as many
        draws of the prior (model.prior.{temperature, top_k}, absent: 1.0 and no filter) from a generator of their own, seeded
        from (seed, epoch) - the training's random streams are not touched."""
        tr = self.trainer
        n_save = int(_get(self.config.save, "n_save_images", 0) or 0)
        losses, uncond, image, ids = [], [], None, None
        for i, batch in enumerate(self.loader("val")):
            if i >= limit:
                break
            image = self._to_device(batch)
            last = self._step_batch(batch, image)
            out = tr.validation_step(last)
            losses.append(out["loss"])
            if out.get("loss_uncond") is not None:          # a conditional prior with the null embedding: the same codes under it
                uncond.append(out["loss_uncond"])
            ids = out["ids"]
        if not losses:
            return None
        val_loss = float(torch.stack(losses).mean())
        ppl = float(np.exp(val_loss))
        self.print("epoch %d: validation cross-entropy %.4f, perplexity %.2f" % (epoch, val_loss, ppl))
        metrics = {"epoch": epoch, "iteration": self.global_step, "val_loss": val_loss, "ppl": ppl}
        if uncond:
            metrics["val_loss_uncond"] = float(torch.stack(uncond).mean())
            self.print("epoch %d: validation cross-entropy under the null condition %.4f" % (epoch, metrics["val_loss_uncond"]))
        if self.logger is not None:
            self.logger.log_metrics(metrics)
        n = min(n_save, image.shape[0])
        if n <= 0 or self.logger is None:
            return None
        p = self.config.model.prior
        gen = torch.Generator(device=self.device).manual_seed(self.seed * 1000003 + epoch)
        recon = tr.vqgan.decode_from_ids(ids[:n], tr.h, tr.w)
        if self.cond is None:
            draws = tr.sample_images(n, temperature=float(_get(p, "temperature", 1.0)), top_k=_get(p, "top_k"), generator=gen)
        else:          # the bottom row: one draw per slice from its own label map
            draws = tr.synthesize(label=last["label"][:n], n_candidates=1, temperature=float(_get(p, "temperature", 1.0)),
                                  top_k=_get(p, "top_k"), generator=gen)["image"]
        rows = [ops.export_grey(t)[0].cpu().numpy() for t in (image[:n], recon, draws)]
        picture = np.concatenate([np.concatenate(list(r), axis=1) for r in rows], axis=0)
        os.makedirs(self.logger.log_dir, exist_ok=True)
        path = os.path.join(self.logger.log_dir, "%06d.png" % epoch)
        png.save(path, picture)
        return path

    # ---------------------------------------------------------------- -p -m edit
    def edit(self):
        """`-p -m edit`: PriorTrainer.edit over the first edit.n_slices slices of the test split with the prior of
        run.resume_checkpoint; the region is edit.box (y0, y1, x0, x1 in pixels), edit.mask_path (a .npy mask at pixel or code
        resolution), edit.nll_threshold or, with the masked prior, edit.pnll_threshold (its pseudo-likelihood map under the optional
        edit.stride).  Under <run dir>/edit/: slice_<i>.png - four grey tiles side by side: the slice, its
        reconstruction from its own codes, the best edit, the composite (blended when edit.blend is 'pyramid', with the optional
        edit.blend_levels and edit.blend_source: ops.blend_cells in place of the hard paste); codes_<i>.npy - (3, h, w) int64: the codes before,
        after, and the cell mask; edit.csv - slice, candidate, score, rank (0: the best), n_resampled.  All draws come from one
        generator seeded with edit.seed: a seed reproduces every file byte for byte."""
        if not self.prior:
            raise ValueError("editing needs the prior trainer (-p)")
        self._load_weights_for_test()
        if self.rank != 0:
            return []
        e, tr = self.config.edit, self.trainer
        n_slices = int(e.n_slices)
        from .config import edit_pnll
        selector = {}
        if _get(e, "box") is not None:
            selector["box"] = tuple(int(v) for v in e.box)
        elif _get(e, "mask_path") is not None:
            selector["mask"] = np.load(e.mask_path)
        elif edit_pnll(self.config) is not None:          # the masked prior's own pick: its pseudo-likelihood map above a threshold
            selector["pnll_threshold"], stride = edit_pnll(self.config)
            if stride is not None:
                selector["stride"] = stride
        else:
            selector["nll_threshold"] = float(e.nll_threshold)
        from .config import guidance, edit_n_steps
        scale, rank = guidance(self.config, "edit")
        if scale != 1.0:          # classifier-free guidance: the conditional trainer's keywords
            selector.update(guidance_scale=scale, rank=rank)
        n_steps = edit_n_steps(self.config)
        if n_steps is not None:   # the masked prior's keyword: the number of parallel decoding passes
            selector.update(n_steps=n_steps)
        from .config import blend
        blending = blend(self.config, "edit")
        if blending["blend"] is not None:     # edit.{blend, blend_levels, blend_source}: how the composite tile is put together
            selector.update(blending)
        gen = torch.Generator(device=self.device).manual_seed(int(e.seed or 0))
        out_dir = os.path.join(self.logger.log_dir, "edit")
        os.makedirs(out_dir, exist_ok=True)
        rows, written, done = ["slice,candidate,score,rank,n_resampled"], [], 0
        for batch in self.loader("test"):
            if done >= n_slices:
                break
            image = self._to_device(batch)[:n_slices - done]
            out = tr.edit(self._step_batch(batch, image, n_slices - done), n_candidates=int(e.n_candidates), temperature=float(e.temperature or 1.0),
                          top_k=e.top_k or None, top_p=e.top_p or None, generator=gen, **selector)
            tiles = [ops.export_grey(t)[0].cpu().numpy() for t in (image, out["recon"], out["edit"], out["composite"])]
            scores, cells = out["scores"].cpu().numpy(), out["cellmask"].cpu().numpy()
            before = out["source_ids"].cpu().numpy().reshape(cells.shape)
            after = out["ids"].cpu().numpy().reshape(cells.shape)
            for b in range(image.shape[0]):
                i = done + b
                path = os.path.join(out_dir, "slice_%04d.png" % i)
                png.save(path, np.concatenate([t[b] for t in tiles], axis=1))
                np.save(os.path.join(out_dir, "codes_%04d.npy" % i), np.stack([before[b], after[b], cells[b].astype(np.int64)]))
                rank = np.argsort(np.argsort(-scores[b], kind="stable"), kind="stable")
                for c in range(scores.shape[1]):
                    rows.append("%d,%d,%.17g,%d,%d" % (i, c, scores[b, c], rank[c], int(cells[b].sum())))
                written.append(path)
            done += image.shape[0]
        with open(os.path.join(out_dir, "edit.csv"), "w") as f:
            f.write("\n".join(rows) + "\n")
        self.print("Edited slices are saved: {}".format(out_dir))
        return written

    # ---------------------------------------------------------------- -p -m synth
    def synth(self):
        """`-p -m synth`: the conditional prior of run.resume_checkpoint over the first synth.n_slices slices of the test split.
        Under <run dir>/synth/: slice_<i>.png - tiles side by side: the label map (grey over its own range), the slice, the
        synthesis from the label map alone (ConditionalPriorTrainer.synthesize) and, with synth.discs, the label map with the
        discs [cy, cx, radius, value] drawn in and the composite of edit(new_label=...); synth.csv - slice, the winner among the
        candidates, its score, the cells the edit redrew (0 without discs).  All draws come from one generator seeded with
        synth.seed: a seed reproduces every file byte for byte."""
        if self.cond is None:
            raise ValueError("synthesising needs the conditional prior trainer (-p with model.prior.cond or model.prior.masked.cond)")
        self._load_weights_for_test()
        if self.rank != 0:
            return []
        e, tr = self.config.synth, self.trainer
        n_slices = int(e.n_slices)
        discs = e.discs if e.discs else []
        kw = dict(n_candidates=int(e.n_candidates), temperature=float(e.temperature or 1.0), top_k=e.top_k or None, top_p=e.top_p or None)
        from .config import guidance, synth_n_steps
        scale, rank = guidance(self.config, "synth")
        if scale != 1.0:          # classifier-free guidance, for the synthesis and for the edit through the label map
            kw.update(guidance_scale=scale, rank=rank)
        n_steps = synth_n_steps(self.config)
        if n_steps is not None:   # the conditional masked prior's keyword: the number of parallel decoding passes
            kw.update(n_steps=n_steps)
        from .config import blend
        blending = blend(self.config, "synth")          # synth.{blend, blend_levels, blend_source}: the composite of the edit below
        blending = blending if blending["blend"] is not None else {}
        gen = torch.Generator(device=self.device).manual_seed(int(e.seed or 0))
        out_dir = os.path.join(self.logger.log_dir, "synth")
        os.makedirs(out_dir, exist_ok=True)
        rows, written, done = ["slice,winner,score,cells_redrawn"], [], 0
        for batch in self.loader("test"):
            if done >= n_slices:
                break
            image = self._to_device(batch)[:n_slices - done]
            step = self._step_batch(batch, image, n_slices - done)
            label = step["label"]
            B = image.shape[0]
            out = tr.synthesize(label=label, generator=gen, **kw)
            grey_of = lambda lab: ops.export_grey_auto(lab.reshape(B, 1, *lab.shape[-2:]).float()).cpu().numpy()  # noqa: E731
            tiles = [grey_of(label)] + [ops.export_grey(t)[0].cpu().numpy() for t in (image, out["image"])]
            redrawn = np.zeros(B, dtype=np.int64)
            if discs:
                new = label.clone()
                yy, xx = torch.meshgrid(torch.arange(new.shape[-2], device=self.device), torch.arange(new.shape[-1], device=self.device), indexing="ij")
                for cy, cx, radius, value in discs:
                    new.reshape(B, *new.shape[-2:])[:, (yy - int(cy)) ** 2 + (xx - int(cx)) ** 2 <= int(radius) ** 2] = int(value)
                edited = tr.edit(step, new_label=new, generator=gen, **kw, **blending)
                tiles += [grey_of(new), ops.export_grey(edited["composite"])[0].cpu().numpy()]
                redrawn = edited["cellmask"].reshape(B, -1).sum(1).cpu().numpy()
            best, scores = out["best"].cpu().numpy(), out["scores"].cpu().numpy()
            for b in range(B):
                path = os.path.join(out_dir, "slice_%04d.png" % (done + b))
                png.save(path, np.concatenate([t[b] for t in tiles], axis=1))
                rows.append("%d,%d,%.17g,%d" % (done + b, best[b], scores[b, best[b]], int(redrawn[b])))
                written.append(path)
            done += B
        with open(os.path.join(out_dir, "synth.csv"), "w") as f:
            f.write("\n".join(rows) + "\n")
        self.print("Synthesised slices are saved: {}".format(out_dir))
        return written

    # ---------------------------------------------------------------- -p -m detect
    def detect(self):
        """`-p -m detect`: PriorTrainer.detect over the first detect.n_slices slices of the test split (0: all of it) with the prior
        of run.resume_checkpoint.  Into the run directory: detect_<i>.png for the first save.n_save_images slices - three grey tiles
        side by side: the slice, the restored slice, and the map over its own range; detect.csv - per slice: n_resampled, the mean
        token_nll, the largest value of the map, the winner's score and, with labels, the slice's positive pixels;
        with labels detect_result.csv - the eight values of ops.detection_scores over all scored pixels: the maps go into ONE
        histogram on the device (ops.score_histogram per batch), read once at the end.  All draws come from one generator seeded
        with detect.seed: a seed reproduces every file byte for byte.  With model.prior.masked and detect.pseudo = {threshold, stride} it is
        MaskedPriorTrainer.detect_pseudo instead: the codes whose pseudo-likelihood map exceeds the threshold are restored in parallel
        passes, and detect.csv's mean_nll column holds the mean pseudo-NLL.  With detect.lesionwise = {thresholds, min_size,
        connectivity} (and labels) every batch's map also goes to functions.LesionScores, and detect_lesions.csv holds one row per
        threshold - threshold, slices, gt_lesions, gt_detected, sensitivity, pred_components, pred_false, fp_per_slice, precision, f1,
        dice_filtered - read once at the end and returned under "lesionwise"; without the section no file is added or changed."""
        from .config import detect_labels, detect_lesionwise, detect_pseudo
        if not self.prior:
            raise ValueError("detecting needs the prior trainer (-p)")
        pseudo = detect_pseudo(self.config)
        lesionwise = detect_lesionwise(self.config)
        self._load_weights_for_test()
        if self.rank != 0:
            return None
        e, tr = self.config.detect, self.trainer
        n_slices = int(e.n_slices or 0)
        label_modality, lesions = detect_labels(self.config)
        labelled = label_modality is not None or lesions is not None
        loader = build_loader(self.config, "test", self.data_seed, label_modality=label_modality, lesions=lesions)
        n_save = int(_get(_get(self.config, "save"), "n_save_images", 0) or 0)
        gen = torch.Generator(device=self.device).manual_seed(int(e.seed or 0))
        out_dir = self.logger.log_dir
        os.makedirs(out_dir, exist_ok=True)
        hist, err = ops.new_score_histogram(self.device)
        lesions_acc = None
        if lesionwise is not None:
            from functions import LesionScores
            lesions_acc = LesionScores(lesionwise["thresholds"], lesionwise["min_size"], lesionwise["connectivity"])
        per_slice, done = [], 0                          # device tensors per batch: read once, after the loop
        for batch in loader:
            if n_slices and done >= n_slices:
                break
            take = n_slices - done if n_slices else None
            image = self._to_device(batch)[:take]
            kw = dict(n_candidates=int(e.n_candidates), temperature=float(e.temperature or 1.0), top_k=e.top_k or None, top_p=e.top_p or None,
                      sigma=float(e.sigma or 0.0), against=e.against, weight=e.weight, generator=gen)
            if pseudo is not None:          # the masked prior: its pseudo-likelihood map selects, out["nll"] holds it
                out = tr.detect_pseudo({"image": image}, pseudo["threshold"], stride=pseudo["stride"], **kw)
            else:
                out = tr.detect({"image": image}, nll_threshold=float(e.nll_threshold), **kw)
            B = image.shape[0]
            stats = [out["n_resampled"].double(), out["nll"].double().mean((1, 2)), out["map"].reshape(B, -1).max(1).values.double(),
                     out["score"].double()]
            if labelled:
                label = batch["label"][:take].to(self.device).reshape(B, -1)
                if label.shape[1] != out["map"][0].numel():
                    raise ValueError("detect: a label of %d pixels per slice for a map of %d" % (label.shape[1], out["map"][0].numel()))
                label = (label != 0).to(torch.uint8)
                ops.score_histogram(out["map"], label, hist, err)
                if lesions_acc is not None:
                    lesions_acc.update(out["map"], label.reshape(out["map"].shape))
                stats.append(label.sum(1, dtype=torch.long).double())
            per_slice.append(torch.stack(stats, dim=1))
            if done < n_save:
                k = min(B, n_save - done)
                tiles = [ops.export_grey(t[:k])[0].cpu().numpy() for t in (image, out["restored"])]
                tiles.append(ops.export_grey_auto(out["map"][:k, None]).cpu().numpy())
                for b in range(k):
                    png.save(os.path.join(out_dir, "detect_%04d.png" % (done + b)), np.concatenate([t[b] for t in tiles], axis=1))
            done += B
        table = torch.cat(per_slice).cpu().numpy() if per_slice else np.zeros((0, 5 if labelled else 4))
        with open(os.path.join(out_dir, "detect.csv"), "w") as f:
            f.write("slice,n_resampled,mean_nll,max_map,score" + (",positives" if labelled else "") + "\n")
            for i, row in enumerate(table):
                f.write("%d,%d,%.9g,%.9g,%.17g" % (i, int(row[0]), row[1], row[2], row[3]) + (",%d" % int(row[4]) if labelled else "") + "\n")
        result = None
        if labelled:
            result = dict(zip(ops.DETECTION_SCORES[:7], ops.detection_scores(hist, err).cpu().tolist()))      # the one read of the scores
            result["err"] = int(err.cpu())
            with open(os.path.join(out_dir, "detect_result.csv"), "w") as f:
                f.write("auroc,ap,best_dice,best_threshold,P,N,err_free,err\n")
                f.write("%.17g,%.17g,%.17g,%.9g,%d,%d,%d,%d\n" % (result["auroc"], result["ap"], result["best_dice"], result["best_threshold"],
                                                               int(result["P"]), int(result["N"]), int(result["err_free"]), result["err"]))
            if lesions_acc is not None:
                from functions import LESION_CSV, lesion_csv_row
                result["lesionwise"] = lesions_acc.result()          # the one read of the lesion-wise counts
                if any(r["err"] for r in result["lesionwise"]):
                    raise RuntimeError("detect: the component kernels reported error word %d" % result["lesionwise"][0]["err"])
                with open(os.path.join(out_dir, "detect_lesions.csv"), "w") as f:
                    f.write(",".join(LESION_CSV) + "\n")
                    for r in result["lesionwise"]:
                        f.write(lesion_csv_row(r) + "\n")
        self.print("Detection results are saved: {}".format(out_dir))
        return result

    # ---------------------------------------------------------------- -p -m score
    def score(self):
        """`-p -m score`: PriorTrainer.score of the prior of run.resume_checkpoint against the first score.n_slices slices of the
        test split - Frechet distance, precision / recall, density / coverage in the first stage's own feature space, and the code
        histograms - each beside its floor, the same score between the two halves of the real set.  Under <run dir>/score/:
        score.csv - one row per score: score,value,floor; score.json - the same values plus the config keys used.  All draws come
        from one generator seeded with score.seed: a seed reproduces both files byte for byte."""
        import json
        from .config import check_score_config
        if not self.prior:
            raise ValueError("scoring needs the prior trainer (-p)")
        kw = check_score_config(self.config)
        self._load_weights_for_test()
        if self.rank != 0:
            return None
        e, tr = self.config.score, self.trainer
        n_slices = int(e.n_slices)
        n_test = len(self.loader("test").dataset)
        if n_test < n_slices:
            raise ValueError("scoring: score.n_slices=%d but the test split has %d slices" % (n_slices, n_test))

        def held_out():
            done = 0
            for batch in self.loader("test"):
                if done >= n_slices:
                    return
                image = self._to_device(batch)[:n_slices - done]
                yield self._step_batch(batch, image, n_slices - done)
                done += image.shape[0]

        gen = torch.Generator(device=self.device).manual_seed(int(e.seed or 0))
        res = tr.score(held_out(), generator=gen, **kw)
        scores, floor = res["scores"], res["floor"]
        out_dir = os.path.join(self.logger.log_dir, "score")
        os.makedirs(out_dir, exist_ok=True)
        fmt = lambda v: "%d" % v if isinstance(v, int) else "%.17g" % v  # noqa: E731
        with open(os.path.join(out_dir, "score.csv"), "w") as f:
            f.write("score,value,floor\n")
            for key in scores:
                f.write("%s,%s,%s\n" % (key, fmt(scores[key]), fmt(floor[key])))
        used = dict(kw, n_slices=n_slices, seed=int(e.seed or 0))
        with open(os.path.join(out_dir, "score.json"), "w") as f:
            json.dump({"scores": scores, "floor": floor, "config": used}, f, indent=1, sort_keys=True)
            f.write("\n")
        self.print("Scores are saved: {}".format(out_dir))
        return res

    # ---------------------------------------------------------------- -m test
    def _load_weights_for_test(self):
        resume = _get(self.config.run, "resume_checkpoint")
        if resume:
            self.print("Loading model from {}".format(resume))
            state, _, _, _ = ckpt_io.load_run_checkpoint(resume)
            state = {"modules": state["modules"], "optimizers": {}, "extra": {"init_embed": True}}
            self.trainer.load_state_dict(state)

    def test(self):
        """`-m test` for the training modes: Evaluator over the test loader -> result.csv in the run directory."""
        if self.prior:
            raise ValueError("the prior trainer has no test step")
        if self.vqgan:
            raise ValueError("the VQGAN trainer has no test step (the reference defines none)")
        self._load_weights_for_test()
        if self.rank != 0:
            return None
        ev = Evaluator(self.trainer.encoder, self.trainer.decoder, self.dict_size)
        result = ev.run(self.loader("test"), self.logger.log_dir)
        self.print("Test results are saved: {}".format(os.path.join(self.logger.log_dir, "result.csv")))
        return result

    def export(self):
        """training_mode 'inference' (single_window_trainer.py:716-779): per test slice, under
        <save_dir>/<study_name>/<patient_id>/: image_%04d / recon_%04d / label_%04d as .png (the export kernels' bytes: grey
        over [-1, 1], ids through the palette) and as .nii.gz (float32 image / recon, int32 label; to_nifti orientation).
        NCCLungDataset: image and recon through the lung window first; CRCDataset: all three flipped upside down."""
        if self.prior:
            raise ValueError("the prior trainer has no inference export")
        if self.vqgan:
            raise ValueError("the VQGAN trainer has no inference export (the reference defines none)")
        self._load_weights_for_test()
        if self.rank != 0:
            return []
        cfg = self.config
        name = cfg.dataset.dataset_name
        flip = name == "CRCDataset"
        dw = dataset_window(cfg)
        lung = ops.window_map(dw, LUNG_WINDOW) if (name == "NCCLungDataset" and dw is not None) else None
        root = os.path.join(cfg.save.save_dir, cfg.save.study_name)
        palette = ops.default_palette(self.dict_size)
        written = []
        for batch in self.loader("test"):
            image = self._to_device(batch)
            recon, ids = self._eval_forward(image)
            grey_i = ops.export_grey(image, windows=(lung,), flip=flip)[0].cpu().numpy()
            grey_r = ops.export_grey(recon, windows=(lung,), flip=flip)[0].cpu().numpy()
            lab = ops.export_labels(ids, self.dict_size, palette=palette, counts=False, flip=flip)
            index, rgb = lab.index.cpu().numpy(), lab.rgb.cpu().numpy()
            img_f, rec_f = image[:, 0].cpu().numpy(), recon[:, 0].cpu().numpy()
            if lung is not None:
                a, b, lo, hi = (np.float32(v) for v in lung)
                img_f, rec_f = np.clip(a * img_f + b, lo, hi), np.clip(a * rec_f + b, lo, hi)
            if flip:
                img_f, rec_f = img_f[:, ::-1], rec_f[:, ::-1]
            patient_ids, slice_nums = batch["patient_id"], batch["slice_num"]
            for i in range(image.shape[0]):
                out_dir = os.path.join(root, str(patient_ids[i]))
                os.makedirs(out_dir, exist_ok=True)
                num = "%04d" % int(slice_nums[i])
                png.save(os.path.join(out_dir, "image_%s.png" % num), grey_i[i])
                png.save(os.path.join(out_dir, "recon_%s.png" % num), grey_r[i])
                png.save(os.path.join(out_dir, "label_%s.png" % num), rgb[i])
                for stem, arr in (("image", img_f[i].astype(np.float32)), ("recon", rec_f[i].astype(np.float32)),
                                  ("label", index[i].astype(np.int32))):
                    nifti.save(np.ascontiguousarray(np.transpose(arr)[::-1, ::-1]), os.path.join(out_dir, "%s_%s.nii.gz" % (stem, num)))
                written.append(os.path.join(out_dir, num))
        return written
