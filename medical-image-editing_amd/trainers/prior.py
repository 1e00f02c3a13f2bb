"""Training the GPT code prior on the codes of a frozen VQGAN (the launcher's -p).  The reference has no trainer for its
networks.GPT; the recipe is minGPT's and taming-transformers': AdamW over decay / no-decay parameter groups, gradient clipping by
the global norm, linear warm-up and cosine decay of the learning rate, teacher forcing behind a start token, and `pkeep` token
corruption and, when asked for, dropout as the regularisers.  Dropout is opt-in by seed: `dropout_seed` seeds the GPT's
counter-based masks (GPT.seed_dropout) and every step sets the dropout call to the step counter, so the masks of step n are a
function of (dropout_seed, n) alone and a resumed run needs no further state; a GPT with a dropout probability above 0 and no
dropout_seed is refused here.

One step, from {'image'} (encoded by the frozen VQGAN, VQGAN.encode_to_ids: raster order) or {'ids': (B, T) long}:
    inp    = ops.prior_tokens(ids, sos, pkeep, V, u_keep, u_rand)      uniforms from the trainer's own device generator
    gpt.set_dropout_call(step)                                         with a dropout_seed
    logits = gpt(inp)
    loss   = ops.cross_entropy(logits, ids)                            mean over B T
    TrainerBase.update(loss, [optim])                                  hipops.AdamW: norm, clip and update on the device
Nothing is read back: the step returns {'loss', 'grad_norm', 'lr', 'ids'} with the scalars on the device (lr is a host float).

`modules()` is {'decoder': vqgan, 'transformer': gpt}: a -v checkpoint's decoder.* keys load into the frozen first stage
(run.first_stage_ckpt_path), and a prior checkpoint carries both.  `extra` holds the generator's state, the step counter the
learning rate and the dropout call are computed from, and the dropout seed (a resumed run verifies it), so a resumed run
continues bit for bit.

Two hooks make room for a conditional prior (trainers/cond_prior.py): _prefix(batch), the embeddings that stand in front of the
prompt (None here), and _logits(inp, prefix), the logits of the code positions (gpt(inp) here); the step, the validation, token_nll
and _edit go through them.

Editing (the launcher's -p -m edit).  token_nll(batch) is the prior's opinion of a slice code by code, -log p(code | the codes
before it) as an (h, w) map.  edit(batch, mask | box | nll_threshold) redraws the selected codes n_candidates times with
GPT.generate_masked, keeps every other code, scores each candidate by the log-probability of its whole sequence and pastes the best
one back into the slice cell by cell (ops.paste_cells), or, with blend='pyramid', blends it in over a pyramid (ops.blend_cells: no
step along the boundaries of the edited cells; blend_source='delta' blends the difference of the two decodes onto the slice).

Detecting (the launcher's -p -m detect).  detect(batch, nll_threshold) is one edit(nll_threshold=...) - the prior restores the codes
it finds unlikely - and ops.anomaly_map of what was there against what the prior put there: the smoothed pixel residual, the
anomaly map of a slice (Fit.detect scores it against lesion labels with ops.score_histogram / ops.detection_scores).

Scoring (the launcher's -p -m score).  features(images) are the frozen first stage's pooled encoder outputs; score(batches,
n_samples) compares the prior's samples with held-out slices there - Frechet distance, precision / recall, density / coverage and
the code histograms (functions/sample_scores.py over csrc/sample_scores.hip) - and returns the same scores between the two halves of
the real set beside them, the floor.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from hipops import AdamW, ops
from networks.gpt import GPT
from networks.vqgan_model import VQGAN

from .base import TrainerBase
from .config import check_blend, default_blend_levels


def learning_rate(step, lr, warmup_steps=0, decay_steps=0, final_ratio=0.1):
    """The rate of optimiser step `step` (0-based): linear warm-up lr (step + 1) / warmup_steps over the first warmup_steps steps,
    then a cosine from lr down to final_ratio lr at step decay_steps and constant behind it; decay_steps = 0: constant after the
    warm-up."""
    if step < warmup_steps:
        return lr * (step + 1) / warmup_steps
    if decay_steps <= 0:
        return lr
    if step >= decay_steps:
        return lr * final_ratio
    progress = (step - warmup_steps) / max(1, decay_steps - warmup_steps)
    return lr * (final_ratio + (1.0 - final_ratio) * 0.5 * (1.0 + math.cos(math.pi * progress)))


def parameter_groups(gpt, weight_decay):
    """minGPT's rule -> [decayed group, undecayed group] (each {'params', 'weight_decay'}) and the names in each: nn.Linear
    weights decay; biases, nn.LayerNorm weights, tok_embed.weight and pos_embed do not; a parameter in neither raises."""
    decay, no_decay = [], []
    for mn, m in gpt.named_modules():
        for pn, _ in m.named_parameters(recurse=False):
            name = "%s.%s" % (mn, pn) if mn else pn
            if pn.endswith("bias"):
                no_decay.append(name)
            elif pn == "weight" and isinstance(m, nn.Linear):
                decay.append(name)
            elif pn == "weight" and isinstance(m, (nn.LayerNorm, nn.Embedding)):
                no_decay.append(name)
            elif name == "pos_embed":
                no_decay.append(name)
            else:
                raise ValueError("parameter_groups: %s falls in neither the decayed nor the undecayed group" % name)
    params = dict(gpt.named_parameters())
    missing = sorted(set(params) - set(decay) - set(no_decay))
    if missing or len(decay) + len(no_decay) != len(params):
        raise ValueError("parameter_groups: not every parameter is in exactly one group (%s)" % ", ".join(missing))
    groups = [{"params": [params[n] for n in decay], "weight_decay": float(weight_decay)},
              {"params": [params[n] for n in no_decay], "weight_decay": 0.0}]
    return groups, (decay, no_decay)


class PriorTrainer(TrainerBase):
    def __init__(self, vqgan, gpt, pkeep=1.0, sos_token=0, lr=4.5e-4, betas=(0.9, 0.95), weight_decay=0.01, grad_norm_clip=1.0,
                 warmup_steps=0, decay_steps=0, seed=0, device="cuda", dropout_seed=None):
        if not isinstance(vqgan, VQGAN):
            raise TypeError("PriorTrainer trains on the codes of a networks.VQGAN")
        if not isinstance(gpt, GPT):
            raise TypeError("PriorTrainer trains a networks.GPT")
        super().__init__(device)
        self.h, self.w = self._latent_grid(vqgan)
        self.dict_size = int(vqgan.vq.dict_size)
        if gpt.config.vocab_size != self.dict_size:
            raise ValueError("PriorTrainer: the GPT's vocab_size=%d must equal the VQGAN's dict_size=%d" % (gpt.config.vocab_size, self.dict_size))
        if gpt.block_size < self.h * self.w:
            raise ValueError("PriorTrainer: the GPT's block_size=%d must be at least the latent's h w = %d" % (gpt.block_size, self.h * self.w))
        if not 0 <= int(sos_token) < self.dict_size:
            raise ValueError("PriorTrainer: sos_token=%d must be a code in [0, %d)" % (sos_token, self.dict_size))
        if not 0.0 <= float(pkeep) <= 1.0:
            raise ValueError("PriorTrainer: pkeep=%r must lie in [0, 1]" % (pkeep,))
        if warmup_steps < 0 or decay_steps < 0 or (decay_steps and decay_steps < warmup_steps):
            raise ValueError("PriorTrainer: warmup_steps=%r and decay_steps=%r: non-negative, decay_steps 0 or >= warmup_steps" % (warmup_steps, decay_steps))
        gpt.train()
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        if self.dropout_seed is not None:
            gpt.seed_dropout(self.dropout_seed)
        gpt._check_dropout()             # NotImplementedError for a dropout probability above 0 without a seed, before any kernel runs
        self.vqgan = vqgan.to(self.device).eval().requires_grad_(False)          # frozen: never stepped, never in train mode
        self.gpt = gpt.to(self.device)
        self.pkeep, self.sos_token = float(pkeep), int(sos_token)
        self.lr, self.warmup_steps, self.decay_steps = float(lr), int(warmup_steps), int(decay_steps)
        groups, self.group_names = parameter_groups(self.gpt, weight_decay)
        self.optim = AdamW(groups, lr=lr, betas=tuple(betas), weight_decay=weight_decay, max_grad_norm=grad_norm_clip)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))
        self.step_count = 0

    def _latent_grid(self, vqgan):
        """(h, w) of the code sequences: the latent of the VQGAN at its own resolution (the conditional trainer: its condition's)."""
        enc = vqgan.encoder
        side = int(enc.resolution) // 2 ** (int(enc.num_resolutions) - 1)
        return side, side

    def modules(self):
        return {"decoder": self.vqgan, "transformer": self.gpt}

    def optimizers(self):
        return {"prior_optim": self.optim}

    def state_dict(self):
        state = super().state_dict()
        state["extra"].update(prior_generator=self.generator.get_state(), prior_step=int(self.step_count), prior_dropout_seed=self.dropout_seed)
        return state

    def load_state_dict(self, state):
        extra = state.get("extra") or {}
        has_dropout = any(m.p > 0 for m in self.gpt.modules() if isinstance(m, nn.Dropout))
        if has_dropout and extra.get("prior_dropout_seed", self.dropout_seed) != self.dropout_seed:
            raise ValueError("PriorTrainer: the checkpoint was trained with dropout_seed=%r, this trainer has %r: the run would not "
                             "continue with the same masks" % (extra["prior_dropout_seed"], self.dropout_seed))
        super().load_state_dict(state)
        if "prior_generator" in extra:
            self.generator.set_state(extra["prior_generator"].cpu())
        if "prior_step" in extra:
            self.step_count = int(extra["prior_step"])

    # ---------------------------------------------------------------- the step
    def current_lr(self):
        return learning_rate(self.step_count, self.lr, self.warmup_steps, self.decay_steps)

    def codes(self, batch):
        """batch {'ids': (B, T) long} or {'image': ...} (or the image itself) -> ids (B, T) long on the device."""
        if isinstance(batch, dict) and batch.get("ids") is not None:
            ids = batch["ids"].to(self.device)
        else:
            image = batch["image"] if isinstance(batch, dict) else batch
            ids = self.vqgan.encode_to_ids(image.to(self.device))
        if ids.dim() != 2 or ids.shape[1] > self.gpt.block_size:
            raise ValueError("PriorTrainer: ids of shape (B, T) with T <= block_size=%d expected, got %s" % (self.gpt.block_size, tuple(ids.shape)))
        return ids

    def _inputs(self, ids, pkeep):
        u_keep = u_rand = None
        if pkeep < 1:
            u_keep = torch.rand(ids.shape, generator=self.generator, device=self.device)
            u_rand = torch.rand(ids.shape, generator=self.generator, device=self.device)
        return ops.prior_tokens(ids, self.sos_token, pkeep, self.dict_size, u_keep, u_rand)

    # the two hooks of a conditional prior (trainers/cond_prior.py); here: no prefix, the logits of every position
    def _prefix(self, batch):
        """The embeddings (B, Tc, E) that stand in front of the prompt as a fully visible prefix, or None."""
        return None

    def _logits(self, inp, prefix):
        """The logits (B, T, V) of the code positions of inp (B, T) behind `prefix`."""
        return self.gpt(inp)

    def _train_prefix(self, batch):
        """The prefix of a training step: _prefix(batch) (the conditional trainer may drop the condition of some samples)."""
        return self._prefix(batch)

    def _null_prefix(self, B):
        """The prefix of the null condition for B rows (the conditional trainer's, under guidance)."""
        raise NotImplementedError("PriorTrainer: guidance needs a condition (trainers/cond_prior.py)")

    def training_step(self, batch, mark=None):
        self.throttle.begin()
        ids = self.codes(batch)
        self.gpt.train()
        inp = self._inputs(ids, self.pkeep)
        if self.dropout_seed is not None:
            self.gpt.set_dropout_call(self.step_count)          # the masks of a step: a function of (dropout_seed, step) alone
        loss = ops.cross_entropy(self._logits(inp, self._train_prefix(batch)), ids)
        lr = self.current_lr()
        for group in self.optim.param_groups:
            group["lr"] = lr
        self.update(loss, [self.optim], mark=mark)
        self.step_count += 1
        self.throttle.end()
        return {"loss": loss.detach(), "grad_norm": self.optim.last_grad_norm, "lr": lr, "ids": ids}

    @torch.no_grad()
    def validation_step(self, batch):
        """Mean cross-entropy of one batch without corruption (pkeep = 1), eval mode, no gradients -> {'loss', 'ids'}."""
        ids = self.codes(batch)
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            loss = ops.cross_entropy(self._logits(self._inputs(ids, 1.0), self._prefix(batch)), ids)
        finally:
            self.gpt.train(was_training)
        return {"loss": loss, "ids": ids}

    @staticmethod
    def scalars(out):
        """Host copies of a step's scalars (one sync; keep out of timed regions)."""
        return {k: float(v) for k, v in out.items() if k != "ids" and v is not None}

    # ---------------------------------------------------------------- sampling
    @torch.no_grad()
    def sample_ids(self, n, temperature=1.0, top_k=None, generator=None):
        """n code sequences (n, h w) drawn from the start token alone.  GPT.generate where the model has room for the start
        token and h w sampled ones (1 + h w <= block_size); a model with block_size == h w - the sequences it was trained on -
        runs the same loop here (prefill, then ops.sample_topk and decode_step per token) on a cache of h w rows: the last
        sampled token is never fed back, so h w positions are all it needs."""
        steps = self.h * self.w
        start = torch.full((n, 1), self.sos_token, dtype=torch.long, device=self.device)
        if 1 + steps <= self.gpt.block_size:
            return self.gpt.generate(start, steps, temperature=temperature, top_k=top_k, generator=generator)[:, 1:]
        if not temperature > 0:
            raise ValueError("PriorTrainer.sample_ids: temperature=%r must be positive" % (temperature,))
        gpt = self.gpt
        was_training = gpt.training
        gpt.eval()
        try:
            cache = gpt.new_cache(n, capacity=steps)
            logits = gpt.prefill(start, cache)[:, -1, :]
            out = []
            for k in range(steps):
                new = ops.sample_topk(logits, torch.rand(n, generator=generator, device=logits.device), temperature, top_k)
                out.append(new.unsqueeze(1))
                if k + 1 < steps:
                    logits = gpt.decode_step(new, cache)
        finally:
            gpt.train(was_training)
        return torch.cat(out, dim=1)

    @torch.no_grad()
    def sample_images(self, n, temperature=1.0, top_k=None, generator=None):
        """n pictures: sample_ids, then VQGAN.decode_from_ids."""
        return self.vqgan.decode_from_ids(self.sample_ids(n, temperature, top_k, generator), self.h, self.w)

    # ---------------------------------------------------------------- scoring the samples
    @torch.no_grad()
    def features(self, images):
        """The feature rows the sample scores live in: the frozen first stage's encoder output, before quantisation, averaged over
        the latent grid -> (B, emb_dim) fp32.  Eval mode (the first stage never leaves it), no gradients."""
        return self._pool(self.vqgan.encoder(images.to(self.device)))

    @staticmethod
    def _pool(z):
        return z.mean(dim=(2, 3)).contiguous()

    def _score_condition(self, batch):
        """What score() keeps of a held-out batch to draw its samples from (the conditional trainer: the conditioning tokens)."""
        return None

    def _score_draws(self, conditions, n_samples, batch_size, temperature, top_k, top_p, generator, **sample_kw):
        """The code sequences score() scores, batch by batch: n_samples draws from the start token alone."""
        done = 0
        while done < n_samples:
            n = min(batch_size, n_samples - done)
            yield self._score_sample_ids(n, temperature, top_k, top_p, generator, **sample_kw)
            done += n

    def _score_sample_ids(self, n, temperature, top_k, top_p, generator):
        if top_p is None:
            return self.sample_ids(n, temperature, top_k, generator)
        # top-p: the sampler of generate_masked with every position redrawn
        T = self.h * self.w
        start = torch.full((n, 1), self.sos_token, dtype=torch.long, device=self.device)
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            return self.gpt.generate_masked(start, torch.zeros((n, T), dtype=torch.long, device=self.device), np.ones((n, T), dtype=bool),
                                            temperature=temperature, top_k=top_k, top_p=top_p, generator=generator)[0]
        finally:
            self.gpt.train(was_training)

    @torch.no_grad()
    def score(self, batches, n_samples, batch_size=16, k=3, temperature=1.0, top_k=None, top_p=None, against="image", generator=None,
              **sample_kw):
        """Score the prior's samples against held-out slices in the first stage's own feature space (functions/sample_scores.py).

        batches: the held-out slices, batch by batch ({'image'[, 'label']} or the images).  Real features: features(slice) with
        against='image', features(decode(encode(slice))) with against='recon', which takes the first stage's own reconstruction
        error out of the comparison.  Fake features: n_samples draws (_score_draws: sample_ids here) -> decode_from_ids ->
        features.  Every feature is centred on the fp32 mean of the first real batch.  Returns {'scores', 'floor'}: two dicts of
        sample_scores's keys - the samples against the real set, and the real set's even arrival indices against its odd ones:
        the same scores between two halves of one distribution at half the n, without which nobody can tell a Frechet distance of 3
        from sampling noise."""
        from functions.sample_scores import FeatureStats, sample_scores
        k, n_samples, batch_size = int(k), int(n_samples), int(batch_size)
        if against not in ("image", "recon"):
            raise ValueError("PriorTrainer.score: against=%r must be 'image' or 'recon'" % (against,))
        if n_samples < k + 1:
            raise ValueError("PriorTrainer.score: n_samples=%d must be at least k + 1 = %d" % (n_samples, k + 1))
        if batch_size < 1:
            raise ValueError("PriorTrainer.score: batch_size=%d must be at least 1" % batch_size)
        real = halves = None
        real_ids, conditions, seen = [], [], 0
        for batch in batches:
            image = (batch["image"] if isinstance(batch, dict) else batch).to(self.device)
            z = self.vqgan.encoder(image)                # one encoder pass gives the slice's codes and, against='image', its features
            ids = self.vqgan.raster_from_vq_ids(self.vqgan.vq(z)[2]).contiguous()
            f = self._pool(z) if against == "image" else self.features(self.vqgan.decode_from_ids(ids, self.h, self.w))
            if real is None:
                shift = f.mean(dim=0)
                real = FeatureStats(f.shape[1], shift, keep=2 ** 31)
                halves = [FeatureStats(f.shape[1], shift, keep=2 ** 31) for _ in range(2)]
            real.add(f)
            first = seen % 2                             # the parity of this batch's first arrival index
            halves[first].add(f[0::2])
            halves[1 - first].add(f[1::2])
            real_ids.append(ids)
            conditions.append(self._score_condition(batch))
            seen += int(f.shape[0])
        if real is None or min(h.n for h in halves) < k + 1:
            raise ValueError("PriorTrainer.score: %d held-out slices: each half of the real set needs at least k + 1 = %d" % (seen, k + 1))
        fake = FeatureStats(real.D, real.shift, keep=2 ** 31)
        fake_ids = []
        for ids in self._score_draws(conditions, n_samples, batch_size, temperature, top_k, top_p, generator, **sample_kw):
            image = self.vqgan.decode_from_ids(ids, self.h, self.w)
            fake.add(self.features(image))
            fake_ids.append(ids)
        real_ids, fake_ids = torch.cat(real_ids), torch.cat(fake_ids)
        scores = sample_scores(real, fake, k, real_ids, fake_ids, self.dict_size)
        floor = sample_scores(halves[0], halves[1], k, real_ids[0::2], real_ids[1::2], self.dict_size)
        return {"scores": scores, "floor": floor}

    # ---------------------------------------------------------------- editing
    @torch.no_grad()
    def _token_nll(self, ids, prefix=None):
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            nll = ops.cross_entropy(self._logits(self._inputs(ids, 1.0), prefix), ids, reduction="none")
        finally:
            self.gpt.train(was_training)
        return nll

    def token_nll(self, batch):
        """What the prior thinks of a slice, code by code: -log p(code | the codes before it) as a map (B, h, w) fp32 in raster
        order - one full forward in eval mode without corruption (pkeep = 1) and ops.cross_entropy(reduction='none').  Its mean
        is validation_step's loss; a high value marks a code the prior did not expect (the anomaly map of a code prior)."""
        ids = self.codes(batch)
        if ids.shape[1] != self.h * self.w:
            raise ValueError("PriorTrainer.token_nll: sequences of h w = %d codes expected, got %d" % (self.h * self.w, ids.shape[1]))
        return self._token_nll(ids, self._prefix(batch)).reshape(-1, self.h, self.w)

    def cell_mask(self, B, mask=None, box=None, image_size=None):
        """The host bool array (B, h, w) of the codes a user's selection touches.  mask: a host array at pixel resolution (H, W)
        or (B, H, W), or at code resolution (h, w) or (B, h, w); box = (y0, y1, x0, x1) in pixels.  A code is selected iff any
        pixel of its cell is set.  H, W: image_size, else the VQGAN's resolution."""
        h, w = self.h, self.w
        H, W = image_size if image_size is not None else (int(self.vqgan.encoder.resolution),) * 2
        if H % h or W % w:
            raise ValueError("PriorTrainer.edit: the picture's %d x %d is no multiple of the latent's %d x %d" % (H, W, h, w))
        if box is not None:
            y0, y1, x0, x1 = (int(v) for v in box)
            if not (0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
                raise ValueError("PriorTrainer.edit: box [%d, %d) x [%d, %d) outside %d x %d" % (y0, y1, x0, x1, H, W))
            mask = np.zeros((H, W), dtype=bool)
            mask[y0:y1, x0:x1] = True
        mask = np.asarray(mask) != 0
        if mask.ndim == 2:
            mask = mask[None]
        if mask.ndim != 3 or mask.shape[0] not in (1, B) or mask.shape[1:] not in ((H, W), (h, w)):
            raise ValueError("PriorTrainer.edit: a mask of shape (H, W) = (%d, %d), (h, w) = (%d, %d) or either behind B = %d expected, got %s" % (
                H, W, h, w, B, mask.shape))
        if mask.shape[1:] != (h, w):
            mask = mask.reshape(mask.shape[0], h, H // h, w, W // w).any(axis=(2, 4))
        return np.broadcast_to(mask, (B, h, w)).copy()

    @torch.no_grad()
    def edit(self, batch, mask=None, box=None, nll_threshold=None, n_candidates=4, temperature=1.0, top_k=None, top_p=None,
             generator=None, blend=None, blend_levels=None, blend_source="edit"):
        """Redraw the codes of a region of every slice with the prior and keep the rest.  Exactly one selector: `mask` (a host
        array at pixel or code resolution, cell_mask), `box` = (y0, y1, x0, x1) in pixels, or `nll_threshold`, which selects the
        codes whose token_nll exceeds it - the prior picks the region itself; this costs one device-to-host read of the map.

        Every slice is repeated n_candidates times in the batch and ONE GPT.generate_masked call behind the start token draws all
        B n_candidates rows (the uniforms are drawn per candidate from `generator`, candidate 0 first, so a seed gives candidate 0
        the same codes whatever n_candidates is); a candidate's score is the sum of logp over the whole sequence (in double) - the kept codes behind
        the region included, scored given the drawn ones, which is how a raster-order prior prefers what fits the codes that
        follow.  One device-to-host read ranks them.  A slice with no code selected comes back unchanged, with its own score.

        Returns a dict: ids (B, T) the best candidate (source_ids: the slice's own codes); candidates (B, n, T) and scores (B, n) float64 in draw order; best (B,);
        cellmask (B, h, w) uint8; recon and edit, the slice's own codes and the best candidate's through decode_from_ids; and
        composite = ops.paste_cells(image, edit, cellmask).  A {'ids'} batch has no image and no composite.

        blend: None or 'paste' - that hard per-cell paste - or 'pyramid': composite = ops.blend_cells(image, edit, cellmask,
        blend_levels, recon if blend_source == 'delta' else None), multi-band blending that leaves no step along the cells'
        boundaries; nothing else in the dict changes.  blend_levels: the depth of the pyramid, default min(3, the largest L with 2^L
        dividing both sides of a cell in pixels).  blend_source 'edit' blends edit - image, 'delta' the difference of the two
        decodes edit - recon: the first stage's own error cancels where the codes did not change.  A bad value raises ValueError
        before any device work."""
        blending = self._blending(batch, blend, blend_levels, blend_source)
        return self._edit(batch, mask, box, nll_threshold, n_candidates, temperature, top_k, top_p, generator, blending=blending)[0]

    def _blending(self, batch, blend, blend_levels, blend_source):
        """edit()'s three blending keywords -> None (the hard paste) or (levels, source) of ops.blend_cells; ValueError for a bad
        value, a depth whose 2^levels does not divide the picture, or a cell of odd size without blend_levels.  Shapes only: no
        device work.  A {'ids'} batch has no composite: its values are checked and otherwise unused."""
        blend, levels, source = check_blend(blend, blend_levels, blend_source)
        if blend != "pyramid" or (isinstance(batch, dict) and batch.get("ids") is not None):
            return None
        H, W = (batch["image"] if isinstance(batch, dict) else batch).shape[-2:]
        if H % self.h or W % self.w:
            raise ValueError("PriorTrainer.edit: the picture's %d x %d is no multiple of the latent's %d x %d" % (H, W, self.h, self.w))
        if levels is None:
            levels = default_blend_levels(H // self.h, W // self.w)
        elif H % (1 << levels) or W % (1 << levels):
            raise ValueError("PriorTrainer.edit: blend_levels=%d: 2^%d does not divide the picture's %d x %d" % (levels, levels, H, W))
        return levels, source

    def _edit(self, batch, mask, box, nll_threshold, n_candidates, temperature, top_k, top_p, generator, cells=None, image_size=None,
              guidance=None, blending=None):
        """edit()'s work -> (edit()'s dict, the token_nll map (B, h, w) the nll_threshold selector computed, else None): what edit
        and detect share.  cells: a host bool array (B, h, w) in place of the three selectors (the conditional trainer's fourth);
        image_size: the (H, W) a mask or box of a batch without a picture refers to (cell_mask's default otherwise).  guidance:
        None or (scale, rank) of the conditional trainer - the null prefix runs beside the batch's, the dict gains scores_uncond
        and rank 'gain' ranks by sum(logp - logp_u).  blending: _blending's value for the composite."""
        if cells is None and (mask is not None) + (box is not None) + (nll_threshold is not None) != 1:
            raise ValueError("PriorTrainer.edit: exactly one of mask, box and nll_threshold selects the region")
        n = int(n_candidates)
        if n < 1:
            raise ValueError("PriorTrainer.edit: n_candidates=%r must be at least 1" % (n_candidates,))
        has_image = not (isinstance(batch, dict) and batch.get("ids") is not None)
        image = (batch["image"] if isinstance(batch, dict) else batch).to(self.device) if has_image else None
        ids = self.codes({"image": image} if has_image else batch)
        B, T = ids.shape
        if T != self.h * self.w:
            raise ValueError("PriorTrainer.edit: sequences of h w = %d codes expected, got %d" % (self.h * self.w, T))
        prefix = self._prefix(batch)
        nll = None
        if cells is None and nll_threshold is not None:
            nll = self._token_nll(ids, prefix).reshape(B, self.h, self.w)
            cells = (nll > float(nll_threshold)).cpu().numpy()      # the one read of the selector
        elif cells is None:
            cells = self.cell_mask(B, mask, box, tuple(image.shape[-2:]) if has_image else image_size)
        resample = np.repeat(cells.reshape(B, T), n, axis=0)
        known = ids.repeat_interleave(n, dim=0)
        start = torch.full((B * n, 1), self.sos_token, dtype=torch.long, device=self.device)
        # one torch.rand call per candidate, candidate 0 first: its uniforms - and so its codes - do not depend on n_candidates
        cols = np.flatnonzero(resample.any(axis=0))
        steps = T - int(cols[0]) if cols.size else 0
        uniforms = torch.stack([torch.rand(steps, B, generator=generator, device=self.device) for _ in range(n)])      # (n, steps, B)
        uniforms = uniforms.permute(1, 2, 0).reshape(steps, B * n)
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, uniforms=uniforms,
                      embeddings=None if prefix is None else prefix.repeat_interleave(n, dim=0))
            if guidance is not None:
                kw.update(uncond_embeddings=self._null_prefix(B * n), guidance_scale=guidance[0])
            tokens, logp, *rest = self.gpt.generate_masked(start, known, resample, **kw)
        finally:
            self.gpt.train(was_training)
        scores = logp.double().sum(1).reshape(B, n)
        key = scores
        if guidance is not None and guidance[1] == "gain":
            key = (logp.double() - rest[0].double()).sum(1).reshape(B, n)
        out = self._edit_result(ids, tokens, scores, key, cells, image, blending)
        if guidance is not None:
            out["scores_uncond"] = rest[0].double().sum(1).reshape(B, n)
        return out, nll

    def _edit_result(self, ids, tokens, scores, key, cells, image, blending=None):
        """edit()'s dict from the drawn candidates: tokens (B n, T) in draw order, scores and the ranking key (B, n) float64, cells
        the host bool array (B, h, w), image the slices or None ({'ids'} batch: no composite).  One device-to-host read ranks.
        blending: None - the composite is ops.paste_cells - or _blending's (levels, source) for ops.blend_cells."""
        (B, T), n = ids.shape, scores.shape[1]
        best = torch.from_numpy(np.argmax(key.cpu().numpy(), axis=1)).to(self.device)      # the read of the ranking; first maximum
        candidates = tokens.reshape(B, n, T)
        best_ids = candidates[torch.arange(B, device=self.device), best]
        cellmask = torch.from_numpy(cells.astype(np.uint8)).to(self.device)
        out = {"ids": best_ids, "source_ids": ids, "candidates": candidates, "scores": scores, "best": best, "cellmask": cellmask,
               "recon": self.vqgan.decode_from_ids(ids, self.h, self.w), "edit": self.vqgan.decode_from_ids(best_ids, self.h, self.w)}
        if image is not None and blending is None:
            out["composite"] = ops.paste_cells(image, out["edit"], cellmask)
        elif image is not None:
            levels, source = blending
            out["composite"] = ops.blend_cells(image, out["edit"], cellmask, levels, out["recon"] if source == "delta" else None)
        return out

    # ---------------------------------------------------------------- anomaly detection
    @torch.no_grad()
    def detect(self, batch, nll_threshold, n_candidates=4, temperature=1.0, top_k=None, top_p=None, sigma=2.0, against="image",
               weight="mask", generator=None):
        """Unsupervised anomaly localisation: restore the codes the prior finds unlikely - ONE edit(nll_threshold=...), the same
        draws under the same generator - and smooth the pixel residual between what was there and what the prior put there into a
        map, ops.anomaly_map(a, b, cellmask, sigma) = G_sigma(mean_c |a - b| o U(cellmask)).

        against='image': a = the slice, b = the composite (the winner pasted into the slice cell by cell); outside the restored
        cells the residual is exactly 0, so a slice with no code above the threshold gets an all-zero map.
        against='reconstruction': a = decode(the slice's own codes), b = decode(the winner's codes) - the VQGAN's own
        reconstruction error cancels; a {'ids'} batch has this mode only.
        weight='mask': the residual is weighted by the bilinearly up-sampled cell mask; weight='none': no cell mask is passed.

        Returns a dict: map (B, H, W) fp32; restored (B, C, H, W) = b; nll (B, h, w), token_nll of the slice; cellmask (B, h, w)
        uint8; score (B,) float64, the winner's log-probability; n_resampled (B,) long, the restored codes per slice."""
        if nll_threshold is None:
            raise ValueError("PriorTrainer.detect: nll_threshold selects the codes to restore and is required")
        self._detect_checks("PriorTrainer.detect", batch, sigma, against, weight)
        out, nll = self._edit(batch, None, None, nll_threshold, n_candidates, temperature, top_k, top_p, generator)
        return self._detect_result(batch, out, nll, sigma, against, weight)

    def _detect_checks(self, name, batch, sigma, against, weight):
        """What a detection refuses before any device work (detect here, MaskedPriorTrainer.detect_pseudo)."""
        if against not in ("image", "reconstruction"):
            raise ValueError("%s: against=%r must be 'image' or 'reconstruction'" % (name, against))
        if weight not in ("mask", "none"):
            raise ValueError("%s: weight=%r must be 'mask' or 'none'" % (name, weight))
        ops.gauss_taps(sigma)                # a bad sigma is refused before any device work
        if against == "image" and isinstance(batch, dict) and batch.get("ids") is not None:
            raise ValueError("%s: against='image' needs a batch with an image ({'ids'} has none)" % name)

    def _detect_result(self, batch, out, nll, sigma, against, weight):
        """detect()'s dict from an edit's dict `out` and the map `nll` that selected its cells: everything behind the edit."""
        if against == "image":
            image = batch["image"] if isinstance(batch, dict) else batch
            a, b = image.to(self.device), out["composite"]
        else:
            a, b = out["recon"], out["edit"]
        cellmask = out["cellmask"]
        amap = ops.anomaly_map(a, b, cellmask if weight == "mask" else None, sigma)
        rows = torch.arange(cellmask.shape[0], device=self.device)
        return {"map": amap, "restored": b, "nll": nll, "cellmask": cellmask, "score": out["scores"][rows, out["best"]],
                "n_resampled": cellmask.reshape(cellmask.shape[0], -1).sum(1, dtype=torch.long)}
