"""Training and using the bidirectional masked code prior (networks.MaskedGPT; MaskGIT's recipe) on the codes of a frozen VQGAN:
the launcher's -p with model.prior.masked.  PriorTrainer's optimiser, schedule, checkpointing and editing contract; what differs is
what the model is asked.

One step, from {'image'} or {'ids': (B, T) long}:
    inp, masked, n = ops.mask_tokens(ids, V, mask_seed, step)          n_b = clamp(ceil(cos(pi/2 u_b) T), 1, T) codes of sample b
    gpt.set_dropout_call(step)                                         with a dropout_seed
    logits = gpt(inp)                                                  every position sees every position
    loss   = sum(ops.cross_entropy(logits, ids, 'none') masked) / sum(n)      the mean over the MASKED positions only
    TrainerBase.update(loss, [optim])                                  hipops.AdamW: norm, clip and update on the device
The mask of a step is a function of (mask_seed, step) alone - no mask tensor, no generator state - so a resumed run continues bit
for bit with what PriorTrainer saves.  There is no start token and no pkeep corruption.  validation_step masks half of every sample
(ratio = 0.5) under call 0: one batch gives one number at every epoch.

Sampling starts from an all-masked grid and editing from the slice's codes with the region masked; both are
MaskedGPT.generate_parallel, n_steps forwards of all B n rows whatever the size of the region.  edit() keeps PriorTrainer.edit's
contract and dict; a candidate's score is the sum of fixed_logp over the redrawn positions - each code's log-probability under the
pass that fixed it, given both sides of the region.  It is a ranking among candidates of one region, not a likelihood: a
raster-order likelihood is not defined for this model, so token_nll, the nll_threshold selector, detect and guidance raise
NotImplementedError.  Conditioning on label maps, with guidance, is trainers/masked_cond_prior.py, through the hooks _forward_of /
_train_forward, _pseudo_cond and _edit_parallel.

What the model thinks of a slice code by code has a name of its own: pseudo_nll(batch, stride) is MaskedGPT.pseudo_nll of the
slice's codes, -log p(code | the codes outside its lattice group) as an (h, w) map, S = sy sx passes side by side (stride (h, w): the
exact pseudo-likelihood; (2, 2), the default: four passes; (1, 1): the all-masked marginal).  It is not a likelihood either - the
terms do not multiply to a probability of the slice - but it is the training objective evaluated where it is asked, from both sides
of every code.  edit(pnll_threshold=, stride=) lets it select the region (one device-to-host read), and detect_pseudo(batch,
pnll_threshold, ...) is PriorTrainer.detect's contract and dict on it: the codes above the threshold are restored in n_steps
parallel passes and ops.anomaly_map smooths the residual (the launcher's -p -m detect with detect.pseudo).
"""
import numpy as np
import torch

from hipops import ops
from networks.gpt import MaskedGPT

from .prior import PriorTrainer


class MaskedPriorTrainer(PriorTrainer):
    VAL_RATIO = 0.5          # validation_step's share of masked positions, under call 0

    def __init__(self, vqgan, gpt, n_steps=8, choice_temperature=4.5, mask_seed=0, **kwargs):
        if not isinstance(gpt, MaskedGPT):
            raise TypeError("MaskedPriorTrainer trains a networks.MaskedGPT")
        for k in ("pkeep", "sos_token"):          # the autoregressive trainer's corruption and start token: nothing here reads them
            kwargs.pop(k, None)
        if int(n_steps) < 1:
            raise ValueError("MaskedPriorTrainer: n_steps=%r must be at least 1" % (n_steps,))
        if not (np.isfinite(float(choice_temperature)) and float(choice_temperature) >= 0):
            raise ValueError("MaskedPriorTrainer: choice_temperature=%r must be finite and not negative" % (choice_temperature,))
        super().__init__(vqgan, gpt, pkeep=1.0, sos_token=0, **kwargs)
        self.n_steps, self.choice_temperature, self.mask_seed = int(n_steps), float(choice_temperature), int(mask_seed)
        self.mask_token = self.gpt.mask_token

    def _no_likelihood(self, what):
        raise NotImplementedError("MaskedPriorTrainer.%s: a raster-order likelihood is not defined for the bidirectional masked prior "
                                  "(every code is predicted from both sides); use the autoregressive PriorTrainer" % what)

    # ---------------------------------------------------------------- the step
    def _masked_loss(self, ids, call, ratio=None, forward=None):
        """-> the mean cross-entropy over the masked positions under ops.mask_tokens(ids, V, mask_seed, call, ratio).  The masked
        count is at least B: the division is never by zero.  forward: inp -> logits (None: the model itself)."""
        inp, masked, n = ops.mask_tokens(ids, self.mask_token, self.mask_seed, call, ratio)
        nll = ops.cross_entropy((self.gpt if forward is None else forward)(inp), ids, reduction="none")
        return (nll * masked.to(nll.dtype)).sum() / n.sum().to(nll.dtype)

    # the two hooks of a conditional masked prior (trainers/masked_cond_prior.py); here: the model itself
    def _forward_of(self, batch):
        """inp -> logits for this batch, or None for gpt(inp)."""
        return None

    def _train_forward(self, batch):
        """The same for training step step_count (the conditional trainer may drop the condition of some samples)."""
        return self._forward_of(batch)

    def training_step(self, batch, mark=None):
        self.throttle.begin()
        ids = self.codes(batch)
        self.gpt.train()
        if self.dropout_seed is not None:
            self.gpt.set_dropout_call(self.step_count)
        loss = self._masked_loss(ids, self.step_count, forward=self._train_forward(batch))      # the mask: a function of (mask_seed, step) alone
        lr = self.current_lr()
        for group in self.optim.param_groups:
            group["lr"] = lr
        self.update(loss, [self.optim], mark=mark)
        self.step_count += 1
        self.throttle.end()
        return {"loss": loss.detach(), "grad_norm": self.optim.last_grad_norm, "lr": lr, "ids": ids}

    @torch.no_grad()
    def validation_step(self, batch):
        """The mean cross-entropy over the masked positions with half of every sample masked (ratio 0.5, call 0: the same mask for
        the same batch at every epoch), eval mode, no gradients -> {'loss', 'ppl' = exp(loss), 'ids'}."""
        ids = self.codes(batch)
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            loss = self._masked_loss(ids, 0, self.VAL_RATIO, forward=self._forward_of(batch))
        finally:
            self.gpt.train(was_training)
        return {"loss": loss, "ppl": torch.exp(loss), "ids": ids}

    # ---------------------------------------------------------------- sampling
    @torch.no_grad()
    def sample_ids(self, n, temperature=1.0, top_k=None, generator=None, top_p=None, n_steps=None):
        """n code sequences (n, h w) decoded from an all-masked grid in n_steps (default: the trainer's) parallel passes."""
        T = self.h * self.w
        ids = torch.full((n, T), self.mask_token, dtype=torch.long, device=self.device)
        masked = torch.ones((n, T), dtype=torch.uint8, device=self.device)
        return self.gpt.generate_parallel(ids, masked, self.n_steps if n_steps is None else n_steps, temperature=temperature, top_k=top_k,
                                          top_p=top_p, choice_temperature=self.choice_temperature, generator=generator)[0]

    def _score_sample_ids(self, n, temperature, top_k, top_p, generator, n_steps=None):
        """score()'s draws: this trainer's own sample_ids; n_steps and top_p are passed on."""
        return self.sample_ids(n, temperature, top_k, generator, top_p=top_p, n_steps=n_steps)

    # ---------------------------------------------------------------- what needs a raster-order likelihood
    def token_nll(self, batch):
        self._no_likelihood("token_nll")

    def _token_nll(self, ids, prefix=None):
        self._no_likelihood("token_nll")

    def detect(self, *args, **kwargs):
        self._no_likelihood("detect")

    # ---------------------------------------------------------------- the pseudo-likelihood map
    def _pseudo_cond(self, batch):
        """MaskedGPT.pseudo_nll's cond for this batch (the conditional trainer: its label tokens); here: None."""
        return None

    @torch.no_grad()
    def pseudo_nll(self, batch, stride=(2, 2), max_rows=64):
        """What the prior thinks of a slice code by code, from both sides: MaskedGPT.pseudo_nll of codes(batch) on the latent grid
        -> (B, h, w) fp32, -log p(code | the codes outside its lattice group), S = sy sx passes.  stride (h, w) is the exact
        pseudo-likelihood, (1, 1) the all-masked marginal.  Not a likelihood (its terms do not multiply to a probability of the
        slice): a high value marks a code the prior did not expect where it stands.  token_nll stays undefined for this model."""
        ids = self.codes(batch)
        if ids.shape[1] != self.h * self.w:
            raise ValueError("MaskedPriorTrainer.pseudo_nll: sequences of h w = %d codes expected, got %d" % (self.h * self.w, ids.shape[1]))
        return self.gpt.pseudo_nll(ids, (self.h, self.w), stride=stride, max_rows=max_rows, cond=self._pseudo_cond(batch))

    def _pseudo_cells(self, batch, pnll_threshold, stride):
        """The pnll_threshold selector -> (the host bool array (B, h, w) of the codes whose pseudo_nll exceeds it, the map): one
        device-to-host read, as PriorTrainer._edit's nll_threshold."""
        try:
            thr = float(pnll_threshold)
        except (TypeError, ValueError):
            thr = float("nan")
        if thr != thr:
            raise ValueError("MaskedPriorTrainer: pnll_threshold=%r must be a number (it may be infinite)" % (pnll_threshold,))
        pnll = self.pseudo_nll(batch, stride=(2, 2) if stride is None else stride)
        return (pnll > thr).cpu().numpy(), pnll          # the one read of the selector

    # ---------------------------------------------------------------- editing
    @torch.no_grad()
    def edit(self, batch, mask=None, box=None, nll_threshold=None, n_candidates=4, n_steps=None, temperature=1.0, top_k=None, top_p=None,
             generator=None, guidance_scale=None, rank=None, pnll_threshold=None, stride=None, blend=None, blend_levels=None,
             blend_source="edit"):
        """PriorTrainer.edit's contract and dict on the bidirectional prior: the codes of the region (`mask` or `box`, cell_mask) are
        masked and filled in again n_candidates times by ONE MaskedGPT.generate_parallel call over the B n_candidates rows -
        n_steps (default: the trainer's) forwards, whatever the size of the region, each seeing the kept codes on both sides.  Each
        candidate's uniforms (n_steps, 2, B, T) are one torch.rand call, candidate 0 first: its codes do not depend on
        n_candidates.  A candidate's score is fixed_logp.double().sum(1), over the redrawn positions (0 elsewhere).  A slice with
        no code selected comes back unchanged with the score 0.  The third selector, pnll_threshold, lets the prior pick the region:
        the codes whose pseudo_nll (under `stride`, default (2, 2)) exceeds it, at the cost of one device-to-host read of the map.
        nll_threshold and guidance raise NotImplementedError; stride without pnll_threshold raises ValueError.  blend, blend_levels
        and blend_source as in PriorTrainer.edit, on every selector."""
        blending = self._blending(batch, blend, blend_levels, blend_source)
        if nll_threshold is not None:
            self._no_likelihood("edit(nll_threshold=...)")
        if guidance_scale is not None and float(guidance_scale) != 1.0:
            raise NotImplementedError("MaskedPriorTrainer.edit: guidance needs a conditional prior: ConditionalMaskedPriorTrainer "
                                      "(model.prior.masked.cond)")
        if (mask is not None) + (box is not None) + (pnll_threshold is not None) != 1:
            raise ValueError("MaskedPriorTrainer.edit: exactly one of mask and box selects the region, or pnll_threshold in their place")
        if stride is not None and pnll_threshold is None:
            raise ValueError("MaskedPriorTrainer.edit: stride=%r is the lattice of pnll_threshold and needs it" % (stride,))
        cells = None if pnll_threshold is None else self._pseudo_cells(batch, pnll_threshold, stride)[0]
        return self._edit_parallel(batch, mask, box, n_candidates, n_steps, temperature, top_k, top_p, generator, cells=cells,
                                   blending=blending)

    # ---------------------------------------------------------------- anomaly detection
    @torch.no_grad()
    def detect_pseudo(self, batch, pnll_threshold, stride=(2, 2), n_candidates=4, n_steps=None, temperature=1.0, top_k=None, top_p=None,
                      sigma=2.0, against="image", weight="mask", generator=None):
        """PriorTrainer.detect's contract and dict on the bidirectional prior: restore the codes whose pseudo_nll (under `stride`)
        exceeds pnll_threshold - ONE edit(pnll_threshold=...), the same draws under the same generator: n_steps parallel passes
        whatever the region - and smooth the pixel residual between what was there and what the prior put there,
        ops.anomaly_map(a, b, cellmask, sigma).  against and weight as in PriorTrainer.detect.  Returns its dict: map (B, H, W);
        restored; nll (B, h, w), here the pseudo-likelihood map; cellmask (B, h, w) uint8; score (B,) float64, the winner's
        fixed_logp sum (0 where nothing was restored); n_resampled (B,) long."""
        if pnll_threshold is None:
            raise ValueError("MaskedPriorTrainer.detect_pseudo: pnll_threshold selects the codes to restore and is required")
        self._detect_checks("MaskedPriorTrainer.detect_pseudo", batch, sigma, against, weight)
        cells, pnll = self._pseudo_cells(batch, pnll_threshold, stride)
        out = self._edit_parallel(batch, None, None, n_candidates, n_steps, temperature, top_k, top_p, generator, cells=cells)
        return self._detect_result(batch, out, pnll, sigma, against, weight)

    def _edit_parallel(self, batch, mask, box, n_candidates, n_steps, temperature, top_k, top_p, generator, cells=None, image_size=None,
                       cond=None, guidance=None, blending=None):
        """edit()'s work behind its selector checks.  cells: a host bool array (B, h, w) in place of mask and box; image_size: the
        (H, W) a mask or box of a batch without a picture refers to.  cond: the conditional trainer's (tokens (B, T), table,
        null_index) - generate_parallel's, repeated per candidate here; guidance: None or (scale, rank) - the dict gains
        scores_uncond and rank 'gain' ranks by sum(fixed_logp - fixed_logp_u).  blending: PriorTrainer._blending's value."""
        n = int(n_candidates)
        if n < 1:
            raise ValueError("MaskedPriorTrainer.edit: n_candidates=%r must be at least 1" % (n_candidates,))
        n_steps = self.n_steps if n_steps is None else int(n_steps)
        has_image = not (isinstance(batch, dict) and batch.get("ids") is not None)
        image = (batch["image"] if isinstance(batch, dict) else batch).to(self.device) if has_image else None
        ids = self.codes({"image": image} if has_image else batch)
        B, T = ids.shape
        if T != self.h * self.w:
            raise ValueError("MaskedPriorTrainer.edit: sequences of h w = %d codes expected, got %d" % (self.h * self.w, T))
        if cells is None:
            cells = self.cell_mask(B, mask, box, tuple(image.shape[-2:]) if has_image else image_size)
        masked = torch.from_numpy(np.repeat(cells.reshape(B, T), n, axis=0).astype(np.uint8)).to(self.device)
        known = ids.repeat_interleave(n, dim=0)
        # one torch.rand call per candidate, candidate 0 first: its uniforms - and so its codes - do not depend on n_candidates
        uniforms = torch.stack([torch.rand(n_steps, 2, B, T, generator=generator, device=self.device) for _ in range(n)], dim=3)
        uniforms = uniforms.reshape(n_steps, 2, B * n, T)          # row b n + c: candidate c of slice b, as in `known`
        kw = {}
        if cond is not None:
            kw["cond"] = (cond[0].repeat_interleave(n, dim=0), cond[1], cond[2])
        if guidance is not None:
            kw["guidance_scale"] = guidance[0]
        tokens, fixed_logp, *rest = self.gpt.generate_parallel(
            known, masked, n_steps, temperature=temperature, top_k=top_k, top_p=top_p,
            choice_temperature=self.choice_temperature, uniforms=uniforms, **kw)
        scores = fixed_logp.double().sum(1).reshape(B, n)
        if guidance is None:
            return self._edit_result(ids, tokens, scores, scores, cells, image, blending)
        key = (fixed_logp.double() - rest[0].double()).sum(1).reshape(B, n) if guidance[1] == "gain" else scores
        out = self._edit_result(ids, tokens, scores, key, cells, image, blending)
        out["scores_uncond"] = rest[0].double().sum(1).reshape(B, n)
        return out
