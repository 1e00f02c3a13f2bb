"""The bidirectional masked code prior conditioned on a label map (the launcher's -p with model.prior.masked.cond): p(codes | label
tokens) decoded in n_steps parallel passes, with classifier-free guidance.  MaskedPriorTrainer's step, schedule, checkpointing and
editing; ConditionalPriorTrainer's condition (networks.LabelCondition: tokens, the table, null_index) and its synthesize / edit
contract, through trainers/label_cond.py.

The condition is ADDED, not prefixed.  The latent grid and the label-token grid are the same h x w grid and every position of a
bidirectional model sees every position, so the label token of cell t is added to the embedding of position t
(MaskedGPT.forward_conditioned, ops.embedding_cond: one pass, x = (tok[idx] + pos) + table[token]).  The sequence stays T = h w long
and the MaskedGPT keeps block_size = h w; a prefix would double the rows of every layer.

One step, from {'image', 'label'} or {'ids', 'cond'}:
    inp, masked, n = ops.mask_tokens(ids, V, mask_seed, step)
    logits = gpt.forward_conditioned(inp, tokens, table, null_index, drop=(p_uncond, cond_drop_seed, step))      drop with p_uncond > 0
    loss   = the masked mean cross-entropy, as in the parent
The table joins the undecayed AdamW group.  The mask is a function of (mask_seed, step), the dropped samples of (cond_drop_seed,
step): a resumed run continues bit for bit with no new checkpoint state; with p_uncond > 0 the seed goes into the checkpoint's
`extra` and a mismatch on load raises.  validation_step is the parent's under the label; with a null embedding it also returns
loss_uncond, the same mask under the null condition.

synthesize(label | cond) starts from an all-masked grid; edit(batch, mask | box | new_label) masks the region - with new_label the
cells ops.cells_changed reports, redrawn under the new map's tokens - and keeps every other code.  Both are ONE
MaskedGPT.generate_parallel call over the B n_candidates rows; under guidance a pass runs the label's rows and the null rows side by
side (2 B n rows) and ops.sample_guided mixes them inside the sampler.  A candidate's score is fixed_logp.double().sum(1), the
conditional log-probabilities of its codes under the passes that fixed them; rank='gain' ranks by sum(fixed_logp - fixed_logp_u).
nll_threshold, token_nll and detect raise as in the parent, sample_ids as in ConditionalPriorTrainer.  pseudo_nll is the parent's map
under the batch's own label tokens and edit(pnll_threshold=) a fourth selector on it; detect_pseudo raises: a prior that is told
where the lesion is cannot detect it.
"""
import torch

from hipops import AdamW, ops

from .label_cond import LabelConditionMixin
from .masked_prior import MaskedPriorTrainer
from .prior import parameter_groups


class ConditionalMaskedPriorTrainer(LabelConditionMixin, MaskedPriorTrainer):
    _NAME = "ConditionalMaskedPriorTrainer"
    _KEY = "model.prior.masked.cond"

    def __init__(self, vqgan, gpt, cond, lr=4.5e-4, betas=(0.9, 0.95), weight_decay=0.01, grad_norm_clip=1.0, p_uncond=0.0,
                 cond_drop_seed=None, **kwargs):
        self._init_condition(cond, p_uncond, cond_drop_seed)
        super().__init__(vqgan, gpt, lr=lr, betas=betas, weight_decay=weight_decay, grad_norm_clip=grad_norm_clip, **kwargs)
        if cond.n_embed != gpt.config.n_embed:
            raise ValueError("ConditionalMaskedPriorTrainer: the condition's n_embed=%d must equal the GPT's n_embed=%d" % (
                cond.n_embed, gpt.config.n_embed))
        self.cond = cond.to(self.device).train()
        self.Tc = self.h * self.w
        groups, self.group_names = parameter_groups(self.gpt, weight_decay)
        groups[1]["params"].append(self.cond.embed.weight)          # an embedding table: undecayed, as the GPT's own
        self.optim = AdamW(groups, lr=lr, betas=tuple(betas), weight_decay=weight_decay, max_grad_norm=grad_norm_clip)

    def modules(self):
        return {"decoder": self.vqgan, "transformer": self.gpt, "cond": self.cond}

    def codes(self, batch):
        ids = super().codes(batch)
        if ids.shape[1] != self.h * self.w:
            raise ValueError("ConditionalMaskedPriorTrainer: sequences of h w = %d x %d = %d codes expected, got %d" % (
                self.h, self.w, self.h * self.w, ids.shape[1]))
        return ids

    # ---------------------------------------------------------------- the step
    def _conditioned(self, tokens, drop=None):
        """inp -> logits under the conditioning tokens (B, T); drop = (p, seed, call): whole samples under the null embedding."""
        return lambda inp: self.gpt.forward_conditioned(inp, tokens, self.cond.embed.weight, self.cond.null_index, drop)

    def _null_tokens(self, B):
        return torch.full((B, self.Tc), self.cond.null_index, dtype=torch.long, device=self.device)

    def _forward_of(self, batch):
        return self._conditioned(self.cond_tokens(batch))

    def _train_forward(self, batch):
        """Training step step_count: with p_uncond > 0 the dropped samples are a function of (cond_drop_seed, step_count) alone."""
        drop = (self.p_uncond, self.cond_drop_seed, self.step_count) if self.p_uncond > 0 else None
        return self._conditioned(self.cond_tokens(batch), drop)

    @torch.no_grad()
    def validation_step(self, batch):
        """The parent's under the batch's label; with a null embedding also loss_uncond, the same codes under the same mask (ratio
        0.5, call 0) and the null condition: how much the label is worth is loss_uncond - loss."""
        out = super().validation_step(batch)
        if self.cond.null_index is not None:
            ids = out["ids"]
            was_training = self.gpt.training
            self.gpt.eval()
            try:
                out["loss_uncond"] = self._masked_loss(ids, 0, self.VAL_RATIO, forward=self._conditioned(self._null_tokens(ids.shape[0])))
            finally:
                self.gpt.train(was_training)
        return out

    # ---------------------------------------------------------------- sampling
    def _cond_arg(self, tokens):
        return tokens, self.cond.embed.weight, self.cond.null_index

    @torch.no_grad()
    def synthesize(self, label=None, cond=None, n_candidates=4, n_steps=None, temperature=1.0, top_k=None, top_p=None, generator=None,
                   uniforms=None, guidance_scale=None, rank="cond"):
        """Slices from label maps alone: every code is drawn, from an all-masked grid, in n_steps (default: the trainer's) parallel
        passes.  label (B, H, W) or (B, 1, H, W), or cond (B, T) torch.long - exactly one.  ONE MaskedGPT.generate_parallel call
        draws all B n_candidates rows; each candidate's uniforms (n_steps, 2, B, T) are one torch.rand call, candidate 0 first: its
        codes do not depend on n_candidates.  uniforms (n_candidates, n_steps, 2, B, T): the draws, in place of the generator.
        A candidate's score is fixed_logp.double().sum(1) and the first maximum wins.  Returns ConditionalPriorTrainer.synthesize's
        dict: ids (B, T) the winner, candidates (B, n, T), scores (B, n) float64, best (B,), cond (B, T) and image, the winner
        through decode_from_ids.

        guidance_scale other than None or 1: classifier-free guidance (generate_parallel's guided route); scores stay the
        conditional log-probabilities, the dict gains scores_uncond (B, n) float64, the null rows' sums, and rank='gain' ranks by
        sum(fixed_logp - fixed_logp_u) in double in place of rank='cond'."""
        guided, scale = self._guidance("synthesize", guidance_scale, rank)
        if (label is None) == (cond is None):
            raise ValueError("ConditionalMaskedPriorTrainer.synthesize: exactly one of label and cond gives the condition")
        n = int(n_candidates)
        if n < 1:
            raise ValueError("ConditionalMaskedPriorTrainer.synthesize: n_candidates=%r must be at least 1" % (n_candidates,))
        n_steps = self.n_steps if n_steps is None else int(n_steps)
        tokens = self.cond_tokens({"cond": cond} if cond is not None else {"label": label})
        B, T = tokens.shape
        if uniforms is None:
            uniforms = torch.stack([torch.rand(n_steps, 2, B, T, generator=generator, device=self.device) for _ in range(n)], dim=3)
        elif tuple(uniforms.shape) != (n, n_steps, 2, B, T):
            raise ValueError("ConditionalMaskedPriorTrainer.synthesize: uniforms of shape %s, (n_candidates, n_steps, 2, B, T) = "
                             "(%d, %d, 2, %d, %d) expected" % (tuple(uniforms.shape), n, n_steps, B, T))
        else:
            uniforms = uniforms.to(device=self.device, dtype=torch.float32).permute(1, 2, 3, 0, 4)
        uniforms = uniforms.reshape(n_steps, 2, B * n, T)          # row b n + c: candidate c of slice b
        ids = torch.full((B * n, T), self.mask_token, dtype=torch.long, device=self.device)
        masked = torch.ones((B * n, T), dtype=torch.uint8, device=self.device)
        drawn, logp, *rest = self.gpt.generate_parallel(
            ids, masked, n_steps, temperature=temperature, top_k=top_k, top_p=top_p, choice_temperature=self.choice_temperature,
            uniforms=uniforms, cond=self._cond_arg(tokens.repeat_interleave(n, dim=0)), guidance_scale=scale)
        scores, scores_u, key = self._rank(logp, rest[0] if guided else None, B, n, rank)
        best = torch.from_numpy(key.cpu().numpy().argmax(axis=1)).to(self.device)      # the read of the ranking; first maximum
        candidates = drawn.reshape(B, n, T)
        ids = candidates[torch.arange(B, device=self.device), best]
        out = {"ids": ids, "candidates": candidates, "scores": scores, "best": best, "cond": tokens,
               "image": self.vqgan.decode_from_ids(ids, self.h, self.w)}
        if guided:
            out["scores_uncond"] = scores_u
        return out

    # ---------------------------------------------------------------- scoring the samples
    def _score_draws(self, conditions, n_samples, batch_size, temperature, top_k, top_p, generator, guidance_scale=None, n_steps=None):
        """One sample per held-out slice, drawn from that slice's own label map (synthesize with one candidate): n_samples must be
        the number of held-out slices."""
        n_real = sum(int(c.shape[0]) for c in conditions)
        if n_samples != n_real:
            raise ValueError("ConditionalMaskedPriorTrainer.score: one sample is drawn per held-out slice: n_samples=%d must equal the %d "
                             "slices" % (n_samples, n_real))
        tokens = torch.cat(conditions)
        for i in range(0, n_real, batch_size):
            yield self.synthesize(cond=tokens[i:i + batch_size], n_candidates=1, n_steps=n_steps, temperature=temperature, top_k=top_k,
                                  top_p=top_p, generator=generator, guidance_scale=guidance_scale)["ids"]

    # ---------------------------------------------------------------- editing
    def _pseudo_cond(self, batch):
        """pseudo_nll under the batch's own label tokens: -log p(code | the other codes, the label map)."""
        return self._cond_arg(self.cond_tokens(batch))

    def detect_pseudo(self, *args, **kwargs):
        raise NotImplementedError("ConditionalMaskedPriorTrainer.detect_pseudo: a prior that is told where the lesion is (the label map "
                                  "it is conditioned on) cannot detect it; use the unconditional MaskedPriorTrainer (model.prior.masked "
                                  "without cond)")

    @torch.no_grad()
    def edit(self, batch, mask=None, box=None, nll_threshold=None, n_candidates=4, n_steps=None, temperature=1.0, top_k=None, top_p=None,
             generator=None, new_label=None, guidance_scale=None, rank="cond", pnll_threshold=None, stride=None, blend=None,
             blend_levels=None, blend_source="edit"):
        """MaskedPriorTrainer.edit under a condition, with ConditionalPriorTrainer.edit's third selector: exactly one of mask, box
        and new_label.  With mask or box the condition is the batch's own.  new_label (the batch's 'label' with the user's changes
        drawn in; same dtype and shape): the condition comes from new_label, the redrawn cells are those in which any pixel of the
        label changed (ops.cells_changed; one device-to-host read) and every other code is kept; a label unchanged everywhere
        returns the slice unchanged with the score 0.  Returns the parent's dict plus cond (B, T), the tokens of the condition, and
        label_cells (B, h, w), the same as a map over the latent.  guidance_scale and rank as in synthesize: under guidance the
        dict gains scores_uncond.  pnll_threshold (with `stride`, default (2, 2)) is the fourth selector: the codes whose pseudo_nll
        under the batch's own label exceeds it, redrawn under that label (one device-to-host read of the map).  nll_threshold raises
        NotImplementedError, stride without pnll_threshold ValueError.  blend, blend_levels and blend_source as in
        PriorTrainer.edit, on every selector."""
        blending = self._blending(batch, blend, blend_levels, blend_source)
        if nll_threshold is not None:
            self._no_likelihood("edit(nll_threshold=...)")
        guided, scale = self._guidance("edit", guidance_scale, rank)
        if (mask is not None) + (box is not None) + (new_label is not None) + (pnll_threshold is not None) != 1:
            raise ValueError("ConditionalMaskedPriorTrainer.edit: exactly one of mask, box and new_label selects the region, or "
                             "pnll_threshold in their place")
        if stride is not None and pnll_threshold is None:
            raise ValueError("ConditionalMaskedPriorTrainer.edit: stride=%r is the lattice of pnll_threshold and needs it" % (stride,))
        cells = None
        has_label = isinstance(batch, dict) and batch.get("label") is not None
        label_size = tuple(batch["label"].shape[-2:]) if has_label else None          # what a mask or box of an {'ids'} batch refers to
        if new_label is not None:
            if not has_label:
                raise ValueError("ConditionalMaskedPriorTrainer.edit: new_label needs the batch's own 'label' to compare against")
            changed = ops.cells_changed(self._label(batch["label"]), self._label(new_label), self.h, self.w)
            cells = changed.cpu().numpy() != 0                         # the one read of the selector
            tokens = self.cond.tokens(self._label(new_label))
        else:
            tokens = self.cond_tokens(batch)
            if pnll_threshold is not None:
                cells = self._pseudo_cells(batch, pnll_threshold, stride)[0]
        out = self._edit_parallel(batch, mask, box, n_candidates, n_steps, temperature, top_k, top_p, generator, cells=cells,
                                  image_size=label_size, cond=self._cond_arg(tokens), guidance=(scale, rank) if guided else None,
                                  blending=blending)
        out["cond"], out["label_cells"] = tokens, tokens.reshape(-1, self.h, self.w)
        return out
