"""The code prior conditioned on a label map (the launcher's -p with model.prior.cond): p(codes | label tokens), taming-transformers'
recipe for a segmentation-conditioned transformer restated on this project's kernels.

A label map becomes one conditioning token per latent cell (networks.LabelCondition.tokens, ops.cell_labels: the majority label of
the cell) and the Tc = h w tokens, embedded by a table of their own, stand in front of the code sequence as a fully visible prefix:
the GPT runs with n_unmasked = Tc on [cond embeddings | sos, code 0 .. code T - 2] and GPT.forward_tail leaves the prefix's rows
out of ln_f, the head and the loss.  Positions: Tc + T <= block_size.  The start token and the pkeep corruption are the
unconditional trainer's, on the codes only.  The table's one parameter joins the undecayed group of the fused AdamW: the global
gradient norm and the clip cover it.

Batches: {'image', 'label'} (codes from the frozen VQGAN, tokens from the label map) or {'ids', 'cond'} with cond (B, Tc)
torch.long; 'cond', where a batch has it, is the prefix.

synthesize(label | cond) draws every code from the label alone; edit(batch, new_label=...) redraws the cells whose label changed
under the new label's prefix and keeps every other code.  detect is refused: lesion labels as a condition would leak the answer.

Classifier-free guidance.  Training (p_uncond > 0, a condition built with null_token=True, a cond_drop_seed): the prefix of step n
is LabelCondition.forward(tokens, drop=(p_uncond, cond_drop_seed, n)) - whole samples read the null embedding, decided by the
counter-based draw of csrc/dropout.h, a function of (cond_drop_seed, n) alone, so a resumed run continues bit for bit with no new
checkpoint state; the seed goes into the checkpoint's `extra` and a mismatch on load raises.  validation_step also returns
loss_uncond, the cross-entropy under the null prefix.  Sampling (synthesize / edit with guidance_scale other than None or 1): the
null prefix runs beside the label's in GPT.generate_masked's guided route; the result gains scores_uncond and rank='gain' picks the
candidate whose sum(logp - logp_u) is largest - how much the label explains it - in place of rank='cond', the conditional score.
"""
import numpy as np
import torch

from hipops import AdamW, ops

from .label_cond import LabelConditionMixin
from .prior import PriorTrainer, parameter_groups


class ConditionalPriorTrainer(LabelConditionMixin, PriorTrainer):
    """The batch -> tokens logic, the guidance checks, the ranking, the drop seed's place in the checkpoint and cell_mask's default
    are LabelConditionMixin's (trainers/label_cond.py), shared with the conditional masked prior."""

    def __init__(self, vqgan, gpt, cond, pkeep=1.0, sos_token=0, lr=4.5e-4, betas=(0.9, 0.95), weight_decay=0.01, grad_norm_clip=1.0,
                 warmup_steps=0, decay_steps=0, seed=0, device="cuda", dropout_seed=None, p_uncond=0.0, cond_drop_seed=None):
        self._init_condition(cond, p_uncond, cond_drop_seed)
        super().__init__(vqgan, gpt, pkeep=pkeep, sos_token=sos_token, lr=lr, betas=betas, weight_decay=weight_decay,
                         grad_norm_clip=grad_norm_clip, warmup_steps=warmup_steps, decay_steps=decay_steps, seed=seed, device=device,
                         dropout_seed=dropout_seed)
        T = self.h * self.w
        if cond.n_embed != gpt.config.n_embed:
            raise ValueError("ConditionalPriorTrainer: the condition's n_embed=%d must equal the GPT's n_embed=%d" % (cond.n_embed, gpt.config.n_embed))
        if gpt.block_size < 2 * T:
            raise ValueError("ConditionalPriorTrainer: the GPT's block_size=%d must be at least Tc + T = 2 h w = %d" % (gpt.block_size, 2 * T))
        if gpt.config.n_unmasked != T:
            raise ValueError("ConditionalPriorTrainer: the GPT's n_unmasked=%d must be Tc = h w = %d, the fully visible conditioning prefix" % (
                gpt.config.n_unmasked, T))
        self.cond = cond.to(self.device).train()
        self.Tc = T
        groups, self.group_names = parameter_groups(self.gpt, weight_decay)
        groups[1]["params"].append(self.cond.embed.weight)          # an embedding table: undecayed, as the GPT's own
        self.optim = AdamW(groups, lr=lr, betas=tuple(betas), weight_decay=weight_decay, max_grad_norm=grad_norm_clip)

    def modules(self):
        return {"decoder": self.vqgan, "transformer": self.gpt, "cond": self.cond}

    def codes(self, batch):
        ids = super().codes(batch)
        if ids.shape[1] != self.h * self.w:
            raise ValueError("ConditionalPriorTrainer: sequences of h w = %d x %d = %d codes expected, got %d" % (self.h, self.w, self.h * self.w, ids.shape[1]))
        return ids

    # ---------------------------------------------------------------- the prefix
    def _prefix(self, batch):
        return self.cond(self.cond_tokens(batch))

    def _null_prefix(self, B):
        return self.cond.null_prefix(B)

    def _train_prefix(self, batch):
        """The prefix of training step step_count: with p_uncond > 0 whole samples are dropped onto the null embedding."""
        if self.p_uncond > 0:
            return self.cond(self.cond_tokens(batch), drop=(self.p_uncond, self.cond_drop_seed, self.step_count))
        return self._prefix(batch)

    @torch.no_grad()
    def validation_step(self, batch):
        """The parent's; with a null embedding also loss_uncond, the cross-entropy of the same codes under the null prefix (eval
        mode, no corruption): how much the label is worth is loss_uncond - loss."""
        out = super().validation_step(batch)
        if self.cond.null_index is not None:
            ids = out["ids"]
            was_training = self.gpt.training
            self.gpt.eval()
            try:
                out["loss_uncond"] = ops.cross_entropy(self._logits(self._inputs(ids, 1.0), self.cond.null_prefix(ids.shape[0])), ids)
            finally:
                self.gpt.train(was_training)
        return out

    def _logits(self, inp, prefix):
        return self.gpt.forward_tail(inp, prefix, n_tail=inp.shape[1])

    # ---------------------------------------------------------------- sampling
    @torch.no_grad()
    def synthesize(self, label=None, cond=None, n_candidates=4, temperature=1.0, top_k=None, top_p=None, generator=None, uniforms=None,
                   guidance_scale=None, rank="cond"):
        """Slices from label maps alone: every code is drawn.  label (B, H, W) or (B, 1, H, W), or cond (B, Tc) torch.long - exactly
        one.  ONE GPT.generate_masked call behind the prompt [cond prefix | sos] draws all B n_candidates rows with every position
        resampled (the uniforms per candidate, candidate 0 first, as edit draws them); a candidate's score is the sum of its logp in
        double and the first maximum wins.  uniforms (n_candidates, T, B): the draws, in place of the generator.  Returns a dict: ids (B, T) the winner, candidates (B, n, T), scores (B, n) float64, best
        (B,), cond (B, Tc) and image, the winner through decode_from_ids.

        guidance_scale other than None or 1: classifier-free guidance - the null prefix runs beside the label's (GPT.generate_masked's
        guided route); scores stay the conditional log-probabilities, the dict gains scores_uncond (B, n) float64, the same under
        the null prefix, and rank='gain' ranks by sum(logp - logp_u) in double (first maximum) in place of rank='cond', the
        conditional score."""
        guided, scale = self._guidance("synthesize", guidance_scale, rank)
        if (label is None) == (cond is None):
            raise ValueError("ConditionalPriorTrainer.synthesize: exactly one of label and cond gives the condition")
        n = int(n_candidates)
        if n < 1:
            raise ValueError("ConditionalPriorTrainer.synthesize: n_candidates=%r must be at least 1" % (n_candidates,))
        tokens = self.cond_tokens({"cond": cond} if cond is not None else {"label": label})
        B, T = tokens.shape[0], self.h * self.w
        start = torch.full((B * n, 1), self.sos_token, dtype=torch.long, device=self.device)
        known = torch.zeros((B * n, T), dtype=torch.long, device=self.device)
        if uniforms is None:
            uniforms = torch.stack([torch.rand(T, B, generator=generator, device=self.device) for _ in range(n)])
        elif tuple(uniforms.shape) != (n, T, B):
            raise ValueError("ConditionalPriorTrainer.synthesize: uniforms of shape %s, (n_candidates, T, B) = (%d, %d, %d) expected" % (
                tuple(uniforms.shape), n, T, B))
        uniforms = uniforms.to(device=self.device, dtype=torch.float32).permute(1, 2, 0).reshape(T, B * n)
        was_training = self.gpt.training
        self.gpt.eval()
        try:
            kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, uniforms=uniforms, embeddings=self.cond(tokens).repeat_interleave(n, dim=0))
            if guided:
                kw.update(uncond_embeddings=self.cond.null_prefix(B * n), guidance_scale=scale)
            drawn, logp, *rest = self.gpt.generate_masked(start, known, np.ones(T, dtype=bool), **kw)
        finally:
            self.gpt.train(was_training)
        scores, scores_u, key = self._rank(logp, rest[0] if guided else None, B, n, rank)
        best = torch.from_numpy(np.argmax(key.cpu().numpy(), axis=1)).to(self.device)      # the read of the ranking; first maximum
        candidates = drawn.reshape(B, n, T)
        ids = candidates[torch.arange(B, device=self.device), best]
        out = {"ids": ids, "candidates": candidates, "scores": scores, "best": best, "cond": tokens,
               "image": self.vqgan.decode_from_ids(ids, self.h, self.w)}
        if guided:
            out["scores_uncond"] = scores_u
        return out

    # ---------------------------------------------------------------- scoring the samples
    def _score_draws(self, conditions, n_samples, batch_size, temperature, top_k, top_p, generator, guidance_scale=None):
        """One sample per held-out slice, drawn from that slice's own label map (synthesize with one candidate): the score is then
        paired with the condition distribution of the held-out split.  n_samples must be the number of held-out slices."""
        n_real = sum(int(c.shape[0]) for c in conditions)
        if n_samples != n_real:
            raise ValueError("ConditionalPriorTrainer.score: one sample is drawn per held-out slice: n_samples=%d must equal the %d "
                             "slices" % (n_samples, n_real))
        tokens = torch.cat(conditions)
        for i in range(0, n_real, batch_size):
            yield self.synthesize(cond=tokens[i:i + batch_size], n_candidates=1, temperature=temperature, top_k=top_k, top_p=top_p,
                                  generator=generator, guidance_scale=guidance_scale)["ids"]

    # ---------------------------------------------------------------- editing
    @torch.no_grad()
    def edit(self, batch, mask=None, box=None, nll_threshold=None, n_candidates=4, temperature=1.0, top_k=None, top_p=None,
             generator=None, new_label=None, guidance_scale=None, rank="cond", blend=None, blend_levels=None, blend_source="edit"):
        """PriorTrainer.edit under a condition, with a fourth selector: exactly one of mask, box, nll_threshold and new_label.
        With mask, box or nll_threshold the prefix is the batch's own condition.  new_label (the batch's 'label' with the user's
        changes drawn in; same dtype and shape): the prefix comes from new_label, the redrawn cells are those in which any pixel of
        the label changed (ops.cells_changed; one device-to-host read) and every other code is kept.  Returns the parent's dict plus
        cond (B, Tc), the tokens of the prefix, and label_cells (B, h, w), the same tokens as a map over the latent.
        guidance_scale and rank as in synthesize: under guidance the dict gains scores_uncond.  blend, blend_levels and blend_source
        as in PriorTrainer.edit, on every selector."""
        guided, scale = self._guidance("edit", guidance_scale, rank)
        blending = self._blending(batch, blend, blend_levels, blend_source)
        if (mask is not None) + (box is not None) + (nll_threshold is not None) + (new_label is not None) != 1:
            raise ValueError("ConditionalPriorTrainer.edit: exactly one of mask, box, nll_threshold and new_label selects the region")
        cells = None
        has_label = isinstance(batch, dict) and batch.get("label") is not None
        label_size = tuple(batch["label"].shape[-2:]) if has_label else None          # what a mask or box of an {'ids'} batch refers to
        if new_label is not None:
            if not isinstance(batch, dict) or batch.get("label") is None:
                raise ValueError("ConditionalPriorTrainer.edit: new_label needs the batch's own 'label' to compare against")
            changed = ops.cells_changed(self._label(batch["label"]), self._label(new_label), self.h, self.w)
            cells = changed.cpu().numpy() != 0                         # the one read of the selector
            tokens = self.cond.tokens(self._label(new_label))
        else:
            tokens = self.cond_tokens(batch)
        out = self._edit(dict(batch, cond=tokens), mask, box, nll_threshold, n_candidates, temperature, top_k, top_p, generator, cells=cells,
                         image_size=label_size, guidance=(scale, rank) if guided else None, blending=blending)[0]
        out["cond"], out["label_cells"] = tokens, tokens.reshape(-1, self.h, self.w)
        return out

    def detect(self, *args, **kwargs):
        raise NotImplementedError("ConditionalPriorTrainer.detect: a prior conditioned on the labels would be told where the lesion is; "
                                  "anomaly detection needs the unconditional PriorTrainer")
