"""What the two label-conditioned code priors share (trainers/cond_prior.py: the autoregressive prior behind a conditioning prefix;
trainers/masked_cond_prior.py: the masked prior with the condition added to every position): a batch's conditioning tokens, the
checks of the classifier-free guidance arguments, the ranking of candidates, the seed of the dropped samples in the checkpoint and
the default picture size of a mask.  A mixin in front of a PriorTrainer: it reads self.cond (networks.LabelCondition), self.Tc = h w,
self.h, self.w, self.vqgan and self.device, and names the class and its config key in every message (_NAME, _KEY).
"""
import numpy as np
import torch


class LabelConditionMixin:
    _NAME = "ConditionalPriorTrainer"
    _KEY = "model.prior.cond"

    def _init_condition(self, cond, p_uncond, cond_drop_seed):
        """The constructor's checks of the condition and of the drop, before the parent's constructor runs: sets p_uncond,
        cond_drop_seed and _cond_grid (read by _latent_grid inside the parent's constructor)."""
        from networks.label_condition import LabelCondition
        if not isinstance(cond, LabelCondition):
            raise TypeError("%s conditions on a networks.LabelCondition" % self._NAME)
        p_uncond = float(p_uncond)
        if not 0.0 <= p_uncond < 1.0:
            raise ValueError("%s: p_uncond=%r must lie in [0, 1)" % (self._NAME, p_uncond))
        if p_uncond > 0 and cond.null_index is None:
            raise ValueError("%s: p_uncond=%g needs a condition with the null embedding, LabelCondition(..., "
                             "null_token=True) (%s.null_token)" % (self._NAME, p_uncond, self._KEY))
        if p_uncond > 0 and cond_drop_seed is None:
            raise ValueError("%s: p_uncond=%g needs cond_drop_seed (%s.drop_seed): the drop of a step "
                             "is a function of (cond_drop_seed, step)" % (self._NAME, p_uncond, self._KEY))
        self.p_uncond, self.cond_drop_seed = p_uncond, None if cond_drop_seed is None else int(cond_drop_seed)
        self._cond_grid = (cond.h, cond.w)

    def _latent_grid(self, vqgan):
        """The condition's grid: the square one of the VQGAN's own resolution, or that of the pictures a run feeds the (fully
        convolutional) VQGAN; codes() holds every batch to it."""
        return self._cond_grid

    # ---------------------------------------------------------------- the tokens
    def cond_tokens(self, batch):
        """The conditioning tokens (B, Tc) torch.long of a batch: its 'cond', else LabelCondition.tokens of its 'label'."""
        if not isinstance(batch, dict) or (batch.get("cond") is None and batch.get("label") is None):
            has_ids = isinstance(batch, dict) and batch.get("ids") is not None
            raise ValueError("%s: the batch has no '%s'" % (self._NAME, "cond" if has_ids else "label"))
        if batch.get("cond") is not None:
            tokens = batch["cond"].to(self.device)
        else:
            tokens = self.cond.tokens(self._label(batch["label"]))
        if tokens.dim() != 2 or tokens.shape[1] != self.Tc or tokens.dtype != torch.long:
            raise ValueError("%s: cond (B, Tc) = (B, %d) torch.long expected, got %s of %s" % (self._NAME, self.Tc, tuple(tokens.shape), tokens.dtype))
        return tokens

    def _label(self, label):
        return label.to(self.device).contiguous()

    # ---------------------------------------------------------------- the checkpoint
    def state_dict(self):
        state = super().state_dict()
        if self.p_uncond > 0:          # off: the checkpoint's extra is what it was
            state["extra"].update(cond_drop_seed=self.cond_drop_seed)
        return state

    def load_state_dict(self, state):
        extra = state.get("extra") or {}
        if self.p_uncond > 0 and extra.get("cond_drop_seed", self.cond_drop_seed) != self.cond_drop_seed:
            raise ValueError("%s: the checkpoint was trained with cond_drop_seed=%r, this trainer has %r: the run "
                             "would not continue with the same dropped samples" % (self._NAME, extra["cond_drop_seed"], self.cond_drop_seed))
        super().load_state_dict(state)

    # ---------------------------------------------------------------- guidance and ranking
    def _guidance(self, what, guidance_scale, rank):
        """(guided?, scale) of a synthesize / edit call, refused before any kernel."""
        if rank not in ("cond", "gain"):
            raise ValueError("%s.%s: rank=%r must be 'cond' or 'gain'" % (self._NAME, what, rank))
        guided = guidance_scale is not None and float(guidance_scale) != 1.0
        if guided:
            scale = float(guidance_scale)
            if not (np.isfinite(scale) and scale >= 0.0):
                raise ValueError("%s.%s: guidance_scale=%r must be finite and not negative" % (self._NAME, what, guidance_scale))
            if self.cond.null_index is None:
                raise ValueError("%s.%s: guidance_scale=%r needs a prior trained with the null embedding "
                                 "(%s.null_token)" % (self._NAME, what, guidance_scale, self._KEY))
        elif rank == "gain":
            raise ValueError("%s.%s: rank='gain' compares the conditional and the unconditional score and needs "
                             "guidance (guidance_scale other than 1)" % (self._NAME, what))
        return guided, (float(guidance_scale) if guided else None)

    @staticmethod
    def _rank(logp, logp_u, B, n, rank):
        """(scores (B, n), scores_uncond or None, the ranking key): sums in double; rank 'gain': sum(logp - logp_u)."""
        scores = logp.double().sum(1).reshape(B, n)
        if logp_u is None:
            return scores, None, scores
        scores_u = logp_u.double().sum(1).reshape(B, n)
        key = (logp.double() - logp_u.double()).sum(1).reshape(B, n) if rank == "gain" else scores
        return scores, scores_u, key

    def sample_ids(self, n, temperature=1.0, top_k=None, generator=None):
        raise NotImplementedError("%s: sampling needs a condition: synthesize(label=...) or synthesize(cond=...)" % self._NAME)

    def _score_condition(self, batch):
        return self.cond_tokens(batch)

    def cell_mask(self, B, mask=None, box=None, image_size=None):
        """The parent's; without image_size: the VQGAN's resolution where the latent grid divides it, else the grid itself (a mask
        at code resolution, a box in cells)."""
        if image_size is None:
            res = int(self.vqgan.encoder.resolution)
            image_size = (res, res) if res % self.h == 0 and res % self.w == 0 else (self.h, self.w)
        return super().cell_mask(B, mask, box, image_size)
