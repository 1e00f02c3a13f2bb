"""Training the GPT code prior on the codes of a frozen VQGAN (the launcher's -p).  The reference has no trainer for its
networks.GPT; the recipe is minGPT's and taming-transformers': AdamW over decay / no-decay parameter groups, gradient clipping by
the global norm, linear warm-up and cosine decay of the learning rate, teacher forcing behind a start token, and `pkeep` token
corruption as the regulariser (training-mode dropout has no kernel: a GPT with a dropout probability above 0 is refused here).

One step, from {'image'} (encoded by the frozen VQGAN, VQGAN.encode_to_ids: raster order) or {'ids': (B, T) long}:
    inp    = ops.prior_tokens(ids, sos, pkeep, V, u_keep, u_rand)      uniforms from the trainer's own device generator
    logits = gpt(inp)
    loss   = ops.cross_entropy(logits, ids)                            mean over B T
    TrainerBase.update(loss, [optim])                                  hipops.AdamW: norm, clip and update on the device
Nothing is read back: the step returns {'loss', 'grad_norm', 'lr', 'ids'} with the scalars on the device (lr is a host float).

`modules()` is {'decoder': vqgan, 'transformer': gpt}: a -v checkpoint's decoder.* keys load into the frozen first stage
(run.first_stage_ckpt_path), and a prior checkpoint carries both.  `extra` holds the generator's state and the step counter
the learning rate is computed from, so a resumed run continues bit for bit.
"""
import math

import torch
import torch.nn as nn

from hipops import AdamW, ops
from networks.gpt import GPT
from networks.vqgan_model import VQGAN

from .base import TrainerBase


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
                 warmup_steps=0, decay_steps=0, seed=0, device="cuda"):
        if not isinstance(vqgan, VQGAN):
            raise TypeError("PriorTrainer trains on the codes of a networks.VQGAN")
        if not isinstance(gpt, GPT):
            raise TypeError("PriorTrainer trains a networks.GPT")
        super().__init__(device)
        enc = vqgan.encoder
        self.h = self.w = int(enc.resolution) // 2 ** (int(enc.num_resolutions) - 1)
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
        gpt._check_dropout()             # NotImplementedError for a dropout probability above 0, before any kernel runs
        self.vqgan = vqgan.to(self.device).eval().requires_grad_(False)          # frozen: never stepped, never in train mode
        self.gpt = gpt.to(self.device)
        self.pkeep, self.sos_token = float(pkeep), int(sos_token)
        self.lr, self.warmup_steps, self.decay_steps = float(lr), int(warmup_steps), int(decay_steps)
        groups, self.group_names = parameter_groups(self.gpt, weight_decay)
        self.optim = AdamW(groups, lr=lr, betas=tuple(betas), weight_decay=weight_decay, max_grad_norm=grad_norm_clip)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))
        self.step_count = 0

    def modules(self):
        return {"decoder": self.vqgan, "transformer": self.gpt}

    def optimizers(self):
        return {"prior_optim": self.optim}

    def state_dict(self):
        state = super().state_dict()
        state["extra"].update(prior_generator=self.generator.get_state(), prior_step=int(self.step_count))
        return state

    def load_state_dict(self, state):
        super().load_state_dict(state)
        extra = state.get("extra") or {}
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

    def training_step(self, batch, mark=None):
        self.throttle.begin()
        ids = self.codes(batch)
        self.gpt.train()
        inp = self._inputs(ids, self.pkeep)
        loss = ops.cross_entropy(self.gpt(inp), ids)
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
            loss = ops.cross_entropy(self.gpt(self._inputs(ids, 1.0)), ids)
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
