"""The GPT model of the code prior on the MI355X HIP kernels: the reference's GPT class (networks/mingpt.py:122-224) over the blocks of
networks/mingpt.py.  It lives in a module of its own; `networks.GPT` is the public name, as in the reference's networks/__init__.py.

Same constructor signature, attribute names, submodule and parameter creation order and state_dict keys as the reference's class, so
a seed gives the reference's initial values and a reference checkpoint loads with strict=True.  forward() is ops.embedding (token +
position embedding, with the reference's optional `embeddings=` prefix), the blocks, ops.layer_norm and ops.linear without bias; the
loss of the prior is ops.cross_entropy, a token is drawn by ops.sample_topk.

GPT.forward_tail(idx, embeddings, n_tail) is forward() with ln_f and the head on the last n_tail positions only: behind a conditioning
prefix (trainers/cond_prior.py) the prefix's rows of the head and of the logits are never computed.

Dropout: `drop` exists (the trees match); at p = 0 or in eval mode it is the identity.  GPT.seed_dropout(seed, call=0) numbers the
sites of the tree - 0 is `drop`, then per block att_drop, att.res_drop, mlp[3] - and stores seed and call; a training forward of a
seeded model runs ops.dropout behind the embedding, the attention kernels' dropout policy and ops.add_dropout in the residual
adds under (seed, call, site) and then advances call by one; GPT.set_dropout_call(n) sets it (networks/mingpt.py, csrc/dropout.h:
counter-based masks, nothing stored).  A training forward with emb_pdrop, res_pdrop or att_pdrop above 0 on a model that has not
been seeded raises NotImplementedError before any kernel runs.

GPT.forward_with_past.  The reference's body cannot run (`present.append(present)`, mingpt.py:219); what it evidently means is
built: `presents.append(present)`, returning (logits, torch.stack(presents)) of shape (n_layer, 2, B, n_head, T, hs).  With a
past the reference adds pos_embed[:, past_length, :] - ONE position - to every new token, which is only right for one token:
anything but exactly one new token (idx and `embeddings` rows together) behind a past raises ValueError, and past_length + 1 >
block_size raises RuntimeError.  The cached route concatenates the past per step, as the reference does; it applies no mask
(mingpt.py:79-80), so with n_unmasked > 0 it equals the full forward only when the first call carries at least n_unmasked tokens.

Cached generation.  GPT.generate is sample() on a preallocated KV cache: GPT.new_cache builds a KVCache (the kv tensor, its length
and capacity, the model's weights packed into one buffer, the step's workspace), GPT.prefill runs the prompt through the
full-sequence kernels and copies every layer's k and v into the cache, GPT.decode_step is ONE ops.gpt_decode_step call per token:
the whole step - embedding, per layer ln1 + q|k|v (k and v written straight into the cache row), attention over the cache, proj +
residual, ln2 + fc1 + GELU, fc2 + residual, then ln_f + head - is 2 + 5 n_layer launches issued from C, with no copy of the past,
no allocation and no synchronisation.  sample() stays as it is: the yardstick of the new path.  Neither has dropout (eval mode).

Masked resampling.  GPT.generate_masked redraws some positions of a sequence and keeps the others, on the same cache: one prefill over
the prompt and the kept codes in front of the first redrawn position, then per position ONE ops.sample_filtered launch - a draw
(top-k, then top-p) or the kept token, and the log-probability of whichever stands there - and one decode_step.  The resample mask is a
host array: the plan is made without a synchronisation.  The sum of the log-probabilities scores a candidate (trainers/prior.py).
With guidance_scale (classifier-free guidance, trainers/cond_prior.py) the same loop runs on ONE cache of 2B rows - the condition's
prefix in front of the first B, the null condition's in front of the others - and ops.sample_guided draws from z_u + s (z_c - z_u)
inside the sampler: still one sampler launch and one decode_step per position.

Bidirectional masked prior.  MaskedGPT is the same tree with n_unmasked = block_size - every position sees every position - a token
table of vocab_size + 1 rows, the last one the mask token, and a head of vocab_size outputs, so the mask token can never be drawn.
It is trained to fill in masked codes (trainers/masked_prior.py) and decoded in a few parallel passes, MaskedGPT.generate_parallel:
per pass one forward, one ops.sample_filtered launch over all B T rows and one ops.unmask_step launch, which fixes the confident
codes and masks the others again (MaskGIT).  A bidirectional model has no past: the cached routes raise NotImplementedError.
MaskedGPT.forward_conditioned adds one label token's embedding to every position (ops.embedding_cond: the latent grid and the
label-token grid are the same grid, so the sequence stays h w long) and generate_parallel(cond=..., guidance_scale=...) decodes under
it, with classifier-free guidance as one forward over 2B rows and one ops.sample_guided launch per pass.
MaskedGPT.pseudo_nll is the model's opinion of a sequence code by code, -log p(code | the codes outside its lattice group): the
passes of a sample side by side as batch rows (ops.lattice_inputs), ln_f on the rows the map reads only (ops.lattice_gather_ln), the
head and the cross-entropy over B T rows whatever the number of passes (csrc/pseudo_nll.hip).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from hipops import ops

from .mingpt import Block, GPTConfig, SeededDropout, _no_dropout


class GPT(SeededDropout, nn.Module):
    """Token + position embedding, n_layer Blocks, a final LayerNorm and a bias-free head onto the vocabulary; block_size is the
    longest sequence it can see.  Submodules and parameters are created in the reference's order (mingpt.py:149-158): tok_embed,
    pos_embed, drop, blocks, ln_f, head - the random stream of a seed and the state_dict order depend on it."""

    def __init__(self, vocab_size, block_size, n_layer=12, n_head=8, n_embed=256, emb_pdrop=0.0, res_pdrop=0.0, att_pdrop=0.0,
                 n_unmasked=0):
        super().__init__()
        config = GPTConfig(vocab_size, block_size, n_layer=n_layer, n_head=n_head, n_embed=n_embed, emb_pdrop=emb_pdrop,
                           res_pdrop=res_pdrop, att_pdrop=att_pdrop, n_unmasked=n_unmasked)
        self.tok_embed = nn.Embedding(vocab_size, n_embed)
        self.pos_embed = nn.Parameter(torch.zeros(1, block_size, n_embed))
        self.drop = nn.Dropout(emb_pdrop)          # identity at p = 0 or in eval mode; in training mode the p of site 0 (seed_dropout)
        self.blocks = nn.Sequential(*(Block(config) for _ in range(n_layer)))
        self.ln_f = nn.LayerNorm(n_embed)
        self.head = nn.Linear(n_embed, vocab_size, bias=False)
        self.block_size = block_size
        self.apply(self._init_weights)
        self.config = config

    def get_block_size(self):
        return self.block_size

    @staticmethod
    def _init_weights(module):
        """N(0, 0.02) weights for nn.Linear and nn.Embedding, zero biases, LayerNorm at (1, 0): mingpt.py:167-175, drawn in the
        same order from the same generator."""
        if isinstance(module, nn.LayerNorm):
            nn.init.ones_(module.weight)
            nn.init.zeros_(module.bias)
        elif isinstance(module, (nn.Linear, nn.Embedding)):
            nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if getattr(module, "bias", None) is not None:
                nn.init.zeros_(module.bias)

    def _check_dropout(self):
        """Every dropout of the model, before any kernel runs."""
        _no_dropout(self, self.drop, "emb_pdrop")
        for block in self.blocks:
            block.att._check_dropout()
            _no_dropout(block, block.mlp[3], "res_pdrop")

    def _seed_sites(self, seed, site):
        self.dropout_seed, self.dropout_site = seed, site          # `drop`
        site += 1
        for block in self.blocks:
            site = block._seed_sites(seed, site)
        return site

    @staticmethod
    def _new_tokens(idx, embeddings):
        return idx.shape[1] + (embeddings.shape[1] if embeddings is not None else 0)

    def _head(self, x):
        x = ops.layer_norm(x, self.ln_f.weight, self.ln_f.bias, self.ln_f.eps)
        return ops.linear(x, self.head.weight)

    def forward(self, idx, embeddings=None):
        self._check_dropout()
        t = self._new_tokens(idx, embeddings)
        if t > self.block_size:
            raise RuntimeError("GPT: cannot forward T=%d tokens, the model's block_size=%d is exhausted" % (t, self.block_size))
        call = self._dropout_call()
        x = ops.embedding(idx, self.tok_embed.weight, self.pos_embed, embeddings)          # token (or given) + position embedding
        if call is not None and self.drop.p > 0:
            x = ops.dropout(x, self.drop.p, self._key(call, self.dropout_site))
        for block in self.blocks:
            x = block._forward(x, None, call)[0]
        x = self._head(x)
        if call is not None:
            self.set_dropout_call(call + 1)
        return x

    def _trunk(self, idx, embeddings):
        """Everything of a training or evaluation forward in front of ln_f: embedding, its dropout, the blocks -> (x, the dropout call
        or None).  forward() has the same lines in place (it is the reference's method and stays as it was)."""
        call = self._dropout_call()
        x = ops.embedding(idx, self.tok_embed.weight, self.pos_embed, embeddings)
        if call is not None and self.drop.p > 0:
            x = ops.dropout(x, self.drop.p, self._key(call, self.dropout_site))
        for block in self.blocks:
            x = block._forward(x, None, call)[0]
        return x, call

    def forward_tail(self, idx, embeddings=None, n_tail=None):
        """forward() up to the last block, then ln_f and head on the last n_tail positions only -> (B, n_tail, V): behind a
        conditioning prefix (`embeddings`) the prefix's rows of the head and of the logits are never computed.  n_tail None:
        idx's own positions.  With n_tail = every position it is forward() bit for bit.  Dropout bookkeeping is forward()'s: the
        same sites under the same call, which it advances by one."""
        self._check_dropout()
        t = self._new_tokens(idx, embeddings)
        n_tail = idx.shape[1] if n_tail is None else int(n_tail)
        if t > self.block_size:
            raise RuntimeError("GPT: cannot forward T=%d tokens, the model's block_size=%d is exhausted" % (t, self.block_size))
        if not 1 <= n_tail <= t:
            raise ValueError("GPT.forward_tail: n_tail=%d must lie in [1, T = %d]" % (n_tail, t))
        x, call = self._trunk(idx, embeddings)
        x = self._head(x[:, t - n_tail:])
        if call is not None:
            self.set_dropout_call(call + 1)
        return x

    def forward_with_past(self, idx, embeddings=None, past=None, past_length=None):
        # inference only
        assert not self.training
        t = self._new_tokens(idx, embeddings)
        if past is not None:
            assert past_length is not None
            if t != 1:
                raise ValueError("GPT.forward_with_past: %d new tokens behind a past; the one position pos_embed[:, past_length] "
                                 "is only right for exactly one" % t)
            if past_length + 1 > self.block_size:
                raise RuntimeError("GPT.forward_with_past: past_length + 1 = %d exceeds block_size=%d" % (past_length + 1, self.block_size))
            past = torch.cat(past, dim=-2)          # the calls so far, joined along the token axis
            want = (self.config.n_layer, 2, idx.shape[0], self.config.n_head, past_length, self.config.n_embed // self.config.n_head)
            assert tuple(past.shape) == want, "past of shape %s, (n_layer, 2, B, n_head, past_length, hs) = %s expected" % (tuple(past.shape), want)
            t0 = past_length
        else:
            if t > self.block_size:
                raise RuntimeError("GPT: cannot forward T=%d tokens, the model's block_size=%d is exhausted" % (t, self.block_size))
            t0 = 0

        x = ops.embedding(idx, self.tok_embed.weight, self.pos_embed, embeddings, t0=t0)
        presents = []
        for i, block in enumerate(self.blocks):
            x, present = block(x, layer_past=past[i, ...] if past is not None else None, return_present=True)
            presents.append(present)

        return self._head(x), torch.stack(presents)

    @torch.no_grad()
    def sample(self, idx, steps, temperature=1.0, top_k=None, generator=None, embeddings=None):
        """idx (B, Tp) with `steps` sampled tokens appended, in eval mode: the whole prompt (behind `embeddings`, if given) goes through
        forward_with_past once, then one token per call behind the accumulated past.  Each step draws torch.rand(B, generator=...)
        on the device and picks by ops.sample_topk from the last position's logits."""
        t = self._new_tokens(idx, embeddings)
        if steps < 0 or t + steps > self.block_size:
            raise RuntimeError("GPT.sample: prompt of %d tokens + %d steps exceeds block_size=%d" % (t, steps, self.block_size))
        if not temperature > 0:
            raise ValueError("GPT.sample: temperature=%r must be positive" % (temperature,))
        was_training = self.training
        self.eval()
        try:
            past, new, emb = None, idx, embeddings
            for k in range(steps):
                logits, present = self.forward_with_past(new, embeddings=emb, past=past, past_length=None if past is None else t + k - 1)
                past = [present] if past is None else past + [present]
                u = torch.rand(idx.shape[0], generator=generator, device=logits.device)
                new = ops.sample_topk(logits[:, -1, :], u, temperature, top_k).unsqueeze(1)
                idx, emb = torch.cat((idx, new), dim=1), None
        finally:
            self.train(was_training)
        return idx

    # ---- cached generation: a preallocated KV cache and one host call per token (module docstring, "Cached generation")
    def new_cache(self, batch_size, capacity=None):
        """A KVCache for `batch_size` rows and `capacity` positions (default: block_size) on the model's device, with the weights
        packed as they are now."""
        capacity = self.block_size if capacity is None else int(capacity)
        if batch_size < 1 or capacity < 1:
            raise ValueError("GPT.new_cache: batch_size=%d and capacity=%d must be at least 1" % (batch_size, capacity))
        return KVCache(self, int(batch_size), capacity)

    def _check_cache(self, what, cache, B):
        if self.training:
            raise RuntimeError("GPT.%s: inference only, the model is in training mode (call .eval())" % what)
        if cache.batch_size != B:
            raise RuntimeError("GPT.%s: the cache was built for batch size %d, got %d rows" % (what, cache.batch_size, B))

    @torch.no_grad()
    def prefill(self, idx, cache, embeddings=None):
        """The whole prompt idx (B, Tp) (behind `embeddings`, if given) through the full-sequence kernels - forward_with_past's first
        call - with every layer's k and v copied into the cache rows [0, T) (one copy_ per layer); sets cache.length = T and returns
        the logits (B, T, V).  Under the model's causal mask; the steps behind it apply none (forward_with_past's caveat): with
        n_unmasked > 0 the prompt must carry at least n_unmasked tokens for the route to equal the full forward."""
        self._check_cache("prefill", cache, idx.shape[0])
        t = self._new_tokens(idx, embeddings)
        if t < 1 or t > self.block_size or t > cache.capacity:
            raise RuntimeError("GPT.prefill: a prompt of T=%d tokens; 1 <= T <= block_size=%d and T <= the cache's capacity=%d are needed" % (
                t, self.block_size, cache.capacity))
        nh = self.config.n_head
        x = ops.embedding(idx, self.tok_embed.weight, self.pos_embed, embeddings)
        for i, block in enumerate(self.blocks):
            x, present = block(x, return_present=True)                                  # (2, B, nh, T, hs)
            cache.kv[i][:, :, :t].unflatten(-1, (nh, -1)).copy_(present.transpose(2, 3))     # -> (2, B, T, nh, hs): the heads side by side
        cache.length = t
        return self._head(x)

    @torch.no_grad()
    def decode_step(self, idx, cache):
        """One token per row, idx (B,) or (B, 1) torch.long on the device, behind the cache: ONE ops.gpt_decode_step call - the whole
        step is launched from C, nothing is allocated but the logits, nothing synchronises.  Writes row cache.length of every
        plane, advances cache.length and returns the logits (B, V) of the new position.  No mask (the layer_past route)."""
        self._check_cache("decode_step", cache, idx.shape[0])
        if idx.numel() != idx.shape[0]:
            raise ValueError("GPT.decode_step: one token per row expected, got idx of shape %s" % (tuple(idx.shape),))
        if cache.length >= cache.capacity:
            raise RuntimeError("GPT.decode_step: the cache is full (length = capacity = %d)" % cache.capacity)
        if cache.length + 1 > self.block_size:
            raise RuntimeError("GPT.decode_step: length + 1 = %d exceeds block_size=%d" % (cache.length + 1, self.block_size))
        logits = torch.empty(cache.batch_size, self.config.vocab_size, dtype=torch.float32, device=cache.kv.device)
        ops.gpt_decode_step(cache.packed, self.tok_embed.weight, self.pos_embed, idx.reshape(-1), cache.kv, logits, cache.ws, cache.length,
                            self.config.n_head, self.ln_f.eps)
        cache.length += 1
        return logits

    @torch.no_grad()
    def generate(self, idx, steps, temperature=1.0, top_k=None, generator=None, embeddings=None, uniforms=None):
        """sample() on the cached route: idx (B, Tp) with `steps` sampled tokens appended, in eval mode.  The prompt goes through
        prefill once, then every step is ops.sample_topk on the last logits and one decode_step.  Without `uniforms` each step draws
        torch.rand(B, generator=...) on the device exactly as sample() does - a seed means the same stream in both; with `uniforms`
        (steps, B) nothing is drawn and step k uses uniforms[k]."""
        t = self._new_tokens(idx, embeddings)
        if steps < 0 or t + steps > self.block_size:
            raise RuntimeError("GPT.generate: prompt of %d tokens + %d steps exceeds block_size=%d" % (t, steps, self.block_size))
        if not temperature > 0:
            raise ValueError("GPT.generate: temperature=%r must be positive" % (temperature,))
        B = idx.shape[0]
        if uniforms is not None and tuple(uniforms.shape) != (steps, B):
            raise ValueError("GPT.generate: uniforms of shape %s, (steps, B) = (%d, %d) expected" % (tuple(uniforms.shape), steps, B))
        if steps == 0:
            return idx
        was_training = self.training
        self.eval()
        try:
            cache = self.new_cache(B, capacity=t + steps - 1)          # the last sampled token is never fed back
            if uniforms is not None:
                uniforms = uniforms.to(device=cache.kv.device, dtype=torch.float32)
            logits = self.prefill(idx, cache, embeddings)[:, -1, :]
            out = [idx]
            for k in range(steps):
                u = uniforms[k] if uniforms is not None else torch.rand(B, generator=generator, device=logits.device)
                new = ops.sample_topk(logits, u, temperature, top_k)
                out.append(new.unsqueeze(1))
                if k + 1 < steps:
                    logits = self.decode_step(new, cache)
        finally:
            self.train(was_training)
        return torch.cat(out, dim=1)

    @torch.no_grad()
    def generate_masked(self, idx, known, resample, temperature=1.0, top_k=None, top_p=None, generator=None, uniforms=None,
                        embeddings=None, uncond_embeddings=None, guidance_scale=None):
        """Redraw some positions of a sequence and keep the others: behind the prompt idx (B, Tp) (and `embeddings`), position k
        of the S new ones takes known[:, k] where resample is false and a draw - top-k, then top-p, ops.sample_filtered - where it
        is true.  Either way the token goes into the cache: what follows is conditioned on what was kept and on what was drawn.
        known (B, S) torch.long on the device; resample a HOST bool array (S,) or (B, S) - the plan below is made from it without
        a synchronisation.  Returns (tokens (B, S) torch.long, logp (B, S) fp32), logp[:, k] the model's log-probability
        (temperature 1, unfiltered) of the token that stands at k.

        With j0 the first column in which any row resamples, the prompt and known[:, :j0] go through prefill once (their logp:
        minus the cross-entropy of the prefill logits); from j0 on each position is one ops.sample_filtered launch - forced to
        that column of where(resample, -1, known) - and one decode_step; the last token is not fed back.  Nothing resampled: one
        prefill and nothing else.  uniforms (S - j0, B), or a generator, as in generate().  Refused before any kernel: training
        mode, Tp + S - 1 > block_size, n_unmasked > Tp + j0 (the decode steps apply no mask: prefill's caveat), shapes, top_p
        outside (0, 1].

        Classifier-free guidance.  guidance_scale None or 1.0: the route above, bit for bit; no unconditional row is computed.
        Otherwise `embeddings` and `uncond_embeddings` (one shape: the condition's prefix and the null condition's) are needed and
        every draw is made from z = z_u + guidance_scale (z_c - z_u): ONE cache of 2B rows - the rows [0, B) behind `embeddings`,
        the rows [B, 2B) behind `uncond_embeddings` - ONE prefill over cat(embeddings, uncond_embeddings) with the prompt and the
        kept prefix repeated, then per position ONE ops.sample_guided launch (the mix is made inside the sampler; its (2B,) output
        is the next step's idx for both halves) and ONE decode_step at 2B rows: the launch count of the unguided route.  Returns
        (tokens (B, S), logp (B, S), logp_u (B, S)): the log-probabilities of the tokens under the conditional and under the
        unconditional rows.  Refused before any kernel as well: guidance without uncond_embeddings (or without embeddings), a shape
        mismatch between the two, a guidance_scale that is negative or not finite."""
        guided = guidance_scale is not None and float(guidance_scale) != 1.0
        if guided:
            guidance_scale = float(guidance_scale)
            if not (np.isfinite(guidance_scale) and guidance_scale >= 0.0):
                raise ValueError("GPT.generate_masked: guidance_scale=%r must be finite and not negative" % (guidance_scale,))
            if embeddings is None or uncond_embeddings is None:
                raise ValueError("GPT.generate_masked: guidance_scale=%r needs embeddings and uncond_embeddings, the prefixes of the "
                                 "condition and of the null condition" % (guidance_scale,))
            if tuple(uncond_embeddings.shape) != tuple(embeddings.shape):
                raise ValueError("GPT.generate_masked: uncond_embeddings of shape %s, the shape of embeddings %s expected" % (
                    tuple(uncond_embeddings.shape), tuple(embeddings.shape)))
        if self.training:
            raise RuntimeError("GPT.generate_masked: inference only, the model is in training mode (call .eval())")
        t = self._new_tokens(idx, embeddings)
        if known.dim() != 2 or known.shape[0] != idx.shape[0] or known.shape[1] < 1 or known.dtype != torch.long:
            raise ValueError("GPT.generate_masked: known (B, S) torch.long with B = %d and S >= 1 expected, got %s of %s" % (
                idx.shape[0], tuple(known.shape), known.dtype))
        B, S = known.shape
        mask = np.asarray(resample)
        if mask.dtype != np.bool_ or mask.shape not in ((S,), (B, S)):
            raise ValueError("GPT.generate_masked: resample must be a host bool array of shape (S,) = (%d,) or (B, S) = (%d, %d), got %s of %s" % (
                S, B, S, mask.shape, mask.dtype))
        mask = np.broadcast_to(mask, (B, S)).copy()
        if t < 1 or t + S - 1 > self.block_size:
            raise RuntimeError("GPT.generate_masked: a prompt of %d tokens + %d positions - 1 exceeds block_size=%d" % (t, S, self.block_size))
        if not temperature > 0:
            raise ValueError("GPT.generate_masked: temperature=%r must be positive" % (temperature,))
        if top_p is not None and not 0 < top_p <= 1:
            raise ValueError("GPT.generate_masked: top_p=%r must lie in (0, 1]" % (top_p,))
        cols = np.flatnonzero(mask.any(axis=0))
        j0 = int(cols[0]) if cols.size else S
        if self.config.n_unmasked > t + j0:
            raise RuntimeError("GPT.generate_masked: n_unmasked=%d exceeds the %d tokens of the prefill (prompt %d + kept prefix %d); the "
                               "decode steps apply no mask" % (self.config.n_unmasked, t + j0, t, j0))
        if uniforms is not None and tuple(uniforms.shape) != (S - j0, B):
            raise ValueError("GPT.generate_masked: uniforms of shape %s, (S - j0, B) = (%d, %d) expected" % (tuple(uniforms.shape), S - j0, B))

        if guided:
            return self._generate_guided(idx, known, mask, j0, t, temperature, top_k, top_p, generator, uniforms, embeddings,
                                         uncond_embeddings, guidance_scale)
        n_pre = min(j0, S - 1)                         # known columns behind the prompt in the prefill
        cache = self.new_cache(B, capacity=t + S - 1)
        dev = cache.kv.device
        logits = self.prefill(torch.cat((idx, known[:, :n_pre]), dim=1), cache, embeddings)
        tokens = torch.empty(B, S, dtype=torch.long, device=dev)
        logp = torch.empty(B, S, dtype=torch.float32, device=dev)
        n_xe = n_pre if j0 < S else S                  # positions whose log-probability the prefill logits give
        if n_xe:
            tokens[:, :n_xe] = known[:, :n_xe]
            logp[:, :n_xe] = -ops.cross_entropy(logits[:, t - 1:t - 1 + n_xe], known[:, :n_xe], reduction="none")
        if j0 < S:
            if uniforms is not None:
                uniforms = uniforms.to(device=dev, dtype=torch.float32)
            forced = torch.where(torch.from_numpy(mask).to(dev), torch.full_like(known, -1), known).t().contiguous()      # (S, B)
            step_logits = logits[:, -1, :]
            for k in range(j0, S):
                u = uniforms[k - j0] if uniforms is not None else torch.rand(B, generator=generator, device=dev)
                new, lp = ops.sample_filtered(step_logits, u, forced[k], temperature, top_k, top_p)
                tokens[:, k], logp[:, k] = new, lp
                if k + 1 < S:
                    step_logits = self.decode_step(new, cache)
        return tokens, logp

    def _generate_guided(self, idx, known, mask, j0, t, temperature, top_k, top_p, generator, uniforms, embeddings, uncond_embeddings,
                         scale):
        """generate_masked's guided route behind its checks: the unguided body on 2B rows, ops.sample_guided in place of
        ops.sample_filtered."""
        B, S = known.shape
        n_pre = min(j0, S - 1)
        cache = self.new_cache(2 * B, capacity=t + S - 1)
        dev = cache.kv.device
        prompt = torch.cat((idx, known[:, :n_pre]), dim=1)
        logits = self.prefill(prompt.repeat(2, 1), cache, torch.cat((embeddings, uncond_embeddings), dim=0))      # (2B, T, V)
        tokens = torch.empty(B, S, dtype=torch.long, device=dev)
        logp = torch.empty(B, S, dtype=torch.float32, device=dev)
        logp_u = torch.empty(B, S, dtype=torch.float32, device=dev)
        n_xe = n_pre if j0 < S else S
        if n_xe:
            tokens[:, :n_xe] = known[:, :n_xe]
            lp = -ops.cross_entropy(logits[:, t - 1:t - 1 + n_xe], known[:, :n_xe].repeat(2, 1), reduction="none")
            logp[:, :n_xe], logp_u[:, :n_xe] = lp[:B], lp[B:]
        if j0 < S:
            if uniforms is not None:
                uniforms = uniforms.to(device=dev, dtype=torch.float32)
            forced = torch.where(torch.from_numpy(mask).to(dev), torch.full_like(known, -1), known).t().contiguous()      # (S, B)
            step_logits = logits[:, -1, :]
            for k in range(j0, S):
                u = uniforms[k - j0] if uniforms is not None else torch.rand(B, generator=generator, device=dev)
                new, lp, lpu = ops.sample_guided(step_logits, u, scale, forced[k], temperature, top_k, top_p)
                tokens[:, k], logp[:, k], logp_u[:, k] = new[:B], lp, lpu
                if k + 1 < S:
                    step_logits = self.decode_step(new, cache)
        return tokens, logp, logp_u


def unmask_schedule(k, n_steps, choice_temperature):
    """(gamma, tau) of iteration k of n_steps of MaskedGPT.generate_parallel: the share cos(pi/2 (k + 1) / n_steps) of the initially
    masked positions that stays masked behind it - exactly 0 at the last iteration - and the temperature choice_temperature (1 -
    (k + 1) / n_steps) of the Gumbel noise on the confidences."""
    r = (k + 1) / n_steps
    return (0.0 if k + 1 >= n_steps else math.cos(0.5 * math.pi * r)), float(choice_temperature) * (1.0 - r)


class MaskedGPT(GPT):
    """The bidirectional code prior: GPT's tree, parameter names and order, with tok_embed of vocab_size + 1 rows (row vocab_size is
    the mask token), a head of vocab_size outputs and n_unmasked = block_size.  No start token.  forward() is GPT's; seeded dropout
    works unchanged.  config.vocab_size stays the number of codes; mask_token = vocab_size."""

    def __init__(self, vocab_size, block_size, n_layer=12, n_head=8, n_embed=256, emb_pdrop=0.0, res_pdrop=0.0, att_pdrop=0.0):
        super().__init__(vocab_size, block_size, n_layer=n_layer, n_head=n_head, n_embed=n_embed, emb_pdrop=emb_pdrop,
                         res_pdrop=res_pdrop, att_pdrop=att_pdrop, n_unmasked=block_size)
        self.mask_token = int(vocab_size)
        self.tok_embed = nn.Embedding(vocab_size + 1, n_embed)          # takes tok_embed's place in the tree: the order stays GPT's
        self._init_weights(self.tok_embed)

    def _no_past(self, what):
        raise NotImplementedError("MaskedGPT.%s: a bidirectional model has no past - every position sees every position, so nothing "
                                  "can be cached; use forward() or generate_parallel()" % what)

    def new_cache(self, *args, **kwargs):
        self._no_past("new_cache")

    def prefill(self, *args, **kwargs):
        self._no_past("prefill")

    def decode_step(self, *args, **kwargs):
        self._no_past("decode_step")

    def generate(self, *args, **kwargs):
        self._no_past("generate")

    def generate_masked(self, *args, **kwargs):
        self._no_past("generate_masked")

    def sample(self, *args, **kwargs):
        self._no_past("sample")

    def forward_with_past(self, *args, **kwargs):
        self._no_past("forward_with_past")

    def forward_conditioned(self, idx, cond_tokens, cond_table, null_index=None, drop=None):
        """forward(idx) with one conditioning token per position ADDED to the embedding: GPT.forward's lines with ops.embedding_cond
        in place of ops.embedding.  cond_tokens (B, T) torch.long - the label token of every latent cell (LabelCondition.tokens) -
        cond_table (L, n_embed), the condition's own table.  drop = (p, seed, call) with null_index: whole samples read
        cond_table[null_index] (classifier-free guidance's training side, ops.embedding_cond).  The embedding dropout applies after
        the sum, at forward()'s site and under forward()'s call bookkeeping.  The sequence stays T long."""
        self._check_dropout()
        t = idx.shape[1]
        if t > self.block_size:
            raise RuntimeError("GPT: cannot forward T=%d tokens, the model's block_size=%d is exhausted" % (t, self.block_size))
        call = self._dropout_call()
        x = ops.embedding_cond(idx, self.tok_embed.weight, self.pos_embed, cond_tokens, cond_table, null_index, drop)
        if call is not None and self.drop.p > 0:
            x = ops.dropout(x, self.drop.p, self._key(call, self.dropout_site))
        for block in self.blocks:
            x = block._forward(x, None, call)[0]
        x = self._head(x)
        if call is not None:
            self.set_dropout_call(call + 1)
        return x

    @torch.no_grad()
    def pseudo_nll(self, ids, grid, stride=(2, 2), max_rows=64, cond=None):
        """What the model thinks of a slice code by code, as a map (B, h, w) fp32: ids (B, T) torch.long with T = h w of grid =
        (h, w).  The lattice of stride = (sy, sx), 1 <= sy <= h, 1 <= sx <= w, splits the grid into S = sy sx groups - position
        t = y w + x belongs to group g(t) = (y mod sy) sx + (x mod sx) - and pass s sees the slice with the mask token at every
        position of group s:
            map[b, t] = -log p(ids[b, t] | ids[b, u] for g(u) != g(t); the mask token where g(u) = g(t)),
        read off pass g(t).  stride (h, w): T passes of one masked position each, the exact pseudo-likelihood -log p(code | all
        the others); (2, 2), the default: four passes, every masked code sees its eight neighbours; (1, 1): one all-masked pass,
        the per-position marginal.  It is NOT a likelihood: the terms do not multiply to a probability of the slice, and their sum
        ranks nothing but positions of one slice under one stride (the training objective of the model, evaluated where it is
        asked).

        Eval mode, no gradients, no host read, no random numbers; the training flag is restored.  The passes of a sample run side
        by side as batch rows, ns = max(1, max_rows // B) passes per chunk: ops.lattice_inputs, the trunk in front of ln_f, and
        ops.lattice_gather_ln, which normalises into ONE y (B, T, E) only the rows the map reads.  After the last chunk ln_f is
        done, and the head and the cross-entropy run once over B T rows - the logits are (B, T, V) whatever S is.  cond = (tokens
        (B, T) torch.long, table, null_index): generate_parallel's triple; the stem is ops.embedding_cond under the tokens repeated
        per pass (null_index is not read: nothing is dropped).  Anything else raises ValueError naming the value."""
        try:
            h, w = (int(v) for v in grid)
        except (TypeError, ValueError):
            raise ValueError("MaskedGPT.pseudo_nll: grid=%r must be a pair (h, w)" % (grid,)) from None
        if not torch.is_tensor(ids) or ids.dim() != 2 or ids.dtype != torch.long or h < 1 or w < 1 or ids.shape[1] != h * w \
                or ids.shape[0] < 1 or h * w > self.block_size:
            raise ValueError("MaskedGPT.pseudo_nll: ids (B, T) torch.long with T = h w = %d x %d <= block_size=%d expected, got %s of %s" % (
                h, w, self.block_size, tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__, getattr(ids, "dtype", None)))
        try:
            sy, sx = (int(v) for v in stride)
            ok = all(float(v) == int(v) for v in stride)
        except (TypeError, ValueError):
            sy = sx = 0
            ok = False
        if not (ok and 1 <= sy <= h and 1 <= sx <= w):
            raise ValueError("MaskedGPT.pseudo_nll: stride=%r must be a pair (sy, sx) of integers in [1, h = %d] x [1, w = %d]" % (stride, h, w))
        if isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or max_rows < 1:
            raise ValueError("MaskedGPT.pseudo_nll: max_rows=%r must be an integer >= 1" % (max_rows,))
        B, T = ids.shape
        dev, E = self.head.weight.device, self.config.n_embed
        ctok = ctab = None
        if cond is not None:
            ctok, ctab, _ = cond
            if not torch.is_tensor(ctok) or ctok.dtype != torch.long or tuple(ctok.shape) != (B, T):
                raise ValueError("MaskedGPT.pseudo_nll: cond tokens (B, T) = (%d, %d) torch.long expected, got %s of %s" % (
                    B, T, tuple(ctok.shape) if torch.is_tensor(ctok) else type(ctok).__name__, getattr(ctok, "dtype", None)))
            ctok = ctok.to(dev).contiguous()
        S, per = sy * sx, max(1, int(max_rows) // B)
        ids = ids.to(dev).contiguous()
        was_training = self.training
        self.eval()
        try:
            y = torch.empty(B, T, E, dtype=torch.float32, device=dev)          # every row belongs to exactly one pass: all are written
            for s0 in range(0, S, per):
                ns = min(per, S - s0)
                inp = ops.lattice_inputs(ids, (h, w), (sy, sx), s0, ns, self.mask_token)
                if cond is None:
                    x = self._trunk(inp, None)[0]
                else:
                    x = ops.embedding_cond(inp, self.tok_embed.weight, self.pos_embed, ctok.repeat_interleave(ns, dim=0), ctab)
                    for block in self.blocks:
                        x = block._forward(x, None, None)[0]
                ops.lattice_gather_ln(x, self.ln_f.weight, self.ln_f.bias, y, (h, w), (sy, sx), s0, ns, self.ln_f.eps)
            nll = ops.cross_entropy(ops.linear(y, self.head.weight), ids, reduction="none")
        finally:
            self.train(was_training)
        return nll.reshape(B, h, w)

    @torch.no_grad()
    def generate_parallel(self, ids, masked, n_steps, temperature=1.0, top_k=None, top_p=None, choice_temperature=4.5, generator=None,
                          uniforms=None, cond=None, guidance_scale=None):
        """Fill in the masked positions of ids (B, T) torch.long in n_steps parallel passes, in eval mode: masked (B, T) torch.uint8 /
        bool on the device (what ids holds there is not read).  Iteration k: one forward of the current ids (the mask token at the
        masked positions), one ops.sample_filtered launch over the (B T, V) rows - forced to the code where it is known, a draw
        (temperature, top-k, top-p) where it is masked - and one ops.unmask_step launch with unmask_schedule(k, n_steps,
        choice_temperature): the floor(gamma m0) least confident draws are masked again, the others are fixed.  The last iteration
        fixes everything.  m0, the masked count at the start, is a device tensor: no host read inside the loop.

        Returns (ids (B, T), fixed_logp (B, T) fp32): a fixed position's log-probability (temperature 1, unfiltered) under the pass
        that fixed it, 0 at the positions that were known.  A sample with nothing masked comes back unchanged.  Without `uniforms`
        each iteration draws torch.rand(B T) for the sampler and then torch.rand(B, T) for the confidences from `generator`;
        uniforms (n_steps, 2, B, T) replaces them: index 0 feeds the sampler, index 1 the confidences.

        cond = (tokens (B, T) torch.long, table (L, n_embed), null_index or None): every pass is forward_conditioned under the label
        tokens in place of forward; nothing else changes.  With guidance_scale other than None or 1 (classifier-free guidance;
        needs null_index) a pass is ONE forward_conditioned over 2B rows - the rows [0, B) under the label tokens, the rows [B, 2B)
        under null_index at every position, both halves holding the current ids - ONE ops.sample_guided launch over the (2 B T, V)
        logits, which draws from z_u + scale (z_c - z_u), and ONE ops.unmask_step on the conditional log-probabilities: the
        confidence of a draw is its log-probability under the label.  The guided call returns (ids, fixed_logp, fixed_logp_u),
        fixed_logp_u the null rows' log-probability of a position in the pass that fixed it, 0 where it was known.  uniforms stays
        (n_steps, 2, B, T).  Without cond: the code path and the bits of the unconditional model; guidance without cond raises."""
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("MaskedGPT.generate_parallel: n_steps=%r must be at least 1" % (n_steps,))
        if ids.dim() != 2 or ids.dtype != torch.long or ids.shape[1] < 1 or ids.shape[1] > self.block_size:
            raise ValueError("MaskedGPT.generate_parallel: ids (B, T) torch.long with 1 <= T <= block_size=%d expected, got %s of %s" % (
                self.block_size, tuple(ids.shape), ids.dtype))
        B, T = ids.shape
        if tuple(masked.shape) != (B, T) or masked.dtype not in (torch.uint8, torch.bool):
            raise ValueError("MaskedGPT.generate_parallel: masked (B, T) = (%d, %d) torch.uint8 or torch.bool expected, got %s of %s" % (
                B, T, tuple(masked.shape), masked.dtype))
        if not temperature > 0:
            raise ValueError("MaskedGPT.generate_parallel: temperature=%r must be positive" % (temperature,))
        if top_p is not None and not 0 < top_p <= 1:
            raise ValueError("MaskedGPT.generate_parallel: top_p=%r must lie in (0, 1]" % (top_p,))
        if not (math.isfinite(float(choice_temperature)) and choice_temperature >= 0):
            raise ValueError("MaskedGPT.generate_parallel: choice_temperature=%r must be finite and not negative" % (choice_temperature,))
        if uniforms is not None and tuple(uniforms.shape) != (n_steps, 2, B, T):
            raise ValueError("MaskedGPT.generate_parallel: uniforms of shape %s, (n_steps, 2, B, T) = (%d, 2, %d, %d) expected" % (
                tuple(uniforms.shape), n_steps, B, T))
        guided = guidance_scale is not None and float(guidance_scale) != 1.0
        if guided:
            guidance_scale = float(guidance_scale)
            if not (math.isfinite(guidance_scale) and guidance_scale >= 0.0):
                raise ValueError("MaskedGPT.generate_parallel: guidance_scale=%r must be finite and not negative" % (guidance_scale,))
            if cond is None or cond[2] is None:
                raise ValueError("MaskedGPT.generate_parallel: guidance_scale=%r needs cond = (tokens, table, null_index) with a null "
                                 "index, the condition of the unconditional rows" % (guidance_scale,))
        dev, V = self.head.weight.device, self.config.vocab_size
        if cond is not None:
            ctok, ctab, null_index = cond
            if ctok.dtype != torch.long or tuple(ctok.shape) != (B, T):
                raise ValueError("MaskedGPT.generate_parallel: cond tokens (B, T) = (%d, %d) torch.long expected, got %s of %s" % (
                    B, T, tuple(ctok.shape), ctok.dtype))
            ctok = ctok.to(dev).contiguous()
            if guided:
                return self._generate_parallel_guided(ids, masked, n_steps, temperature, top_k, top_p, choice_temperature, generator, uniforms,
                                                      ctok, ctab, int(null_index), guidance_scale)
        was_training = self.training
        self.eval()
        try:
            if uniforms is not None:
                uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
            masked = masked.to(dev).contiguous().view(torch.uint8)
            m0 = masked.sum(1, dtype=torch.int32)
            cur = torch.where(masked != 0, torch.full_like(ids, self.mask_token), ids.to(dev))
            fixed_logp = torch.zeros(B, T, dtype=torch.float32, device=dev)
            for k in range(n_steps):
                gamma, tau = unmask_schedule(k, n_steps, choice_temperature)
                logits = self(cur) if cond is None else self.forward_conditioned(cur, ctok, ctab)
                if uniforms is not None:
                    u_draw, u_conf = uniforms[k, 0].reshape(-1), uniforms[k, 1]
                else:
                    u_draw = torch.rand(B * T, generator=generator, device=dev)
                    u_conf = torch.rand(B, T, generator=generator, device=dev)
                forced = torch.where(masked != 0, torch.full_like(cur, -1), cur).reshape(-1)
                tokens, logp = ops.sample_filtered(logits.reshape(B * T, V), u_draw, forced, temperature, top_k, top_p)
                cur, masked, fixed_logp = ops.unmask_step(tokens.view(B, T), logp.view(B, T), masked, m0, gamma, tau, self.mask_token,
                                                          u=u_conf, fixed_logp=fixed_logp)
        finally:
            self.train(was_training)
        return cur, fixed_logp

    def _generate_parallel_guided(self, ids, masked, n_steps, temperature, top_k, top_p, choice_temperature, generator, uniforms, ctok, ctab,
                                  null_index, scale):
        """generate_parallel's guided route behind its checks: the unguided body with the forward on 2B rows and ops.sample_guided in
        place of ops.sample_filtered."""
        B, T = ids.shape
        dev, V = self.head.weight.device, self.config.vocab_size
        was_training = self.training
        self.eval()
        try:
            if uniforms is not None:
                uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
            masked = masked.to(dev).contiguous().view(torch.uint8)
            m0 = masked.sum(1, dtype=torch.int32)
            cur = torch.where(masked != 0, torch.full_like(ids, self.mask_token), ids.to(dev))
            ctok2 = torch.cat((ctok, torch.full_like(ctok, null_index)), dim=0)          # the label's rows, then the null rows
            fixed_logp = torch.zeros(B, T, dtype=torch.float32, device=dev)
            fixed_logp_u = torch.zeros(B, T, dtype=torch.float32, device=dev)
            for k in range(n_steps):
                gamma, tau = unmask_schedule(k, n_steps, choice_temperature)
                logits = self.forward_conditioned(torch.cat((cur, cur), dim=0), ctok2, ctab)          # (2B, T, V)
                if uniforms is not None:
                    u_draw, u_conf = uniforms[k, 0].reshape(-1), uniforms[k, 1]
                else:
                    u_draw = torch.rand(B * T, generator=generator, device=dev)
                    u_conf = torch.rand(B, T, generator=generator, device=dev)
                forced = torch.where(masked != 0, torch.full_like(cur, -1), cur).reshape(-1)
                tokens, logp, logp_u = ops.sample_guided(logits.reshape(2 * B * T, V), u_draw, scale, forced, temperature, top_k, top_p)
                before = masked
                cur, masked, fixed_logp = ops.unmask_step(tokens[:B * T].view(B, T), logp.view(B, T), masked, m0, gamma, tau, self.mask_token,
                                                          u=u_conf, fixed_logp=fixed_logp)
                fixed_logp_u = torch.where((before != 0) & (masked == 0), logp_u.view(B, T), fixed_logp_u)      # fixed in this pass
        finally:
            self.train(was_training)
        return cur, fixed_logp, fixed_logp_u


def decode_pack_layout(n_layer, n_embed, vocab_size):
    """[(state_dict key or tuple of keys stacked along the rows, offset in floats, shape)] of the packed-weights buffer
    ops.gpt_decode_step reads - the layout documented in include/vqwnet_hip.h - and its size in floats."""
    E, layout, off = n_embed, [], 0

    def put(keys, shape):
        nonlocal off
        layout.append((keys, off, shape))
        off += shape[0] * (shape[1] if len(shape) > 1 else 1)

    for i in range(n_layer):
        b = "blocks.%d." % i
        put(b + "ln1.weight", (E,))
        put(b + "ln1.bias", (E,))
        put((b + "att.q.weight", b + "att.k.weight", b + "att.v.weight"), (3 * E, E))
        put((b + "att.q.bias", b + "att.k.bias", b + "att.v.bias"), (3 * E,))
        put(b + "att.proj.weight", (E, E))
        put(b + "att.proj.bias", (E,))
        put(b + "ln2.weight", (E,))
        put(b + "ln2.bias", (E,))
        put(b + "mlp.0.weight", (4 * E, E))
        put(b + "mlp.0.bias", (4 * E,))
        put(b + "mlp.2.weight", (E, 4 * E))
        put(b + "mlp.2.bias", (E,))
    put("ln_f.weight", (E,))
    put("ln_f.bias", (E,))
    put("head.weight", (vocab_size, E))
    return layout, off


@torch.no_grad()
def pack_decode_weights(model, out=None):
    """The model's weights in one contiguous buffer with decode_pack_layout's layout, by plain copy_ of the parameters; `out`: a
    buffer of the right size to refill (the parameters may have changed), else a new one on the model's device."""
    c = model.config
    layout, n = decode_pack_layout(c.n_layer, c.n_embed, c.vocab_size)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=model.head.weight.device)
    if out.numel() != n or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("pack_decode_weights: a contiguous fp32 buffer of %d floats expected, got %s of %s" % (n, tuple(out.shape), out.dtype))
    params, flat = dict(model.named_parameters()), out.view(-1)
    for keys, off, shape in layout:
        for key in ((keys,) if isinstance(keys, str) else keys):
            p = params[key]
            flat[off:off + p.numel()].view(p.shape).copy_(p)
            off += p.numel()
    return out


class KVCache:
    """What GPT.decode_step works on, built by GPT.new_cache:

        kv          (n_layer, 2, B, capacity, E) fp32: per layer a k-plane and a v-plane, the heads side by side in the last axis -
                    the (B, T, E) layout ops.causal_attention takes, so kv[l, 0] can be handed to it unchanged
        length      the rows [0, length) of every plane are valid (set by GPT.prefill, advanced by GPT.decode_step; setting it back
                    rewinds the sequence)
        capacity    rows of a plane
        batch_size  B
        packed      the model's weights as ops.gpt_decode_step reads them (pack_decode_weights): a snapshot taken at construction -
                    call pack(model) after the parameters changed
        ws          the step's activations workspace
    """

    def __init__(self, model, batch_size, capacity):
        c, dev = model.config, model.head.weight.device
        self.batch_size, self.capacity, self.length = batch_size, capacity, 0
        self.kv = torch.empty(c.n_layer, 2, batch_size, capacity, c.n_embed, dtype=torch.float32, device=dev)
        self.ws = torch.empty(ops.gpt_decode_ws_floats(batch_size, c.n_embed, c.vocab_size), dtype=torch.float32, device=dev)
        if ops.gpt_decode_pack_floats(c.n_layer, c.n_embed, c.vocab_size) != decode_pack_layout(c.n_layer, c.n_embed, c.vocab_size)[1]:
            raise RuntimeError("KVCache: the library's packed-weights size differs from decode_pack_layout's")
        self.packed = pack_decode_weights(model)

    def pack(self, model):
        """Refill the packed weights from the model's parameters."""
        pack_decode_weights(model, self.packed)
        return self
