"""The GPT model of the code prior on the MI355X HIP kernels: the reference's GPT class (networks/mingpt.py:122-224) over the blocks of
networks/mingpt.py.  It lives in a module of its own; `networks.GPT` is the public name, as in the reference's networks/__init__.py.

Same constructor signature, attribute names, submodule and parameter creation order and state_dict keys as the reference's class, so
a seed gives the reference's initial values and a reference checkpoint loads with strict=True.  forward() is ops.embedding (token +
position embedding, with the reference's optional `embeddings=` prefix), the blocks, ops.layer_norm and ops.linear without bias; the
loss of the prior is ops.cross_entropy, a token is drawn by ops.sample_topk.

Dropout: `drop` exists (the trees match); at p = 0 or in eval mode it is the identity.  A training forward with emb_pdrop,
res_pdrop or att_pdrop above 0 raises NotImplementedError before any kernel runs; there is no dropout kernel.

GPT.forward_with_past.  The reference's body cannot run (`present.append(present)`, mingpt.py:219); what it evidently means is
built: `presents.append(present)`, returning (logits, torch.stack(presents)) of shape (n_layer, 2, B, n_head, T, hs).  With a
past the reference adds pos_embed[:, past_length, :] - ONE position - to every new token, which is only right for one token:
anything but exactly one new token (idx and `embeddings` rows together) behind a past raises ValueError, and past_length + 1 >
block_size raises RuntimeError.  The cached route concatenates the past per step, as the reference does; it applies no mask
(mingpt.py:79-80), so with n_unmasked > 0 it equals the full forward only when the first call carries at least n_unmasked tokens.
"""
import torch
import torch.nn as nn

from hipops import ops

from .mingpt import Block, GPTConfig, _no_dropout


class GPT(nn.Module):
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
        self.drop = nn.Dropout(emb_pdrop)          # identity at p = 0 or in eval mode; anything else raises in forward
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
        x = ops.embedding(idx, self.tok_embed.weight, self.pos_embed, embeddings)          # token (or given) + position embedding
        for block in self.blocks:
            x = block(x)
        return self._head(x)

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
