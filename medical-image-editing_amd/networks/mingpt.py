"""The minGPT blocks on the MI355X HIP kernels: the building blocks of the code prior of the taming-transformers line.

Same classes, constructor signatures, attribute names, parameter-creation order and state_dict keys as the reference's
networks/mingpt.py (GPTConfig :15-24, GPT1Config :27-31, CausalSelfAttention :34-90, Block :93-119), the buffer `att.mask` of
shape (1, 1, block_size, block_size) included, so a seed gives the reference's initial values and a reference checkpoint loads
with strict=True.  The forward passes call hipops.ops: ops.layer_norm, ops.linear (the 1 x 1 convolution on the exact-fp32
matrix cores), ops.causal_attention (the heads stay side by side in the (B, T, E) projections; the T x T scores never reach
memory), ops.gelu and ops.add.

The attention kernel takes the mask as the integer n_unmasked (query i sees key j iff j <= (i < n_unmasked ? n_unmasked - 1 :
i)) and never reads the buffer.  n_unmasked comes from the config at construction and is re-derived from the buffer whenever a
state is loaded; a loaded mask that is no tril with an all-ones u x u corner raises - nothing is computed under another mask
than the stored one.

Dropout: the three nn.Dropout members exist (the trees match) and hold the probabilities; at p = 0 or in eval mode they are the
identity.  The masks are counter-based (csrc/dropout.h): whether an element is kept is a pure integer function of (seed, call,
site, element index), generated inside the kernels - ops.causal_attention's dropout on the probabilities, ops.add_dropout for the
two residual adds - and never stored.  So dropout is opt-in by seed: seed_dropout(seed, call=0) numbers the module's sites
(att_drop, att.res_drop, mlp[3] in module-tree order) and stores seed and call; every training forward uses (seed, call, site)
and then advances call by one, so a seed reproduces a run bit for bit and a resumed run needs nothing but the call it stopped
at (set_dropout_call).  A training forward with any p > 0 on a module that has NOT been seeded raises NotImplementedError before
any kernel runs - GPTConfig's class defaults of 0.1 included: an unseeded, irreproducible mask has no kernel here.

The model over these blocks, the reference's GPT class (mingpt.py:122-224), is networks/gpt.py (networks.GPT).
"""
import torch
import torch.nn as nn

from hipops import ops


class GPTConfig:
    emb_pdrop = 0.1
    res_pdrop = 0.1
    att_pdrop = 0.1

    def __init__(self, vocab_size, block_size, **kwargs):
        self.vocab_size = vocab_size
        self.block_size = block_size
        for k, v in kwargs.items():
            setattr(self, k, v)


class GPT1Config(GPTConfig):
    """The 12-layer, 12-head, 768-wide preset."""
    n_layer = 12
    n_head = 12
    n_embed = 768


def causal_mask(block_size, n_unmasked=0):
    """tril(ones(block_size, block_size)) with mask[:n_unmasked, :n_unmasked] = 1 (mingpt.py:53-56)."""
    mask = torch.tril(torch.ones(block_size, block_size))
    mask[:n_unmasked, :n_unmasked] = 1
    return mask


def n_unmasked_of(mask):
    """The n_unmasked of a (.., T, T) mask buffer: row 0 of causal_mask(T, u) holds max(u, 1) ones.  Raises ValueError when the mask
    is not causal_mask(T, u) for any u (u = 1 and u = 0 give the same mask; 0 is returned)."""
    m = mask.detach().reshape(mask.shape[-2], mask.shape[-1]).float().cpu()
    if m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError("attention mask of shape %s is not square" % (tuple(mask.shape),))
    u = int(m[0].sum().item())
    u = u if u > 1 else 0
    if not (0 <= u <= m.shape[0]) or not torch.equal(m, causal_mask(m.shape[0], u)):
        raise ValueError("attention mask is not tril with an all-ones n_unmasked x n_unmasked corner: the attention kernel "
                         "computes under no other mask")
    return u


def _no_dropout(module, drop, what):
    if module.training and drop.p > 0 and getattr(module, "dropout_seed", None) is None:
        raise NotImplementedError("%s: dropout with p = %g in training mode has no kernel; build the config with %s = 0.0 "
                                  "or call .eval(), or seed the dropout: seed_dropout(seed)" % (type(module).__name__, drop.p, what))


class SeededDropout:
    """The dropout state of a module: the seed (None: not seeded), the call counter and the number of the module's first site."""
    dropout_seed = None
    dropout_call = 0
    dropout_site = 0

    def seed_dropout(self, seed, call=0):
        """Seed every dropout site of this module's tree, numbered from 0 in module-tree order, and set the call counter."""
        self._seed_sites(int(seed), 0)
        self.set_dropout_call(call)
        return self

    def _seed_sites(self, seed, site):
        """-> the first site number behind this module's"""
        raise NotImplementedError

    def set_dropout_call(self, n):
        """The call the next training forward uses (a training forward advances it by one)."""
        for m in self.modules():
            if isinstance(m, SeededDropout):
                m.dropout_call = int(n)
        return self

    def _dropout_call(self):
        """The call of this forward, or None: eval mode or not seeded (then every p is 0, or _no_dropout has raised)"""
        return self.dropout_call if self.training and self.dropout_seed is not None else None

    def _key(self, call, site):
        return (self.dropout_seed, call, site)


class CausalSelfAttention(SeededDropout, nn.Module):

    def __init__(self, config):
        super().__init__()
        assert config.n_embed % config.n_head == 0

        # the three projections, created in the order k, q, v; every head lives in one E-wide output
        self.k = nn.Linear(config.n_embed, config.n_embed)
        self.q = nn.Linear(config.n_embed, config.n_embed)
        self.v = nn.Linear(config.n_embed, config.n_embed)

        # identity at p = 0 or in eval mode; in training mode they give the probabilities of the seeded kernels (seed_dropout)
        self.att_drop = nn.Dropout(config.att_pdrop)
        self.res_drop = nn.Dropout(config.res_pdrop)

        self.proj = nn.Linear(config.n_embed, config.n_embed)

        n_unmasked = getattr(config, "n_unmasked", 0)
        mask = causal_mask(config.block_size, n_unmasked)
        self.register_buffer("mask", mask.view(1, 1, config.block_size, config.block_size))
        self.n_head = config.n_head
        self.n_unmasked = n_unmasked_of(self.mask)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # validated BEFORE anything is copied: a mask the kernel cannot express raises with the module's buffer and n_unmasked
        # untouched, so whoever catches the error still computes under the mask that is stored
        loaded = state_dict.get(prefix + "mask")
        if torch.is_tensor(loaded) and loaded.dim() >= 2:
            n_unmasked_of(loaded)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        # the buffer now holds the validated mask, or - key missing or of another shape, which load_state_dict reports - the old one
        self.n_unmasked = n_unmasked_of(self.mask)

    def _check_dropout(self):
        _no_dropout(self, self.att_drop, "att_pdrop")
        _no_dropout(self, self.res_drop, "res_pdrop")

    def _seed_sites(self, seed, site):
        self.dropout_seed, self.dropout_site = seed, site          # att_drop: site, res_drop: site + 1
        return site + 2

    def forward(self, x, layer_past=None):
        """-> (res_drop(proj(attention)), present)"""
        self._check_dropout()
        call = self._dropout_call()
        y, present = self._attend(x, layer_past, call)
        if call is not None:
            if self.res_drop.p > 0:
                y = ops.dropout(y, self.res_drop.p, self._key(call, self.dropout_site + 1))
            self.dropout_call = call + 1
        return y, present

    def _attend(self, x, layer_past, call):
        """(proj(attention), present) in front of res_drop - a Block applies that inside its residual add; call: the dropout call
        of this forward or None"""
        B, T, C = x.size()
        if layer_past is None and T > self.mask.shape[-1]:
            raise RuntimeError("CausalSelfAttention: T=%d exceeds block_size=%d" % (T, self.mask.shape[-1]))
        nh, hs = self.n_head, C // self.n_head

        k = ops.linear(x, self.k.weight, self.k.bias)          # (B, T, C): head h in the columns [h hs, (h + 1) hs)
        q = ops.linear(x, self.q.weight, self.q.bias)
        v = ops.linear(x, self.v.weight, self.v.bias)

        present = torch.stack((k.view(B, T, nh, hs).transpose(1, 2), v.view(B, T, nh, hs).transpose(1, 2)))   # (2, B, nh, T, hs)

        drop = dict(dropout_p=self.att_drop.p, dropout_key=self._key(call, self.dropout_site)) if call is not None else {}
        if layer_past is not None:
            if drop and self.att_drop.p > 0:
                raise RuntimeError("CausalSelfAttention: the layer_past route is inference only, it has no dropout (call .eval())")
            past_k, past_v = layer_past                        # (B, nh, Tp, hs) each
            k = torch.cat((past_k.transpose(1, 2).reshape(B, -1, C), k), dim=1)
            v = torch.cat((past_v.transpose(1, 2).reshape(B, -1, C), v), dim=1)
            y = ops.causal_attention(q, k, v, nh, causal=False)          # no mask on this route (mingpt.py:79-80)
        else:
            # the mask's top-left T x T window: tril with a corner of min(n_unmasked, T)
            y = ops.causal_attention(q, k, v, nh, n_unmasked=min(self.n_unmasked, T), causal=True, **drop)

        y = ops.linear(y, self.proj.weight, self.proj.bias)
        return y, present


class Block(SeededDropout, nn.Module):
    """x + att(ln1(x)), then x + mlp(ln2(x))."""
    def __init__(self, config):
        super().__init__()
        self.ln1 = nn.LayerNorm(config.n_embed)
        self.ln2 = nn.LayerNorm(config.n_embed)
        self.att = CausalSelfAttention(config)
        self.mlp = nn.Sequential(
            nn.Linear(config.n_embed, 4 * config.n_embed),
            nn.GELU(),
            nn.Linear(4 * config.n_embed, config.n_embed),
            nn.Dropout(config.res_pdrop),
        )

    def _mlp(self, x):
        h = ops.linear(x, self.mlp[0].weight, self.mlp[0].bias)
        h = ops.gelu(h)
        return ops.linear(h, self.mlp[2].weight, self.mlp[2].bias)

    @staticmethod
    def _add(a, b):
        """a + b through ops.add, on the (B, C, T, 1) channels-last view of the two (B, T, C) tensors: the same memory."""
        return ops.add(a.transpose(1, 2).unsqueeze(-1), b.transpose(1, 2).unsqueeze(-1)).squeeze(-1).transpose(1, 2)

    def _seed_sites(self, seed, site):
        self.dropout_seed = seed
        self.dropout_site = self.att._seed_sites(seed, site)          # mlp[3]: the site behind the attention's two
        return self.dropout_site + 1

    def _add_drop(self, a, b, p, call, site):
        """a + dropout(b): one pass, as _add is"""
        if call is None or p == 0:
            return self._add(a, b)
        return ops.add_dropout(a, b, p, self._key(call, site))

    def forward(self, x, layer_past=None, return_present=False):
        if return_present:
            assert not self.training
        self.att._check_dropout()                       # before any kernel runs
        _no_dropout(self, self.mlp[3], "res_pdrop")
        call = self._dropout_call()
        out = self._forward(x, layer_past, call)
        if call is not None:
            self.set_dropout_call(call + 1)
        return out if layer_past is not None or return_present else out[0]

    def _forward(self, x, layer_past, call):
        """-> (x, present); call: the dropout call of this forward (the block's own or the model's) or None"""
        att, present = self.att._attend(ops.layer_norm(x, self.ln1.weight, self.ln1.bias, self.ln1.eps), layer_past, call)

        x = self._add_drop(x, att, self.att.res_drop.p, call, self.att.dropout_site + 1)
        x = self._add_drop(x, self._mlp(ops.layer_norm(x, self.ln2.weight, self.ln2.bias, self.ln2.eps)), self.mlp[3].p, call, self.dropout_site)
        return x, present

