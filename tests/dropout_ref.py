"""Host restatement of the counter-based dropout of csrc/dropout.h - the keep mask in numpy, integer arithmetic only, bit for bit
what the kernels generate - and of the modules with dropout (mingpt.py:83, :88, :104, :189) in plain torch with the masks given.

    key        z = sm(sm(sm(seed) ^ call) ^ site) on 64 bits, sm = splitmix64's step; k0 = low word, k1 = high word
    row        r0 = mix(hi ^ k0), r1 = mix(r0 ^ k1), mix = the 32-bit multiply-xorshift finaliser 16 / 0x7feb352d / 15 / 0x846ca68b / 16
    draw       x = (lo ^ r0) 0x7feb352d; x ^= x >> 15; x = (x ^ r1) 0x846ca68b; r = x ^ x >> 16
    keep       r >= round(p 2^32), p the float32 probability; scale = float32(1 / (1 - p)) from the float32 p in double
    index      element-wise: the linear index, hi = index >> 32, lo = its low word; attention: hi = (b n_head + h) Tq + i, lo = j
"""
import math

import numpy as np
import torch

import mingpt_ref as M

M64 = (1 << 64) - 1
U32 = np.uint32


def _sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key_words(seed, call, site):
    """(k0, k1) of (seed, call, site): Python integers, two's complement on 64 bits"""
    z = _sm64(_sm64(_sm64(int(seed) & M64) ^ (int(call) & M64)) ^ (int(site) & M64))
    return z & 0xFFFFFFFF, z >> 32


def threshold(p):
    return int(round(float(np.float32(p)) * 4294967296.0))          # round-half-even, as llrint


def scale(p):
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def _mix(x):
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def draws(hi, lo, seed, call, site):
    """The 32-bit draw of every (hi, lo) pair (uint32 arrays that broadcast)"""
    k0, k1 = key_words(seed, call, site)
    hi, lo = np.asarray(hi, dtype=U32), np.asarray(lo, dtype=U32)
    r0 = _mix(hi ^ U32(k0))
    r1 = _mix(r0 ^ U32(k1))
    x = (lo ^ r0) * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = (x ^ r1) * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def keep_mask(n, p, seed, call, site, start=0):
    """bool (n,): element start + e of an element-wise site is kept"""
    idx = np.arange(start, start + n, dtype=np.uint64)
    return draws((idx >> np.uint64(32)).astype(U32), (idx & np.uint64(0xFFFFFFFF)).astype(U32), seed, call, site) >= np.uint64(threshold(p))


def attention_keep_mask(B, nh, Tq, Tk, p, seed, call, site):
    """bool (B, nh, Tq, Tk): probability (b, h, i, j) is kept"""
    hi = (np.arange(B * nh, dtype=np.uint64)[:, None] * np.uint64(Tq) + np.arange(Tq, dtype=np.uint64)[None, :]).astype(U32)
    r = draws(hi[:, :, None], np.arange(Tk, dtype=U32)[None, None, :], seed, call, site)
    return (r >= np.uint64(threshold(p))).reshape(B, nh, Tq, Tk)


# ------------------------------------------------------------------------------------------------ the modules, masks given
def _m(mask, like):
    return torch.as_tensor(np.asarray(mask)).to(like.dtype)


def drop_ref(x, mask, p):
    """x * mask / (1 - p) in x's dtype; mask None: x"""
    return x if mask is None else x * _m(mask, x).reshape(x.shape) / (1.0 - float(np.float32(p)))


def causal_attention_drop_ref(q, k, v, nh, nu, mask, p):
    """mingpt_ref.causal_attention_ref's softmax, then probabilities * mask / (1 - p), then . v (mingpt.py:83); mask (B, nh, T, T)
    or None -> (o (B, T, E), lse (B, nh, T))"""
    B, T, E = q.shape
    hs = E // nh
    qh, kh, vh = (t.reshape(B, T, nh, hs).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-2, -1)) * (1.0 / math.sqrt(hs))
    s = s.masked_fill(~M.visible(T, T, nu, True)[None, None], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    o = torch.matmul(drop_ref(torch.exp(s - lse[..., None]), mask, p), vh)
    return o.transpose(1, 2).reshape(B, T, E), lse


def block_drop_ref(x, st, pre, nh, nu, masks, p_att, p_res):
    """Block.forward in training mode from its state dict; masks = (att_drop (B, nh, T, T), att.res_drop (B T E), mlp[3] (B T E))"""
    h = M.layer_norm_ref(x, st[pre + "ln1.weight"], st[pre + "ln1.bias"])
    k, q, v = (M.linear_ref(h, st, pre + "att." + n + ".") for n in "kqv")
    o, _ = causal_attention_drop_ref(q, k, v, nh, nu, masks[0], p_att)
    x = x + drop_ref(M.linear_ref(o, st, pre + "att.proj."), masks[1], p_res)
    h = M.layer_norm_ref(x, st[pre + "ln2.weight"], st[pre + "ln2.bias"])
    h = M.linear_ref(M.gelu_ref(M.linear_ref(h, st, pre + "mlp.0.")), st, pre + "mlp.2.")
    return x + drop_ref(h, masks[2], p_res)


def gpt_drop_ref(idx, st, n_layer, nh, nu, masks, p_emb, p_att, p_res):
    """GPT.forward in training mode from its state dict -> logits; masks[0] the embedding's, then three per block"""
    T = idx.shape[1]
    x = drop_ref(st["tok_embed.weight"][idx] + st["pos_embed"][:, :T], masks[0], p_emb)
    for i in range(n_layer):
        x = block_drop_ref(x, st, "blocks.%d." % i, nh, nu, masks[1 + 3 * i:4 + 3 * i], p_att, p_res)
    x = M.layer_norm_ref(x, st["ln_f.weight"], st["ln_f.bias"])
    return torch.matmul(x, st["head.weight"].t())


def module_masks(B, T, E, nh, n_layer, p_emb, p_att, p_res, seed, call, with_emb=True):
    """The masks of one training forward of a seeded GPT (with_emb) or Block in site order: site 0 `drop`, then per block att_drop,
    att.res_drop, mlp[3].  A stand-alone Block numbers its own three sites 0, 1, 2.  A site with p = 0 gets None."""
    masks, site = [], 0
    if with_emb:
        masks.append(keep_mask(B * T * E, p_emb, seed, call, 0) if p_emb > 0 else None)
        site = 1
    for _ in range(n_layer):
        masks.append(attention_keep_mask(B, nh, T, T, p_att, seed, call, site) if p_att > 0 else None)
        masks.append(keep_mask(B * T * E, p_res, seed, call, site + 1) if p_res > 0 else None)
        masks.append(keep_mask(B * T * E, p_res, seed, call, site + 2) if p_res > 0 else None)
        site += 3
    return masks
