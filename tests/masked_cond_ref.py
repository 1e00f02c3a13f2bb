"""The label-conditioned masked prior restated in Python integers and float64 (csrc/cond.hip vqw_embed_cond_fwd,
MaskedGPT.forward_conditioned, ConditionalMaskedPriorTrainer's step), written from the definitions, and the case tables of
tests/test_masked_cond_host.py and tests/test_gpu_masked_cond.py.  Nothing here is read by the code under test, and nothing of the
package under test is imported.

    drop        sample b is dropped at (seed, call) iff draw(b) < round-half-even(float32(p) 2^32), draw the counter-based mix of
                csrc/dropout.h for element b of the site COND_DROP_SITE = -1: restated below in Python integers on its own, and held
                against tests/dropout_ref.py by the host test
    embedding   e[b][t] = null_index if b is dropped else cidx[b][t]
                x[b][t] = (tok[idx[b][t]] + pos[t]) + ctab[e[b][t]]; a row whose idx or e is out of range is NaN
    gradients   gtok[v] = sum of gx over the rows with idx == v, gpos[t] = sum_b gx[b][t], gctab[l] = sum over the rows with e == l
    sum bound   a sum of n fp32 terms added one by one in a fixed order differs from the exact sum by at most (n - 1) u sum|terms|
                to first order in u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2): the a-priori allowance of
                every gradient element, with n the number of its terms.  n <= 1: the element is exact.
    model       forward_conditioned = the blocks, ln_f and the head of tests/gpt_ref.py behind the embedding above
    step        loss = sum(nll masked) / sum(n) under tests/masked_prior_ref.py's mask
"""
import numpy as np
import torch

import mingpt_ref as M

COND_DROP_SITE = -1
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
U = 2.0 ** -24          # the unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ the drop, in Python integers
def _sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _mix32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def draw(b, seed, call, site=COND_DROP_SITE):
    """The 32-bit draw of element b of `site` under (seed, call): csrc/dropout.h, one Python integer"""
    z = _sm64(_sm64(_sm64(int(seed) & M64) ^ (int(call) & M64)) ^ (int(site) & M64))
    k0, k1 = z & M32, z >> 32
    hi, lo = (int(b) >> 32) & M32, int(b) & M32
    r0 = _mix32(hi ^ k0)
    r1 = _mix32(r0 ^ k1)
    x = ((lo ^ r0) * 0x7feb352d) & M32
    x ^= x >> 15
    x = ((x ^ r1) * 0x846ca68b) & M32
    return x ^ (x >> 16)


def threshold(p):
    return int(round(float(np.float32(p)) * 4294967296.0))          # Python's round is round-half-even, as llrint


def dropped(B, p, seed, call):
    """bool (B,): sample b is dropped; p = 0 drops nobody whatever the key"""
    thr = threshold(p)
    return np.array([draw(b, seed, call) < thr for b in range(B)], dtype=bool)


# ------------------------------------------------------------------------------------------------ the embedding
def effective(cidx, null_index=None, drop=None):
    """cidx (B, T) long -> e (B, T) long"""
    if drop is None or drop[0] == 0:
        return cidx.clone()
    gone = torch.from_numpy(dropped(cidx.shape[0], *drop))
    return torch.where(gone[:, None], torch.full_like(cidx, int(null_index)), cidx)


def embedding_cond_ref(idx, tok, pos, cidx, ctab, null_index=None, drop=None):
    """-> (x (B, T, E) in the dtype of tok, e (B, T) long); pos (block_size, E) or (1, block_size, E)"""
    B, T = idx.shape
    V, L = tok.shape[0], ctab.shape[0]
    e = effective(cidx, null_index, drop)
    bad = (idx < 0) | (idx >= V) | (e < 0) | (e >= L)
    pos = pos.reshape(-1, pos.shape[-1])
    x = (tok[idx.clamp(0, V - 1)] + pos[:T]) + ctab[e.clamp(0, L - 1)]
    return torch.where(bad[..., None], torch.full_like(x, float("nan")), x), e


def embedding_cond_grads(idx, e, gx, V, L, block_size):
    """float64 (gtok (V, E), gpos (block_size, E), gctab (L, E)) and, for each, the sum of |terms| and the number of terms per row:
    what sum_bound needs.  Rows of idx / e out of range add nothing."""
    B, T, E = gx.shape
    g = gx.double()
    out = []
    for index, rows in ((idx, V), (None, block_size), (e, L)):
        val, mag, cnt = torch.zeros(rows, E, dtype=torch.float64), torch.zeros(rows, E, dtype=torch.float64), torch.zeros(rows, dtype=torch.long)
        if index is None:
            val[:T], mag[:T], cnt[:T] = g.sum(0), g.abs().sum(0), B
        else:
            ok = (index >= 0) & (index < rows)
            val.index_add_(0, index[ok], g[ok])
            mag.index_add_(0, index[ok], g[ok].abs())
            cnt.index_add_(0, index[ok], torch.ones_like(index[ok]))
        out.append((val, mag, cnt))
    return out


def sum_bound(mag, cnt):
    """The allowance of every element of a fixed-order fp32 sum: (n - 1) u sum|terms|, with the second-order term's factor
    1 / (1 - (n - 1) u); n <= 1: 0, the element is a copy."""
    n1 = (cnt.double() - 1).clamp(min=0)[:, None]
    return n1 * U / (1 - n1 * U) * mag


# (B, T, E, V, L, block_size): the issue's five shapes and one with block_size > T; block_size None = T
EMBED_CASES = [(1, 1, 4, 1, 1, None), (3, 15, 36, 7, 3, None), (2, 64, 256, 64, 4, None), (2, 257, 128, 1000, 256, None),
               (1, 3, 4096, 5, 2, None), (3, 15, 36, 7, 3, 20)]
EMBED_P = (0.0, 0.5)
# three (seed, call) pairs for cases of 2 or 3 samples at p = 0.5; the host test asserts that over them every such case has a dropped
# and a kept sample (at B = 1 the three pairs together drop it once and keep it once)
EMBED_KEYS = [(21, 3), (3, 2), (2 ** 40 + 7, 12345)]


def embed_inputs(B, T, E, V, L, block_size, seed=0):
    """(idx, tok, pos, cidx, ctab with L + 1 rows - the last the null row - gx).  Plain randn: both additions of the forward round,
    so the ORDER of the three summands shows in the bits (the host test asserts that the other orders give other bits on these very
    inputs).  The restatement adds in fp32 in the kernel's order, and an IEEE fp32 addition has one result: it stays bit-comparable."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + E + V + L + seed)
    bs = T if block_size is None else block_size
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return (torch.randint(0, V, (B, T), generator=g), r(V, E), r(1, bs, E), torch.randint(0, L, (B, T), generator=g), r(L + 1, E),
            torch.randn(B, T, E, generator=g))


def other_orders(idx, tok, pos, cidx, ctab):
    """The same sum in the orders and roundings the kernel must NOT use, in fp32: tok + (pos + ctab), (tok + ctab) + pos, and the
    float64 sum rounded once"""
    T = idx.shape[1]
    a, p, c = tok[idx], pos.reshape(-1, pos.shape[-1])[:T], ctab[cidx]
    return a + (p + c), (a + c) + p, (a.double() + p.double() + c.double()).float()


# ------------------------------------------------------------------------------------------------ the model and the step
# 2 layers, 2 heads, V = 16, T = 16, B = 2.  E = 64: the attention kernels take head sizes that are multiples of 32 (vqw_causal_attention_fwd
# refuses hs = 16), so 64 is the smallest width with two heads - the width of tests/test_gpu_masked_prior.py's tiny model
TINY = dict(vocab_size=16, block_size=16, n_layer=2, n_head=2, n_embed=64)
N_LABELS = 4
B_TINY = 2


def forward_conditioned_ref(idx, ctok, st, table, n_layer, n_head):
    """MaskedGPT.forward_conditioned from the model's state dict and the condition's table, in their dtype -> logits (B, T, V)"""
    x = embedding_cond_ref(idx, st["tok_embed.weight"], st["pos_embed"], ctok, table)[0]
    for i in range(n_layer):
        x = M.block_ref(x, st, "blocks.%d." % i, n_head, None)[0]
    x = M.layer_norm_ref(x, st["ln_f.weight"], st["ln_f.bias"])
    return torch.matmul(x, st["head.weight"].t())


def masked_mean(logits, ids, masked, n):
    """float64: sum(nll masked) / sum(n)"""
    z = logits.double()
    nll = torch.logsumexp(z, -1) - z.gather(-1, ids[..., None])[..., 0]
    return float((nll * torch.as_tensor(masked != 0)).sum() / int(np.asarray(n).sum()))


# the learning check: the codes are a function of the label tokens, code = token (V >= L): under the label a masked code is known,
# under the null condition it is one of L
LEARN_STEPS = 60          # chosen on the GPU (at most 200 allowed); DESIGN records the losses behind it
LEARN_LR = 1e-2


def learn_batch(B=8, T=16, L=N_LABELS, seed=7):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, L, (B, T), generator=g)
    return tokens.clone(), tokens          # (ids, cond tokens)
