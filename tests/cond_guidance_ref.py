"""Restatement of what classifier-free guidance adds to the conditional code prior (csrc/gpt_head.hip k_sample's guided logits
source, csrc/cond.hip vqw_embed_lookup_drop, GPT.generate_masked's guided route, ConditionalPriorTrainer's p_uncond), written from
the definitions, and the case tables of tests/test_cond_guidance_host.py and tests/test_gpu_cond_guidance.py.

    the mix       z = fmaf(scale, z_c - z_u, z_u) in fp32: d = float32(z_c - z_u), then scale d + z_u rounded ONCE.  In numpy: the
                  product float64(scale) float64(d) is exact (24 x 24 bits), the double sum rounds once to 53 bits and float32()
                  rounds again; the two roundings differ from the single one only where the double sum is inexact (TwoSum error
                  not 0) AND lands on a float32 rounding tie: mix_ref flags those elements and the host test asserts that no
                  seeded input used on the device has one.
    the drop      sample b of a step is dropped iff the draw of tests/dropout_ref.py for element b under (seed, call, site -1) is
                  below round(p 2^32); a dropped sample reads the null row of the table in all its rows
    guided run    per position two full forwards (the label's prefix, the null prefix), the mix in float64, the filter and the draw
                  of tests/prior_edit_ref.py on the mixed logits, the same uniforms
"""
import numpy as np
import torch

import cond_prior_ref as C
import dropout_ref as DR
import gpt_ref as G
import prior_edit_ref as R
from prior_ref import adamw_ref_, clip_ref, decays, tokens_ref

COND_DROP_SITE = -1          # csrc/cond.hip
NULL = C.L                   # the null row of the tiny model's table (C.L + 1 rows)


# ------------------------------------------------------------------------------------------------ the mix
def mix_ref(zc, zu, scale):
    """zc, zu float32 arrays, scale a float32-representable number -> (z float32, flagged bool): flagged marks the elements where
    float32(the double sum) may differ from the fused multiply-add's single rounding."""
    zc, zu = np.asarray(zc, dtype=np.float32), np.asarray(zu, dtype=np.float32)
    s = np.float64(np.float32(scale))
    assert float(s) == float(scale), "the scale must be a float32 number"
    d = (zc - zu).astype(np.float32)
    a, b = s * d.astype(np.float64), zu.astype(np.float64)          # the product is exact in double
    t = a + b
    bb = t - a
    err = (a - (t - bb)) + (b - bb)                                 # TwoSum: a + b = t + err exactly
    z = t.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        z64 = z.astype(np.float64)
        other = np.nextafter(z, np.where(t > z64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
        tie = (z64 != t) & ((t - z64) == (other - t))               # t exactly midway between two neighbouring float32
    return z, (err != 0) & tie


# ---- sample_guided cases: the smallest sizes at which each pass can go wrong - one entry, fewer than a wave, one short of / exactly /
# one more than the 256 threads of the workgroup (chunks of 1 and 2), a chunked row that is no multiple of 256, the default vocabulary
GUIDED_V = (1, 7, 255, 256, 257, 1000, 1024)
GUIDED_B = (1, 3)
GUIDED_SCALES = (0.0, 0.5, 1.5, 3.0, 7.5)
GUIDED_TOP_P = (1.0, 0.9, 0.3)
GUIDED_TEMPS = (1.0, 0.7)


def guided_top_ks(V):
    return sorted({0, 1, min(5, V), V})


def guided_inputs(V, B, seed=0):
    """(zc, zu (B, V) fp32, u (B,) fp32): randn logits, the unconditional row the conditional one plus a smaller randn"""
    g = torch.Generator().manual_seed(7000 + 31 * V + B + 1000003 * seed)
    zu = 2.0 * torch.randn(B, V, generator=g)
    zc = zu + torch.randn(B, V, generator=g)
    return zc, zu, torch.rand(B, generator=g)


def guided_forced(B, V):
    """forced (B,) mixing a draw (-1), a valid token and an entry >= V (NaN log-probabilities) where B allows it"""
    return torch.tensor([-1, V - 1, V + 2][:B] if B > 1 else [-1], dtype=torch.long)


# The tie case.  Logits on the grid of multiples of 2^-10 within +-16 and a dyadic scale: z_c - z_u, the product and the sum are all
# exact (|z| <= 16 + 4 * 32 needs 8 bits in front of the 12 behind the point), so the mixed values are known exactly and DIFFERENT
# (z_c, z_u) pairs can be built to mix to EQUAL values.  Row layout (V = 12, scale 2): mixed values 5 (once), 3 (three times, from
# three different pairs), 1 (twice, two pairs), then -4 and below.  top_k = 2 puts the k-th largest on the 3s: all three stay or
# none (kept set {5, 3, 3, 3}); top_p: with kept masses e^0, 3 e^-2, 2 e^-4, ... the nucleus threshold can be put between the 3s and
# the 1s or inside neither group - the tied entries share one fate.
TIE_SCALE = 2.0
TIE_MIXED = [3.0, 5.0, -4.0, 3.0, 1.0, -6.0, 3.0, 1.0, -8.0, -4.5, -7.25, -9.0]


def tie_inputs():
    """(zc, zu (2, 12) fp32, mixed (2, 12) float64): row 1 is row 0 with other pairs behind the same mixed values"""
    mixed = np.array([TIE_MIXED, TIE_MIXED[::-1]], dtype=np.float64)
    rng = np.random.RandomState(5)
    zu = rng.randint(-2048, 2049, size=mixed.shape) / 512.0           # multiples of 2^-9 in [-4, 4]
    zc = zu + (mixed - zu) / TIE_SCALE                                # multiples of 2^-10: every operation of the mix is exact
    assert np.all(np.abs(zc) <= 16) and np.array_equal(zc.astype(np.float32).astype(np.float64), zc)
    return torch.from_numpy(zc.astype(np.float32)), torch.from_numpy(zu.astype(np.float32)), mixed


# ------------------------------------------------------------------------------------------------ the drop
def dropped_ref(B, p, seed, call):
    """bool (B,): sample b is dropped at (seed, call)"""
    return ~DR.keep_mask(B, p, seed, call, COND_DROP_SITE)


def lookup_drop_ref(idx, table, null_index, p, seed, call):
    """idx (B, T) long, table (L, E) -> (out (B, T, E), eff (B, T) long)"""
    drop = torch.from_numpy(dropped_ref(idx.shape[0], p, seed, call))
    eff = torch.where(drop[:, None], torch.full_like(idx, null_index), idx)
    return table[eff], eff


LOOKUP_CASES = [(5, 6, 32, 3), (1, 1, 4, 1), (64, 16, 8, 256)]          # (B, Tc, E, L): the table has L + 1 rows, the last the null row
LOOKUP_PS = (0.0, 0.5)
LOOKUP_KEY = (1234, 7)                                                   # (seed, call)


def lookup_inputs(B, Tc, E, L):
    g = torch.Generator().manual_seed(100 * B + Tc + E + L)
    return torch.randint(0, L, (B, Tc), generator=g), torch.randn(L + 1, E, generator=g), torch.randn(B, Tc, E, generator=g)


# ------------------------------------------------------------------------------------------------ the tiny model with a null row
def state(seed=C.SEED):
    """cond_prior_ref's initial state with a table of C.L + 1 rows (the caller adds the GPT's keys)"""
    return C.init_table_(torch.empty(C.L + 1, C.E), seed)


DROP_SEED, P_UNCOND = 6, 0.5


def steps_drop_ref(state, ids, cond, dtype, p_uncond=P_UNCOND, drop_seed=DROP_SEED, steps=C.STEPS, variant="threads8", optim=C.OPTIM,
                   max_norm=C.STEP_CLIP):
    """cond_prior_ref.steps_ref at pkeep 1 with the condition of step n (0-based) dropped per sample by dropped_ref(B, p, seed, n):
    a dropped sample's prefix is the null row.  -> steps_ref's dict plus dropped [steps][B]."""
    st = C.state_as(state, dtype, grad=True)
    rev = variant == "batch_reversed"
    flip = (lambda t: t.flip(0)) if rev else (lambda t: t)
    keys = [k for k in st if not k.endswith("mask")]
    mom = {k: (torch.zeros_like(st[k]), torch.zeros_like(st[k])) for k in keys}
    out = dict(loss=[], norm=[], coef=[], dropped=[])
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        for t in range(1, steps + 1):
            for k in keys:
                st[k].grad = None
            drop = torch.from_numpy(dropped_ref(ids.shape[0], p_uncond, drop_seed, t - 1))
            eff = torch.where(drop[:, None], torch.full_like(cond, NULL), cond)
            inp = tokens_ref(flip(ids), C.SOS, 1.0, C.V)
            loss = G.xent_ref(C.cond_logits(st, inp, flip(eff)), flip(ids))[0].mean()
            loss.backward()
            grads = {k: st[k].grad for k in keys}
            norm, coef = clip_ref([grads[k] for k in keys], max_norm)
            if t == 1:
                out["g0"] = {k: grads[k].detach().clone() for k in keys}
            with torch.no_grad():
                for k in keys:
                    adamw_ref_(st[k], grads[k] * coef, mom[k][0], mom[k][1], t, optim["lr"], optim["betas"], optim["eps"],
                               optim["weight_decay"] if k != C.TABLE and decays(k) else 0.0)
            for key, val in (("loss", loss), ("norm", norm), ("coef", coef)):
                out[key].append(float(val.detach()))
            out["dropped"].append(drop.tolist())
    finally:
        torch.set_num_threads(n)
    out["P"] = {k: st[k].detach().clone() for k in keys}
    return out


# ---- generate_masked with guidance against the float64 run.  Top-k only (the nucleus is the kernel-level tests' ground): the two
# margins are gpt_decode_ref's.  GEN_SEED: the seed of the uniforms (T, GEN_B), chosen on the CPU from the float64 run alone so that
# it clears GEN_MIN_DIST and GEN_MIN_GAP at GEN_SCALE in both cases below (the test recomputes and asserts both).
GEN_SCALE, GEN_TOPK, GEN_TEMP, GEN_B = 3.0, 4, 1.0, 2
GEN_SEED = 0
GEN_J0 = 4          # the second case keeps the first GEN_J0 columns of every row and, behind them, a per-row mask


def gen_mask(kind):
    """The host resample mask (GEN_B, T) of a case: 'all', or 'kept' - a kept prefix of GEN_J0 columns, then per-row choices"""
    if kind == "all":
        return np.ones((GEN_B, C.T), dtype=bool)
    m = np.random.RandomState(3).rand(GEN_B, C.T) < 0.6
    m[:, :GEN_J0] = False
    m[0, GEN_J0] = True          # column GEN_J0 is the first resampled one, in row 0 only
    m[1, GEN_J0] = False
    return m


def guided_truth(st64, cond, known, mask, uniforms, scale=GEN_SCALE):
    """The float64 run: known (B, T), mask (B, T) host bool, uniforms (T - j0, B) fp32 -> (tokens (B, T), smallest draw distance,
    smallest gap between the k-th and (k + 1)-th mixed logit) over the resampled positions."""
    Bc = cond.shape[0]
    null = torch.full_like(cond, NULL)
    seq = torch.full((Bc, 1), C.SOS, dtype=torch.long)
    cols = np.flatnonzero(mask.any(axis=0))
    j0 = int(cols[0]) if cols.size else C.T
    min_dist, min_gap = float("inf"), float("inf")
    with torch.no_grad():
        for k in range(C.T):
            if k < j0:
                pick = known[:, k]
            else:
                zc = C.cond_logits(st64, seq, cond, n_tail=1)[:, 0]
                zu = C.cond_logits(st64, seq, null, n_tail=1)[:, 0]
                z = zu + scale * (zc - zu)
                kept, _ = R.filter_ref(z, GEN_TEMP, GEN_TOPK, 1.0)
                draw, dist = R.draw_ref(z, kept, uniforms[k - j0], GEN_TEMP)
                row = torch.from_numpy(mask[:, k])
                pick = torch.where(row, draw, known[:, k])
                top = torch.topk(z / GEN_TEMP, GEN_TOPK + 1, dim=-1).values
                if bool(row.any()):
                    min_dist = min(min_dist, float(dist[row].min()))
                    min_gap = min(min_gap, float((top[:, GEN_TOPK - 1] - top[:, GEN_TOPK])[row].min()))
            seq = torch.cat((seq, pick[:, None]), dim=1)
    return seq[:, 1:], min_dist, min_gap


# ---- guidance sharpens the condition: the restatement trained with p_uncond = 0.5 on cond_prior_ref.learn_batch
def learn_drop_ref(state, dtype=torch.float64):
    ids, cond = C.learn_batch()
    optim = dict(C.OPTIM, lr=C.LEARN_LR)
    ref = steps_drop_ref(state, ids, cond, dtype, steps=C.LEARN_STEPS, optim=optim)
    return dict(ref["P"], **{k: v for k, v in state.items() if k.endswith("mask")})


def first_code_logp(st, cond, scale):
    """log p_scale(the label-consistent first code) for learn_batch's two sequences: log_softmax of the mixed first-position logits"""
    ids, _ = C.learn_batch()
    seq = torch.full((2, 1), C.SOS, dtype=torch.long)
    with torch.no_grad():
        zc = C.cond_logits(st, seq, cond, n_tail=1)[:, 0]
        zu = C.cond_logits(st, seq, torch.full_like(cond, NULL), n_tail=1)[:, 0]
        z = zu + scale * (zc - zu)
        return torch.log_softmax(z.double(), dim=-1).gather(-1, ids[:, :1])[:, 0]
