"""The bidirectional masked prior's kernels (csrc/masked_prior.hip) restated in numpy integers and float64: the select as a lexsort
on (key, position), mask_tokens on dropout_ref.draws, unmask_step, and the two schedules.  Everything that decides a set is an
integer or a float64 expression of integers; nothing here is read by the code under test."""
import math

import numpy as np

import dropout_ref as D

MASK_RATIO_SITE = -2
MASK_KEY_SITE = -3
U_LO, U_HI = np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24)

# the (seed, call, B, T) cases of the GPU test of mask_tokens; tests/test_masked_prior_host.py asserts for every one of them that
# cos(pi/2 u_b) T lies farther than 1e-9 from every integer, so that a one-ulp difference between two double cosines moves no ceil
MASK_CASES = [(seed, call, 5, T) for T in (16, 256, 1000) for seed, call in ((3, 0), (3, 1), (2 ** 40 + 7, 12345))]


def float_keys(x):
    """The order-preserving unsigned image of fp32 bits: -0 < +0, the infinities order as numbers"""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select_lowest_keys(keys, n, eligible=None):
    """keys (B, T) unsigned integers -> (B, T) uint8: per row the min(max(n, 0), count) eligible entries of smallest (key, position)"""
    keys = np.asarray(keys)
    B, T = keys.shape
    eligible = np.ones((B, T), dtype=bool) if eligible is None else np.asarray(eligible) != 0
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (B,))
    out = np.zeros((B, T), dtype=np.uint8)
    pos = np.arange(T)
    for b in range(B):
        order = np.lexsort((pos, keys[b].astype(np.uint64)))          # the last key is the primary one
        order = order[eligible[b][order]]
        take = min(max(int(n[b]), 0), order.size)
        out[b, order[:take]] = 1
    return out


def select_lowest(keys, n, eligible=None):
    """ops.select_lowest: fp32 keys"""
    return select_lowest_keys(float_keys(keys), n, eligible)


def mask_ratio(seed, call, B):
    """cos(pi/2 u_b) in float64, u_b = the draw of element b under MASK_RATIO_SITE over 2^32"""
    u = D.draws(np.zeros(B, dtype=np.uint32), np.arange(B, dtype=np.uint32), seed, call, MASK_RATIO_SITE).astype(np.float64) / 4294967296.0
    return np.cos(1.5707963267948966 * u)


def masked_count(r, T):
    """clamp(ceil(r T), 1, T), the product in float64"""
    return np.clip(np.ceil(np.asarray(r, dtype=np.float64) * float(T)), 1, T).astype(np.int32)


def mask_tokens(ids, mask_token, seed, call, ratio=None):
    """-> (inp (B, T) int64, masked (B, T) uint8, n (B,) int32)"""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    n = masked_count(mask_ratio(seed, call, B) if ratio is None else np.full(B, float(ratio)), T)
    e = np.arange(B * T, dtype=np.uint64).reshape(B, T)
    keys = D.draws((e >> np.uint64(32)).astype(np.uint32), (e & np.uint64(0xFFFFFFFF)).astype(np.uint32), seed, call, MASK_KEY_SITE)
    masked = select_lowest_keys(np.asarray(keys, dtype=np.uint64), n)
    return np.where(masked != 0, np.int64(mask_token), ids), masked, n


def confidence(logp, u, tau):
    """float64: logp + tau g, g = -log(-log(clamp(u, 2^-24, 1 - 2^-24))), the clamp in fp32 as the kernel's; tau = 0: logp"""
    logp = np.asarray(logp, dtype=np.float32).astype(np.float64)
    if tau == 0:
        return logp
    uc = np.clip(np.asarray(u, dtype=np.float32), U_LO, U_HI).astype(np.float64)
    return logp + float(np.float32(tau)) * -np.log(-np.log(uc))


def n_keep(cur, m0, gamma):
    """0 if gamma <= 0 else max(0, min(cur - 1, floor(gamma m0))), the product in float64"""
    cur, m0 = np.asarray(cur, dtype=np.int64), np.asarray(m0, dtype=np.int64)
    if gamma <= 0:
        return np.zeros_like(cur)
    return np.maximum(0, np.minimum(cur - 1, np.floor(float(gamma) * m0.astype(np.float64)).astype(np.int64)))


def unmask_step(tokens, logp, masked, m0, gamma, mask_token, conf, fixed_logp=None):
    """One iteration from the confidences `conf` (B, T) fp32 - the device's own returned bits, so that no float comparison decides
    the kept set - -> (ids_out, masked_out, fixed_logp)"""
    tokens, masked = np.asarray(tokens, dtype=np.int64), np.asarray(masked) != 0
    logp = np.asarray(logp, dtype=np.float32)
    keep = select_lowest(conf, n_keep(masked.sum(1), m0, gamma), masked) != 0
    fixed = np.zeros(logp.shape, dtype=np.float32) if fixed_logp is None else np.array(fixed_logp, dtype=np.float32)
    newly = masked & ~keep
    fixed[newly] = logp[newly]
    return np.where(keep, np.int64(mask_token), tokens), keep.astype(np.uint8), fixed


def unmask_schedule(k, n_steps, choice_temperature):
    """(gamma, tau) of iteration k: cos(pi/2 (k + 1) / n_steps), exactly 0 at the last one; choice_temperature (1 - (k + 1) / n_steps)"""
    r = (k + 1) / n_steps
    return (0.0 if k + 1 >= n_steps else math.cos(0.5 * math.pi * r)), float(choice_temperature) * (1.0 - r)


def masked_counts_after(m0, n_steps):
    """[(B,) the masked count behind iteration k for k in range(n_steps)] of a decoding that starts with m0 masked positions"""
    cur, out = np.asarray(m0, dtype=np.int64), []
    for k in range(n_steps):
        cur = n_keep(cur, m0, unmask_schedule(k, n_steps, 0.0)[0])
        out.append(cur)
    return out
