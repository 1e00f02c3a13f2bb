"""Restatement of the anomaly-detection operators (csrc/detect.hip) in plain torch / numpy, in the dtype asked for (float64 for
the truth, float32 for the gate's other side): the map through F.interpolate and a replicate-padded conv2d, the quantiser, and
AUROC / average precision / best Dice by SORTING the quantised keys into explicit tie groups - no histogram anywhere, so the
metrics do not share the kernels' method.  `scores_exact` is the same definition in Python integers and fractions."""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F


def taps_ref(sigma, dtype=torch.float64):
    """K = 2 ceil(3 sigma) + 1 taps exp(-d^2 / 2 sigma^2), normalised in double, rounded to fp32 (what the kernel is handed), as
    `dtype`.  sigma = 0: [1]."""
    if sigma == 0:
        return torch.ones(1, dtype=dtype)
    R = int(math.ceil(3.0 * sigma))
    d = torch.arange(-R, R + 1, dtype=torch.float64)
    t = torch.exp(-d * d / (2.0 * sigma * sigma))
    return (t / t.sum()).float().to(dtype)


def anomaly_map_ref(a, b, cellmask, sigma, dtype=torch.float64):
    """a, b (N, C, H, W); cellmask (N, h, w) uint8 or None -> (N, H, W) in `dtype`."""
    a, b = a.to(dtype), b.to(dtype)
    r = (a - b).abs().mean(dim=1, keepdim=True)
    if cellmask is not None:
        m = (cellmask != 0).to(dtype)[:, None]
        r = r * F.interpolate(m, size=r.shape[-2:], mode="bilinear", align_corners=False)
    t = taps_ref(sigma, dtype).to(a.device)
    R = (t.numel() - 1) // 2
    if R:
        r = F.conv2d(F.pad(r, (R, R, 0, 0), mode="replicate"), t.reshape(1, 1, 1, -1))
        r = F.conv2d(F.pad(r, (0, 0, R, R), mode="replicate"), t.reshape(1, 1, -1, 1))
    return r[:, 0]


def keys_ref(scores):
    """fp32 scores (numpy) -> int64 keys: bits >> 15 of a finite score >= 0, -0 as 0, and -1 for a NaN, an infinity or a negative
    score (not binned)."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    bits = s.view(np.uint32).astype(np.int64)
    bits = np.where(bits == 0x80000000, 0, bits)
    return np.where(bits >= 0x7F800000, -1, bits >> 15)


def key_floor(key):
    """The float whose bits are key << 15: the lower edge of a bin."""
    return float(np.array([int(key) << 15], dtype=np.uint32).view(np.float32)[0])


def scores_sorted(keys, labels):
    """[auroc, ap, best_dice, best_threshold, P, N] in float64 from the keys (>= 0 only) and labels of the pixels, by a stable
    argsort and one walk over the groups of equal keys in descending order."""
    keys, labels = np.asarray(keys, dtype=np.int64), np.asarray(labels) != 0
    keep = keys >= 0
    keys, labels = keys[keep], labels[keep]
    P, N = int(labels.sum()), int((~labels).sum())
    if P == 0 or N == 0:
        return [float("nan")] * 4 + [float(P), float(N)]
    order = np.argsort(-keys, kind="stable")
    k, y = keys[order], labels[order]
    starts = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    ends = np.concatenate((starts[1:], [k.size]))
    tp = fp = 0
    area = ap = 0.0
    best, best_key = -1.0, None
    for s, e in zip(starts, ends):
        pb = int(y[s:e].sum())
        nb = (e - s) - pb
        tp, fp = tp + pb, fp + nb
        area += pb * ((N - fp) + 0.5 * nb)
        ap += (pb / P) * (tp / (tp + fp))
        dice = 2.0 * tp / (tp + fp + P)
        if dice > best:                      # strictly: the first (highest) key keeps a tie
            best, best_key = dice, int(k[s])
    return [area / (float(P) * float(N)), ap, best, key_floor(best_key), float(P), float(N)]


def scores_exact(hist):
    """The definitions on a histogram (2, 65536) of Python integers ([0]: negatives, [1]: positives) in exact rational arithmetic
    -> [auroc, ap, best_dice, best_threshold, P, N] as floats (each rounded once)."""
    neg, pos = [int(v) for v in hist[0]], [int(v) for v in hist[1]]
    P, N = sum(pos), sum(neg)
    if P == 0 or N == 0:
        return [float("nan")] * 4 + [float(P), float(N)]
    tp = fp = 0
    area = Fraction(0)
    ap = Fraction(0)
    best, best_bin = Fraction(-1), None
    for b in range(len(pos) - 1, -1, -1):
        if pos[b] == 0 and neg[b] == 0:
            continue
        tp, fp = tp + pos[b], fp + neg[b]
        area += Fraction(pos[b]) * (Fraction(N - fp) + Fraction(neg[b], 2))
        ap += Fraction(pos[b], P) * Fraction(tp, tp + fp)
        dice = Fraction(2 * tp, tp + fp + P)
        if dice > best:
            best, best_bin = dice, b
    return [float(area / (P * N)), float(ap), float(best), key_floor(best_bin), float(P), float(N)]
