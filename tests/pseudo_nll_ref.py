"""The pseudo-likelihood map of the masked prior restated in numpy integers and float64 (csrc/pseudo_nll.hip,
MaskedGPT.pseudo_nll), written from the definitions.  Nothing here is read by the code under test, and nothing of the package under
test is imported.

    lattice     position t = y w + x of an h x w grid belongs to group g(t) = (y mod sy) sx + (x mod sx) of S = sy sx groups
    inputs      row b ns + (s - s0) of the chunk [s0, s0 + ns) = ids[b] with the mask token at every position of group s
    gather      y[b][t] = x[b ns + g(t) - s0][t] for s0 <= g(t) < s0 + ns; every other row of y stays as it was
    map         pnll[b][t] = -log softmax(logits of pass g(t) at position t)[ids[b][t]]: one float64 forward of tests/gpt_ref.py per
                pass (under an all-ones attention mask, the state dict's), a float64 log-softmax and a pick
"""
import numpy as np
import torch

import gpt_ref as G


def groups(h, w, sy, sx):
    """(T,) int64: the group of every position, raster order"""
    y, x = np.divmod(np.arange(h * w, dtype=np.int64), w)
    return (y % sy) * sx + (x % sx)


def lattice_inputs(ids, h, w, sy, sx, s0, ns, mask_token):
    """ids (B, T) int64 -> (B ns, T) int64"""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    assert T == h * w and 1 <= sy <= h and 1 <= sx <= w and 0 <= s0 and ns >= 1 and s0 + ns <= sy * sx
    g = groups(h, w, sy, sx)
    out = np.empty((B * ns, T), dtype=np.int64)
    for b in range(B):
        for k in range(ns):
            out[b * ns + k] = np.where(g == s0 + k, mask_token, ids[b])
    return out


def gather(x, y, h, w, sy, sx, s0, ns):
    """x (B ns, T, ...) -> a copy of y (B, T, ...) with the rows of the groups in [s0, s0 + ns) taken from their pass"""
    y = np.array(y, copy=True)
    g = groups(h, w, sy, sx)
    for b in range(y.shape[0]):
        for t in range(h * w):
            if s0 <= g[t] < s0 + ns:
                y[b, t] = x[b * ns + g[t] - s0, t]
    return y


def pseudo_logits_ref(ids, st, n_layer, n_head, h, w, sy, sx, mask_token, chunk=None, forward=None):
    """float64 logits (B, T, V) of the gathered rows: pass s through `forward` (inp (rows, T) long -> logits; default gpt_ref on
    the float64 state dict st), `chunk` passes at a time (None: all S in one)."""
    ids = torch.as_tensor(ids).long().cpu()
    B, T = ids.shape
    S = sy * sx
    chunk = S if chunk is None else int(chunk)
    if forward is None:
        forward = lambda inp, ns: G.gpt_ref(inp, st, n_layer, n_head)[0]          # noqa: E731
    z = None
    for s0 in range(0, S, chunk):
        ns = min(chunk, S - s0)
        inp = torch.from_numpy(lattice_inputs(ids.numpy(), h, w, sy, sx, s0, ns, mask_token))
        logits = forward(inp, ns).double().numpy()
        if z is None:
            z = np.full((B, T, logits.shape[-1]), np.nan)
        z = gather(logits, z, h, w, sy, sx, s0, ns)
    assert not np.isnan(z).any()          # the groups partition the grid: every row was written
    return torch.from_numpy(z)


def pseudo_nll_ref(ids, st, n_layer, n_head, h, w, sy, sx, mask_token, chunk=None, forward=None):
    """-> (pnll (B, h, w) float64, the float64 logits (B, T, V) of the gathered rows)"""
    ids = torch.as_tensor(ids).long().cpu()
    z = pseudo_logits_ref(ids, st, n_layer, n_head, h, w, sy, sx, mask_token, chunk, forward)
    nll = torch.logsumexp(z, -1) - z.gather(-1, ids[..., None])[..., 0]
    return nll.reshape(ids.shape[0], h, w), z


def state64(model):
    """The model's state dict on the host in float64 (attention masks as they are)"""
    return {k: (v.detach().cpu() if k.endswith("mask") else v.detach().cpu().double()) for k, v in model.state_dict().items()}


def nll_bound(z_ref, nll_ref, sp):
    """The a-priori bound on ||device map - float64 map||_2: a row's |d nll| <= 2 ||d z_row||_2 (|d lse| <= max|d z| and
    |d z[target]| <= max|d z|), so ||d nll||_2 <= 2 ||d z||_2 <= 2 (2 sp) ||z_ref||_2 with 2 sp the relative bound of the logits;
    plus one fp32 ulp of max(1, |nll|) per element for the cross-entropy's own rounding (added as the 2-norm of the per-element
    allowances)."""
    ulp = 2.0 ** -23
    own = float(np.linalg.norm(ulp * np.maximum(1.0, np.abs(np.asarray(nll_ref, dtype=np.float64))).ravel()))
    return 2.0 * (2.0 * sp) * float(np.linalg.norm(np.asarray(z_ref, dtype=np.float64).ravel())) + own


# (h, w) grids and their strides of the kernel tests; (h, w) itself - one masked position per pass - is added per grid
GRIDS = [(4, 4), (3, 5), (1, 7)]
STRIDES = [(1, 1), (2, 2), (3, 2)]


def strides_of(h, w):
    out = [s for s in STRIDES if s[0] <= h and s[1] <= w]
    return out + [(h, w)]


def chunks_of(S):
    """Every (s0, ns) split for S <= 6; first, middle and last chunks otherwise"""
    if S <= 6:
        return [(s0, ns) for s0 in range(S) for ns in range(1, S - s0 + 1)]
    return [(0, 1), (0, 3), (S // 2 - 1, 3), (S - 2, 2), (S - 1, 1), (0, S)]
