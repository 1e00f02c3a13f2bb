"""Plain-torch / numpy restatement of the conditional code prior (csrc/cond.hip, networks.LabelCondition,
trainers.ConditionalPriorTrainer), written from the definitions, and the case tables of tests/test_cond_prior_host.py and
tests/test_gpu_cond_prior.py.

    cell labels     tokens[b, cy, cx] = the label in [0, L) most pixels of the cell carry; the smallest label on a tie; a pixel outside
                    [0, L) counts for nothing; -1 for a cell with no counted pixel; purity = float32(count) / float32(pixels per cell)
    cells changed   1 iff any pixel of the cell differs
    the model       logits = GPT([table[cond] | tok[inp]] + pos)[:, Tc:] under the mask with n_unmasked = Tc (gpt_ref: the model's own
                    mask buffer), inp = [sos, codes shifted right] with the pkeep corruption on the codes only (prior_ref.tokens_ref)
    the step        the unconditional recipe (prior_ref: clip by the global norm, AdamW) with the table among the undecayed parameters
"""
import numpy as np
import torch

import gpt_ref as G
import prior_ref as P
from gpt_ref import gpt_ref, init_gpt_, xent_ref
from prior_ref import adamw_ref_, clip_ref, decays, tokens_ref

TABLE = "cond.embed.weight"          # the table's name among the restatement's parameters


# ------------------------------------------------------------------------------------------------ the label kernels
def cell_labels_ref(label, h, w, L):
    """label (B, H, W) integer array -> (tokens (B, h, w) int64, purity (B, h, w) float32)"""
    label = np.asarray(label)
    if label.ndim == 4:
        label = label[:, 0]
    B, H, W = label.shape
    fy, fx = H // h, W // w
    cells = label.reshape(B, h, fy, w, fx).transpose(0, 1, 3, 2, 4).reshape(B, h, w, fy * fx).astype(np.int64)
    counts = np.stack([(cells == v).sum(-1) for v in range(L)], axis=-1)          # (B, h, w, L)
    best = counts.max(-1)
    tokens = np.where(best > 0, counts.argmax(-1), -1).astype(np.int64)          # argmax: the first (smallest) label of a tie
    purity = best.astype(np.float32) / np.float32(fy * fx)
    return tokens, purity.astype(np.float32)


def cells_changed_ref(a, b, h, w):
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 4:
        a, b = a[:, 0], b[:, 0]
    B, H, W = a.shape
    return (a != b).reshape(B, h, H // h, w, W // w).any(axis=(2, 4)).astype(np.uint8)


# (B, H, W, h, w, L)
LABEL_CASES = [(1, 1, 1, 1, 1, 1), (2, 24, 40, 3, 5, 5), (2, 24, 40, 4, 4, 2), (1, 8, 8, 8, 8, 3), (1, 64, 48, 1, 1, 7), (3, 96, 96, 3, 3, 256)]
LABEL_FULL_CASES = [((1, 512, 512, 16, 16, 256), torch.long), ((1, 512, 512, 32, 32, 2), torch.uint8)]
LABEL_DTYPES = (torch.uint8, torch.int32, torch.long)


def label_inputs(case, dtype, seed=0):
    """Random labels in [0, L) with the values -1 and L injected (255 for uint8 where L < 256; uint8 has no -1), then cells rebuilt
    as exact half / half ties of two labels (where a cell has an even number of pixels and L >= 2; the larger label first in
    memory, an eighth of the cell invalid), then one cell with no valid pixel (where the dtype has an invalid value at all; a map of ONE cell keeps its tie)."""
    B, H, W, h, w, L = case
    fy, fx = H // h, W // w
    rng = np.random.RandomState(1000 + seed + 7 * H + 13 * W + L)
    lab = rng.randint(0, L, size=(B, H, W)).astype(np.int64)
    invalid = [255] if dtype == torch.uint8 else [-1, L]
    if dtype == torch.uint8 and L == 256:
        invalid = []
    if invalid:
        hit = rng.rand(B, H, W) < 0.1
        lab[hit] = rng.choice(invalid, size=int(hit.sum()))
    n_cells = h * w
    order = rng.permutation(n_cells)
    ties = fy * fx % 2 == 0 and L >= 2
    empty = (B - 1, int(order[-1])) if invalid and not (ties and B * n_cells == 1) else None
    if ties:
        for c in order[:max(1, n_cells // 4)]:
            b = int(rng.randint(B))
            if (b, int(c)) == empty:
                continue
            cy, cx = divmod(int(c), w)
            lo, hi = sorted(rng.choice(L, size=2, replace=False).tolist())
            half, k = fy * fx // 2, fy * fx // 16 if invalid else 0          # k invalid pixels in each half: the tie stays exact
            cell = np.array([hi] * half + [lo] * half)
            cell[:k] = cell[half:half + k] = invalid[0] if invalid else 0
            lab[b, cy * fy:(cy + 1) * fy, cx * fx:(cx + 1) * fx] = cell.reshape(fy, fx)
    if empty is not None:
        cy, cx = divmod(empty[1], w)
        lab[empty[0], cy * fy:(cy + 1) * fy, cx * fx:(cx + 1) * fx] = invalid[0]
    return torch.from_numpy(lab).to(dtype)


def label_features(case, dtype):
    """(has out-of-range pixels, has a tie cell, has a cell with no valid pixel): what label_inputs builds into a case"""
    B, H, W, h, w, L = case
    even = (H // h) * (W // w) % 2 == 0 and L >= 2
    has_invalid = not (dtype == torch.uint8 and L == 256)
    return has_invalid, even, has_invalid and not (even and B * h * w == 1)


# ------------------------------------------------------------------------------------------------ the tiny conditional model
V, L, LAT_H, LAT_W, N_LAYER, N_HEAD, E, B = 16, 3, 3, 5, 2, 2, 64, 3          # E = 64: a head size of 32, the smallest the attention kernels serve
T = TC = LAT_H * LAT_W
GPT_KW = dict(vocab_size=V, block_size=TC + T, n_layer=N_LAYER, n_head=N_HEAD, n_embed=E, n_unmasked=TC)
SEED, SOS, STEPS, GRAD_NORM_CLIP = 141, 0, 3, 2.5          # the float64 norms are 5.75, 1.97, 3.43: the clip binds at steps 0 and 2 and not at step 1
OPTIM = P.OPTIM
# The step test's case (initial values and batch) is seeded with STEP_SEED, chosen on the CPU alone.  AdamW's first update of an
# element is lr g / (|g| + eps) with eps = 1e-8: an element whose gradient lies near eps turns an absolute fp32 error d of its
# gradient into lr eps d / (|g| + eps)^2 of parameter, up to lr d / (4 eps), and what follows in steps 2 and 3 inherits it.
# adam_step_sensitivity predicts that error from the float64 gradients of step 0 with d = 2^-23 rms(the tensor's gradient); over the
# seeds 141 .. 156 it ranges from 1.0e-5 (147) to 6.8e-4 (143), and where it is large ONE element carries it (141: 2.3e-4 predicted,
# of which 2.0e-4 from one element of blocks.1.mlp.2.weight; measured on the MI355X there: 5.2e-4 on that tensor after one step, the
# CPU's fp32 run 1.1e-4, while every gradient tensor of both sits 2e-7 .. 9e-7 from float64).  147 is the best-conditioned case of
# the range; the test asserts its figure before the device runs.  The optimiser is the trainer's own, eps = 1e-8.
STEP_SEED, STEP_MAX_SENSITIVITY = 147, 2e-5
STEP_CLIP = 4.0          # at STEP_SEED the float64 norms are 4.21, 7.40, 3.23: the clip binds at steps 0 and 1 and not at step 2


def adam_step_sensitivity(g0, coef, optim=OPTIM):
    """The parameter error (L2 over all parameters) that fp32 noise on the step-0 gradients g0 {name: float64 gradient}, clipped by
    coef, is predicted to leave after AdamW's first update; analytically zero gradients (|g| <= 1e-12) are left out."""
    total = 0.0
    for g in g0.values():
        g = (g.double() * coef).reshape(-1)
        g = g[g.abs() > 1e-12]
        if g.numel():
            d = 2.0 ** -23 * float(g.pow(2).mean().sqrt())
            total += float(((optim["lr"] * optim["eps"] * d / (g.abs() + optim["eps"]) ** 2) ** 2).sum())
    return total ** 0.5
VARIANTS = G.VARIANTS


def init_table_(weight, seed):
    """init_gpt_'s rounding rule for an embedding table: eight times the N(0, 0.02) draw under `seed`, rounded to multiples of 1/64"""
    import mingpt_ref as M
    with torch.no_grad():
        weight.copy_(M.round64(8 * 0.02 * torch.randn(weight.shape, generator=torch.Generator().manual_seed(seed + 3000))))
    return weight


def tiny_batch(seed=SEED):
    g = torch.Generator().manual_seed(seed + 2000)
    return torch.randint(0, V, (B, T), generator=g), torch.randint(0, L, (B, TC), generator=g)


def cond_logits(st, inp, cond, n_layer=N_LAYER, n_head=N_HEAD, n_tail=None):
    """st: the GPT's state dict (mask buffers included) plus TABLE -> the logits of the last n_tail positions (default: inp's own)"""
    gpt = {k: v for k, v in st.items() if k != TABLE}
    logits = gpt_ref(inp, gpt, n_layer, n_head, prefix=st[TABLE][cond])[0]
    return logits[:, logits.shape[1] - (inp.shape[1] if n_tail is None else n_tail):]


def state_as(state, dtype, grad=False):
    out = {}
    for k, v in state.items():
        v = v.detach().clone().cpu()
        out[k] = v if k.endswith("mask") else v.to(dtype).requires_grad_(grad)
    return out


def steps_ref(state, ids, cond, dtype, pkeep=1.0, uniforms=None, steps=STEPS, variant="threads8", optim=OPTIM, max_norm=STEP_CLIP):
    """`steps` steps of the conditional recipe from `state` (GPT state dict + TABLE).  uniforms: per step (u_keep, u_rand) (B, T)
    fp32, needed below pkeep = 1.  -> dict(loss, norm, coef [steps], g0 {key: the unclipped gradient of step 0}, P {key: the
    parameter after the last step}).  Variants as prior_ref.steps_ref's."""
    st = state_as(state, dtype, grad=True)
    rev = variant == "batch_reversed"
    flip = (lambda t: t.flip(0)) if rev else (lambda t: t)
    ids, cond = flip(ids), flip(cond)
    keys = [k for k in st if not k.endswith("mask")]
    mom = {k: (torch.zeros_like(st[k]), torch.zeros_like(st[k])) for k in keys}
    out = dict(loss=[], norm=[], coef=[])
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        for t in range(1, steps + 1):
            for k in keys:
                st[k].grad = None
            uk, ur = (None, None) if pkeep >= 1 else (flip(u) for u in uniforms[t - 1])
            inp = tokens_ref(ids, SOS, pkeep, V, uk, ur)
            loss = xent_ref(cond_logits(st, inp, cond), ids)[0].mean()
            loss.backward()
            grads = {k: st[k].grad for k in keys}
            norm, coef = clip_ref([grads[k] for k in keys], max_norm)
            if t == 1:
                out["g0"] = {k: grads[k].detach().clone() for k in keys}
            with torch.no_grad():
                for k in keys:
                    adamw_ref_(st[k], grads[k] * coef, mom[k][0], mom[k][1], t, optim["lr"], optim["betas"], optim["eps"],
                               optim["weight_decay"] if k != TABLE and decays(k) else 0.0)
            for key, val in (("loss", loss), ("norm", norm), ("coef", coef)):
                out[key].append(float(val.detach()))
    finally:
        torch.set_num_threads(n)
    out["P"] = {k: st[k].detach().clone() for k in keys}
    return out


def token_nll_ref(st, ids, cond):
    """-log p(code | the codes before it, the condition) (B, T), in st's dtype"""
    with torch.no_grad():
        return xent_ref(cond_logits(st, tokens_ref(ids, SOS, 1.0, V), cond), ids)[0]


# ---- the prior learns the condition: two sequences whose first codes differ, told apart by the condition alone
# Chosen with this restatement in float64 (test_gpu_cond_prior.py asserts it before the device runs): lr 1e-2 and 30 steps give a gap
# token_nll(first code | swapped condition) - token_nll(first code | right condition) of 6.85 and 8.42 nats for the two sequences
# (60 steps: 9.8 and 8.7; lr 3e-2, 30 steps: 8.8 and 8.0), against the 1 nat the test asks of the restatement.
LEARN_LR, LEARN_STEPS, LEARN_MIN_GAP = 1e-2, 30, 1.0


def learn_batch():
    a = (torch.arange(T) * 3 + 1) % V
    b = (torch.arange(T) * 5 + 2) % V
    assert int(a[0]) != int(b[0])
    ids = torch.stack((a, b))
    cond = torch.stack((torch.zeros(TC, dtype=torch.long), torch.ones(TC, dtype=torch.long)))
    return ids, cond


def learn_gap(st, ids, cond):
    """(gap of sequence A, gap of sequence B): nll of the first code under the swapped condition minus under the right one"""
    right = token_nll_ref(st, ids, cond)[:, 0]
    wrong = token_nll_ref(st, ids, cond.flip(0))[:, 0]
    return (wrong - right).tolist()


# ---- synthesize on the cached route against the float64 run
SYN_TOPK, SYN_TEMP, SYN_CANDIDATES, SYN_B = 4, 1.0, 2, 2
# The seed of the uniforms (SYN_CANDIDATES, T, SYN_B) is chosen on the CPU from the float64 run alone: of the seeds 0 .. 7 four (1, 2,
# 5, 7) clear gpt_decode_ref's GEN_MIN_DIST and GEN_MIN_GAP on both candidates; 2 has the largest smaller margin (dist 2.8e-3, gap
# 1.3e-2).  The test recomputes and asserts both.
SYN_SEED = 2


def synth_truth(st64, cond, uniforms):
    """The float64 run of synthesize for ONE candidate: uniforms (T, B) fp32 -> (tokens (B, T), the smallest sample_ref dist, the
    smallest gap between the k-th and (k + 1)-th scaled logit)."""
    Bc = cond.shape[0]
    seq = torch.full((Bc, 1), SOS, dtype=torch.long)
    min_dist, min_gap = float("inf"), float("inf")
    with torch.no_grad():
        for k in range(T):
            logits = cond_logits(st64, seq, cond, n_tail=1)[:, 0]
            pick, dist, _ = G.sample_ref(logits, uniforms[k], SYN_TEMP, SYN_TOPK)
            top = torch.topk(logits / SYN_TEMP, SYN_TOPK + 1, dim=-1).values
            min_dist = min(min_dist, float(dist.min()))
            min_gap = min(min_gap, float((top[:, SYN_TOPK - 1] - top[:, SYN_TOPK]).min()))
            seq = torch.cat((seq, pick[:, None]), dim=1)
    return seq[:, 1:], min_dist, min_gap
