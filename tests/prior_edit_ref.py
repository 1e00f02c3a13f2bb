"""Plain-torch restatement of what editing with the code prior adds (tests/test_gpu_prior_edit.py, tests/test_prior_edit_host.py),
written from the formulas on top of tests/gpt_ref.py and evaluated in float64 on the kernel's own fp32 inputs.

    filter      s = z / temperature; K1 = {c: s_c >= the top_k-th largest s} (top_k = 0 or >= V: all); p_c = exp(s_c - max) on K1;
                G_c = sum of p over the entries of K1 STRICTLY greater than s_c; c stays iff G_c <= top_p sum_{K1} p
                (top_k_top_p_filtering's rule: tied entries share one fate, the largest entry always stays); top_p >= 1: K1
    draw        gpt_ref.sample_ref's inverse CDF in index order over the kept set
    forced      forced_b in [0, V): the token, u_b unread; < 0: a draw; >= V: a draw and logp NaN
    logp        log_softmax(z)[token]: temperature 1, unfiltered
    paste       out[b, c, y, x] = edit if cellmask[b, y // fy, x // fx] else image
    masked      position k takes known[:, k] or a draw from the teacher-forced distribution of the sequence so far
"""
import torch

import gpt_ref as G

TOP_PS = (0.3, 0.9, 1.0)
TINY_TOP_P = 1e-6          # keeps the maximum and its ties only


def filter_ref(logits, temperature=1.0, top_k=0, top_p=1.0, dtype=torch.float64):
    """logits (B, V) -> (kept (B, V) bool, margin (B,)).  margin: the smallest distance of a K1 entry's strictly-greater mass
    to top_p, both relative to the mass of K1 - how far the nucleus decision is from flipping (inf without a nucleus filter; the
    row's maxima, whose strictly-greater mass is exactly 0, always stay and are left out).
    Sort-based: the strictly-greater mass of an entry is the exclusive running sum at the first entry of its tie group."""
    s = logits.to(dtype) / temperature
    B, V = s.shape
    if top_k and top_k < V:
        k1 = s >= torch.topk(s, top_k, dim=-1).values[:, -1:]
    else:
        k1 = torch.ones_like(s, dtype=torch.bool)
    if top_p is None or top_p >= 1:
        return k1, torch.full((B,), float("inf"), dtype=torch.float64)
    p = torch.where(k1, torch.exp(s - s.max(dim=-1, keepdim=True).values), torch.zeros_like(s))
    order = torch.argsort(s, dim=-1, descending=True, stable=True)
    ss, ps = s.gather(1, order), p.gather(1, order)
    excl = torch.cumsum(ps, dim=-1) - ps
    first = torch.searchsorted((-ss).contiguous(), (-ss).contiguous(), right=False)          # the first entry of each tie group
    g_sorted = excl.gather(1, first) / ps.sum(dim=-1, keepdim=True)
    g = torch.empty_like(g_sorted).scatter_(1, order, g_sorted)
    kept = k1 & (g <= top_p)
    # the maxima have G = 0 exactly, in any arithmetic, and 0 <= top_p cannot flip: they do not enter the margin
    margin = torch.where(k1 & (g > 0), (g - top_p).abs(), torch.full_like(g, float("inf"))).min(dim=-1).values
    return kept, margin.double()


def draw_ref(logits, kept, u, temperature=1.0, dtype=torch.float64):
    """gpt_ref.sample_ref's draw over a given kept set -> (pick (B,), dist (B,))"""
    s = logits.to(dtype) / temperature
    V = s.shape[1]
    p = torch.where(kept, torch.exp(s - s.max(dim=-1, keepdim=True).values), torch.zeros_like(s))
    cdf = torch.cumsum(p, dim=-1)
    total = cdf[:, -1]
    goal = u.to(dtype) * total
    ar = torch.arange(V)
    last = torch.where(kept, ar, torch.full_like(ar, -1)).max(dim=-1).values
    first = torch.where((cdf > goal[:, None]) & kept, ar, torch.full_like(ar, V)).min(dim=-1).values
    pick = torch.where(first < V, first, last)
    hi = cdf.gather(-1, pick[:, None])[:, 0]
    lo = hi - p.gather(-1, pick[:, None])[:, 0]
    return pick, (torch.minimum((goal - lo).abs(), (hi - goal).abs()) / total).double()


def logp_ref(logits, tokens, dtype=torch.float64):
    return torch.log_softmax(logits.to(dtype), dim=-1).gather(-1, tokens[:, None])[:, 0]


def sample_filtered_ref(logits, u, forced=None, temperature=1.0, top_k=0, top_p=1.0):
    """-> (tokens (B,), logp (B,) float64, clear (B,) bool, kept (B, V) bool).  clear: both float64 distances - u total to the
    nearer CDF boundary, any K1 entry's strictly-greater mass to top_p - are above gpt_ref.SAMPLE_CLEAR (a forced row is clear)."""
    V = logits.shape[1]
    kept, margin = filter_ref(logits, temperature, top_k, top_p)
    pick, dist = draw_ref(logits, kept, u, temperature)
    clear = (dist > G.SAMPLE_CLEAR) & (margin > G.SAMPLE_CLEAR)
    nan = torch.zeros(logits.shape[0], dtype=torch.bool)
    if forced is not None:
        take = (forced >= 0) & (forced < V)
        pick = torch.where(take, forced, pick)
        clear = clear | take
        nan = forced >= V
    logp = logp_ref(logits, pick)
    return pick, torch.where(nan, torch.full_like(logp, float("nan")), logp), clear, kept


def paste_ref(image, edit, cellmask):
    """image, edit (B, C, H, W), cellmask (B, h, w) -> torch.where on the repeated mask"""
    H, W = image.shape[-2:]
    h, w = cellmask.shape[-2:]
    m = cellmask.bool().repeat_interleave(H // h, dim=1).repeat_interleave(W // w, dim=2)
    return torch.where(m[:, None], edit, image)


def state64(model):
    return {k: (v.detach().cpu() if k.endswith("mask") else v.detach().cpu().double()) for k, v in model.state_dict().items()}


def teacher_forced_logits(state, n_layer, n_head, prompt, tokens, dtype=torch.float64):
    """The full forward on [prompt, tokens[:, :-1]] -> the logits (B, S, V) of the S positions of `tokens`."""
    st = {k: (v if k.endswith("mask") else v.to(dtype)) for k, v in state.items()}
    with torch.no_grad():
        logits, _ = G.gpt_ref(torch.cat((prompt, tokens[:, :-1]), dim=1), st, n_layer, n_head)
    return logits[:, prompt.shape[1] - 1:]


def token_logp_ref(state, n_layer, n_head, prompt, tokens, dtype=torch.float64):
    """log p(tokens[:, k] | prompt, tokens[:, :k]) (B, S) from one full forward"""
    z = teacher_forced_logits(state, n_layer, n_head, prompt, tokens, dtype)
    return -G.xent_ref(z, tokens)[0]
