"""Plain-torch restatement of what the GPT code prior adds to the minGPT blocks (tests/mingpt_ref.py): the token / position
embedding, the cross-entropy over the last axis, top-k sampling and the GPT model, written from the formulas and evaluated in any
dtype: the float64 truth of tests/test_gpu_mingpt_gpt.py and the check of tests/golden/mingpt_gpt_*.npz in
tests/test_mingpt_gpt_host.py.  Also the case tables of both and of tests/golden/make_golden_mingpt_gpt.py.

    embedding   x[b, t] = (prefix[b, t] if t < Te else tok[idx[b, t - Te]]) + pos[t0 + t]
    xent        lse_r = log sum_c exp(z_rc), loss_r = lse_r - z[r, target_r]
    sampling    s = z / temperature; thr = the k-th largest s; keep every s >= thr; p = exp(s - max) over the kept entries; the sample
                is the first kept index whose running sum of p exceeds u total, the last kept index if there is none
"""
import torch

import mingpt_ref as M


def embedding_ref(idx, tok, pos, prefix=None, t0=0):
    """idx (B, Ti) long, tok (V, E), pos (block_size, E) or (1, block_size, E), prefix (B, Te, E) or None -> (B, Te + Ti, E)"""
    x = tok[idx]
    if prefix is not None:
        x = torch.cat((prefix, x), dim=1)
    pos = pos.reshape(-1, pos.shape[-1])
    return x + pos[t0:t0 + x.shape[1]]


def xent_ref(z, target):
    """z (..., V), target (...) long -> (loss (...), lse (...))"""
    lse = torch.logsumexp(z, dim=-1)
    return lse - z.gather(-1, target.unsqueeze(-1)).squeeze(-1), lse


def sample_ref(logits, u, temperature=1.0, top_k=0, dtype=torch.float64):
    """logits (B, V), u (B,) -> (sample (B,) long, dist (B,), kept (B, V) bool).  dist: the distance of u total to the nearer of the
    two CDF boundaries around the chosen index, relative to total - how far the decision is from flipping."""
    s = logits.to(dtype) / temperature
    B, V = s.shape
    if top_k and top_k < V:
        thr = torch.topk(s, top_k, dim=-1).values[:, -1:]
        kept = s >= thr
    else:
        kept = torch.ones_like(s, dtype=torch.bool)
    p = torch.where(kept, torch.exp(s - s.max(dim=-1, keepdim=True).values), torch.zeros_like(s))
    cdf = torch.cumsum(p, dim=-1)
    total = cdf[:, -1]
    goal = u.to(dtype) * total
    hit = (cdf > goal[:, None]) & kept
    ar = torch.arange(V)
    last = torch.where(kept, ar, torch.full_like(ar, -1)).max(dim=-1).values
    first = torch.where(hit, ar, torch.full_like(ar, V)).min(dim=-1).values
    pick = torch.where(first < V, first, last)
    hi = cdf.gather(-1, pick[:, None])[:, 0]
    lo = hi - p.gather(-1, pick[:, None])[:, 0]
    dist = torch.minimum((goal - lo).abs(), (hi - goal).abs()) / total
    return pick, dist.double(), kept


def gpt_ref(idx, st, n_layer, n_head, prefix=None, past=None, t0=0):
    """GPT.forward / forward_with_past from its state dict -> (logits (B, T, V), presents (n_layer, 2, B, n_head, T, hs)).
    past: (n_layer, 2, B, n_head, Tp, hs) or None; t0: the position of the first new token."""
    x = embedding_ref(idx, st["tok_embed.weight"], st["pos_embed"], prefix, t0)
    presents = []
    for i in range(n_layer):
        x, present = M.block_ref(x, st, "blocks.%d." % i, n_head, None if past is None else past[i])
        presents.append(present)
    x = M.layer_norm_ref(x, st["ln_f.weight"], st["ln_f.bias"])
    return torch.matmul(x, st["head.weight"].t()), torch.stack(presents)


# the fixture cases of tests/golden/make_golden_mingpt_gpt.py: name -> (V, block_size, n_layer, n_head, E, n_unmasked, B, Ti, Te)
CASES = {
    "gpt64": (100, 40, 2, 2, 64, 5, 2, 40, 0),
    "gpt96p": (257, 70, 1, 3, 96, 0, 2, 37, 3),
}
SEEDS = {"gpt64": 91, "gpt96p": 92}
VARIANTS = M.VARIANTS
CACHED_CASE, CACHED_PROMPT = "gpt96p", 20          # the cached route: one call on the first 20 tokens, then one token per call


def gpt_kwargs(name):
    V, bs, nl, nh, E, nu, B, Ti, Te = CASES[name]
    return dict(vocab_size=V, block_size=bs, n_layer=nl, n_head=nh, n_embed=E, n_unmasked=nu)


def init_gpt_(model, seed):
    """The fixture's initial state of a freshly constructed GPT (reference or this project's) built under torch.manual_seed(seed):
    every value a multiple of 1/64.  nn.Linear and nn.Embedding weights: eight times the seeded N(0, 0.02) draw, rounded (the
    draw itself would round to three levels); nn.Linear biases, LayerNorm weights and biases and pos_embed - all constants after
    _init_weights, pos_embed all zeros - from a generator seeded with seed + 1000, so that every gradient formula is exercised."""
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.Embedding)):
                m.weight.copy_(M.round64(8 * m.weight))
                if isinstance(m, torch.nn.Linear) and m.bias is not None:
                    m.bias.copy_(M.round64(torch.randn(m.bias.shape, generator=g) / 8))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(M.round64(1 + torch.randn(m.weight.shape, generator=g) / 4))
                m.bias.copy_(M.round64(torch.randn(m.bias.shape, generator=g) / 4))
        model.pos_embed.copy_(M.round64(torch.randn(model.pos_embed.shape, generator=g) / 4))
    return model


def case_inputs(name, seed):
    """(idx (B, Ti) long, target (B, Te + Ti) long, prefix (B, Te, E) or None)"""
    V, bs, nl, nh, E, nu, B, Ti, Te = CASES[name]
    g = torch.Generator().manual_seed(seed + 2000)
    idx = torch.randint(0, V, (B, Ti), generator=g)
    target = torch.randint(0, V, (B, Te + Ti), generator=g)
    prefix = M.round64(torch.randn(B, Te, E, generator=g) / 4) if Te else None
    return idx, target, prefix


def grads_ref(name, state, idx, target, prefix, dtype, variant="threads8"):
    """(logits, loss, {parameter name / "input": gradient}) of the mean cross-entropy through the restatement; "input" is the prefix
    (only where the case has one).  The variants are mathematically identical evaluations: eight threads, one thread, the batch
    in reversed order."""
    V, bs, nl, nh, E, nu, B, Ti, Te = CASES[name]
    st = {}
    for k, v in state.items():
        v = v.detach().clone()
        st[k] = v if k.endswith("mask") else v.to(dtype).requires_grad_(True)
    rev = variant == "batch_reversed"
    flip = (lambda t: t.flip(0)) if rev else (lambda t: t)
    pin = None if prefix is None else flip(prefix).detach().clone().to(dtype).requires_grad_(True)
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        logits, _ = gpt_ref(flip(idx), st, nl, nh, pin)
        loss = xent_ref(logits, flip(target))[0].mean()
        loss.backward()
    finally:
        torch.set_num_threads(n)
    grads = {k: v.grad for k, v in st.items() if not k.endswith("mask")}
    if pin is not None:
        grads["input"] = flip(pin.grad)
    return flip(logits.detach()), loss.detach(), grads


# ---- kernel cases of tests/test_gpu_mingpt_gpt.py
# embedding (B, Ti, E, V, Te, t0, kind): kind "rand" = random indices (with repeats in every case of 40 or more), "same" = every index equal
EMBED_CASES = [
    (1, 1, 32, 1, 0, 0, "rand"), (2, 40, 64, 100, 0, 0, "rand"), (2, 40, 64, 100, 0, 0, "same"), (1, 64, 32, 7, 0, 0, "rand"),
    (1, 65, 32, 7, 0, 0, "rand"), (2, 37, 96, 257, 3, 0, "rand"), (3, 1, 64, 100, 0, 17, "rand"), (2, 1, 4, 5, 0, 0, "rand"),
    (1, 2, 4096, 3, 0, 0, "rand"),
]
# sampling (V, k) x temperatures, B rows each
SAMPLE_CASES = [(1, 0), (100, 0), (100, 1), (100, 10), (100, 100), (1000, 100), (16384, 100)]
SAMPLE_TEMPS = (0.5, 1.0, 2.0)
SAMPLE_B = 64
SAMPLE_CLEAR = 1e-5          # a row whose sample_ref distance exceeds this must match exactly
SAMPLE_UNCLEAR_CAP = 0.02    # at most this fraction of a case's rows may be unclear


def sample_inputs(V, k, temperature):
    """logits: 0.25 randn rounded to multiples of 1/4 - so that ties straddle the k-th value - and uniforms in [0, 1)"""
    g = torch.Generator().manual_seed(1000 * V + 10 * k + int(4 * temperature))
    logits = torch.round(0.25 * torch.randn(SAMPLE_B, V, generator=g) * 4) / 4
    return logits, torch.rand(SAMPLE_B, generator=g)
