"""Plain-torch restatement of the decode kernels of the GPT code prior (csrc/gpt_decode.hip) in any dtype - the skinny fused linear,
the one-row attention over a cache, one decode step over gpt_ref / mingpt_ref - and the case tables of
tests/test_gpu_gpt_decode.py and tests/test_gpt_decode_host.py.

    dec_linear      y = act(LN?(x) W^T + bias) (+ residual) on x (M, K), W (N, K)
    dec_attention   o[b] = softmax(q[b] k[b, :Tk]^T / sqrt(hs)) v[b, :Tk] per head, no mask
    cache layout    (n_layer, 2, B, capacity, E): the presents (n_layer, 2, B, n_head, T, hs) with the heads side by side
"""
import torch

import gpt_ref as G
import mingpt_ref as M


def dec_linear_ref(x, w, bias=None, ln=None, gelu=False, residual=None):
    """x (M, K), w (N, K), bias (N,), ln = (gamma, beta, eps), residual (M, N) -> (M, N), in the dtype of x"""
    if ln is not None:
        x = M.layer_norm_ref(x, ln[0], ln[1], ln[2])
    y = torch.matmul(x, w.t())
    if bias is not None:
        y = y + bias
    if gelu:
        y = M.gelu_ref(y)
    return y if residual is None else y + residual


def dec_attention_ref(q, k_cache, v_cache, Tk, n_head):
    """q (B, E), k_cache, v_cache (B, capacity, E) -> (B, E): the rows [0, Tk) only"""
    o, _ = M.causal_attention_ref(q[:, None, :], k_cache[:, :Tk], v_cache[:, :Tk], n_head, causal=False)
    return o[:, 0]


def presents_to_cache(presents):
    """(n_layer, 2, B, n_head, T, hs) -> (n_layer, 2, B, T, E): the cache layout"""
    nl, two, B, nh, T, hs = presents.shape
    return presents.transpose(3, 4).reshape(nl, two, B, T, nh * hs)


def decode_step_ref(tok, st, n_layer, n_head, past, t0):
    """One token tok (B,) at position t0 behind past (n_layer, 2, B, n_head, t0, hs) -> (logits (B, V), the grown past)"""
    logits, present = G.gpt_ref(tok[:, None], st, n_layer, n_head, None, past=past, t0=t0)
    return logits[:, 0], torch.cat((past, present), dim=-2)


def state_as(state, dtype):
    return {k: (v if k.endswith("mask") else v.to(dtype)) for k, v in state.items()}


def pack_keys(n_layer):
    """The state_dict keys of the packed-weights buffer, in the order of the layout documented in include/vqwnet_hip.h"""
    keys = []
    for i in range(n_layer):
        b = "blocks.%d." % i
        keys += [b + "ln1.weight", b + "ln1.bias", b + "att.q.weight", b + "att.k.weight", b + "att.v.weight", b + "att.q.bias",
                 b + "att.k.bias", b + "att.v.bias", b + "att.proj.weight", b + "att.proj.bias", b + "ln2.weight", b + "ln2.bias",
                 b + "mlp.0.weight", b + "mlp.0.bias", b + "mlp.2.weight", b + "mlp.2.bias"]
    return keys + ["ln_f.weight", "ln_f.bias", "head.weight"]


# ---- dec_linear cases: (M, K, N) with M written against DEC_ROWS (R): every M of {1, 2, R - 1, R, R + 1}, every K of {4, 64, 96,
# 1024} and every N of {1, 3, 100, 257} - no tile divides them (four columns per workgroup, 64 float4 lanes per step)
LINEAR_M = ("1", "2", "R-1", "R", "R+1")
LINEAR_K = (4, 64, 96, 1024)
LINEAR_N = (1, 3, 100, 257)
LINEAR_SHAPES = [("1", 64, 257), ("2", 96, 100), ("R-1", 1024, 3), ("R", 4, 257), ("R+1", 64, 100), ("R", 1024, 257), ("R+1", 96, 1),
                 ("1", 1024, 100), ("R-1", 4, 3), ("R", 96, 1), ("2", 4, 100), ("R+1", 1024, 1)]
LINEAR_EDGE_SHAPES = [("1", 4, 1), ("R+1", 1024, 257), ("R-1", 96, 3)]          # each option alone runs here
LINEAR_ALL_OPTIONS_SHAPE = ("R", 96, 100)                                       # all sixteen combinations run here
OPTIONS = ("ln", "bias", "gelu", "residual")
# K above DEC_KC = 4096 floats walks chunks of the staged rows (a last chunk of one float4; the largest K), K = DEC_KC is the longest
# row the fused LayerNorm takes and the largest LDS request: (M, K, N, options)
LINEAR_CHUNKED = [("R+1", 4100, 3, ("bias",)), ("2", 16384, 5, ("bias", "gelu", "residual")), ("R", 4096, 3, OPTIONS)]


def rows_of(m, dec_rows):
    return {"1": 1, "2": 2, "R-1": dec_rows - 1, "R": dec_rows, "R+1": dec_rows + 1}[m]


def linear_inputs(Mr, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(Mr, K, generator=g) + 0.5, torch.randn(N, K, generator=g) / K ** 0.5
    bias, res = torch.randn(N, generator=g), torch.randn(Mr, N, generator=g)
    gamma, beta = 1 + torch.randn(K, generator=g) / 4, torch.randn(K, generator=g) / 4
    return x, w, bias, gamma, beta, res


# ---- dec_attention cases: (B, n_head, hs) x Tk; DA_CHUNK = 64 keys per chunk, four waves: 257 is the first key of wave 0's second chunk
ATTN_HEADS = [(1, 1, 32), (2, 3, 32), (3, 2, 64)]
ATTN_TK = (1, 2, 63, 64, 65, 257)
ATTN_PAD = 3          # capacity = Tk + ATTN_PAD: the rows behind Tk are NaN
ATTN_WIDE = [(1, 1, 96, 65), (2, 1, 128, 257), (1, 2, 96, 257)]          # (B, n_head, hs, Tk): the kernel's two other head sizes


def attention_inputs(B, nh, hs, Tk, seed):
    g = torch.Generator().manual_seed(seed)
    E, cap = nh * hs, Tk + ATTN_PAD
    q, k, v = torch.randn(B, E, generator=g), torch.randn(B, cap, E, generator=g), torch.randn(B, cap, E, generator=g)
    k[:, Tk:], v[:, Tk:] = float("nan"), float("nan")
    return q, k, v


# ---- generate on gpt64: prompt, steps, top_k as tests/test_gpu_mingpt_gpt.py's sample test; the uniforms come from a CPU generator
GEN_CASE, GEN_PROMPT, GEN_STEPS, GEN_TOPK, GEN_TEMP = "gpt64", 6, 12, 10, 1.0
# The seed is chosen on the CPU, from the float64 run alone (generate_truth): of the seeds 0 .. 11 five meet both conditions below
# (2, 3, 4, 6, 8); 6 is the one whose smaller margin is largest (dist 2.1e-3, gap 9.9e-3).  The test recomputes and asserts both.
GEN_SEED = 6
GEN_MIN_DIST = 100 * G.SAMPLE_CLEAR
GEN_MIN_GAP = 1e-3


def generate_truth(state, idx, seed):
    """The float64 run of generate on GEN_CASE: gpt_ref + sample_ref step by step on its own tokens -> (tokens (B, prompt + steps),
    uniforms (steps, B) fp32, the smallest sample_ref dist, the smallest gap between the k-th and (k + 1)-th scaled logit)."""
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[GEN_CASE]
    st = state_as(state, torch.float64)
    u = torch.rand(GEN_STEPS, B, generator=torch.Generator().manual_seed(seed))
    seq, min_dist, min_gap = idx[:, :GEN_PROMPT].clone(), float("inf"), float("inf")
    with torch.no_grad():
        for k in range(GEN_STEPS):
            logits = G.gpt_ref(seq, st, nl, nh)[0][:, -1, :]
            pick, dist, _ = G.sample_ref(logits, u[k], GEN_TEMP, GEN_TOPK)
            top = torch.topk(logits / GEN_TEMP, GEN_TOPK + 1, dim=-1).values
            min_dist = min(min_dist, float(dist.min()))
            min_gap = min(min_gap, float((top[:, GEN_TOPK - 1] - top[:, GEN_TOPK]).min()))
            seq = torch.cat((seq, pick[:, None]), dim=1)
    return seq, u, min_dist, min_gap
