"""GPU tests of the cached generation of the GPT code prior: the skinny fused linear and the decode attention against the float64
restatement (tests/gpt_decode_ref.py) at the smallest shapes that can go wrong, run-to-run bit-identity, and the model - prefill,
decode_step token by token, the cache's contents, generate() - on the reference's fixtures (tests/golden/mingpt_gpt_*.npz); one
decode_step against the same step rebuilt from its pieces, bit for bit, and a token outside the vocabulary.  Run with
`pytest -m gpu` on an MI355X.

Tolerances.  Kernel cases: the relative L2 distance of the kernel's result from the float64 restatement may be at most twice the
distance of the fp32 restatement (the same formulas in plain torch on the host, same input) from it - `_gate` of
tests/test_gpu_mingpt_blocks.py, measured per case and printed.  The decode attention and ops.causal_attention(causal=False) are both
held to that gate on the same input; two results that each lie within 2 x spread of the truth lie within 4 x spread of each other
(triangle inequality), which is asserted too.  Model cases: on gpt96p every position's logits within twice the fixture's own
fp32-against-fp64 spread of the fixture's eval logits; on gpt64 the gate rule against gpt_ref in float64, the fp32 side being gpt_ref
in fp32 on the host.  generate(): the float64 run's tokens exactly - the test first asserts that every decision of that run is far
from flipping (gpt_decode_ref.generate_truth), so no row is excused."""
import itertools
import os
import re

import pytest
import torch

from helpers import assert_close, rel_err
import gpt_decode_ref as D
import gpt_ref as G
from test_gpu_mingpt_blocks import _dev, _gate          # the blocks' gate rule, written once

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.0


def _define(name):
    """An integer #define of csrc/gpt_decode.hip"""
    src = open(os.path.join(ROOT, "medical-image-editing_amd", "csrc", "gpt_decode.hip")).read()
    return int(re.search(r"(?m)^#define\s+%s\s+(\d+)" % name, src).group(1))


# ------------------------------------------------------------------------------------------------ dec_linear
def _linear_case(m, K, N, opts, seed):
    """(kernel result, float64 truth, fp32 restatement) of one case; opts: a subset of D.OPTIONS"""
    from hipops import ops
    Mr = D.rows_of(m, _define("DEC_ROWS"))
    x, w, bias, gamma, beta, res = D.linear_inputs(Mr, K, N, seed)

    def ref(dtype):
        c = lambda t: t.to(dtype)
        return D.dec_linear_ref(c(x), c(w), c(bias) if "bias" in opts else None, (c(gamma), c(beta), 1e-5) if "ln" in opts else None,
                                "gelu" in opts, c(res) if "residual" in opts else None)

    with torch.no_grad():
        got = ops.dec_linear(_dev(x), _dev(w), _dev(bias) if "bias" in opts else None, (_dev(gamma), _dev(beta), 1e-5) if "ln" in opts else None,
                             "gelu" in opts, _dev(res) if "residual" in opts else None)
    torch.cuda.synchronize()
    assert got.shape == (Mr, N) and bool(torch.isfinite(got).all())
    return got, ref(torch.float64), ref(torch.float32)


def _linear_check(m, K, N, opts):
    seed = 7 * K + N + len(m) + sum(D.OPTIONS.index(o) + 1 for o in opts)
    got, truth, ref32 = _linear_case(m, K, N, opts, seed)
    _gate(got, truth, ref32, "dec_linear M=%s K%d N%d [%s]" % (m, K, N, " ".join(opts) or "plain"))
    again, _, _ = _linear_case(m, K, N, opts, seed)
    assert torch.equal(got, again), "two runs differ"


@pytest.mark.parametrize("m,K,N", D.LINEAR_SHAPES)
def test_dec_linear_shapes(m, K, N):
    _linear_check(m, K, N, ())
    _linear_check(m, K, N, D.OPTIONS)


@pytest.mark.parametrize("m,K,N", D.LINEAR_EDGE_SHAPES)
def test_dec_linear_each_option_alone_at_the_edge_shapes(m, K, N):
    for opt in D.OPTIONS:
        _linear_check(m, K, N, (opt,))


@pytest.mark.parametrize("m,K,N,opts", D.LINEAR_CHUNKED)
def test_dec_linear_rows_longer_than_a_staged_chunk(m, K, N, opts):
    kc = _define("DEC_KC")
    assert {K > kc for _, K, _, _ in D.LINEAR_CHUNKED} == {True, False} and max(K for _, K, _, _ in D.LINEAR_CHUNKED) == _define("DEC_MAX_K")
    assert ("ln" in opts) <= (K <= kc)
    _linear_check(m, K, N, opts)


def test_dec_linear_every_combination_of_options():
    m, K, N = D.LINEAR_ALL_OPTIONS_SHAPE
    for r in range(len(D.OPTIONS) + 1):
        for opts in itertools.combinations(D.OPTIONS, r):
            _linear_check(m, K, N, opts)


def test_dec_linear_in_place_residual_and_layer_norm_equals_the_kernel():
    """y may be the residual itself (the step's x += proj(att)); the fused LayerNorm restates vqw_layernorm_fwd operation by operation:
    the same bits as ops.layer_norm followed by the plain launch."""
    from hipops import ops
    x, w, bias, gamma, beta, res = (_dev(t) for t in D.linear_inputs(_define("DEC_ROWS"), 96, 96, 5))
    with torch.no_grad():
        want = ops.dec_linear(x, w, bias, residual=res)
        buf = res.clone()
        assert ops.dec_linear(x, w, bias, residual=buf, out=buf) is buf and torch.equal(buf, want)
        fused = ops.dec_linear(x, w, bias, ln=(gamma, beta, 1e-5))
        two = ops.dec_linear(ops.layer_norm(x, gamma, beta, 1e-5), w, bias)
    assert torch.equal(fused, two)


def test_dec_linear_strided_offset_output_touches_nothing_else():
    """The q | k | v launch's addressing: N columns at a column offset of rows with a larger stride, in a buffer with rows before and
    behind - everything outside the written columns and rows keeps its sentinel bits."""
    from hipops import ops
    R = _define("DEC_ROWS")
    for Mr, K, N, ld, col in ((R + 1, 64, 100, 257, 31), (1, 96, 3, 8, 5), (2, 4, 257, 300, 0)):
        x, w, bias, gamma, beta, res = D.linear_inputs(Mr, K, N, 11 + Mr)
        big = torch.full((Mr + 2, ld), SENTINEL, device=DEV)
        out = big[1:Mr + 1]
        with torch.no_grad():
            dense = ops.dec_linear(_dev(x), _dev(w), _dev(bias))
            assert ops.dec_linear(_dev(x), _dev(w), _dev(bias), out=out, out_col=col) is out
        torch.cuda.synchronize()
        assert torch.equal(big[1:Mr + 1, col:col + N], dense), "the strided result has the dense launch's bits"
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:Mr + 1, col:col + N] = False
        assert bool((big[mask] == SENTINEL).all()), "M%d K%d N%d ld%d col%d: bytes outside the written block changed" % (Mr, K, N, ld, col)
        truth = D.dec_linear_ref(x.double(), w.double(), bias.double())
        _gate(big[1:Mr + 1, col:col + N], truth, D.dec_linear_ref(x, w, bias), "dec_linear strided M%d K%d N%d ld%d col%d" % (Mr, K, N, ld, col))


# ------------------------------------------------------------------------------------------------ dec_attention
def test_attention_cases_cover_the_kernels_chunk():
    chunk = _define("DA_CHUNK")
    assert {chunk - 1, chunk, chunk + 1} <= set(D.ATTN_TK) and D.ATTN_HEADS[0] == (1, 1, 32)
    from hipops import _lib
    L, P = _lib.load(), 4096          # 32 is the smallest head the kernel accepts
    assert L.vqw_dec_attention(P, P, P, P, 1, 1, 1, 1, 16, 1.0, None) != 0 and b"32 <= hs" in L.vqw_last_error()


@pytest.mark.parametrize("B,nh,hs,Tk", D.ATTN_WIDE)
def test_dec_attention_wide_heads(B, nh, hs, Tk):
    test_dec_attention(B, nh, hs, Tk)


@pytest.mark.parametrize("B,nh,hs", D.ATTN_HEADS)
@pytest.mark.parametrize("Tk", D.ATTN_TK)
def test_dec_attention(B, nh, hs, Tk):
    from hipops import ops
    q, k, v = D.attention_inputs(B, nh, hs, Tk, seed=100 * Tk + 10 * nh + B)
    assert k.shape[1] == Tk + D.ATTN_PAD and bool(torch.isnan(k[:, Tk:]).all()) and bool(torch.isnan(v[:, Tk:]).all())
    truth = D.dec_attention_ref(q.double(), k.double(), v.double(), Tk, nh)
    ref32 = D.dec_attention_ref(q, k, v, Tk, nh)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)          # the NaN rows travel as they are
    with torch.no_grad():
        got = ops.dec_attention(qd, kd, vd, Tk, nh)
        again = ops.dec_attention(qd, kd, vd, Tk, nh)
        full = ops.causal_attention(qd[:, None, :], kd[:, :Tk], vd[:, :Tk], nh, causal=False)[:, 0]
    torch.cuda.synchronize()
    what = "dec_attention B%d nh%d hs%d Tk%d " % (B, nh, hs, Tk)
    assert got.shape == (B, nh * hs) and bool(torch.isfinite(got).all()), what + "the rows at or beyond Tk are NaN: they must not be read"
    _gate(got, truth, ref32, what)
    _gate(full, truth, ref32, what + "causal_attention")
    spread = rel_err(ref32, truth)
    print("%-44s %.3e from ops.causal_attention(causal=False) (4 x spread = %.3e)" % (what, rel_err(got, full), 4 * spread))
    assert_close(got, full, 4.0 * spread, what + "against ops.causal_attention")
    assert torch.equal(got, again), what + "two runs differ"
    if Tk == 1:          # one key: the softmax is 1, the output is its value row
        assert torch.equal(got.cpu(), v[:, 0])


# ------------------------------------------------------------------------------------------------ the model, teacher-forced
_cache = {}


def _fixture(golden, name):
    if name not in _cache:
        g = golden("mingpt_gpt_%s.npz" % name)
        state = {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}
        idx = g.t(name + "/in")
        prefix = g.t(name + "/prefix") if name + "/prefix" in g.files else None
        V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
        refs = []
        with torch.no_grad():          # the full forward in float64 and fp32 on the host: computed once, shared, never changed
            for dtype in (torch.float64, torch.float32):
                logits, presents = G.gpt_ref(idx, D.state_as(state, dtype), nl, nh, None if prefix is None else prefix.to(dtype))
                refs.append((logits, D.presents_to_cache(presents)))
        _cache[name] = (g, state, idx, prefix, refs)
    return _cache[name]


def _model(name, state):
    import networks
    m = networks.GPT(**G.gpt_kwargs(name))
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


def _teacher_forced(name, state, idx, prefix, n_prompt):
    """prefill on the first n_prompt positions (the prefix included), then decode_step token by token with the fixture's own tokens ->
    (logits (B, T, V), the cache)"""
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    m = _model(name, state).eval()
    cache = m.new_cache(B, capacity=Te + Ti + 2)
    cache.kv.fill_(SENTINEL)
    n0 = n_prompt - Te
    tokens = idx.to(DEV)
    logits = m.prefill(tokens[:, :n0], cache, embeddings=None if prefix is None else _dev(prefix))
    assert logits.shape == (B, n_prompt, V) and cache.length == n_prompt
    out = [logits]
    for t in range(n0, Ti):
        step = m.decode_step(tokens[:, t], cache)
        assert step.shape == (B, V) and cache.length == Te + t + 1
        out.append(step[:, None])
    torch.cuda.synchronize()
    return torch.cat(out, dim=1), cache


def _check_cache(name, cache, refs):
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    (_, kv64), (_, kv32) = refs
    assert cache.length == Te + Ti and cache.kv.shape == (nl, 2, B, Te + Ti + 2, E)
    _gate(cache.kv[:, :, :, :cache.length], kv64, kv32, name + " cache.kv[:, :, :, :length]")
    assert bool((cache.kv[:, :, :, cache.length:] == SENTINEL).all()), "rows at or beyond length must keep their sentinel"


def test_gpt96p_prefill_then_decode_steps_against_the_fixture(golden):
    name = G.CACHED_CASE
    g, state, idx, prefix, refs = _fixture(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    full, sp = g.t(name + "/eval_logits"), float(g[name + "/spread.eval_logits"])
    got, cache = _teacher_forced(name, state, idx, prefix, G.CACHED_PROMPT)
    assert got.shape == full.shape
    worst = max(rel_err(got[:, t], full[:, t]) for t in range(Te + Ti))
    print("%s prefill %d + decode steps: %.3e from the float64 full-sequence logits, worst position %.3e (fixture spread %.1e)" % (
        name, G.CACHED_PROMPT, rel_err(got, full), worst, sp))
    for t in range(Te + Ti):
        assert_close(got[:, t], full[:, t], 2.0 * sp, "%s position %d" % (name, t))
    _check_cache(name, cache, refs)


def test_gpt64_two_layers_from_a_prompt_that_covers_the_unmasked_corner(golden):
    name, n_prompt = "gpt64", D.GEN_PROMPT
    g, state, idx, prefix, refs = _fixture(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    assert nl == 2 and nu == 5 and n_prompt >= nu and prefix is None
    (logits64, _), (logits32, _) = refs
    got, cache = _teacher_forced(name, state, idx, prefix, n_prompt)
    _gate(got[:, :n_prompt], logits64[:, :n_prompt], logits32[:, :n_prompt], name + " prefill logits")
    _gate(got[:, n_prompt:], logits64[:, n_prompt:], logits32[:, n_prompt:], name + " decode_step logits")
    _check_cache(name, cache, refs)


def test_decode_step_rewound_repeats_its_bits_and_repack_sees_new_weights(golden):
    name = "gpt64"
    g, state, idx, prefix, refs = _fixture(golden, name)
    m = _model(name, state).eval()
    cache = m.new_cache(2)
    tokens = idx.to(DEV)
    m.prefill(tokens[:, :6], cache)
    a = m.decode_step(tokens[:, 6], cache)
    kv = cache.kv.clone()
    cache.length = 6
    b = m.decode_step(tokens[:, 6:7], cache)          # (B, 1) is taken too
    assert torch.equal(a, b) and torch.equal(kv[:, :, :, :7], cache.kv[:, :, :, :7])
    with torch.no_grad():
        m.ln_f.bias.add_(0.5)
    cache.length = 6
    assert torch.equal(m.decode_step(tokens[:, 6], cache), a), "the packed weights are a snapshot"
    cache.pack(m).length = 6
    assert not torch.equal(m.decode_step(tokens[:, 6], cache), a)


def _step_from_pieces(m, idx, cache):
    """decode_step's 2 + 5 n_layer launches as one ops call each (q, k and v as three: a wave owns a column, so the bits do not
    depend on the packing) on row cache.length of the cache -> the logits"""
    from hipops import ops
    t, nh, eps = cache.length, m.config.n_head, m.ln_f.eps
    x = ops.embedding(idx[:, None], m.tok_embed.weight, m.pos_embed, t0=t)[:, 0]
    for i, blk in enumerate(m.blocks):
        ln1, ln2 = (blk.ln1.weight, blk.ln1.bias, eps), (blk.ln2.weight, blk.ln2.bias, eps)
        q = ops.dec_linear(x, blk.att.q.weight, blk.att.q.bias, ln=ln1)
        for plane, lin in ((0, blk.att.k), (1, blk.att.v)):
            cache.kv[i, plane, :, t] = ops.dec_linear(x, lin.weight, lin.bias, ln=ln1)
        att = ops.dec_attention(q, cache.kv[i, 0], cache.kv[i, 1], t + 1, nh)
        ops.dec_linear(att, blk.att.proj.weight, blk.att.proj.bias, residual=x, out=x)
        h = ops.dec_linear(x, blk.mlp[0].weight, blk.mlp[0].bias, ln=ln2, gelu=True)
        ops.dec_linear(h, blk.mlp[2].weight, blk.mlp[2].bias, residual=x, out=x)
    cache.length += 1
    return ops.dec_linear(x, m.head.weight, ln=(m.ln_f.weight, m.ln_f.bias, eps))


def test_decode_step_equals_its_pieces_bit_for_bit(golden):
    name, n0 = "gpt64", 3
    g, state, idx, prefix, refs = _fixture(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    assert nl == 2 and prefix is None
    m = _model(name, state).eval()
    tokens = idx.to(DEV)
    one, two = m.new_cache(B), m.new_cache(B)
    with torch.no_grad():
        for cache in (one, two):
            cache.kv.fill_(SENTINEL)
            m.prefill(tokens[:, :n0], cache)
        assert torch.equal(one.kv, two.kv)
        step = m.decode_step(tokens[:, n0], one)
        pieces = _step_from_pieces(m, tokens[:, n0], two)
    torch.cuda.synchronize()
    assert one.length == two.length == n0 + 1 and step.shape == pieces.shape == (B, V) and bool(torch.isfinite(step).all())
    assert torch.equal(step, pieces), "logits: %.3e apart" % rel_err(step, pieces)
    for layer in range(nl):
        for plane in range(2):
            assert torch.equal(one.kv[layer, plane, :, n0], two.kv[layer, plane, :, n0]), "layer %d plane %d row %d" % (layer, plane, n0)
    assert torch.equal(one.kv, two.kv) and bool((one.kv[:, :, :, n0 + 1:] == SENTINEL).all())


def test_decode_step_token_outside_the_vocabulary_gives_nan_rows_and_touches_no_other():
    """B = 5: the fifth row sits in the second workgroup of the embedding launch (four rows a workgroup)."""
    import networks
    V, bs, E, B, bad = 8, 4, 32, 5, (1, 4)
    torch.manual_seed(23)
    m = networks.GPT(vocab_size=V, block_size=bs, n_layer=1, n_head=1, n_embed=E)
    with torch.no_grad():
        for p in m.parameters():          # LayerNorm weights and every bias off their initial 1 and 0
            p.add_(0.1 * torch.randn(p.shape))
    m = m.to(DEV).eval()
    first = torch.tensor([3, 0, 7, 5, 2], device=DEV)
    valid = torch.tensor([6, 1, 0, 7, 4], device=DEV)
    tokens = valid.clone()
    tokens[bad[0]], tokens[bad[1]] = V, -1
    got, want = m.new_cache(B), m.new_cache(B)
    for cache in (got, want):
        cache.kv.fill_(SENTINEL)
        m.prefill(first[:, None], cache)
    logits, ref = m.decode_step(tokens, got), m.decode_step(valid, want)
    torch.cuda.synchronize()
    assert got.length == 2 and logits.shape == (B, V) and bool(torch.isfinite(ref).all()) and bool(torch.isfinite(want.kv[:, :, :, :2]).all())
    good = [b for b in range(B) if b not in bad]
    for b in bad:
        assert bool(torch.isnan(logits[b]).all()), "logits row %d" % b
        assert bool(torch.isnan(got.kv[0, :, b, 1]).all()), "cache row 1 of batch row %d" % b
    assert torch.equal(logits[good], ref[good]) and torch.equal(got.kv[0, :, good, 1], want.kv[0, :, good, 1])
    assert torch.equal(got.kv[:, :, :, 0], want.kv[:, :, :, 0]), "the prefilled row"
    assert bool((got.kv[:, :, :, 2:] == SENTINEL).all()), "rows at or beyond length must keep their sentinel"


# ------------------------------------------------------------------------------------------------ generate
def test_generate_returns_the_float64_tokens(golden):
    name = D.GEN_CASE
    g, state, idx, prefix, refs = _fixture(golden, name)
    seq, u, min_dist, min_gap = D.generate_truth(state, idx, D.GEN_SEED)
    print("%s generate, seed %d: smallest sample_ref dist %.3e (>= %.0e), smallest k / k+1 gap %.3e (>= %.0e)" % (
        name, D.GEN_SEED, min_dist, D.GEN_MIN_DIST, min_gap, D.GEN_MIN_GAP))
    assert min_dist >= D.GEN_MIN_DIST and min_gap >= D.GEN_MIN_GAP          # before anything about the device
    m = _model(name, state).train()          # generate() switches to eval mode and back
    prompt = idx[:, :D.GEN_PROMPT].to(DEV)
    got = m.generate(prompt, D.GEN_STEPS, temperature=D.GEN_TEMP, top_k=D.GEN_TOPK, uniforms=u)
    again = m.generate(prompt, D.GEN_STEPS, temperature=D.GEN_TEMP, top_k=D.GEN_TOPK, uniforms=u.to(DEV))
    torch.cuda.synchronize()
    assert m.training and got.dtype == torch.long and got.shape == seq.shape
    assert torch.equal(got.cpu(), seq), "generate differs from the float64 run:\n%s\n%s" % (got.cpu(), seq)
    assert torch.equal(got, again)


def test_generate_and_sample_share_the_random_stream(golden):
    name, n0, steps, temp, top_k = D.GEN_CASE, D.GEN_PROMPT, D.GEN_STEPS, D.GEN_TEMP, D.GEN_TOPK
    g, state, idx, prefix, refs = _fixture(golden, name)
    m = _model(name, state).train()
    prompt = idx[:, :n0].to(DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    a = m.generate(prompt, steps, temperature=temp, top_k=top_k, generator=gen())
    b = m.generate(prompt, steps, temperature=temp, top_k=top_k, generator=gen())
    s = m.sample(prompt, steps, temperature=temp, top_k=top_k, generator=gen())
    torch.cuda.synchronize()
    assert m.training and a.shape == s.shape == (2, n0 + steps) and torch.equal(a, b) and torch.equal(a[:, :n0], prompt)
    assert torch.equal(m.generate(prompt, 0), prompt)
    # up to the first step whose decision the SAMPLE_CLEAR rule calls unclear, on sample()'s own tokens and the same uniforms
    replay = gen()
    m.eval()
    agreed = 0
    with torch.no_grad():
        for k in range(steps):
            logits = m(s[:, :n0 + k])[:, -1, :]
            u = torch.rand(2, generator=replay, device=DEV)
            _, dist, _ = G.sample_ref(logits.cpu(), u.cpu(), temp, top_k)
            clear = dist > G.SAMPLE_CLEAR
            assert torch.equal(a[:, n0 + k].cpu()[clear], s[:, n0 + k].cpu()[clear]), "step %d" % k
            if not bool(clear.all()):
                break
            agreed += 1
    print("%s generate against sample under one seed: %d of %d steps clear and equal" % (name, agreed, steps))
