"""GPU tests of the GPT code prior: the embedding, cross-entropy and top-k sampling kernels against the float64 restatement
(tests/gpt_ref.py) at the smallest shapes that can go wrong, run-to-run bit-identity, and the GPT model - forward, loss, backward,
the cached route and sample() - on the reference's fixtures (tests/golden/mingpt_gpt_*.npz, made by
tests/golden/make_golden_mingpt_gpt.py).  Run with `pytest -m gpu` on an MI355X.

Tolerances.  Kernel cases: the relative L2 distance of the kernel's result from the float64 restatement may be at most twice the
distance of the fp32 restatement (the same formulas in plain torch on the host, same input) from it - `_gate` of
tests/test_gpu_mingpt_blocks.py, measured per quantity and case and printed.  Exact expectations where they exist: the embedding's
forward is one add (bit-equal to the fp32 restatement), unused rows of gtok and untouched rows of gpos are exactly 0, the mean
loss lies within one fp32 ulp of the float64 mean of the kernel's own per-row losses.  Sampling: every returned index lies in the
float64 kept set; it equals the float64 restatement's wherever that decision is clear (u total further than 1e-5 total from both
CDF boundaries around the chosen index), and at most 2 % of a case's rows may be unclear.  Module cases: logits within twice the
fixture's own fp32-against-fp64 spread, the loss within twice the largest |loss32 - loss64| of the reference's three fp32
evaluations, gradients through helpers.grad_gate at its defaults, twice: on whole tensors against gpt_ref in float64 and on the
fixture's own samples."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import assert_close, grad_gate, rel_err
import gpt_ref as G
from test_gpu_mingpt_blocks import _dev, _fixture_gate, _gate          # the blocks' gate rule, written once

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    """An integer #define of csrc/gpt_head.hip"""
    src = open(os.path.join(ROOT, "medical-image-editing_amd", "csrc", "gpt_head.hip")).read()
    return int(re.search(r"(?m)^#define\s+%s\s+(\d+)" % name, src).group(1))


# ------------------------------------------------------------------------------------------------ embedding
def _embed_inputs(B, Ti, E, V, Te, t0, kind, seed):
    """block_size = t0 + T + 2: two rows of pos behind the ones in use (and t0 in front) that the backward must zero"""
    g = torch.Generator().manual_seed(seed)
    T = Te + Ti
    idx = torch.randint(0, V, (B, Ti), generator=g) if kind == "rand" else torch.full((B, Ti), V // 2, dtype=torch.long)
    tok, pos = torch.randn(V, E, generator=g), torch.randn(1, t0 + T + 2, E, generator=g)
    prefix = torch.randn(B, Te, E, generator=g) if Te else None
    return idx, tok, pos, prefix, torch.randn(B, T, E, generator=g)


def _embed_ref(idx, tok, pos, prefix, gx, t0, dtype):
    tok, pos = (t.detach().to(dtype).requires_grad_(True) for t in (tok, pos))
    prefix = None if prefix is None else prefix.detach().to(dtype).requires_grad_(True)
    x = G.embedding_ref(idx, tok, pos, prefix, t0)
    (x * gx.to(dtype)).sum().backward()
    res = dict(x=x.detach(), gtok=tok.grad, gpos=pos.grad)
    if prefix is not None:
        res["gprefix"] = prefix.grad
    return res


def _embed_run(idx, tok, pos, prefix, gx, t0):
    from hipops import ops
    tokd, posd = (_dev(t).requires_grad_(True) for t in (tok, pos))
    pd = None if prefix is None else _dev(prefix).requires_grad_(True)
    x = ops.embedding(idx.to(DEV), tokd, posd, pd, t0=t0)
    x.backward(_dev(gx))
    torch.cuda.synchronize()
    res = dict(x=x.detach(), gtok=tokd.grad, gpos=posd.grad)
    if pd is not None:
        res["gprefix"] = pd.grad
    return res


@pytest.mark.parametrize("B,Ti,E,V,Te,t0,kind", G.EMBED_CASES)
def test_embedding(B, Ti, E, V, Te, t0, kind):
    idx, tok, pos, prefix, gx = _embed_inputs(B, Ti, E, V, Te, t0, kind, seed=B + Ti + E + V)
    truth = _embed_ref(idx, tok, pos, prefix, gx, t0, torch.float64)
    ref32 = _embed_ref(idx, tok, pos, prefix, gx, t0, torch.float32)
    got = _embed_run(idx, tok, pos, prefix, gx, t0)
    what = "embedding B%d Ti%d E%d V%d Te%d t0=%d %s " % (B, Ti, E, V, Te, t0, kind)
    if B * Ti >= 40:
        assert idx.unique().numel() < idx.numel(), what + "the case is meant to repeat indices"
    assert got["x"].shape == (B, Te + Ti, E) and torch.equal(got["x"].cpu(), ref32["x"]), what + "x: one add, bit-equal"
    for k in ("gtok", "gpos") + (("gprefix",) if Te else ()):
        assert got[k].shape == truth[k].shape, k
        _gate(got[k], truth[k], ref32[k], what + k)
    if Te:
        assert torch.equal(got["gprefix"].cpu(), gx[:, :Te])
    used = torch.zeros(V, dtype=torch.bool)
    used[idx.reshape(-1)] = True
    T = Te + Ti
    assert not bool(got["gtok"].cpu()[~used].any()), what + "unused rows of gtok are exactly 0"
    gpos = got["gpos"].cpu()[0]
    assert gpos.shape[0] == t0 + T + 2 and not bool(gpos[:t0].any()) and not bool(gpos[t0 + T:].any()), what + "untouched rows of gpos are exactly 0"
    if kind == "same":          # the one used row is the ordered sum of all B Ti rows
        assert int(used.sum()) == 1
        acc = torch.zeros(E)
        for row in gx.reshape(-1, E):
            acc = acc + row
        assert torch.equal(got["gtok"].cpu()[V // 2], acc), what + "gtok: ascending (b, t) order"
    again = _embed_run(idx, tok, pos, prefix, gx, t0)
    for k in got:
        assert torch.equal(got[k], again[k]), what + k + " differs between two runs"


def test_embedding_index_out_of_range_is_nan_row_and_skipped():
    from hipops import ops
    idx, tok, pos, _, gx = _embed_inputs(2, 5, 32, 7, 0, 0, "rand", seed=1)
    idx[0, 2], idx[1, 4] = 7, -1
    tokd, posd = (_dev(t).requires_grad_(True) for t in (tok, pos))
    x = ops.embedding(idx.to(DEV), tokd, posd)
    x.backward(_dev(gx))
    torch.cuda.synchronize()
    bad = torch.zeros(2, 5, dtype=torch.bool)
    bad[0, 2] = bad[1, 4] = True
    xc = x.detach().cpu()
    assert bool(torch.isnan(xc[bad]).all()) and bool(torch.isfinite(xc[~bad]).all())
    good = idx.clamp(0, 6)
    want = torch.zeros(7, 32).index_add_(0, good[~bad], gx[~bad])
    assert bool(torch.isfinite(tokd.grad).all()) and rel_err(tokd.grad, want) < 1e-6


# ------------------------------------------------------------------------------------------------ cross-entropy
# XE_REG_V: up to this many columns a row lives in registers, above it is walked with an online maximum and sum; XE_WG_ROWS: rows
# per workgroup, one partial sum of losses each; XE_FOLD_LANES: threads of the fold - up to XE_FOLD_LANES * XE_WG_ROWS rows a
# thread adds at most one partial.
XE_REG_V, XE_WG_ROWS, XE_FOLD_LANES = 1024, 32, 256
XENT_CASES = [(1, 1), (3, 7), (5, 100), (70, 1024), (3, 1025), (3, 16384), (2, 65536), (32, 8), (33, 8), (8192, 8), (8193, 8)]


def _xent_inputs(rows, V, seed, offset_row=None):
    g = torch.Generator().manual_seed(seed)
    z = 2 * torch.randn(rows, V, generator=g)
    if offset_row is not None:
        z[offset_row] += 1e4
    return z, torch.randint(0, V, (rows,), generator=g), torch.randn(rows, generator=g)


def _xent_ref(z, t, gloss, dtype):
    res = {}
    for mode in ("mean", "none"):
        zz = z.detach().to(dtype).requires_grad_(True)
        loss, lse = G.xent_ref(zz, t)
        (loss.mean() if mode == "mean" else (loss * gloss.to(dtype)).sum()).backward()
        res.update({"loss": loss.detach(), "lse": lse.detach(), "mean": loss.detach().mean(), "gz_" + mode: zz.grad})
    return res


def _xent_run(z, t, gloss):
    from hipops import ops
    td = t.to(DEV)
    zm = _dev(z).requires_grad_(True)
    mean = ops.cross_entropy(zm, td)
    mean.backward()
    zn = _dev(z).requires_grad_(True)
    loss = ops.cross_entropy(zn, td, reduction="none")
    loss.backward(_dev(gloss))
    with torch.no_grad():
        loss2, lse = ops.cross_entropy_lse(zn, td)
    torch.cuda.synchronize()
    assert mean.shape == () and loss.shape == t.shape and torch.equal(loss.detach(), loss2)
    return dict(loss=loss.detach(), lse=lse, mean=mean.detach(), gz_mean=zm.grad, gz_none=zn.grad)


def _xent_check(rows, V, seed, offset_row=None):
    z, t, gloss = _xent_inputs(rows, V, seed, offset_row)
    truth, ref32, got = _xent_ref(z, t, gloss, torch.float64), _xent_ref(z, t, gloss, torch.float32), _xent_run(z, t, gloss)
    what = "cross_entropy rows%d V%d%s " % (rows, V, "" if offset_row is None else " +1e4")
    for k in ("loss", "lse", "gz_mean", "gz_none"):
        assert got[k].shape == truth[k].shape and bool(torch.isfinite(got[k]).all()), what + k
        _gate(got[k], truth[k], ref32[k], what + k)
    own = float(got["loss"].double().mean())
    ulp = float(np.spacing(np.float32(abs(own))))
    print("%-44s %.9g, the float64 mean of the kernel's own losses %.12g (%.2f ulp)" % (what + "mean", float(got["mean"]), own,
                                                                                         abs(float(got["mean"]) - own) / ulp))
    assert abs(float(got["mean"]) - own) <= ulp, what + "mean"
    again = _xent_run(z, t, gloss)
    for k in got:
        assert torch.equal(got[k], again[k]), what + k + " differs between two runs"
    return got


@pytest.mark.parametrize("rows,V", XENT_CASES)
def test_cross_entropy(rows, V):
    got = _xent_check(rows, V, seed=rows + V)
    if V == 1:          # one class: loss and gradient are exactly 0
        for k in ("loss", "mean", "gz_mean", "gz_none"):
            assert not bool(got[k].any()), k


def test_cross_entropy_thresholds_are_the_kernels():
    from hipops import ops
    L = ops._L()
    assert _define("XE_REG_V") == XE_REG_V and _define("XE_WG_ROWS") == XE_WG_ROWS and _define("XE_FOLD_LANES") == XE_FOLD_LANES
    assert (XE_REG_V, XE_REG_V + 1) == (1024, 1025) and (70, 1024) in XENT_CASES and (3, 1025) in XENT_CASES
    for rows in (XE_WG_ROWS, XE_WG_ROWS + 1, XE_FOLD_LANES * XE_WG_ROWS, XE_FOLD_LANES * XE_WG_ROWS + 1):
        assert (rows, 8) in XENT_CASES
    assert L.vqw_xent_ws_bytes(XE_WG_ROWS) == 8 and L.vqw_xent_ws_bytes(XE_WG_ROWS + 1) == 16
    assert L.vqw_xent_ws_bytes(XE_FOLD_LANES * XE_WG_ROWS + 1) == (XE_FOLD_LANES + 1) * 8


def test_cross_entropy_row_far_off_zero():
    """1e4 added to every logit of one row: exp overflows without the row maximum; the loss stays finite and passes the gate."""
    _xent_check(5, 100, seed=7, offset_row=3)


def test_cross_entropy_leading_shape():
    from hipops import ops
    z, t, _ = _xent_inputs(6, 11, 2)
    flat = ops.cross_entropy(_dev(z), t.to(DEV), reduction="none")
    shaped = ops.cross_entropy(_dev(z).view(2, 3, 11), t.to(DEV).view(2, 3), reduction="none")
    assert shaped.shape == (2, 3) and torch.equal(shaped.reshape(-1), flat)
    assert torch.equal(ops.cross_entropy(_dev(z).view(2, 3, 11), t.to(DEV).view(2, 3)), ops.cross_entropy(_dev(z), t.to(DEV)))


def test_cross_entropy_target_out_of_range_is_nan_in_that_row_only():
    from hipops import ops
    z, t, gloss = _xent_inputs(5, 100, 3)
    t[2] = 100
    zd = _dev(z).requires_grad_(True)
    loss = ops.cross_entropy(zd, t.to(DEV), reduction="none")
    loss.backward(_dev(gloss))
    torch.cuda.synchronize()
    bad = torch.arange(5) == 2
    assert bool(torch.isnan(loss.detach().cpu()[bad]).all()) and bool(torch.isfinite(loss.detach().cpu()[~bad]).all())
    g = zd.grad.cpu()
    assert bool(torch.isnan(g[bad]).all()) and bool(torch.isfinite(g[~bad]).all())
    assert bool(torch.isnan(ops.cross_entropy(zd.detach(), t.to(DEV))))


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("V,k", G.SAMPLE_CASES)
def test_sample_topk(V, k):
    from hipops import ops
    for temp in G.SAMPLE_TEMPS:
        logits, u = G.sample_inputs(V, k, temp)
        p64, dist, kept = G.sample_ref(logits, u, temp, k)
        got = ops.sample_topk(_dev(logits), _dev(u), temp, k).cpu()
        assert got.dtype == torch.long and got.shape == (G.SAMPLE_B,) and bool(((got >= 0) & (got < V)).all())
        clear = dist > G.SAMPLE_CLEAR
        print("sample_topk V%d k%d temperature %.1f: %d of %d rows unclear, %d differ from float64, %d of them clear" % (
            V, k, temp, int((~clear).sum()), G.SAMPLE_B, int((got != p64).sum()), int((got != p64)[clear].sum())))
        assert bool(kept.gather(1, got[:, None]).all()), "an index outside the float64 kept set"
        assert int((~clear).sum()) <= G.SAMPLE_UNCLEAR_CAP * G.SAMPLE_B
        assert torch.equal(got[clear], p64[clear])
        if k == 1:          # the kept set is the row's maxima (ties are all kept): a maximum for any u, the argmax where it is unique
            top = logits.max(dim=1, keepdim=True).values
            assert bool((logits.gather(1, got[:, None]) == top).all())
            unique = (logits == top).sum(dim=1) == 1
            assert torch.equal(got[unique], logits.argmax(dim=1)[unique])
        ar = torch.arange(V)
        first = torch.where(kept, ar, torch.full_like(ar, V)).min(dim=1).values
        got0 = ops.sample_topk(_dev(logits), torch.zeros(G.SAMPLE_B, device=DEV), temp, k).cpu()
        assert torch.equal(got0, first), "u = 0 gives the first kept index"
        u1 = torch.full((G.SAMPLE_B,), float(np.nextafter(np.float32(1), np.float32(0))))
        got1 = ops.sample_topk(_dev(logits), _dev(u1), temp, k).cpu()
        assert bool(kept.gather(1, got1[:, None]).all()), "u = the largest float below 1 gives a kept index"
        assert torch.equal(got, ops.sample_topk(_dev(logits), _dev(u), temp, k).cpu())


def test_sample_topk_none_is_no_filter():
    from hipops import ops
    logits, u = G.sample_inputs(100, 0, 1.0)
    assert torch.equal(ops.sample_topk(_dev(logits), _dev(u), 1.0, None), ops.sample_topk(_dev(logits), _dev(u), 1.0, 100))


# ------------------------------------------------------------------------------------------------ the model on the fixtures
_cache = {}


def _case(golden, name):
    """The fixture, its state and inputs, the float64 truth and the three fp32 evaluations of the restatement: computed once."""
    if name not in _cache:
        g = golden("mingpt_gpt_%s.npz" % name)
        state = {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}
        idx, target = g.t(name + "/in"), g.t(name + "/target")
        prefix = g.t(name + "/prefix") if name + "/prefix" in g.files else None
        logits64, loss64, truth = G.grads_ref(name, state, idx, target, prefix, torch.float64)
        variants = [G.grads_ref(name, state, idx, target, prefix, torch.float32, v)[2] for v in G.VARIANTS]
        _cache[name] = (g, state, idx, target, prefix, logits64, loss64, truth, variants)
    return _cache[name]


def _model(name, state):
    import networks
    m = networks.GPT(**G.gpt_kwargs(name))
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_gpt_fixture(golden, name):
    from hipops import ops
    g, state, idx, target, prefix, logits64, loss64, truth, variants = _case(golden, name)
    m = _model(name, state).train()
    pd = None if prefix is None else _dev(prefix).requires_grad_(True)
    logits = m(idx.to(DEV), embeddings=pd)
    loss = ops.cross_entropy(logits, target.to(DEV))
    loss.backward()
    ops.join_streams()
    torch.cuda.synchronize()
    assert logits.shape == logits64.shape and loss.shape == ()
    logits, loss = logits.detach(), loss.detach()
    sp = float(g[name + "/spread.out"])
    print("%s logits: %.3e from float64 (fixture spread %.1e)" % (name, rel_err(logits, logits64), sp))
    lsp = float(np.abs(g[name + "/loss32"].astype(np.float64) - float(g[name + "/loss64"])).max())
    print("%s loss: %.9g, float64 %.12g: %.3e apart (the reference's fp32 evaluations at most %.3e)" % (
        name, float(loss), float(loss64), abs(float(loss) - float(loss64)), lsp))
    test = {k: p.grad for k, p in m.named_parameters()}
    if pd is not None:
        test["input"] = pd.grad
    assert set(test) == set(truth)
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
    grad_gate(truth, variants, test, what=name)
    _fixture_gate(g, name, test)
    # the names both gates skip - analytically zero gradients (k.bias) - hold rounding noise only
    gmax = max(float(t.norm()) for t in truth.values())
    dead = [k for k in truth if k not in set(str(n) for n in g[name + "/live"])]
    assert dead == ["blocks.%d.att.k.bias" % i for i in range(G.CASES[name][2])]
    for k in dead:
        print("%s grad %s: analytically zero, norm %.3e (largest gradient %.3e)" % (name, k, float(test[k].norm()), gmax))
        assert float(test[k].norm()) < 1e-4 * gmax, k
    assert_close(logits, logits64, 2.0 * sp, name + " logits")
    assert abs(float(loss) - float(loss64)) <= 2.0 * lsp, "%s loss %.9g vs float64 %.12g: beyond 2 x %.3e" % (name, float(loss), float(loss64), lsp)


def test_gpt_cached_route(golden):
    """One forward_with_past call on the first CACHED_PROMPT tokens, then one-token calls behind the growing past: the logits at
    every position against the fixture's full-sequence eval logits."""
    name = G.CACHED_CASE
    g, state, idx, _, prefix, _, _, _, _ = _case(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    full, sp = g.t(name + "/eval_logits"), float(g[name + "/spread.eval_logits"])
    m = _model(name, state).eval()
    n0 = G.CACHED_PROMPT - Te
    with torch.no_grad():
        logits, present = m.forward_with_past(idx[:, :n0].to(DEV), embeddings=_dev(prefix))
        assert logits.shape == (B, G.CACHED_PROMPT, V) and present.shape == (nl, 2, B, nh, G.CACHED_PROMPT, E // nh)
        out, past = [logits], [present]
        for t in range(n0, Ti):
            logits, present = m.forward_with_past(idx[:, t:t + 1].to(DEV), past=past, past_length=Te + t)
            assert logits.shape == (B, 1, V) and present.shape == (nl, 2, B, nh, 1, E // nh)
            out.append(logits)
            past.append(present)
        fwd = m(idx.to(DEV), embeddings=_dev(prefix))
    torch.cuda.synchronize()
    got = torch.cat(out, dim=1)
    assert got.shape == full.shape == fwd.shape
    worst = max(rel_err(got[:, t], full[:, t]) for t in range(Te + Ti))
    print("%s cached route: %.3e from the float64 full-sequence logits, worst position %.3e; forward() in eval mode %.3e (fixture spread %.1e)" % (
        name, rel_err(got, full), worst, rel_err(fwd, full), sp))
    assert_close(fwd, full, 2.0 * sp, name + " eval forward")
    for t in range(Te + Ti):
        assert_close(got[:, t], full[:, t], 2.0 * sp, "%s cached route, position %d" % (name, t))


def test_gpt_sample_is_reproducible_and_equals_full_recomputation(golden):
    from hipops import ops
    name, steps, temp, top_k = "gpt64", 12, 1.0, 10
    g, state, idx, _, _, _, _, _, _ = _case(golden, name)
    m = _model(name, state).train()          # sample() switches to eval mode and back
    n0 = 6          # at least n_unmasked = 5 tokens: behind a shorter prompt the cached route cannot see what the unmasked corner shows
    prompt = idx[:, :n0].to(DEV)
    a = m.sample(prompt, steps, temperature=temp, top_k=top_k, generator=torch.Generator(device=DEV).manual_seed(5))
    b = m.sample(prompt, steps, temperature=temp, top_k=top_k, generator=torch.Generator(device=DEV).manual_seed(5))
    torch.cuda.synchronize()
    assert m.training and a.shape == (2, n0 + steps) and a.dtype == torch.long and torch.equal(a, b) and torch.equal(a[:, :n0], prompt)
    assert bool(((a >= 0) & (a < 100)).all())
    # the same uniforms, full recomputation: step k sees the tokens sample() produced so far
    gen = torch.Generator(device=DEV).manual_seed(5)
    m.eval()
    clear_n = 0
    with torch.no_grad():
        for k in range(steps):
            logits = m(a[:, :n0 + k])[:, -1, :]
            u = torch.rand(2, generator=gen, device=DEV)
            pick = ops.sample_topk(logits, u, temp, top_k)
            _, dist, _ = G.sample_ref(logits.cpu(), u.cpu(), temp, top_k)
            clear = dist > G.SAMPLE_CLEAR
            clear_n += int(clear.sum())
            assert torch.equal(pick.cpu()[clear], a[:, n0 + k].cpu()[clear]), "step %d" % k
    print("%s sample: %d of %d steps clear, all equal to the full recomputation" % (name, clear_n, 2 * steps))
    assert clear_n >= steps
