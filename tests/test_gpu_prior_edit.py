"""GPU tests of editing with the code prior: ops.sample_filtered and ops.paste_cells against their float64 / plain-torch restatements
(tests/prior_edit_ref.py), GPT.generate_masked on prior_ref's p64 and p96 models, PriorTrainer.token_nll / edit on TINY_VQGAN with
the p64 GPT, and the launcher's `-p -m edit`.  Run with `pytest -m gpu` on an MI355X.

Tolerances.  Sampling: the project's rule (tests/test_gpu_mingpt_gpt.py) - every returned index lies in the float64 kept set; it
equals the float64 restatement's on every clear row (gpt_ref.SAMPLE_CLEAR from both decisions: the CDF boundaries and the nucleus
threshold), and at most gpt_ref.SAMPLE_UNCLEAR_CAP of a case's rows may be unclear (on the CPU: at most 1 row in 64 on every
case).  logp: the gate that holds ops.cross_entropy's per-row loss (twice the fp32 restatement's distance from float64), and within
one fp32 ulp of -ops.cross_entropy: both round one double sum of the same fp32 terms, associated differently.  paste_cells is a
copy: bit-equal.  generate_masked's logp: the same gate against the float64 full forward, the fp32 side being gpt_ref in fp32."""
import os

import numpy as np
import pytest
import torch

from helpers import rel_err
from run_helpers import read_csv, run_launcher, write_config
import gpt_ref as G
import prior_ref as P
import prior_edit_ref as R
from test_gpu_mingpt_blocks import _dev, _gate          # the gate rule, written once

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ sample_filtered
def _one_ulp(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert bool((np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()), what


def _check_sample(V, k, temp, top_p):
    from hipops import ops
    logits, u = G.sample_inputs(V, k, temp)
    p64, lp64, clear, kept = R.sample_filtered_ref(logits, u, None, temp, k, top_p)
    got, logp = ops.sample_filtered(_dev(logits), _dev(u), None, temp, k, top_p)
    xe = -ops.cross_entropy(_dev(logits), got, reduction="none")
    got, logp = got.cpu(), logp.cpu()
    assert got.dtype == torch.long and got.shape == (G.SAMPLE_B,) and logp.dtype == torch.float32 and logp.shape == (G.SAMPLE_B,)
    print("sample_filtered V%d k%d temperature %.1f top_p %g: %d of %d rows unclear, %d differ from float64, %d of them clear" % (
        V, k, temp, top_p, int((~clear).sum()), G.SAMPLE_B, int((got != p64).sum()), int((got != p64)[clear].sum())))
    assert bool(((got >= 0) & (got < V)).all()) and bool(kept.gather(1, got[:, None]).all()), "an index outside the float64 kept set"
    assert int((~clear).sum()) <= G.SAMPLE_UNCLEAR_CAP * G.SAMPLE_B
    assert torch.equal(got[clear], p64[clear])
    what = "sample_filtered V%d k%d T%.1f p%g logp" % (V, k, temp, top_p)
    if V > 1:
        _gate(logp, R.logp_ref(logits, got), R.logp_ref(logits, got, torch.float32), what)
    else:
        assert not bool(logp.any()), "one class: log 1"
    _one_ulp(logp, xe, what + " against -ops.cross_entropy")
    again, logp2 = ops.sample_filtered(_dev(logits), _dev(u), None, temp, k, top_p)
    assert torch.equal(again.cpu(), got) and torch.equal(logp2.cpu(), logp), "two runs differ"
    if top_p >= 1:          # the hard pin
        assert torch.equal(got, ops.sample_topk(_dev(logits), _dev(u), temp, k).cpu())
        assert torch.equal(got, ops.sample_filtered(_dev(logits), _dev(u), None, temp, k, None, return_logp=False)[0].cpu())
    return logits, got, kept


@pytest.mark.parametrize("V,k", G.SAMPLE_CASES)
def test_sample_filtered_against_float64(V, k):
    for temp in G.SAMPLE_TEMPS:
        for top_p in R.TOP_PS:
            _check_sample(V, k, temp, top_p)


def test_sample_filtered_tiny_top_p_keeps_the_maxima():
    logits, got, kept = _check_sample(100, 0, 1.0, R.TINY_TOP_P)
    top = logits.max(dim=1, keepdim=True).values
    assert torch.equal(kept, logits == top) and bool((logits.gather(1, got[:, None]) == top).all())


@pytest.mark.parametrize("V,k,temp,top_p", [(100, 0, 1.0, 0.9), (100, 10, 2.0, 0.3), (1000, 100, 0.5, 0.9)])
def test_sample_filtered_kept_set_by_a_sweep_of_u(V, k, temp, top_p):
    """One row of logits in every workgroup, u swept over [0, 1): the set of returned indices IS the float64 kept set - every
    kept entry's probability is more than two steps of the sweep (asserted on the reference first)."""
    from hipops import ops
    n = 8192
    logits, _ = G.sample_inputs(V, k, temp)
    kept, margin = R.filter_ref(logits, temp, k, top_p)
    row = int(torch.argmax((margin > G.SAMPLE_CLEAR).int()))
    assert float(margin[row]) > G.SAMPLE_CLEAR
    s = logits[row].double() / temp
    p = torch.where(kept[row], torch.exp(s - s.max()), torch.zeros_like(s))
    assert float(p[kept[row]].min() / p.sum()) > 2.0 / n
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    got, _ = ops.sample_filtered(_dev(logits[row:row + 1].expand(n, V)), _dev(u), torch.full((n,), -1, dtype=torch.long, device=DEV), temp, k, top_p)
    seen = torch.zeros(V, dtype=torch.bool)
    seen[got.cpu()] = True
    assert torch.equal(seen, kept[row]), "kept set: %d entries seen, %d in float64" % (int(seen.sum()), int(kept[row].sum()))
    assert bool((got.cpu()[1:] >= got.cpu()[:-1]).all()), "the inverse CDF runs in index order"


def test_sample_filtered_logp_does_not_depend_on_the_filter():
    from hipops import ops
    logits, u = G.sample_inputs(1000, 100, 1.0)
    forced = torch.randint(0, 1000, (G.SAMPLE_B,), generator=torch.Generator().manual_seed(3))
    base = ops.sample_filtered(_dev(logits), _dev(u), forced.to(DEV))[1]
    for temp, k, top_p in ((0.5, 0, None), (2.0, 10, 0.3), (1.0, 100, 0.9), (1.0, 1, 1e-6)):
        tok, lp = ops.sample_filtered(_dev(logits), _dev(u), forced.to(DEV), temp, k, top_p)
        assert torch.equal(tok.cpu(), forced) and torch.equal(lp, base), (temp, k, top_p)
    _gate(base.cpu(), R.logp_ref(logits, forced), R.logp_ref(logits, forced, torch.float32), "forced logp V1000")


@pytest.mark.parametrize("V,k,top_p", [(100, 10, 0.9), (1000, 0, None), (16384, 100, 0.3)])
def test_sample_filtered_forced_rows(V, k, top_p):
    from hipops import ops
    temp = 1.0
    logits, u = G.sample_inputs(V, k, temp)
    B = G.SAMPLE_B
    g = torch.Generator().manual_seed(V + k)
    tok = torch.randint(0, V, (B,), generator=g)
    free = ops.sample_filtered(_dev(logits), _dev(u), None, temp, k, top_p)
    nan_u = torch.full((B,), float("nan"))
    # all forced: the tokens come back, u is not read
    got, lp = ops.sample_filtered(_dev(logits), _dev(nan_u), tok.to(DEV), temp, k, top_p)
    assert torch.equal(got.cpu(), tok)
    _gate(lp.cpu(), R.logp_ref(logits, tok), R.logp_ref(logits, tok, torch.float32), "all forced V%d logp" % V)
    # alternating: a forced row takes its token whatever u holds, a free row draws what it draws without `forced`
    even = torch.arange(B) % 2 == 0
    forced = torch.where(even, tok, torch.full_like(tok, -1))
    got, lp = ops.sample_filtered(_dev(logits), _dev(torch.where(even, nan_u, u)), forced.to(DEV), temp, k, top_p)
    assert torch.equal(got.cpu()[even], tok[even]) and torch.equal(got[~even.to(DEV)], free[0][~even.to(DEV)])
    assert torch.equal(lp[~even.to(DEV)], free[1][~even.to(DEV)]) and bool(torch.isfinite(lp).all())
    # forced = -7 draws; forced = V (and beyond) draws as well, stays inside [0, V) and marks its logp
    forced = torch.full((B,), -7, dtype=torch.long)
    forced[1::4] = V
    forced[3::4] = V + 12345
    got, lp = ops.sample_filtered(_dev(logits), _dev(u), forced.to(DEV), temp, k, top_p)
    bad = (forced >= V).to(DEV)
    assert torch.equal(got, free[0]) and bool(((got >= 0) & (got < V)).all())
    assert bool(torch.isnan(lp[bad]).all()) and torch.equal(lp[~bad], free[1][~bad])


def test_sample_filtered_refusals():
    from hipops import ops
    z, u = torch.zeros(2, 10, device=DEV), torch.zeros(2, device=DEV)
    for kw, msg in ((dict(top_p=0.0), "top_p=0 must be positive"), (dict(top_p=-0.5), "top_p"), (dict(temperature=0.0), "temperature=0 must be positive"),
                    (dict(top_k=-1), "top_k=-1")):
        with pytest.raises(RuntimeError, match=msg):
            ops.sample_filtered(z, u, **kw)
    with pytest.raises(RuntimeError, match="V=0 must satisfy 1 <= V <= 65536"):
        ops.sample_filtered(torch.zeros(2, 0, device=DEV), u)
    with pytest.raises(RuntimeError, match="V=65537 must satisfy"):
        ops.sample_filtered(torch.zeros(1, 65537, device=DEV), u[:1])
    with pytest.raises(RuntimeError, match="logits .B, V. and u .B,. expected"):
        ops.sample_filtered(z, u[:1])
    with pytest.raises(RuntimeError, match="forced"):
        ops.sample_filtered(z, u, torch.zeros(3, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError, match="torch.long"):
        ops.sample_filtered(z, u, torch.zeros(2, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------ paste_cells
# (B, C, H, W), (h, w): equal factors of 2, one cell per 2 x 2 pixels at 16 x 16 cells, unequal factors (4, 2) with 3 channels, a
# factor of 32, widths that are no multiple of 4 (one and three channels: the one-float route and the 16-byte route of fx C = 12)
PASTE_CASES = [((2, 1, 8, 8), (4, 4)), ((1, 1, 32, 32), (16, 16)), ((2, 3, 8, 16), (2, 8)), ((1, 1, 64, 64), (2, 2)),
               ((2, 1, 4, 6), (2, 3)), ((1, 3, 4, 6), (2, 3)), ((1, 3, 6, 12), (3, 3)), ((3, 4, 4, 3), (4, 3))]


@pytest.mark.parametrize("shape,cells", PASTE_CASES)
def test_paste_cells_bit_equal(shape, cells):
    from hipops import ops
    g = torch.Generator().manual_seed(sum(shape) + cells[0])
    image, edit = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    masks = [torch.randint(0, 2, (shape[0],) + cells, generator=g, dtype=torch.uint8), torch.zeros((shape[0],) + cells, dtype=torch.uint8),
             torch.full((shape[0],) + cells, 1, dtype=torch.uint8), torch.randint(0, 2, (shape[0],) + cells, generator=g, dtype=torch.uint8) * 255]
    for m in masks:
        want = R.paste_ref(image, edit, m)
        for fmt in (torch.contiguous_format, torch.channels_last):
            got = ops.paste_cells(image.to(DEV).contiguous(memory_format=fmt), edit.to(DEV).contiguous(memory_format=fmt), m.to(DEV))
            assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert torch.equal(R.paste_ref(image, edit, masks[1]), image) and torch.equal(R.paste_ref(image, edit, masks[2]), edit)


def test_paste_cells_refusals():
    from hipops import ops
    x = torch.zeros(2, 1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of the cell grid 3 x 4"):
        ops.paste_cells(x, x, torch.zeros(2, 3, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="multiples of the cell grid 4 x 3"):
        ops.paste_cells(x, x, torch.zeros(2, 4, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="torch.uint8"):
        ops.paste_cells(x, x, torch.zeros(2, 4, 4, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="B = 2"):
        ops.paste_cells(x, x, torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.paste_cells(x, x[:, :, :4], torch.zeros(2, 4, 4, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ generate_masked
_models = {}


def _gpt(name):
    """prior_ref's model (eval mode, on the device), its float64 state and the case's ids: built once, shared, never changed"""
    if name not in _models:
        from networks import GPT
        seed = P.SEEDS[name]
        torch.manual_seed(seed)
        m = G.init_gpt_(GPT(**P.gpt_kwargs(name)), seed).to(DEV).eval()
        _models[name] = (m, R.state64(m), P.case_ids(name, seed))
    return _models[name]


def _start(B):
    return torch.full((B, 1), P.SOS, dtype=torch.long)


class _Spy:
    """Counts what generate_masked asks of the model: the prefill's length, the decode steps, the cache it built."""

    def __init__(self, monkeypatch, m):
        self.prefill_len, self.steps, self.cache = [], 0, None
        prefill, step, new_cache = m.prefill, m.decode_step, m.new_cache

        def spy_prefill(idx, cache, embeddings=None):
            self.prefill_len.append(idx.shape[1])
            return prefill(idx, cache, embeddings)

        def spy_step(idx, cache):
            self.steps += 1
            return step(idx, cache)

        def spy_cache(*a, **kw):
            self.cache = new_cache(*a, **kw)
            return self.cache

        monkeypatch.setattr(m, "prefill", spy_prefill)
        monkeypatch.setattr(m, "decode_step", spy_step)
        monkeypatch.setattr(m, "new_cache", spy_cache)


def test_generate_masked_all_resampled_is_generate():
    """Every position drawn, no top_p, given uniforms: GPT.generate's tokens (block_size = 16 lets generate append 15 tokens to
    the start token).  On p64 only: p96's n_unmasked = 3 refuses j0 = 0 (test_generate_masked_unmasked_corner_needs_a_kept_prefix)."""
    name = "p64"
    m, st, ids = _gpt(name)
    B, S, temp, k = 2, 15, 1.0, 8
    u = torch.rand(S, B, generator=torch.Generator().manual_seed(5))
    want = m.generate(_start(B).to(DEV), S, temperature=temp, top_k=k, uniforms=u)[:, 1:]
    tokens, logp = m.generate_masked(_start(B).to(DEV), torch.zeros_like(want), np.ones(S, dtype=bool), temperature=temp, top_k=k, uniforms=u)
    assert tokens.dtype == torch.long and logp.dtype == torch.float32 and tokens.shape == logp.shape == (B, S)
    assert torch.equal(tokens, want)
    assert torch.equal(tokens, m.generate_masked(_start(B).to(DEV), want, np.ones((B, S), dtype=bool), temp, k, 1.0, uniforms=u.to(DEV))[0])
    _gate(logp.cpu(), R.token_logp_ref(st, m.config.n_layer, m.config.n_head, _start(B), tokens.cpu()),
          R.token_logp_ref(st, m.config.n_layer, m.config.n_head, _start(B), tokens.cpu(), torch.float32), name + " logp of the drawn tokens")


@pytest.mark.parametrize("name", ["p64", "p96"])
def test_generate_masked_nothing_resampled_scores_the_sequence(monkeypatch, name):
    m, st, ids = _gpt(name)
    B, S = ids.shape
    spy = _Spy(monkeypatch, m)
    tokens, logp = m.generate_masked(_start(B).to(DEV), ids.to(DEV), np.zeros(S, dtype=bool), temperature=0.7, top_k=3, top_p=0.5)
    assert torch.equal(tokens.cpu(), ids) and spy.prefill_len == [S] and spy.steps == 0 and spy.cache.length == S
    nl, nh = m.config.n_layer, m.config.n_head
    _gate(logp.cpu(), R.token_logp_ref(st, nl, nh, _start(B), ids), R.token_logp_ref(st, nl, nh, _start(B), ids, torch.float32), name + " logp, prefill only")
    # only the last code of row 0 is redrawn: the same prefill, one sample_filtered launch, no decode step - the last token is
    # not fed back - and everything else as before, bit for bit
    late = np.zeros((B, S), dtype=bool)
    late[0, S - 1] = True
    spy = _Spy(monkeypatch, m)
    tokens, logp2 = m.generate_masked(_start(B).to(DEV), ids.to(DEV), late, generator=torch.Generator(device=DEV).manual_seed(1))
    assert spy.prefill_len == [S] and spy.steps == 0 and torch.equal(tokens[:, :S - 1].cpu(), ids[:, :S - 1]) and torch.equal(tokens[1].cpu(), ids[1])
    assert torch.equal(logp2[:, :S - 1], logp[:, :S - 1])


def test_generate_masked_window_in_one_row(monkeypatch):
    name = "p64"
    m, st, ids = _gpt(name)
    B, S = ids.shape
    lo, hi, temp, k, top_p = 6, 10, 1.0, 8, 0.9
    resample = np.zeros((B, S), dtype=bool)
    resample[0, lo:hi] = True
    spy = _Spy(monkeypatch, m)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)  # noqa: E731
    tokens, logp = m.generate_masked(_start(B).to(DEV), ids.to(DEV), resample, temperature=temp, top_k=k, top_p=top_p, generator=gen())
    # the plan: the start token and the 6 kept codes in one prefill, then a decode step for each of the positions 6..14
    assert spy.prefill_len == [1 + lo] and spy.steps == S - 1 - lo and spy.cache.length == spy.cache.capacity == S
    keep = torch.from_numpy(~resample)
    assert torch.equal(tokens.cpu()[keep], ids[keep])
    nl, nh = m.config.n_layer, m.config.n_head
    z = R.teacher_forced_logits(st, nl, nh, _start(B), tokens.cpu())
    for pos in range(lo, hi):          # the float64 decisions are clear by far more than the fp32 logits' distance from them
        top = torch.sort(z[0, pos] / temp, descending=True).values
        kept, margin = R.filter_ref(z[:1, pos], temp, k, top_p)
        assert float(top[k - 1] - top[k]) > 1e-4 and float(margin[0]) > 1e-4
        assert bool(kept[0, tokens[0, pos]]), "position %d: token %d outside the float64 kept set" % (pos, int(tokens[0, pos]))
    _gate(logp.cpu(), R.token_logp_ref(st, nl, nh, _start(B), tokens.cpu()), R.token_logp_ref(st, nl, nh, _start(B), tokens.cpu(), torch.float32),
          name + " logp, kept and drawn")
    again = m.generate_masked(_start(B).to(DEV), ids.to(DEV), resample, temperature=temp, top_k=k, top_p=top_p, generator=gen())
    assert torch.equal(again[0], tokens) and torch.equal(again[1], logp), "same seed, same bits"
    other = m.generate_masked(_start(B).to(DEV), ids.to(DEV), resample, temperature=temp, top_k=k, top_p=top_p,
                              generator=torch.Generator(device=DEV).manual_seed(12))
    assert not torch.equal(other[0], tokens)


def test_generate_masked_unmasked_corner_needs_a_kept_prefix():
    m, st, ids = _gpt("p96")
    B, S = ids.shape
    assert m.config.n_unmasked == 3
    for j0 in (0, 1):
        with pytest.raises(RuntimeError, match="n_unmasked=3 exceeds the %d tokens of the prefill" % (1 + j0)):
            m.generate_masked(_start(B).to(DEV), ids.to(DEV), np.arange(S) >= j0)
    tokens, logp = m.generate_masked(_start(B).to(DEV), ids.to(DEV), np.arange(S) >= 2, top_k=8, generator=torch.Generator(device=DEV).manual_seed(2))
    assert torch.equal(tokens[:, :2].cpu(), ids[:, :2]) and bool(((tokens >= 0) & (tokens < 64)).all())
    # three tokens under the mask's unmasked corner, the steps behind them causal: the full forward on the result
    nl, nh = m.config.n_layer, m.config.n_head
    _gate(logp.cpu(), R.token_logp_ref(st, nl, nh, _start(B), tokens.cpu()), R.token_logp_ref(st, nl, nh, _start(B), tokens.cpu(), torch.float32),
          "p96 logp behind a kept prefix of 2")


# ------------------------------------------------------------------------------------------------ token_nll and edit
_tr = {}


def _trainer():
    if "tr" not in _tr:
        from networks import GPT, VQGAN
        from trainers import PriorTrainer
        torch.manual_seed(77)
        vqgan = VQGAN(**P.TINY_VQGAN)
        seed = P.SEEDS["p64"]
        torch.manual_seed(seed)
        gpt = G.init_gpt_(GPT(**P.gpt_kwargs("p64")), seed)
        _tr["tr"] = PriorTrainer(vqgan, gpt, device=DEV)
        _tr["image"] = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    return _tr["tr"], _tr["image"]


def _gen(seed=9):
    return torch.Generator(device=DEV).manual_seed(seed)


def test_token_nll_is_the_validation_loss_per_code():
    tr, image = _trainer()
    nll = tr.token_nll({"image": image})
    assert nll.shape == (2, 4, 4) and nll.dtype == torch.float32 and tr.gpt.training
    loss = float(tr.validation_step({"image": image})["loss"])
    own = float(nll.double().mean())
    assert abs(loss - own) <= float(np.spacing(np.float32(abs(own))))          # test_cross_entropy's rule for the mean
    ids = tr.codes({"image": image})
    assert torch.equal(tr.token_nll({"ids": ids}), nll)


def test_edit_empty_mask_returns_the_slice_with_its_own_score():
    tr, image = _trainer()
    out = tr.edit({"image": image}, mask=np.zeros((8, 8), dtype=bool), n_candidates=2, generator=_gen())
    ids = tr.codes({"image": image})
    assert torch.equal(out["ids"], ids) and torch.equal(out["source_ids"], ids) and not bool(out["cellmask"].any())
    assert torch.equal(out["candidates"], ids[:, None].expand(2, 2, 16)) and out["scores"].dtype == torch.float64
    # the prefill's logits and the full forward's are the same fp32 evaluation up to the route's rounding (1e-6 relative on these
    # models: test_generate_masked_nothing_resampled's figures); a sum of 16 such terms is held to ten times that
    want = -tr.token_nll({"image": image}).double().sum((1, 2))
    assert torch.allclose(out["scores"], want[:, None].expand(2, 2), rtol=1e-5, atol=0)
    assert torch.equal(out["edit"], out["recon"]) and torch.equal(out["composite"].contiguous(), image)


def test_edit_selectors_agree_and_the_best_candidate_wins():
    tr, image = _trainer()
    px = np.zeros((8, 8), dtype=bool)
    px[5, 2] = True
    one = tr.edit({"image": image}, mask=px, n_candidates=1, generator=_gen())
    want = np.zeros((2, 4, 4), dtype=np.uint8)
    want[:, 2, 1] = 1
    assert np.array_equal(one["cellmask"].cpu().numpy(), want), "one pixel selects exactly its cell"

    kw = dict(n_candidates=4, temperature=1.0, top_k=16, top_p=0.95)
    by_box = tr.edit({"image": image}, box=(2, 6, 0, 4), generator=_gen(), **kw)
    cells = np.zeros((4, 4), dtype=bool)
    cells[1:3, 0:2] = True
    pixels = np.zeros((2, 8, 8), dtype=bool)          # one pixel in each of the four cells is enough
    pixels[:, 3, 1] = pixels[:, 2, 3] = pixels[:, 4, 0] = pixels[:, 5, 2] = True
    for other in (tr.edit({"image": image}, mask=cells, generator=_gen(), **kw), tr.edit({"image": image}, mask=pixels, generator=_gen(), **kw),
                  tr.edit({"image": image}, mask=np.repeat(cells[None], 2, 0).astype(np.uint8), generator=_gen(), **kw)):
        for key in by_box:
            assert torch.equal(by_box[key], other[key]), key
    nll = tr.token_nll({"image": image})
    thr = float(nll.median())
    by_nll = tr.edit({"image": image}, nll_threshold=thr, generator=_gen(), **kw)
    by_mask = tr.edit({"image": image}, mask=(nll > thr).cpu().numpy(), generator=_gen(), **kw)
    assert 0 < int(by_nll["cellmask"].sum()) < 32
    for key in by_nll:
        assert torch.equal(by_nll[key], by_mask[key]), key

    out, ids = by_box, tr.codes({"image": image})
    assert out["candidates"].shape == (2, 4, 16) and out["scores"].shape == (2, 4) and out["best"].shape == (2,)
    assert np.array_equal(out["cellmask"].cpu().numpy(), np.repeat(cells[None], 2, 0).astype(np.uint8))
    keep = ~torch.from_numpy(cells.reshape(-1)).to(DEV)
    assert torch.equal(out["candidates"][:, :, keep], ids[:, None, keep].expand(2, 4, int(keep.sum())))
    assert len({tuple(c.tolist()) for c in out["candidates"][0]}) > 1, "the candidates differ"
    for b in range(2):
        j = int(out["best"][b])
        assert float(out["scores"][b, j]) == float(out["scores"][b].max()) and torch.equal(out["ids"][b], out["candidates"][b, j])
    assert torch.equal(out["recon"], tr.vqgan.decode_from_ids(ids, 4, 4)) and torch.equal(out["edit"], tr.vqgan.decode_from_ids(out["ids"], 4, 4))
    assert torch.equal(out["composite"].cpu(), R.paste_ref(image.cpu(), out["edit"].cpu(), out["cellmask"].cpu()))
    inside = out["cellmask"].bool().repeat_interleave(2, 1).repeat_interleave(2, 2)[:, None]
    assert torch.equal(out["composite"][~inside], image[~inside]) and torch.equal(out["composite"][inside], out["edit"][inside])
    # a score is the log-probability of the whole candidate: kept codes behind the region included
    st = R.state64(tr.gpt)
    lp = R.token_logp_ref(st, 2, 2, _start(8), out["candidates"].reshape(8, 16).cpu())
    assert rel_err(out["scores"].reshape(-1).cpu(), lp.sum(1)) < 1e-5
    # the {'ids'} form: no picture to paste into
    from_ids = tr.edit({"ids": ids}, box=(2, 6, 0, 4), generator=_gen(), **kw)
    assert "composite" not in from_ids and torch.equal(from_ids["ids"], out["ids"]) and torch.equal(from_ids["edit"], out["edit"])
    assert tr.gpt.training


def test_edit_candidate_0_does_not_depend_on_n_candidates():
    """By construction only the UNIFORMS of candidate 0 are the same (one torch.rand call per candidate, candidate 0 first); its
    codes follow wherever no draw sits within the fp32 noise of a CDF boundary between the two batch sizes - none does here."""
    tr, image = _trainer()
    kw = dict(box=(0, 8, 0, 8), temperature=1.0, top_k=16)
    one = tr.edit({"image": image}, n_candidates=1, generator=_gen(4), **kw)
    four = tr.edit({"image": image}, n_candidates=4, generator=_gen(4), **kw)
    assert torch.equal(one["candidates"][:, 0], four["candidates"][:, 0])
    assert torch.allclose(one["scores"][:, 0], four["scores"][:, 0], rtol=1e-5, atol=0)
    assert not torch.equal(four["candidates"][:, 0], four["candidates"][:, 1])


def test_edit_refuses_two_selectors_or_none():
    tr, image = _trainer()
    m = np.zeros((8, 8), dtype=bool)
    for kw in (dict(), dict(mask=m, box=(0, 2, 0, 2)), dict(mask=m, nll_threshold=1.0), dict(box=(0, 2, 0, 2), nll_threshold=1.0)):
        with pytest.raises(ValueError, match="exactly one of mask, box and nll_threshold"):
            tr.edit({"image": image}, **kw)
    with pytest.raises(ValueError, match="box"):
        tr.edit({"image": image}, box=(0, 9, 0, 2))
    with pytest.raises(ValueError, match="mask of shape"):
        tr.edit({"image": image}, mask=np.zeros((3, 8), dtype=bool))


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_edits_and_a_seed_repeats_every_byte(tmp_path):
    from utils import png
    save = os.path.join(str(tmp_path), "run")
    out = run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), P.prior_run_config(save)), "-p")
    ckpt = os.path.join(save, "study", "version_0", "ckpt-epoch=0000-total_loss=0.00.ckpt")
    raw = P.prior_run_config(save, resume_checkpoint=ckpt)
    # pixel rows 24..31 are the latent rows 12..15: the prefill shortcut covers the 192 codes in front of them
    raw["edit"] = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[24, 32, 8, 24])
    cfg = write_config(os.path.join(str(tmp_path), "edit.json"), raw)
    files = {}
    for version in (1, 2):
        out = run_launcher(cfg, "-p", "-m", "edit")
        assert "Loading model from" in out and "Edited slices are saved" in out
        edir = os.path.join(save, "study", "version_%d" % version, "edit")
        assert sorted(os.listdir(edir)) == ["codes_0000.npy", "codes_0001.npy", "edit.csv", "slice_0000.png", "slice_0001.png"]
        files[version] = {f: open(os.path.join(edir, f), "rb").read() for f in os.listdir(edir)}
    assert files[1] == files[2], "the same seed writes the same bytes"
    edir = os.path.join(save, "study", "version_1", "edit")
    pixels, _ = png.load(os.path.join(edir, "slice_0000.png"))
    assert pixels.shape == (32, 4 * 32) and pixels.dtype == np.uint8
    codes = np.load(os.path.join(edir, "codes_0001.npy"))
    cells = np.zeros((16, 16), dtype=np.int64)
    cells[12:16, 4:12] = 1
    assert codes.shape == (3, 16, 16) and np.array_equal(codes[2], cells) and np.array_equal(codes[0][cells == 0], codes[1][cells == 0])
    assert codes.min() >= 0 and codes[:2].max() < 8
    # tiles: slice, reconstruction, best edit, composite - the composite is the slice above the box and the edit inside it
    assert np.array_equal(pixels[:24, 96:128], pixels[:24, 0:32]) and np.array_equal(pixels[24:, 104:120], pixels[24:, 72:88])
    header, rows = read_csv(os.path.join(edir, "edit.csv"))
    assert header == ["slice", "candidate", "score", "rank", "n_resampled"] and len(rows) == 6
    for s in range(2):
        mine = [r for r in rows if int(r[0]) == s]
        assert [int(r[1]) for r in mine] == [0, 1, 2] and sorted(int(r[3]) for r in mine) == [0, 1, 2] and all(int(r[4]) == 32 for r in mine)
        best = [r for r in mine if int(r[3]) == 0][0]
        assert float(best[2]) == max(float(r[2]) for r in mine) and all(float(r[2]) < 0 for r in mine)
