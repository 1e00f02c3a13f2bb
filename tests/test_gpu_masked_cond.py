"""The label-conditioned masked prior on the GPU: ops.embedding_cond against the compositions of the operators it replaces (bit for
bit) and against the float64 restatement of tests/masked_cond_ref.py, MaskedGPT.forward_conditioned against float64,
ConditionalMaskedPriorTrainer's step, resume, drop and learning, MaskedGPT.generate_parallel under a condition and under guidance
against the same loops composed from their operators, synthesize / edit, and the launcher.

Parity unpinned: the reference has no masked or conditional prior of this kind, so what is held is the restatement and compositions
of operators that exist without this feature.  Tolerances: the forward and the three gradients are bit-equal to the compositions;
against float64 every gradient element lies within masked_cond_ref.sum_bound, the a-priori error of a fixed-order fp32 sum of its n
terms; the logits within the bound tests/test_gpu_masked_prior.py holds MaskedGPT.forward to; the loss within that test's margin.
The tiny model is 2 layers, 2 heads, V = 16, T = 16, B = 2 at E = 64: the attention kernels refuse a head size of 16."""
import copy
import filecmp
import glob
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, rel_err
from run_helpers import read_csv, run_launcher, write_config
import gpt_ref as G
import masked_cond_ref as MC
import masked_prior_ref as R
import prior_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_ULP = 2.0 ** -23


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    """equal as bit patterns (NaN rows included)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1, 2. the operator
def _run(fn, tensors, gx):
    """fn(*leaves) -> x (or (x, eff)); backward with gx -> (x, eff or None, the leaves' gradients)"""
    leaves = [t.to(DEV).requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    x, eff = out if isinstance(out, tuple) else (out, None)
    x.backward(gx.to(DEV))
    return x.detach(), eff, [t.grad for t in leaves]


@pytest.mark.parametrize("case", MC.EMBED_CASES, ids=lambda c: "B%d-T%d-E%d-V%d-L%d-bs%s" % c)
def test_embedding_cond_forward_and_backward(case):
    from hipops import ops
    B, T, E, V, L, bs = case
    idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*case)
    idd, cid = idx.to(DEV), cidx.to(DEV)
    seen_dropped = seen_kept = False
    for p in MC.EMBED_P:
        for seed, call in MC.EMBED_KEYS:
            drop = None if p == 0 else (p, seed, call)
            what = (case, drop)
            x, eff, (gtok, gpos, gctab) = _run(lambda t, q, c: ops.embedding_cond(idd, t, q, cid, c, L, drop, return_eff=True), (tok, pos, ctab), gx)
            # the composition it replaces: two lookups and an ATen add
            if drop is None:
                cx, ceff, (ctok_g, cpos_g, ctab_g) = _run(lambda t, q, c: ops.embedding(idd, t, q) + ops.embedding_lookup(cid, c), (tok, pos, ctab), gx)
                ceff = cid
            else:
                parts = {}

                def composed(t, q, c):
                    looked, parts["eff"] = ops.embedding_lookup_drop(cid, c, L, p, seed, call, return_eff=True)
                    return ops.embedding(idd, t, q) + looked
                cx, _, (ctok_g, cpos_g, ctab_g) = _run(composed, (tok, pos, ctab), gx)
                ceff = parts["eff"]
            assert x.shape == (B, T, E) and eff.dtype == torch.long and _bits(x, cx), what
            assert torch.equal(eff, ceff), what
            assert _bits(gtok, ctok_g) and _bits(gpos, cpos_g) and _bits(gctab, ctab_g), what
            # the restatement: the forward bit for bit (fp32 additions in the kernel's order on inputs that round), the drop from integers
            rx, re = MC.embedding_cond_ref(idx, tok, pos, cidx, ctab, L, drop)
            assert torch.equal(eff.cpu(), re) and _bits(x.cpu(), rx), what
            gone = (eff.cpu() == L).all(1)
            assert torch.equal(gone, torch.from_numpy(MC.dropped(B, p, seed, call))) and bool(((eff.cpu() == L).any(1) == gone).all()), what
            if p > 0:
                seen_dropped, seen_kept = seen_dropped or bool(gone.any()), seen_kept or bool((~gone).any())
            else:
                assert not bool(gone.any()), what
            # float64: every element within the a-priori bound of a fixed-order fp32 sum of its n terms
            block = pos.shape[1]
            for name, got, (val, mag, cnt) in zip(("gtok", "gpos", "gctab"), (gtok, gpos.reshape(block, E), gctab),
                                                  MC.embedding_cond_grads(idx, re, gx, V, L + 1, block)):
                err = (got.cpu().double() - val).abs()
                bound = MC.sum_bound(mag, cnt)
                assert bool((err <= bound).all()), (what, name, float((err - bound).max()))
                assert not bool(got.cpu()[cnt == 0].any()), (what, name)          # a row nobody used: exactly 0
            if p == 0:
                assert not bool(gctab[L].any()), what          # the null row, unused
            again = _run(lambda t, q, c: ops.embedding_cond(idd, t, q, cid, c, L, drop, return_eff=True), (tok, pos, ctab), gx)
            assert _bits(again[0], x) and torch.equal(again[1], eff) and all(_bits(a, b) for a, b in zip(again[2], (gtok, gpos, gctab))), what
    assert seen_dropped and seen_kept, case          # over the three keys: a dropped sample and a kept one
    # without return_eff, without a null index: the same x
    assert _bits(ops.embedding_cond(idd, tok.to(DEV), pos.to(DEV), cid, ctab.to(DEV)), ops.embedding(idd, tok.to(DEV), pos.to(DEV)) + ctab.to(DEV)[cid])


def test_embedding_cond_out_of_range_rows_are_nan_and_leave_the_others():
    from hipops import ops
    case = MC.EMBED_CASES[1]
    B, T, E, V, L, _ = case
    idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*case)
    clean = ops.embedding_cond(idx.to(DEV), tok.to(DEV), pos.to(DEV), cidx.to(DEV), ctab.to(DEV))
    idx[0, 2], idx[2, 14], cidx[1, 4], cidx[2, 0] = V, -1, -1, L + 1          # cell_labels' -1 among them
    bad = torch.zeros(B, T, dtype=torch.bool)
    bad[0, 2] = bad[2, 14] = bad[1, 4] = bad[2, 0] = True
    x, eff, (gtok, gpos, gctab) = _run(lambda t, q, c: ops.embedding_cond(idx.to(DEV), t, q, cidx.to(DEV), c, return_eff=True), (tok, pos, ctab), gx)
    xc = x.cpu()
    assert bool(torch.isnan(xc[bad]).all()) and _bits(xc[~bad], clean.cpu()[~bad])
    assert torch.equal(eff.cpu(), cidx)
    # the walks are independent (vqw_embed_bwd's rule): an out-of-range row adds to no row of the table whose index it misses, and
    # still enters the position sums and the other table - every element within the bound of a fixed-order fp32 sum of its terms
    for name, got, (val, mag, cnt) in zip(("gtok", "gpos", "gctab"), (gtok, gpos.reshape(T, E), gctab), MC.embedding_cond_grads(idx, cidx, gx, V, L + 1, T)):
        assert bool(torch.isfinite(got).all()), name
        err = (got.cpu().double() - val).abs()
        assert bool((err <= MC.sum_bound(mag, cnt)).all()), (name, float((err - MC.sum_bound(mag, cnt)).max()))
    _, (_, _, npos), _ = MC.embedding_cond_grads(idx, cidx, gx, V, L + 1, T)
    assert npos.tolist() == [B] * T          # the position sums take every row, the NaN rows' gx included
    clean_g = _run(lambda t, q: ops.embedding(idx.clamp(0, V - 1).to(DEV), t, q), (tok, pos), gx)[2][1]
    assert _bits(gpos, clean_g)              # bit for bit ops.embedding's gpos of the same gx


def test_embedding_cond_refusals():
    from hipops import ops
    idx, tok, pos, cidx, ctab, _ = (t.to(DEV) for t in MC.embed_inputs(*MC.EMBED_CASES[1]))
    ok = lambda **kw: ops.embedding_cond(kw.get("idx", idx), kw.get("tok", tok), kw.get("pos", pos), kw.get("cidx", cidx), kw.get("ctab", ctab),  # noqa: E731
                                         kw.get("null_index"), kw.get("drop"))
    with pytest.raises(RuntimeError, match="E=6 must be a multiple of 4 with 4 <= E <= 4096"):
        ok(tok=tok[:, :6].contiguous(), pos=pos[..., :6].contiguous(), ctab=ctab[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="T = 15 exceeds block_size=14"):
        ok(pos=pos[:, :14].contiguous())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ok(ctab=torch.zeros(4 * 36 + 1, device=DEV)[1:].view(4, 36))
    with pytest.raises(RuntimeError, match=r"cidx \(B, T\) = \(3, 15\)"):
        ok(cidx=cidx[:, :14])
    with pytest.raises(RuntimeError, match="cidx must be torch.long"):
        ok(cidx=cidx.int())
    with pytest.raises(ValueError, match=r"null_index=4 must be a row of the table \(L = 4\) when p > 0"):
        ok(null_index=4, drop=(0.5, 1, 0))
    with pytest.raises(ValueError, match=r"p=1.0 must lie in \[0, 1\)"):
        ok(null_index=3, drop=(1.0, 1, 0))
    x = ok(null_index=None, drop=(0.0, 1, 0))          # p = 0 needs no null index and drops nobody
    assert _bits(x, ok())


# ------------------------------------------------------------------------------------------------ 3. the model
_cache = {}


def _tiny():
    if "m" not in _cache:
        from networks import MaskedGPT
        torch.manual_seed(711)
        _cache["m"] = G.init_gpt_(MaskedGPT(**MC.TINY), 711).to(DEV).eval()
        g = torch.Generator().manual_seed(712)
        _cache["table"] = (torch.round(torch.randn(MC.N_LABELS + 1, MC.TINY["n_embed"], generator=g) * 16) / 64).to(DEV)
    return _cache["m"], _cache["table"]


def _tiny_inputs(seed, T=16, B=MC.B_TINY):
    g = torch.Generator().manual_seed(seed)
    V = MC.TINY["vocab_size"]
    return torch.randint(0, V + 1, (B, T), generator=g), torch.randint(0, MC.N_LABELS, (B, T), generator=g)


def test_forward_conditioned(golden):
    m, table = _tiny()
    idx, ctok = _tiny_inputs(713)
    idx[0, 3] = MC.TINY["vocab_size"]          # the mask token is a row of the table
    with torch.no_grad():
        a = m.forward_conditioned(idx.to(DEV), ctok.to(DEV), table)
        plain = m(idx.to(DEV))
        zero = m.forward_conditioned(idx.to(DEV), ctok.to(DEV), torch.zeros_like(table))
        other = ctok.clone()
        other[:, 5] = (other[:, 5] + 1) % MC.N_LABELS
        b = m.forward_conditioned(idx.to(DEV), other.to(DEV), table)
    assert a.shape == (MC.B_TINY, 16, MC.TINY["vocab_size"]) and torch.equal(zero, plain) and not torch.equal(a, plain)
    assert not torch.equal(a[:, 11], b[:, 11]) and not torch.equal(a[:, 0], b[:, 0])          # the label of cell 5 reaches other positions
    st = {k: (v.detach().cpu() if k.endswith("mask") else v.detach().cpu().double()) for k, v in m.state_dict().items()}
    ref = MC.forward_conditioned_ref(idx, ctok, st, table.cpu().double(), MC.TINY["n_layer"], MC.TINY["n_head"])
    sp = float(golden("mingpt_gpt_gpt64.npz")["gpt64/spread.out"])          # test_gpu_masked_prior.py's bound for MaskedGPT.forward
    print("forward_conditioned logits: %.3e from float64 (bound 2 x %.1e)" % (rel_err(a, ref), sp))
    assert_close(a, ref, 2.0 * sp, "forward_conditioned logits")
    assert not m.training and m(idx.to(DEV)).requires_grad          # forward itself is untouched: no no_grad, no mode change


# ------------------------------------------------------------------------------------------------ 4. training
V_TINY = MC.TINY["vocab_size"]
DROP_SEED, P_UNCOND = 31, 0.25


def _trainer(init_seed=811, null_token=True, p_uncond=P_UNCOND, **kw):
    from networks import LabelCondition, MaskedGPT, VQGAN
    from trainers import ConditionalMaskedPriorTrainer
    torch.manual_seed(77)
    vqgan = VQGAN(**dict(P.TINY_VQGAN, dict_size=V_TINY))
    torch.manual_seed(init_seed)
    gpt = G.init_gpt_(MaskedGPT(**MC.TINY), init_seed)
    cond = LabelCondition(MC.N_LABELS, MC.TINY["n_embed"], 4, 4, null_token=null_token)
    args = dict(n_steps=4, mask_seed=21, lr=3e-3, betas=P.OPTIM["betas"], weight_decay=P.OPTIM["weight_decay"], grad_norm_clip=1.0, seed=17,
                device=DEV)
    if p_uncond:
        args.update(p_uncond=p_uncond, cond_drop_seed=DROP_SEED)
    args.update(kw)
    return ConditionalMaskedPriorTrainer(vqgan, gpt, cond, **args)


def _batch(B=8, seed=812):
    g = torch.Generator().manual_seed(seed)
    return {"ids": torch.randint(0, V_TINY, (B, 16), generator=g).to(DEV), "cond": torch.randint(0, MC.N_LABELS, (B, 16), generator=g).to(DEV)}


def test_training_step_loss_drop_and_table_gradient(golden):
    from hipops import ops
    tr, batch = _trainer(), _batch()
    ids, tokens = batch["ids"], batch["cond"]
    g = golden("prior_step_p64.npz")          # test_gpu_masked_prior.py's margin for the loss
    own = max(float((np.abs(g["p64/loss32"] - g["p64/loss64"][None]) / np.abs(g["p64/loss64"][None])).max()), FP32_ULP)
    drops = [MC.dropped(8, P_UNCOND, DROP_SEED, n) for n in range(3)]
    assert any(d.any() for d in drops) and not all(d.all() for d in drops)          # the restatement: somebody is dropped, somebody kept
    seen = []
    inner = tr.gpt.forward_conditioned
    tr.gpt.forward_conditioned = lambda inp, ctok, table, null_index=None, drop=None: (seen.append((ctok, null_index, drop)), inner(inp, ctok, table, null_index, drop))[1]
    for step in range(3):
        inp, masked, n = R.mask_tokens(_np(ids), V_TINY, 21, step)
        with torch.no_grad():          # the device's own logits, before the update
            logits = inner(torch.from_numpy(inp).to(DEV), tokens, tr.cond.embed.weight, tr.cond.null_index, (P_UNCOND, DROP_SEED, step))
        want = MC.masked_mean(logits.cpu(), ids.cpu(), masked, n)
        before = tr.cond.embed.weight.detach().clone()
        out = tr.training_step(batch)
        got = float(out["loss"])
        err = abs(got - want) / abs(want)
        print("conditioned masked step %d: loss %.9g, float64 masked mean %.12g: %.2e apart (bound 2 x %.2e)" % (step, got, want, err, own))
        assert err <= 2 * own and out["grad_norm"].is_cuda and tr.step_count == step + 1
        ctok, null_index, drop = seen[-1]
        assert drop == (P_UNCOND, DROP_SEED, step) and null_index == MC.N_LABELS and torch.equal(ctok, tokens)
        eff = ops.embedding_cond(torch.from_numpy(inp).to(DEV), tr.gpt.tok_embed.weight, tr.gpt.pos_embed, ctok, tr.cond.embed.weight, null_index, drop,
                                 return_eff=True)[1]
        assert torch.equal((eff == MC.N_LABELS).all(1).cpu(), torch.from_numpy(drops[step])), step          # the dropped samples of step n
        assert not torch.equal(tr.cond.embed.weight.detach(), before)          # the table is stepped
    tr.gpt.forward_conditioned = inner


def test_resume_is_bit_exact_with_the_drop():
    from utils.checkpoint import _to_cpu
    batch = _batch()
    full = _trainer()
    full_bits = [(float(o["loss"]), float(o["grad_norm"])) for o in (full.training_step(batch) for _ in range(3))]
    part = _trainer()
    first = [part.training_step(batch) for _ in range(2)]
    state = copy.deepcopy(_to_cpu(part.state_dict()))
    assert state["extra"]["cond_drop_seed"] == DROP_SEED
    fresh = _trainer(init_seed=999, seed=5)               # other weights, another generator; the same mask and drop seeds
    fresh.load_state_dict(state)
    assert fresh.step_count == 2
    nxt = fresh.training_step(batch)
    assert [(float(o["loss"]), float(o["grad_norm"])) for o in first] == full_bits[:2]
    assert (float(nxt["loss"]), float(nxt["grad_norm"])) == full_bits[2]
    for (k, a), (_, b) in zip(list(full.gpt.state_dict().items()) + list(full.cond.state_dict().items()),
                              list(fresh.gpt.state_dict().items()) + list(fresh.cond.state_dict().items())):
        assert torch.equal(a, b), k
    with pytest.raises(ValueError, match="the checkpoint was trained with cond_drop_seed=31"):
        _trainer(cond_drop_seed=32).load_state_dict(state)
    # the drop is really a function of cond_drop_seed: another one ends elsewhere
    assert float(_trainer(cond_drop_seed=32).training_step(batch)["loss"]) != full_bits[0][0]


def test_learning_the_label_lowers_the_loss_below_the_null_condition():
    """One batch whose codes are their label tokens, MC.LEARN_STEPS = 60 steps at lr 1e-2 (chosen on the GPU): the validation loss
    falls, and afterwards the loss under the label lies below the loss under the null condition."""
    ids, tokens = MC.learn_batch()
    batch = {"ids": ids.to(DEV), "cond": tokens.to(DEV)}
    tr = _trainer(lr=MC.LEARN_LR)
    before = tr.validation_step(batch)
    assert set(before) == {"loss", "ppl", "ids", "loss_uncond"} and not before["loss"].requires_grad
    for _ in range(MC.LEARN_STEPS):
        tr.training_step(batch)
    after = tr.validation_step(batch)
    print("validation loss %.4f -> %.4f under the label, %.4f -> %.4f under the null condition, after %d steps" % (
        float(before["loss"]), float(after["loss"]), float(before["loss_uncond"]), float(after["loss_uncond"]), MC.LEARN_STEPS))
    assert float(after["loss"]) < float(before["loss"])
    assert float(after["loss"]) < float(after["loss_uncond"]) and tr.gpt.training
    assert "loss_uncond" not in _trainer(null_token=False, p_uncond=0.0).validation_step(batch)


# ------------------------------------------------------------------------------------------------ 5. parallel decoding
KW = dict(temperature=0.9, top_k=8, top_p=0.9, choice_temperature=4.5)
NULL = MC.N_LABELS


def _decode_inputs(T, n_steps):
    g = torch.Generator().manual_seed(900 + 10 * T + n_steps)
    B, V = MC.B_TINY, V_TINY
    ids = torch.randint(0, V, (B, T), generator=g).to(DEV)
    masked = (torch.rand(B, T, generator=g) < 0.6).to(torch.uint8)
    masked[0, :3], masked[0, 3:6] = 1, 0          # both kinds in every row
    masked[1, :3], masked[1, 3:6] = 0, 1
    ctok = torch.randint(0, MC.N_LABELS, (B, T), generator=g).to(DEV)
    return ids, masked.to(DEV), ctok, torch.rand(n_steps, 2, B, T, generator=g).to(DEV)


def _composed(m, ids, masked, uniforms, n_steps, forward, scale=None):
    """The loop from its operators: forward(cur) -> logits (B T, V) or, with scale, (2 B T, V)"""
    from hipops import ops
    B, T = ids.shape
    m0 = masked.sum(1, dtype=torch.int32)
    counts = R.masked_counts_after(_np(m0), n_steps)
    cur, mk = torch.where(masked != 0, torch.full_like(ids, V_TINY), ids), masked
    fx, fu = torch.zeros(B, T, device=DEV), torch.zeros(B, T, device=DEV)
    with torch.no_grad():
        for k in range(n_steps):
            gamma, tau = R.unmask_schedule(k, n_steps, KW["choice_temperature"])
            forced = torch.where(mk != 0, torch.full_like(cur, -1), cur).reshape(-1)
            if scale is None:
                tokens, logp = ops.sample_filtered(forward(cur), uniforms[k, 0].reshape(-1), forced, KW["temperature"], KW["top_k"], KW["top_p"])
            else:
                tokens, logp, logp_u = ops.sample_guided(forward(cur), uniforms[k, 0].reshape(-1), scale, forced, KW["temperature"], KW["top_k"], KW["top_p"])
                tokens = tokens[:B * T]
            was = mk
            cur, mk, fx = ops.unmask_step(tokens.view(B, T), logp.view(B, T), mk, m0, gamma, tau, V_TINY, u=uniforms[k, 1], fixed_logp=fx)
            if scale is not None:
                fu = torch.where((was != 0) & (mk == 0), logp_u.view(B, T), fu)
            assert _np(mk).sum(1).tolist() == counts[k].tolist(), k          # unmask_schedule's counts behind every pass
    return cur, fx, fu


@pytest.mark.parametrize("T", [15, 16])
@pytest.mark.parametrize("n_steps", [1, 4])
def test_generate_parallel_with_a_condition(T, n_steps):
    m, table = _tiny()
    ids, masked, ctok, uniforms = _decode_inputs(T, n_steps)
    B, V = ids.shape[0], V_TINY
    known = masked == 0
    cond = (ctok, table, NULL)
    # unguided: forward_conditioned, sample_filtered, unmask_step
    out, fixed = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, cond=cond, **KW)
    cur, fx, _ = _composed(m, ids, masked, uniforms, n_steps, lambda c: m.forward_conditioned(c, ctok, table).reshape(B * T, V))
    assert torch.equal(out, cur) and _bits(fixed, fx)
    assert torch.equal(out[known], ids[known]) and int(out.max()) < V and int(out.min()) >= 0 and float(fixed[known].abs().max()) == 0.0
    for same in (None, 1.0):          # no guidance: the unguided route, the same bits, two results
        again = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, cond=cond, guidance_scale=same, **KW)
        assert len(again) == 2 and torch.equal(again[0], out) and _bits(again[1], fixed)
    assert len(m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, cond=(ctok, table, None), **KW)) == 2          # no null index needed
    # guided at scale 3: the 2B-row forward, sample_guided, unmask_step
    ctok2 = torch.cat((ctok, torch.full_like(ctok, NULL)))
    gout, gfixed, gfixed_u = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, cond=cond, guidance_scale=3.0, **KW)
    cur, fx, fu = _composed(m, ids, masked, uniforms, n_steps, lambda c: m.forward_conditioned(torch.cat((c, c)), ctok2, table).reshape(2 * B * T, V), 3.0)
    assert torch.equal(gout, cur) and _bits(gfixed, fx) and _bits(gfixed_u, fu)
    assert torch.equal(gout[known], ids[known]) and int(gout.max()) < V and int(gout.min()) >= 0
    assert float(gfixed[known].abs().max()) == 0.0 and float(gfixed_u[known].abs().max()) == 0.0
    assert bool((gfixed[~known] < 0).all()) and bool((gfixed_u[~known] < 0).all()) and not m.training
    again = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, cond=cond, guidance_scale=3.0, **KW)
    assert torch.equal(again[0], gout) and _bits(again[1], gfixed) and _bits(again[2], gfixed_u)
    # cond=None: the unconditional model's bits (the composed loop of tests/test_gpu_masked_prior.py)
    out0, fixed0 = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, **KW)
    cur, fx, _ = _composed(m, ids, masked, uniforms, n_steps, lambda c: m(c).reshape(B * T, V))
    assert torch.equal(out0, cur) and _bits(fixed0, fx)
    if n_steps == 1:          # scale 0 draws from z_u alone: fmaf(0, z_c - z_u, z_u) is z_u
        zero = m.generate_parallel(ids, masked, 1, uniforms=uniforms, cond=cond, guidance_scale=0.0, **KW)
        null = m.generate_parallel(ids, masked, 1, uniforms=uniforms, cond=(torch.full_like(ctok, NULL), table, NULL), **KW)
        assert torch.equal(zero[0], null[0]) and _bits(zero[2], null[1])
    # a generator in place of the uniforms repeats under its seed
    a = m.generate_parallel(ids, masked, n_steps, generator=torch.Generator(device=DEV).manual_seed(3), cond=cond, guidance_scale=3.0, **KW)
    b = m.generate_parallel(ids, masked, n_steps, generator=torch.Generator(device=DEV).manual_seed(3), cond=cond, guidance_scale=3.0, **KW)
    assert torch.equal(a[0], b[0]) and _bits(a[2], b[2])


# ------------------------------------------------------------------------------------------------ 6. synthesize and edit
def _labels(seed=78):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, MC.N_LABELS, (2, 8, 8), generator=g).to(DEV)          # 8 x 8 pixels, a 4 x 4 latent: cells of 2 x 2


def test_synthesize():
    tr, label = _trainer(p_uncond=0.0), _labels()
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)          # noqa: E731
    out = tr.synthesize(label=label, n_candidates=3, n_steps=4, top_k=8, top_p=0.95, generator=gen())
    assert set(out) == {"ids", "candidates", "scores", "best", "cond", "image"}
    assert out["ids"].shape == (2, 16) and out["candidates"].shape == (2, 3, 16) and out["scores"].shape == (2, 3) and out["best"].shape == (2,)
    assert out["scores"].dtype == torch.float64 and bool((out["scores"] < 0).all()) and out["image"].shape == (2, 1, 8, 8)
    assert torch.equal(out["cond"], tr.cond.tokens(label)) and int(out["candidates"].max()) < V_TINY and int(out["candidates"].min()) >= 0
    rows = torch.arange(2, device=DEV)
    assert torch.equal(out["best"], out["scores"].argmax(1)) and torch.equal(out["ids"], out["candidates"][rows, out["best"]]) and tr.gpt.training
    one = tr.synthesize(label=label, n_candidates=1, n_steps=4, top_k=8, top_p=0.95, generator=gen())          # Fit.validate_prior's call
    assert torch.equal(one["candidates"][:, 0], out["candidates"][:, 0]) and torch.equal(one["scores"][:, 0], out["scores"][:, 0])
    by_cond = tr.synthesize(cond=out["cond"], n_candidates=3, n_steps=4, top_k=8, top_p=0.95, generator=gen())
    assert torch.equal(by_cond["candidates"], out["candidates"])
    u = torch.rand(3, 4, 2, 2, 16, generator=torch.Generator().manual_seed(4))
    a, b = (tr.synthesize(label=label, n_candidates=3, n_steps=4, uniforms=u) for _ in range(2))
    assert torch.equal(a["candidates"], b["candidates"]) and torch.equal(a["scores"], b["scores"])
    # guidance
    guided = tr.synthesize(label=label, n_candidates=3, n_steps=4, top_k=8, generator=gen(), guidance_scale=3.0, rank="gain")
    assert set(guided) == set(out) | {"scores_uncond"} and guided["scores_uncond"].shape == (2, 3) and guided["scores_uncond"].dtype == torch.float64
    assert torch.equal(guided["best"], (guided["scores"] - guided["scores_uncond"]).argmax(1))
    g1 = tr.synthesize(label=label, n_candidates=1, n_steps=4, top_k=8, generator=gen(), guidance_scale=3.0)
    assert torch.equal(g1["candidates"][:, 0], guided["candidates"][:, 0])
    draws = list(tr._score_draws([out["cond"][:1], out["cond"][1:]], 2, 2, 1.0, 8, None, gen(), guidance_scale=2.0, n_steps=2))
    assert len(draws) == 1 and draws[0].shape == (2, 16)
    with pytest.raises(ValueError, match="rank='gain' compares"):
        tr.synthesize(label=label, rank="gain")
    with pytest.raises(ValueError, match=r"uniforms of shape .* \(n_candidates, n_steps, 2, B, T\) = \(3, 4, 2, 2, 16\)"):
        tr.synthesize(label=label, n_candidates=3, n_steps=4, uniforms=u[:2])
    with pytest.raises(ValueError, match=r"guidance_scale=3.0 needs a prior trained with the null embedding \(model\.prior\.masked\.cond\.null_token\)"):
        _trainer(null_token=False, p_uncond=0.0).synthesize(label=label, guidance_scale=3.0)


def test_edit_through_the_label_map():
    from hipops import ops
    tr, label = _trainer(p_uncond=0.0), _labels()
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(79)).to(DEV)
    batch = {"image": image, "label": label}
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)          # noqa: E731
    new = label.clone()
    new[0, 2:5, 2:6] = (new[0, 2:5, 2:6] + 1) % MC.N_LABELS          # slice 0: rows 2..4, columns 2..5 -> cells (1..2, 1..2); slice 1 unchanged
    changed = ops.cells_changed(label, new, 4, 4)
    assert changed.reshape(2, 16).sum(1).tolist() == [4, 0]
    out = tr.edit(batch, new_label=new, n_candidates=3, n_steps=4, top_k=8, top_p=0.95, generator=gen())
    assert set(out) == {"ids", "source_ids", "candidates", "scores", "best", "cellmask", "recon", "edit", "composite", "cond", "label_cells"}
    cells = changed.reshape(2, 16) != 0
    src, cand = out["source_ids"], out["candidates"]
    assert torch.equal(out["cellmask"], changed) and cand.shape == (2, 3, 16) and out["scores"].shape == (2, 3)
    keep = ~cells[:, None].expand_as(cand)
    assert torch.equal(cand[keep], src[:, None].expand_as(cand)[keep])          # every code outside the changed cells is the source's
    assert torch.equal(out["cond"], tr.cond.tokens(new)) and torch.equal(out["label_cells"], out["cond"].reshape(2, 4, 4))
    outside = ~(changed != 0).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, None]
    assert torch.equal(out["composite"][outside], image[outside])          # the composite outside the region is the image
    assert torch.equal(out["ids"][1], src[1]) and out["scores"][1].tolist() == [0.0, 0.0, 0.0] and bool((out["scores"][0] < 0).all())
    same = tr.edit(batch, new_label=label.clone(), n_candidates=2, n_steps=4, generator=gen())          # a label unchanged everywhere
    assert torch.equal(same["ids"], src) and float(same["scores"].abs().max()) == 0.0 and int(same["cellmask"].sum()) == 0
    assert torch.equal(same["composite"], image)
    one = tr.edit(batch, new_label=new, n_candidates=1, n_steps=4, top_k=8, top_p=0.95, generator=gen())
    assert torch.equal(one["candidates"][:, 0], cand[:, 0]) and torch.equal(one["scores"][:, 0], out["scores"][:, 0])
    # the parent's selectors under the batch's own label, and guidance
    box = tr.edit(batch, box=(2, 6, 2, 6), n_candidates=2, n_steps=2, top_k=8, generator=gen(), guidance_scale=3.0, rank="gain")
    assert box["cellmask"].reshape(2, 16).sum(1).tolist() == [4, 4] and torch.equal(box["cond"], tr.cond.tokens(label))
    assert box["scores_uncond"].shape == (2, 2) and torch.equal(box["best"], (box["scores"] - box["scores_uncond"]).argmax(1))
    ids_only = tr.edit({"ids": src, "cond": out["cond"]}, mask=_np(cells).reshape(2, 4, 4), n_candidates=3, n_steps=4, top_k=8, top_p=0.95, generator=gen())
    assert "composite" not in ids_only and torch.equal(ids_only["candidates"], cand)
    with pytest.raises(ValueError, match="rank='gain' compares"):
        tr.edit(batch, new_label=new, rank="gain")
    with pytest.raises(ValueError, match="guidance_scale=3.0 needs a prior trained with the null embedding"):
        _trainer(null_token=False, p_uncond=0.0).edit(batch, new_label=new, guidance_scale=3.0)
    with pytest.raises(NotImplementedError, match="raster-order likelihood"):
        tr.edit(batch, nll_threshold=2.0)
    with pytest.raises(ValueError, match="new_label needs the batch's own 'label'"):
        tr.edit({"image": image}, new_label=new)


# ------------------------------------------------------------------------------------------------ 7. the launcher
def test_launcher_trains_and_synthesises_with_the_conditional_masked_prior(tmp_path):
    """run_vqwnet.py -p picks the conditional masked trainer from model.prior.masked.cond (two steps with the drop on, a validation
    under the label and under the null condition, a picture decoded from the label maps, a checkpoint); -p -m synth from that
    checkpoint, twice with one seed: the files are byte-equal."""
    save = os.path.join(str(tmp_path), "run")

    def raw(**run):
        r = P.prior_run_config(save, **run)
        r["model"]["prior"]["masked"] = dict(n_steps=3, choice_temperature=4.5, mask_seed=4, cond=dict(
            source="label", n_labels=2, labels={"synthetic": dict(n=2, radius=5, contrast=0.8)}, null_token=True, p_uncond=0.25, drop_seed=6))
        r["synth"] = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, discs=[[16, 16, 5, 1]], guidance_scale=2.0,
                          n_steps=2)
        return r
    out = run_launcher(write_config(os.path.join(str(tmp_path), "run.json"), raw()), "-p")
    vdir = os.path.join(save, "study", "version_0")
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == P.PRIOR_MONITORED and len(rows) == 3 and "validation cross-entropy" in out and "under the null condition" in out
    assert all(np.isfinite(float(dict(zip(header, r))["loss"])) for r in rows[:2]) and os.path.exists(os.path.join(vdir, "000000.png"))
    ckpt = os.path.join(vdir, "ckpt-epoch=0000-total_loss=0.00.ckpt")
    ck = torch.load(ckpt, map_location="cpu")
    assert ck["state_dict"]["cond.embed.weight"].shape == (3, 64) and ck["state_dict"]["transformer.pos_embed"].shape == (1, 256, 64)
    assert ck["state_dict"]["transformer.tok_embed.weight"].shape == (9, 64)          # 8 codes + the mask token; the sequence stays h w long
    assert ck["vqw_run_state"]["trainer"]["prior_step"] == 2 and ck["vqw_run_state"]["trainer"]["cond_drop_seed"] == 6
    dirs = []
    for i in (1, 2):
        out = run_launcher(write_config(os.path.join(str(tmp_path), "synth%d.json" % i), raw(resume_checkpoint=ckpt)), "-p", "-m", "synth")
        assert "Synthesised slices are saved" in out
        dirs.append(os.path.join(save, "study", "version_%d" % i, "synth"))
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dirs[0], "*")))
    assert names == ["slice_0000.png", "slice_0001.png", "synth.csv"]
    for name in names:
        assert filecmp.cmp(os.path.join(dirs[0], name), os.path.join(dirs[1], name), shallow=False), name + " differs between two runs"
    header, rows = read_csv(os.path.join(dirs[0], "synth.csv"))
    assert header == ["slice", "winner", "score", "cells_redrawn"] and [r[0] for r in rows] == ["0", "1"]
    assert all(int(r[1]) in (0, 1) and float(r[2]) < 0 and 0 < int(r[3]) <= 49 for r in rows)          # a disc of radius 5: at most 7 x 7 cells of 2 x 2
