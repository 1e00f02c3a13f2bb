"""Classifier-free guidance for the conditional code prior on the GPU.  Run with `pytest -m gpu` on an MI355X.

Kernel level.  ops.sample_guided against ops.sample_filtered - the sampler as it was, not the code under test - on logits mixed by
the restatement (tests/cond_guidance_ref.py mix_ref; the host test asserts that no seeded input has an element on which the
restatement's two roundings could differ from the kernel's one): tokens bit-equal, logp / logp_u bit-equal to sample_filtered's
log-probability of the same token under z_c / z_u, out[B:] == out[:B]; the tie case with exact arithmetic; scale 0, top_k 1, two
calls.  ops.embedding_lookup_drop: out and eff bit-equal to the restatement, embedding_lookup's bits at p = 0, the table's
gradient (the null row's included) through `_gate` of tests/test_gpu_mingpt_blocks.py.

Model level, on the tiny model of tests/cond_prior_ref.py with a null row in the table.  GPT.generate_masked with guidance returns
the tokens of the float64 run (two full forwards per position, the mix, top-k, the same uniforms), whose two margins -
gpt_decode_ref.GEN_MIN_DIST and GEN_MIN_GAP - are asserted BEFORE anything about the device; logp and logp_u summed in double equal
the summed token_nll under the two prefixes to rtol 1e-5 (test_synthesize_returns_the_float64_tokens' bound for the same identity).
A training step with p_uncond = 0.5 against the float64 restatement with the dropped samples taken from the restated draw, through
helpers.grad_gate and the scalar rule of test_gpu_cond_prior.py; resume is bit-exact; a wrong cond_drop_seed raises.
"""
import copy

import numpy as np
import pytest
import torch

from helpers import grad_gate, sample_idx
import cond_guidance_ref as CG
import cond_prior_ref as C
import gpt_decode_ref as D
import gpt_ref as G
import prior_ref as P
from test_gpu_mingpt_blocks import _dev, _gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_ULP = 2.0 ** -23


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ sample_guided
@pytest.mark.parametrize("V", CG.GUIDED_V)
def test_sample_guided_is_sample_filtered_on_the_mixed_logits(V):
    from hipops import ops
    n = 0
    for B in CG.GUIDED_B:
        zc, zu, u = CG.guided_inputs(V, B)
        both, ud = torch.cat((zc, zu)).to(DEV), u.to(DEV)
        zcd, zud = zc.to(DEV), zu.to(DEV)
        forced = CG.guided_forced(B, V)
        bad = (forced >= V).to(DEV)
        for scale in CG.GUIDED_SCALES:
            mixed, flag = CG.mix_ref(zc.numpy(), zu.numpy(), scale)
            assert not flag.any()
            mixed = torch.from_numpy(mixed).to(DEV)
            for f in (None, forced.to(DEV)):
                for temperature in CG.GUIDED_TEMPS:
                    for top_k in CG.guided_top_ks(V):
                        for top_p in CG.GUIDED_TOP_P:
                            kw = dict(temperature=temperature, top_k=top_k, top_p=top_p)
                            what = "V %d B %d scale %g forced %s %s" % (V, B, scale, f is not None, kw)
                            out, logp, logp_u = ops.sample_guided(both, ud, scale, f, **kw)
                            want, _ = ops.sample_filtered(mixed, ud, f, **kw)
                            assert out.shape == (2 * B,) and out.dtype == torch.long and torch.equal(out[:B], want), what
                            assert torch.equal(out[B:], out[:B]), what
                            lc = ops.sample_filtered(zcd, ud, want, **kw)[1]          # the sampler as it was, the token forced
                            lu = ops.sample_filtered(zud, ud, want, **kw)[1]
                            if f is not None and bool(bad.any()):
                                assert bool(torch.isnan(logp[bad]).all()) and bool(torch.isnan(logp_u[bad]).all()), what
                                lc, lu = torch.where(bad, logp, lc), torch.where(bad, logp_u, lu)
                            assert torch.equal(_bits(logp), _bits(lc)) and torch.equal(_bits(logp_u), _bits(lu)), what
                            if scale == 0 and f is None:
                                assert torch.equal(out[:B], ops.sample_filtered(zud, ud, None, **kw)[0]), what + ": scale 0 is the unconditional row"
                            if top_k == 1 and f is None:
                                assert torch.equal(out[:B], mixed.argmax(1)), what + ": top_k 1 is the argmax of the mixed row"
                            n += 1
        again = ops.sample_guided(both, ud, 3.0, forced.to(DEV), temperature=0.7, top_k=min(5, V), top_p=0.9)
        once = ops.sample_guided(both, ud, 3.0, forced.to(DEV), temperature=0.7, top_k=min(5, V), top_p=0.9)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, once)), "two calls give equal bits"
        buf = torch.full((2 * B,), -7, dtype=torch.long, device=DEV)
        assert ops.sample_guided(both, ud, 3.0, out=buf)[0] is buf and bool((buf >= 0).all())
    assert n >= 2 * 5 * 2 * 2 * 1 * 3


def test_sample_guided_tied_entries_share_one_fate():
    """Exact arithmetic (logits on the 2^-10 grid, scale 2): different (z_c, z_u) pairs mix to EQUAL values at the top-k and the nucleus
    thresholds.  256 rows of one pair of rows with u spread over [0, 1): the set of tokens drawn is exactly the kept set."""
    from hipops import ops
    zc, zu, mixed = CG.tie_inputs()
    n = 256
    u = ((torch.arange(n) + 0.5) / n).to(DEV)
    for r in range(2):
        both = torch.cat((zc[r].expand(n, -1), zu[r].expand(n, -1))).contiguous().to(DEV)
        m32 = torch.from_numpy(mixed[r].astype(np.float32)).expand(n, -1).contiguous().to(DEV)
        value = lambda v: set(np.flatnonzero(mixed[r] >= v).tolist())  # noqa: E731
        for kw, kept in ((dict(top_k=2), value(3.0)), (dict(top_k=4), value(3.0)), (dict(top_k=5), value(1.0)), (dict(top_k=6), value(1.0)),
                         (dict(top_p=0.3), value(5.0)), (dict(top_p=0.9), value(3.0)), (dict(top_p=0.98), value(1.0)),
                         (dict(top_k=5, top_p=0.9), value(3.0)), (dict(), set(range(mixed.shape[1])))):
            out, logp, logp_u = ops.sample_guided(both, u, CG.TIE_SCALE, **kw)
            want, _ = ops.sample_filtered(m32, u, **kw)
            assert torch.equal(out[:n], want) and torch.equal(out[n:], want), (r, kw)
            drawn = set(out[:n].cpu().tolist())
            if kw:
                assert drawn == kept, "row %d %s: drew %s, the kept set is %s" % (r, kw, sorted(drawn), sorted(kept))
            else:
                assert drawn <= kept and value(1.0) <= drawn


# ------------------------------------------------------------------------------------------------ embedding_lookup_drop
@pytest.mark.parametrize("p", CG.LOOKUP_PS)
@pytest.mark.parametrize("case", CG.LOOKUP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_embedding_lookup_drop(case, p):
    from hipops import ops
    B, Tc, E, L = case
    idx, table, gx = CG.lookup_inputs(*case)
    seed, call = CG.LOOKUP_KEY
    want, want_eff = CG.lookup_drop_ref(idx, table, L, p, seed, call)
    t = _dev(table).requires_grad_(True)
    out, eff = ops.embedding_lookup_drop(idx.to(DEV), t, L, p, seed, call, return_eff=True)
    out.backward(_dev(gx))
    torch.cuda.synchronize()
    assert out.shape == (B, Tc, E) and eff.dtype == torch.long and not eff.requires_grad
    assert torch.equal(eff.cpu(), want_eff) and torch.equal(out.detach().cpu(), want), "out and eff are the restatement's, bit for bit"
    if p == 0:
        assert torch.equal(out.detach(), ops.embedding_lookup(idx.to(DEV), t.detach())) and torch.equal(eff.cpu(), idx)
    else:
        dropped = CG.dropped_ref(B, p, seed, call)
        assert bool((want_eff[torch.from_numpy(dropped)] == L).all()) and (B < 5 or (dropped.any() and not dropped.all()))
    truth = torch.zeros(L + 1, E, dtype=torch.float64).index_add_(0, want_eff.reshape(-1), gx.reshape(-1, E).double())
    ref32 = torch.zeros(L + 1, E).index_add_(0, want_eff.reshape(-1), gx.reshape(-1, E))
    _gate(t.grad, truth, ref32, "embedding_lookup_drop %s p %g gtable" % (case, p))
    used = torch.zeros(L + 1, dtype=torch.bool)
    used[want_eff.reshape(-1)] = True
    assert not bool(t.grad.cpu()[~used].any()), "unused rows are exactly 0"
    if p > 0 and B >= 5:
        assert float(t.grad[L].abs().sum()) > 0, "the null row has a gradient"
    t2 = _dev(table).requires_grad_(True)
    out2 = ops.embedding_lookup_drop(idx.to(DEV), t2, L, p, seed, call)
    out2.backward(_dev(gx))
    assert torch.equal(out2, out) and torch.equal(t2.grad, t.grad), "the same bits every run"
    if p > 0 and B >= 5:
        other = ops.embedding_lookup_drop(idx.to(DEV), t.detach(), L, p, seed, call + 1, return_eff=True)[1]
        assert not torch.equal(other, eff), "another call, another draw"


# ------------------------------------------------------------------------------------------------ the tiny conditional trainer
def _state(seed=C.SEED):
    """The restatement's initial state: the GPT's state dict (init_gpt_) and a table of C.L + 1 rows, the last the null row."""
    from networks import GPT
    torch.manual_seed(seed)
    gpt = G.init_gpt_(GPT(**C.GPT_KW), seed)
    state = {k: v.detach().clone() for k, v in gpt.state_dict().items()}
    state[C.TABLE] = CG.state(seed)
    return state


def _trainer(state=None, null_token=True, **kw):
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer
    state = _state() if state is None else state
    torch.manual_seed(77)
    vqgan = VQGAN(**dict(P.TINY_VQGAN, dict_size=C.V))
    gpt = GPT(**C.GPT_KW)
    gpt.load_state_dict({k: v for k, v in state.items() if k != C.TABLE})
    cond = LabelCondition(C.L, C.E, C.LAT_H, C.LAT_W, null_token=null_token)
    with torch.no_grad():
        cond.embed.weight.copy_(state[C.TABLE][:cond.embed.weight.shape[0]])
    o = C.OPTIM
    args = dict(pkeep=1.0, sos_token=C.SOS, lr=o["lr"], betas=o["betas"], weight_decay=o["weight_decay"], grad_norm_clip=C.GRAD_NORM_CLIP,
                seed=17, device=DEV)
    args.update(kw)
    return ConditionalPriorTrainer(vqgan, gpt, cond, **args)


def _named(tr):
    return list(tr.gpt.named_parameters()) + [(C.TABLE, tr.cond.embed.weight)]


def _sampled(named):
    return {k: t.detach().double().cpu().reshape(-1)[sample_idx(t.numel(), 256, seed=1)] for k, t in named.items()}


# ------------------------------------------------------------------------------------------------ generate_masked with guidance
def _gen_case(kind):
    ids, cond = C.tiny_batch()
    known, cond = ids[:CG.GEN_B], cond[:CG.GEN_B]
    mask = CG.gen_mask(kind)
    j0 = int(np.flatnonzero(mask.any(axis=0))[0])
    u = torch.rand(C.T, CG.GEN_B, generator=torch.Generator().manual_seed(CG.GEN_SEED))[:C.T - j0]
    return known, cond, mask, j0, u


@pytest.mark.parametrize("kind", ["all", "kept"])
def test_generate_masked_with_guidance_returns_the_float64_tokens(kind):
    state = _state()
    known, cond, mask, j0, u = _gen_case(kind)
    assert j0 == (0 if kind == "all" else CG.GEN_J0) and (kind == "all" or (mask[0] != mask[1]).any()), "a kept prefix and a per-row mask"
    want, min_dist, min_gap = CG.guided_truth(C.state_as(state, torch.float64), cond, known, mask, u)
    print("guided generate_masked, %s, seed %d, scale %g: smallest draw distance %.3e (>= %.0e), smallest k / k+1 gap %.3e (>= %.0e)" % (
        kind, CG.GEN_SEED, CG.GEN_SCALE, min_dist, D.GEN_MIN_DIST, min_gap, D.GEN_MIN_GAP))
    assert min_dist >= D.GEN_MIN_DIST and min_gap >= D.GEN_MIN_GAP          # before anything about the device
    assert torch.equal(want[torch.from_numpy(~mask)], known[torch.from_numpy(~mask)])
    tr = _trainer(state)
    tr.gpt.eval()
    B = CG.GEN_B
    start = torch.full((B, 1), C.SOS, dtype=torch.long, device=DEV)
    cd = cond.to(DEV)
    kw = dict(temperature=CG.GEN_TEMP, top_k=CG.GEN_TOPK, uniforms=u, embeddings=tr.cond(cd))
    with torch.no_grad():
        tokens, logp, logp_u = tr.gpt.generate_masked(start, known.to(DEV), mask, uncond_embeddings=tr.cond.null_prefix(B),
                                                      guidance_scale=CG.GEN_SCALE, **kw)
        again = tr.gpt.generate_masked(start, known.to(DEV), mask, uncond_embeddings=tr.cond.null_prefix(B), guidance_scale=CG.GEN_SCALE, **kw)
    assert tokens.shape == (B, C.T) and tokens.dtype == torch.long and logp.shape == logp_u.shape == (B, C.T)
    assert torch.equal(tokens.cpu(), want), "guided generate_masked differs from the float64 run:\n%s\n%s" % (tokens.cpu(), want)
    assert all(torch.equal(a, b) for a, b in zip((tokens, logp, logp_u), again))
    nll_c = tr.token_nll({"ids": tokens, "cond": cd}).double().sum((1, 2))
    nll_u = tr.token_nll({"ids": tokens, "cond": torch.full_like(cd, CG.NULL)}).double().sum((1, 2))
    assert torch.allclose(logp.double().sum(1), -nll_c, rtol=1e-5, atol=0), (logp.double().sum(1), -nll_c)
    assert torch.allclose(logp_u.double().sum(1), -nll_u, rtol=1e-5, atol=0), (logp_u.double().sum(1), -nll_u)
    assert not torch.equal(logp, logp_u)


def test_guidance_scale_none_and_one_are_the_unguided_call():
    tr = _trainer()
    tr.gpt.eval()
    known, cond, mask, j0, u = _gen_case("kept")
    B = CG.GEN_B
    start = torch.full((B, 1), C.SOS, dtype=torch.long, device=DEV)
    kw = dict(temperature=0.8, top_k=5, top_p=0.9, uniforms=u, embeddings=tr.cond(cond.to(DEV)))
    with torch.no_grad():
        plain = tr.gpt.generate_masked(start, known.to(DEV), mask, **kw)
        for scale in (None, 1.0, 1):
            got = tr.gpt.generate_masked(start, known.to(DEV), mask, guidance_scale=scale, uncond_embeddings=tr.cond.null_prefix(B), **kw)
            assert len(got) == 2 and torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), scale
        got = tr.gpt.generate_masked(start, known.to(DEV), mask, guidance_scale=1.0, **kw)          # no unconditional rows needed at all
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # nothing resampled under guidance: one prefill, the log-probabilities of the kept codes under both prefixes
    none = np.zeros((B, C.T), dtype=bool)
    with torch.no_grad():
        tok, lp, lpu = tr.gpt.generate_masked(start, known.to(DEV), none, embeddings=kw["embeddings"], uncond_embeddings=tr.cond.null_prefix(B),
                                              guidance_scale=2.0)
    assert torch.equal(tok.cpu(), known)
    nll_u = tr.token_nll({"ids": tok, "cond": torch.full_like(cond, CG.NULL).to(DEV)}).double().sum((1, 2))
    assert torch.allclose(lpu.double().sum(1), -nll_u, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ training with the drop
def test_training_step_with_the_condition_dropped_against_the_restatement():
    state = _state(C.STEP_SEED)
    ids, cond = C.tiny_batch(C.STEP_SEED)
    truth = CG.steps_drop_ref(state, ids, cond, torch.float64)
    variants = [CG.steps_drop_ref(state, ids, cond, torch.float32, variant=v) for v in C.VARIANTS]
    # on the CPU first: the drawn pattern mixes kept and dropped samples, the null row and a label row both carry gradient, and the
    # case is well conditioned for AdamW's first update (cond_prior_ref.STEP_SEED's rule, recomputed for this drop)
    assert truth["dropped"] == [[True, False, True], [True, False, False], [True, True, True]]
    g_table = truth["g0"][C.TABLE]
    assert float(g_table[CG.NULL].norm()) > 0.1 and float(g_table[:CG.NULL].norm()) > 0.1
    sens = C.adam_step_sensitivity(truth["g0"], truth["coef"][0])
    print("p_uncond %g, drop seed %d: dropped %s, predicted parameter error of fp32 gradient noise %.2e" % (CG.P_UNCOND, CG.DROP_SEED, truth["dropped"], sens))
    assert sens <= C.STEP_MAX_SENSITIVITY
    assert min(truth["coef"]) < 1.0 and max(truth["coef"]) == 1.0, "the clip binds at some steps of the case and not at others"
    tr = _trainer(state, grad_norm_clip=C.STEP_CLIP, p_uncond=CG.P_UNCOND, cond_drop_seed=CG.DROP_SEED)
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    got = dict(loss=[], norm=[], coef=[])
    for s in range(C.STEPS):
        out = tr.training_step(batch)
        got["loss"].append(float(out["loss"]))
        got["norm"].append(float(out["grad_norm"]))
        got["coef"].append(float(tr.optim.last_clip_coef))
        if s == 0:
            g0 = {k: p.grad.detach().clone() for k, p in _named(tr)}
    assert tr.step_count == C.STEPS and sorted(g0) == sorted(truth["g0"])
    failures = []
    for q in ("loss", "norm", "coef"):
        t64 = np.array(truth[q])
        v32 = np.array([v[q] for v in variants])
        own = max(float((np.abs(v32 - t64[None]) / np.abs(t64[None])).max()), FP32_ULP)
        for s in range(C.STEPS):
            err = abs(got[q][s] - t64[s]) / abs(t64[s])
            print("step %d %s: %.9g, restatement fp64 %.9g: %.2e apart, the restatement's own fp32 distance %.2e" % (s, q, got[q][s], t64[s], err, own))
            if err > 2 * own or (q == "coef" and t64[s] == 1.0 and got[q][s] != 1.0):
                failures.append((q, s, err, own))
    grad_gate(_sampled(truth["g0"]), [_sampled(v["g0"]) for v in variants], _sampled(g0), what="p_uncond gradient")
    grad_gate(_sampled(truth["P"]), [_sampled(v["P"]) for v in variants], _sampled(dict(_named(tr))), what="p_uncond parameter")
    assert not failures, failures


def _everything(tr):
    out = {"p." + k: v for k, v in tr.gpt.state_dict().items()}
    out["table"] = tr.cond.embed.weight
    for i, (_, p) in enumerate(_named(tr)):
        st = tr.optim.state[p]
        out["m.%d" % i], out["v.%d" % i], out["t.%d" % i] = st["exp_avg"], st["exp_avg_sq"], torch.tensor(st["step"])
    out["generator"], out["step"] = tr.generator.get_state(), torch.tensor(tr.step_count)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def test_resume_is_bit_exact_with_the_drop():
    from utils.checkpoint import _to_cpu
    ids, cond = C.tiny_batch()
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    kw = dict(pkeep=0.5, warmup_steps=3, decay_steps=6, p_uncond=0.5, cond_drop_seed=CG.DROP_SEED)
    full = _trainer(**kw)
    losses = [float(full.training_step(batch)["loss"]) for _ in range(4)]
    part = _trainer(**kw)
    first = [float(part.training_step(batch)["loss"]) for _ in range(2)]
    state = copy.deepcopy(_to_cpu(part.state_dict()))
    assert state["extra"]["cond_drop_seed"] == CG.DROP_SEED and state["modules"]["cond"]["embed.weight"].shape == (C.L + 1, C.E)
    fresh = _trainer(_state(999), seed=5, **kw)          # other weights, another table, another generator
    fresh.load_state_dict(state)
    assert fresh.step_count == 2
    rest = [float(fresh.training_step(batch)["loss"]) for _ in range(2)]
    assert first + rest == losses
    a, b = _everything(full), _everything(fresh)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert a.keys() == b.keys() and not diff, diff[:8]
    # the drop did something: the same run without it ends elsewhere; and another seed is refused on load
    plain = _trainer(pkeep=0.5, warmup_steps=3, decay_steps=6)
    assert [float(plain.training_step(batch)["loss"]) for _ in range(4)] != losses
    wrong = _trainer(**dict(kw, cond_drop_seed=CG.DROP_SEED + 1))
    with pytest.raises(ValueError, match="cond_drop_seed=%d, this trainer has %d" % (CG.DROP_SEED, CG.DROP_SEED + 1)):
        wrong.load_state_dict(state)


def test_validation_step_reports_the_loss_under_the_null_prefix():
    tr = _trainer()
    ids, cond = C.tiny_batch()
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    out = tr.validation_step(batch)
    null = tr.validation_step({"ids": batch["ids"], "cond": torch.full_like(batch["cond"], CG.NULL)})
    assert torch.equal(out["loss_uncond"], null["loss"]) and not torch.equal(out["loss"], out["loss_uncond"]) and tr.gpt.training
    assert "loss_uncond" not in _trainer(null_token=False).validation_step(batch)


# ------------------------------------------------------------------------------------------------ guidance sharpens the condition
def test_guidance_sharpens_what_the_prior_learnt_of_the_condition():
    """The restatement trained with p_uncond = 0.5 for C.LEARN_STEPS on C.learn_batch() (lr C.LEARN_LR, drop seed CG.DROP_SEED), then
    the first code under z_u + s (z_c - z_u).  Float64 first, then the device's own training run shows the same ordering.

    What is measured is cond_prior_ref.learn_gap's quantity under guidance - log p_s(the sequence's first code | its own label)
    minus log p_s(the same code | the other label) - which scale 3 must raise over scale 1 by at least C.LEARN_MIN_GAP nats for both
    sequences (the restatement: 0.48 -> 1.62 and 3.46 -> 10.18 nats).  The log-probability of the label-consistent code alone
    cannot rise by a nat on this case and is asserted only to rise: at scale 1 the restatement already gives it -0.018 and -0.969
    nats, so -log p_1 bounds the gain (scale 3: -0.0008 and -0.227; over 150 drop seeds at lr 1e-2 and 24 each at 2e-4 .. 1.5e-3 the
    smaller of the two gains never exceeded 0.2 nats)."""
    state = _state()
    ids, cond = C.learn_batch()
    st = CG.learn_drop_ref(state)

    def gaps(logp):          # logp(cond, scale) -> (right, gap) per sequence
        out = {}
        for s in (1.0, CG.GEN_SCALE):
            right, swapped = logp(cond, s), logp(cond.flip(0), s)
            out[s] = (right, right - swapped)
        return out
    ref = gaps(lambda c, s: CG.first_code_logp(st, c, s))
    print("the restatement: scale 1 right %s gap %s; scale 3 right %s gap %s" % tuple(t.tolist() for s in (1.0, CG.GEN_SCALE) for t in ref[s]))
    assert bool((ref[CG.GEN_SCALE][1] - ref[1.0][1] >= C.LEARN_MIN_GAP).all())          # before anything about the device
    assert bool((ref[CG.GEN_SCALE][0] > ref[1.0][0]).all())
    tr = _trainer(state, lr=C.LEARN_LR, grad_norm_clip=C.STEP_CLIP, p_uncond=CG.P_UNCOND, cond_drop_seed=CG.DROP_SEED)          # the restatement's clip
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    for _ in range(C.LEARN_STEPS):
        tr.training_step(batch)
    tr.gpt.eval()
    start = torch.full((2, 1), C.SOS, dtype=torch.long, device=DEV)

    def device_logp(c, s):
        with torch.no_grad():
            zc = tr._logits(start, tr.cond(c.to(DEV)))[:, 0].double().cpu()
            zu = tr._logits(start, tr.cond.null_prefix(2))[:, 0].double().cpu()
        return torch.log_softmax(zu + s * (zc - zu), dim=-1).gather(-1, ids[:, :1])[:, 0]
    got = gaps(device_logp)
    print("the device: scale 1 right %s gap %s; scale 3 right %s gap %s" % tuple(t.tolist() for s in (1.0, CG.GEN_SCALE) for t in got[s]))
    assert bool((got[CG.GEN_SCALE][1] > got[1.0][1]).all()) and bool((got[CG.GEN_SCALE][0] > got[1.0][0]).all())
    tr.gpt.train()


# ------------------------------------------------------------------------------------------------ synthesize and edit under guidance
def test_synthesize_and_edit_with_guidance():
    tr = _trainer()
    cond = C.tiny_batch()[1][:2].to(DEV)
    n = 3
    u = torch.rand(n, C.T, 2, generator=torch.Generator().manual_seed(4))
    kw = dict(cond=cond, n_candidates=n, temperature=1.0, top_k=8, top_p=0.95, uniforms=u)
    plain = tr.synthesize(**kw)
    for scale in (None, 1.0):
        same = tr.synthesize(guidance_scale=scale, **kw)
        assert "scores_uncond" not in same and all(torch.equal(same[k], plain[k]) for k in plain), "off: the parent's result"
    out = tr.synthesize(guidance_scale=3.0, **kw)
    gain = tr.synthesize(guidance_scale=3.0, rank="gain", **kw)
    assert out["scores_uncond"].shape == (2, n) and out["scores_uncond"].dtype == torch.float64
    assert torch.equal(out["candidates"], gain["candidates"]) and torch.equal(out["scores"], gain["scores"])
    assert torch.equal(out["best"].cpu(), out["scores"].cpu().argmax(1)), "rank 'cond' is the parent's rule"
    assert torch.equal(gain["best"].cpu(), (gain["scores"] - gain["scores_uncond"]).cpu().argmax(1))
    rows = torch.arange(2, device=DEV)
    assert torch.equal(gain["ids"], gain["candidates"][rows, gain["best"]])
    for c in range(n):
        ids = out["candidates"][:, c]
        nll_c = tr.token_nll({"ids": ids, "cond": cond}).double().sum((1, 2))
        nll_u = tr.token_nll({"ids": ids, "cond": torch.full_like(cond, CG.NULL)}).double().sum((1, 2))
        assert torch.allclose(out["scores"][:, c], -nll_c, rtol=1e-5, atol=0) and torch.allclose(out["scores_uncond"][:, c], -nll_u, rtol=1e-5, atol=0)
    one = tr.synthesize(guidance_scale=3.0, **dict(kw, n_candidates=1, uniforms=u[:1]))
    assert torch.equal(one["candidates"][:, 0], out["candidates"][:, 0]), "candidate 0 does not depend on n_candidates"
    # edit: the kept codes stay, the dict gains scores_uncond
    ids = C.tiny_batch()[0][:2].to(DEV)
    mask = np.zeros((C.LAT_H, C.LAT_W), dtype=bool)
    mask[1:, 2:4] = True
    ed = tr.edit({"ids": ids, "cond": cond}, mask=mask, n_candidates=2, top_k=8, guidance_scale=2.0, rank="gain",
                 generator=torch.Generator(device=DEV).manual_seed(9))
    keep = torch.from_numpy(~mask.reshape(-1)).to(DEV)
    assert torch.equal(ed["candidates"][:, 0][:, keep], ids[:, keep]) and ed["scores_uncond"].shape == (2, 2)
    assert torch.equal(ed["best"].cpu(), (ed["scores"] - ed["scores_uncond"]).cpu().argmax(1))
    with pytest.raises(ValueError, match="null_token"):
        _trainer(null_token=False).synthesize(guidance_scale=3.0, **kw)
    assert tr.gpt.training


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_trains_with_the_drop_and_synthesises_with_guidance(tmp_path):
    import filecmp
    import glob
    import os
    from run_helpers import read_csv, run_launcher, write_config
    save = os.path.join(str(tmp_path), "run")

    def raw(**run):
        r = P.prior_run_config(save, **run)
        r["model"]["prior"]["cond"] = dict(source="label", n_labels=2, labels={"synthetic": dict(n=2, radius=5, contrast=0.8)},
                                           null_token=True, p_uncond=0.5, drop_seed=3)
        r["synth"] = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, discs=[[16, 16, 5, 1]], guidance_scale=2,
                          rank="gain")
        return r
    out = run_launcher(write_config(os.path.join(str(tmp_path), "run.json"), raw()), "-p")
    vdir = os.path.join(save, "study", "version_0")
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == P.PRIOR_MONITORED and len(rows) == 3 and "validation cross-entropy under the null condition" in out
    assert all(np.isfinite(float(dict(zip(header, r))["loss"])) for r in rows[:2])
    ckpt = os.path.join(vdir, "ckpt-epoch=0000-total_loss=0.00.ckpt")
    ck = torch.load(ckpt, map_location="cpu")
    assert ck["state_dict"]["cond.embed.weight"].shape == (3, 64)          # two labels and the null row
    assert ck["vqw_run_state"]["trainer"]["prior_step"] == 2 and ck["vqw_run_state"]["trainer"]["cond_drop_seed"] == 3
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
    assert all(int(r[1]) in (0, 1) and float(r[2]) < 0 for r in rows)
