"""The conditional code prior on the GPU: the label kernels of csrc/cond.hip bit for bit against the restatement
(tests/cond_prior_ref.py), ops.embedding_lookup, GPT.forward_tail, and trainers.ConditionalPriorTrainer - the step against the
float64 restatement, what the mask lets through, learning the condition, bit-exact resume, synthesize against the float64 run, and
edit(new_label=...).  Run with `pytest -m gpu` on an MI355X.

Tolerances are the project's own.  Integer results and gathers: bit equality.  embedding_lookup's gradient and forward_tail's
logits: `_gate` of tests/test_gpu_mingpt_blocks.py (at most twice the fp32 restatement's own distance from float64).  The step:
helpers.grad_gate at its defaults for the gradients of step 0 and the parameters after step 3, and the scalar rule of
test_gpu_prior.py's test_training_step_against_the_reference for loss, norm and clip coefficient (within twice the restatement's own
fp32-to-fp64 distance for that quantity over the steps, floored at 2^-23; an unclipped coefficient is exactly 1).  edit's scores
against the summed token_nll: rtol 1e-5, test_edit_empty_mask_returns_the_slice_with_its_own_score's bound for the same identity.

The prior learns the condition (test_the_prior_learns_the_condition): lr 1e-2, 30 steps, chosen with the float64 restatement, whose
own gap is 6.85 and 8.42 nats for the two sequences (cond_prior_ref.LEARN_*); the test asserts the restatement's gap >= 1 nat
before the device runs and then only the inequality on the device.

The step test runs the optimiser as the trainer builds it (eps = 1e-8) on the case cond_prior_ref.STEP_SEED names, chosen on the
CPU as the best conditioned of sixteen for AdamW's first update (cond_prior_ref says how and why); gradients and parameters go
through grad_gate on helpers.sample_idx(numel, 256, seed=1) of every tensor, test_gpu_prior.py's rule.  Measured on the MI355X
at eps = 1e-8 (parameter gate on the sampled entries; predicted sensitivity of the case in brackets): the chosen case 147 median
ratio 0.79, max 1.26 at pkeep 1 (7.0e-6) and 0.74, 1.30 at pkeep 0.7 (1.2e-5), scalars at most 0.6 x and 1.4 x the restatement's own
distance.  Other seeds, for the record and not used for the choice: 145 / 153 at pkeep 1 (8.5e-6, 8.0e-6) 0.84 and 0.78, 143 at pkeep
0.7 (1.9e-5) 0.79 - all five cases below 2e-5 pass; of the five above 2e-4, 141 fails at both pkeep (2.3e-4: median 2.33, 23 of 38
tensors beyond 2 x; 4.0e-4: 1.57, norm 6.2 x) and 145 at pkeep 0.7 (4.1e-4: 1.80), while 153 at 0.7 (4.2e-4) and 143 at 1 (9.4e-4)
pass: near eps the outcome is the draw of one element's rounding error, which is why the case is chosen away from it.

The tiny model is 64 wide with 2 heads, not 32: the attention kernels serve head sizes from 32 up (csrc/attention.hip), so a model
of 2 heads and 32 channels cannot run on them.  Everything else of the case stands: 16 codes, 3 labels, a 3 x 5 latent (T = Tc = 15,
block_size 30, n_unmasked 15), 2 layers, B = 3."""
import copy

import numpy as np
import pytest
import torch

from helpers import grad_gate, rel_err, sample_idx
import cond_prior_ref as C
import gpt_decode_ref as D
import gpt_ref as G
import prior_ref as P
from test_gpu_mingpt_blocks import _dev, _gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_ULP = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ cell_labels
def _check_cell_labels(case, dtype):
    from hipops import ops
    B, H, W, h, w, L = case
    lab = C.label_inputs(case, dtype)
    want_t, want_p = C.cell_labels_ref(lab.numpy(), h, w, L)
    assert bool((want_t == -1).any()) == C.label_features(case, dtype)[2], "the case is meant to hold a cell with no valid pixel"
    d = lab.to(DEV)
    tokens, purity = ops.cell_labels(d, h, w, L, want_purity=True)
    only = ops.cell_labels(d[:, None], h, w, L)          # (B, 1, H, W), tokens alone
    again = ops.cell_labels(d, h, w, L, want_purity=True)
    torch.cuda.synchronize()
    assert tokens.shape == (B, h, w) and tokens.dtype == torch.long and purity.dtype == torch.float32
    assert np.array_equal(tokens.cpu().numpy(), want_t), "tokens %s %s" % (case, dtype)
    assert np.array_equal(purity.cpu().numpy().view(np.uint32), want_p.view(np.uint32)), "purity %s %s" % (case, dtype)
    assert torch.equal(only, tokens) and torch.equal(again[0], tokens) and torch.equal(again[1], purity)


@pytest.mark.parametrize("dtype", C.LABEL_DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", C.LABEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_cell_labels_bit_equal(case, dtype):
    _check_cell_labels(case, dtype)


@pytest.mark.parametrize("case,dtype", C.LABEL_FULL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).split(".")[-1])
def test_cell_labels_bit_equal_at_full_size(case, dtype):
    _check_cell_labels(case, dtype)


def test_cell_labels_ties_go_to_the_smallest_label():
    from hipops import ops
    lab = torch.tensor([[[2, 2, 1, 1], [1, 1, 2, 2]]], dtype=torch.uint8)          # one cell: four 1s, four 2s
    tokens, purity = ops.cell_labels(lab.to(DEV), 1, 1, 3, want_purity=True)
    assert tokens.cpu().tolist() == [[[1]]] and purity.cpu().tolist() == [[[0.5]]]


# ------------------------------------------------------------------------------------------------ cells_changed
@pytest.mark.parametrize("dtype", C.LABEL_DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", [(2, 24, 40, 3, 5, 5), (2, 24, 40, 4, 4, 2), (1, 512, 512, 16, 16, 256), (1, 512, 512, 32, 32, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_cells_changed_bit_equal(case, dtype):
    from hipops import ops
    B, H, W, h, w, L = case
    fy, fx = H // h, W // w
    a = C.label_inputs(case, dtype)
    d = a.to(DEV)
    assert not bool(ops.cells_changed(d, d.clone(), h, w).any()), "identical maps"
    for cy, cx in ((0, 0), (h - 1, w - 1), (h // 2, w // 3)):          # the last pixel of a cell's last row and column
        b = a.clone()
        y, x = cy * fy + fy - 1, cx * fx + fx - 1
        b[B - 1, y, x] = (int(b[B - 1, y, x]) + 1) % 200
        got = ops.cells_changed(d, b.to(DEV), h, w)
        want = np.zeros((B, h, w), dtype=np.uint8)
        want[B - 1, cy, cx] = 1
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (cy, cx)
    b = C.label_inputs(case, dtype, seed=1)          # many differences; a second pointer alignment through the (B, 1, H, W) view
    b[:, : H // 2] = a[:, : H // 2]
    got = ops.cells_changed(d[:, None], b.to(DEV)[:, None], h, w)
    assert np.array_equal(got.cpu().numpy(), C.cells_changed_ref(a.numpy(), b.numpy(), h, w))
    off = torch.empty(b.numel() + 1, dtype=dtype, device=DEV)[1:].view(b.shape).copy_(b)          # not 16-byte aligned against d
    assert torch.equal(ops.cells_changed(d, off, h, w), got)


# ------------------------------------------------------------------------------------------------ embedding_lookup
def _lookup_run(idx, table, gx):
    from hipops import ops
    t = _dev(table).requires_grad_(True)
    x = ops.embedding_lookup(idx.to(DEV), t)
    x.backward(_dev(gx))
    torch.cuda.synchronize()
    return x.detach(), t.grad


@pytest.mark.parametrize("B,T,E,L,kind", [(2, 15, 32, 3, "rand"), (1, 65, 32, 7, "same"), (2, 1, 4, 5, "rand")])
def test_embedding_lookup(B, T, E, L, kind):
    g = torch.Generator().manual_seed(B + T + E + L)
    idx = torch.randint(0, L, (B, T), generator=g) if kind == "rand" else torch.full((B, T), L // 2, dtype=torch.long)
    table, gx = torch.randn(L, E, generator=g), torch.randn(B, T, E, generator=g)
    x, gtable = _lookup_run(idx, table, gx)
    assert x.shape == (B, T, E) and torch.equal(x.cpu(), table[idx]), "the forward is a gather"
    truth = torch.zeros(L, E, dtype=torch.float64).index_add_(0, idx.reshape(-1), gx.reshape(-1, E).double())
    ref32 = torch.zeros(L, E).index_add_(0, idx.reshape(-1), gx.reshape(-1, E))
    _gate(gtable, truth, ref32, "embedding_lookup B%d T%d E%d L%d %s gtable" % (B, T, E, L, kind))
    used = torch.zeros(L, dtype=torch.bool)
    used[idx.reshape(-1)] = True
    assert not bool(gtable.cpu()[~used].any()), "unused rows are exactly 0"
    x2, gtable2 = _lookup_run(idx, table, gx)
    assert torch.equal(x, x2) and torch.equal(gtable, gtable2)


def test_embedding_lookup_bad_index_is_a_nan_row_and_no_gradient():
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 3, (2, 15), generator=g)
    idx[0, 4], idx[1, 14] = -1, 3
    table, gx = torch.randn(3, 32, generator=g), torch.randn(2, 15, 32, generator=g)
    x, gtable = _lookup_run(idx, table, gx)
    bad = (idx < 0) | (idx >= 3)
    xc = x.cpu()
    assert bool(torch.isnan(xc[bad]).all()) and torch.equal(xc[~bad], table[idx[~bad]])
    want = torch.zeros(3, 32).index_add_(0, idx[~bad], gx[~bad])
    assert bool(torch.isfinite(gtable).all()) and rel_err(gtable, want) < 1e-6


# ------------------------------------------------------------------------------------------------ forward_tail
def _gpt64():
    from networks import GPT
    name = "gpt64"
    torch.manual_seed(G.SEEDS[name])
    m = G.init_gpt_(GPT(**G.gpt_kwargs(name)), G.SEEDS[name])
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, G.CASES[name][0], (2, 30), generator=g)
    import mingpt_ref as M
    prefix = M.round64(torch.randn(2, 5, 64, generator=g) / 4)
    return m, idx, prefix


def test_forward_tail_against_float64_and_forward():
    m, idx, prefix = _gpt64()
    assert m.config.n_unmasked == 5
    st = {k: v.detach().clone() for k, v in m.state_dict().items()}
    st64 = {k: (v if k.endswith("mask") else v.double()) for k, v in st.items()}
    with torch.no_grad():
        ref64 = G.gpt_ref(idx, st64, 2, 2, prefix.double())[0]
        ref32 = G.gpt_ref(idx, st, 2, 2, prefix)[0]
    m = m.to(DEV).eval()
    Ti, Te = idx.shape[1], prefix.shape[1]
    with torch.no_grad():
        full = m(idx.to(DEV), embeddings=prefix.to(DEV))
        for n_tail in (1, Ti, Te + Ti):
            tail = m.forward_tail(idx.to(DEV), prefix.to(DEV), n_tail=n_tail)
            assert tail.shape == (2, n_tail, 100)
            _gate(tail, ref64[:, -n_tail:], ref32[:, -n_tail:], "forward_tail n_tail=%d" % n_tail)
        assert torch.equal(tail, full), "n_tail = every position is forward() bit for bit"
        with pytest.raises(ValueError, match="n_tail"):
            m.forward_tail(idx.to(DEV), prefix.to(DEV), n_tail=Te + Ti + 1)


def test_forward_tail_advances_the_dropout_call_by_one():
    from networks import GPT
    torch.manual_seed(3)
    m = GPT(vocab_size=16, block_size=30, n_layer=2, n_head=2, n_embed=64, emb_pdrop=0.1, res_pdrop=0.1, att_pdrop=0.1, n_unmasked=5).to(DEV).train()
    m.seed_dropout(11, call=4)
    idx = torch.randint(0, 16, (2, 10), generator=torch.Generator().manual_seed(1)).to(DEV)
    prefix = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = m.forward_tail(idx, prefix, n_tail=10)
    assert m._dropout_call() == 5
    m.set_dropout_call(4)
    b = m(idx, embeddings=prefix)
    assert m._dropout_call() == 5 and torch.equal(a, b[:, -10:]), "the same sites under the same call"


# ------------------------------------------------------------------------------------------------ the tiny conditional trainer
def _state(seed=C.SEED):
    """The restatement's initial state: the GPT's state dict (init_gpt_) and the table (its rounding rule)."""
    from networks import GPT
    torch.manual_seed(seed)
    gpt = G.init_gpt_(GPT(**C.GPT_KW), seed)
    state = {k: v.detach().clone() for k, v in gpt.state_dict().items()}
    state[C.TABLE] = C.init_table_(torch.empty(C.L, C.E), seed)
    return state


def _trainer(state=None, pkeep=1.0, **kw):
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer
    state = _state() if state is None else state
    torch.manual_seed(77)
    vqgan = VQGAN(**dict(P.TINY_VQGAN, dict_size=C.V))
    gpt = GPT(**C.GPT_KW)
    gpt.load_state_dict({k: v for k, v in state.items() if k != C.TABLE})
    cond = LabelCondition(C.L, C.E, C.LAT_H, C.LAT_W)
    with torch.no_grad():
        cond.embed.weight.copy_(state[C.TABLE])
    o = C.OPTIM
    args = dict(pkeep=pkeep, sos_token=C.SOS, lr=o["lr"], betas=o["betas"], weight_decay=o["weight_decay"], grad_norm_clip=C.GRAD_NORM_CLIP,
                seed=17, device=DEV)
    args.update(kw)
    return ConditionalPriorTrainer(vqgan, gpt, cond, **args)


def _named(tr):
    return list(tr.gpt.named_parameters()) + [(C.TABLE, tr.cond.embed.weight)]


def test_the_mask_does_what_conditioning_needs():
    tr = _trainer()
    ids, cond = (t.to(DEV) for t in C.tiny_batch())
    tr.gpt.eval()
    with torch.no_grad():
        inp = tr._inputs(ids, 1.0)
        base = tr._logits(inp, tr.cond(cond))
        for t in (1, 7, C.T - 1):
            changed = inp.clone()
            changed[:, t] = (changed[:, t] + 1) % C.V
            out = tr._logits(changed, tr.cond(cond))
            assert torch.equal(out[:, :t], base[:, :t]) and not torch.equal(out[:, t], base[:, t]), "code %d is seen from position %d on only" % (t, t)
        for j in (0, C.TC - 1):          # ONE conditioning token reaches the first code's logits: the prefix is fully visible
            other = cond.clone()
            other[:, j] = (other[:, j] + 1) % C.L
            assert not torch.equal(tr._logits(inp, tr.cond(other))[:, 0], base[:, 0]), "conditioning token %d" % j
    assert base.shape == (C.B, C.T, C.V)


def _sampled(named):
    return {k: t.detach().double().cpu().reshape(-1)[sample_idx(t.numel(), 256, seed=1)] for k, t in named.items()}


@pytest.mark.parametrize("pkeep", [1.0, 0.7])
def test_training_step_against_the_restatement(pkeep):
    state = _state(C.STEP_SEED)
    ids, cond = C.tiny_batch(C.STEP_SEED)
    tr = _trainer(state, pkeep=pkeep, grad_norm_clip=C.STEP_CLIP)
    assert all(group["eps"] == C.OPTIM["eps"] == 1e-8 for group in tr.optim.param_groups)          # the optimiser as the trainer builds it
    uniforms = None
    if pkeep < 1:          # the trainer's own draws, step by step, from a generator in the trainer's state
        gen = torch.Generator(device=DEV).manual_seed(17)
        uniforms = [tuple(torch.rand(ids.shape, generator=gen, device=DEV).cpu() for _ in range(2)) for _ in range(C.STEPS)]
    truth = C.steps_ref(state, ids, cond, torch.float64, pkeep, uniforms)
    variants = [C.steps_ref(state, ids, cond, torch.float32, pkeep, uniforms, variant=v) for v in C.VARIANTS]
    assert float(truth["g0"][C.TABLE].norm()) > 0.1, "the table's truth gradient is not zero"          # on the CPU first
    sens = C.adam_step_sensitivity(truth["g0"], truth["coef"][0])
    print("pkeep %g: predicted parameter error of fp32 gradient noise after AdamW's first update %.2e" % (pkeep, sens))
    if pkeep >= 1:          # the case the seed was chosen for (cond_prior_ref.STEP_SEED); below 1 the corruption is the device's draw
        assert sens <= C.STEP_MAX_SENSITIVITY
    got = dict(loss=[], norm=[], coef=[])
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
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
            print("pkeep %g step %d %s: %.9g, restatement fp64 %.9g: %.2e apart, the restatement's own fp32 distance %.2e" % (
                pkeep, s, q, got[q][s], t64[s], err, own))
            if err > 2 * own or (q == "coef" and t64[s] == 1.0 and got[q][s] != 1.0):
                failures.append((q, s, err, own))
    assert min(truth["coef"]) < 1.0 and (pkeep < 1 or max(truth["coef"]) == 1.0), "the clip binds at some steps of the case and not at others"
    # the project's rule (test_gpu_prior.py): helpers.grad_gate on the sampled entries of every tensor
    grad_gate(_sampled(truth["g0"]), [_sampled(v["g0"]) for v in variants], _sampled(g0), what="pkeep %g gradient" % pkeep)
    grad_gate(_sampled(truth["P"]), [_sampled(v["P"]) for v in variants], _sampled(dict(_named(tr))), what="pkeep %g parameter" % pkeep)
    assert not failures, failures


def test_the_prior_learns_the_condition():
    state = _state()
    ids, cond = C.learn_batch()
    optim = dict(C.OPTIM, lr=C.LEARN_LR)
    ref = C.steps_ref(state, ids, cond, torch.float64, steps=C.LEARN_STEPS, optim=optim)
    st = dict(ref["P"], **{k: v for k, v in state.items() if k.endswith("mask")})
    gaps = C.learn_gap(st, ids, cond)
    print("the restatement after %d steps at lr %g: gaps %.3f and %.3f nats" % (C.LEARN_STEPS, C.LEARN_LR, gaps[0], gaps[1]))
    assert min(gaps) >= C.LEARN_MIN_GAP          # before anything about the device
    tr = _trainer(state, lr=C.LEARN_LR)
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    for _ in range(C.LEARN_STEPS):
        tr.training_step(batch)
    right = tr.token_nll(batch)[:, 0, 0]
    wrong = tr.token_nll({"ids": batch["ids"], "cond": batch["cond"].flip(0)})[:, 0, 0]
    print("the device: first-code nll right %s, swapped %s" % (right.tolist(), wrong.tolist()))
    assert bool((right < wrong).all())


# ------------------------------------------------------------------------------------------------ resume
def _everything(tr):
    out = {"p." + k: v for k, v in tr.gpt.state_dict().items()}
    out["table"] = tr.cond.embed.weight
    for i, (_, p) in enumerate(_named(tr)):
        st = tr.optim.state[p]
        out["m.%d" % i], out["v.%d" % i], out["t.%d" % i] = st["exp_avg"], st["exp_avg_sq"], torch.tensor(st["step"])
    out["generator"], out["step"] = tr.generator.get_state(), torch.tensor(tr.step_count)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def test_resume_is_bit_exact():
    from utils.checkpoint import _to_cpu
    ids, cond = C.tiny_batch()
    batch = {"ids": ids.to(DEV), "cond": cond.to(DEV)}
    kw = dict(pkeep=0.5, warmup_steps=3, decay_steps=6)
    full = _trainer(**kw)
    losses = [float(full.training_step(batch)["loss"]) for _ in range(4)]
    part = _trainer(**kw)
    first = [float(part.training_step(batch)["loss"]) for _ in range(2)]
    state = copy.deepcopy(_to_cpu(part.state_dict()))
    assert any(k.startswith("embed.") for k in state["modules"]["cond"]) and set(state["modules"]) == {"decoder", "transformer", "cond"}
    fresh = _trainer(_state(999), seed=5, **kw)          # other weights, another table, another generator
    fresh.load_state_dict(state)
    assert fresh.step_count == 2
    rest = [float(fresh.training_step(batch)["loss"]) for _ in range(2)]
    assert first + rest == losses
    a, b = _everything(full), _everything(fresh)
    assert a.keys() == b.keys()
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff[:8]
    assert int(a["step"]) == 4 and int(a["t.0"]) == 4 and not torch.equal(a["table"], _state()[C.TABLE])


# ------------------------------------------------------------------------------------------------ synthesize
def test_synthesize_returns_the_float64_tokens():
    state = _state()
    cond = C.tiny_batch()[1][:C.SYN_B]
    u = torch.rand(C.SYN_CANDIDATES, C.T, C.SYN_B, generator=torch.Generator().manual_seed(C.SYN_SEED))
    st64 = C.state_as(state, torch.float64)
    runs = [C.synth_truth(st64, cond, u[c]) for c in range(C.SYN_CANDIDATES)]
    min_dist, min_gap = min(r[1] for r in runs), min(r[2] for r in runs)
    print("synthesize, seed %d: smallest sample_ref dist %.3e (>= %.0e), smallest k / k+1 gap %.3e (>= %.0e)" % (
        C.SYN_SEED, min_dist, D.GEN_MIN_DIST, min_gap, D.GEN_MIN_GAP))
    assert min_dist >= D.GEN_MIN_DIST and min_gap >= D.GEN_MIN_GAP          # before anything about the device
    want = torch.stack([r[0] for r in runs], dim=1)          # (B, n, T)
    tr = _trainer(state)
    kw = dict(cond=cond.to(DEV), temperature=C.SYN_TEMP, top_k=C.SYN_TOPK)
    out = tr.synthesize(n_candidates=C.SYN_CANDIDATES, uniforms=u, **kw)
    again = tr.synthesize(n_candidates=C.SYN_CANDIDATES, uniforms=u.to(DEV), **kw)
    assert tr.gpt.training and out["candidates"].shape == want.shape and out["candidates"].dtype == torch.long
    assert torch.equal(out["candidates"].cpu(), want), "synthesize differs from the float64 run:\n%s\n%s" % (out["candidates"].cpu(), want)
    assert all(torch.equal(out[k], again[k]) for k in out)
    one = tr.synthesize(n_candidates=1, uniforms=u[:1], **kw)
    assert torch.equal(one["candidates"][:, 0], out["candidates"][:, 0]), "candidate 0 does not depend on n_candidates"
    # the ranking, the winner and its picture; scores are the candidates' conditional log-probabilities
    rows = torch.arange(C.SYN_B, device=DEV)
    assert out["scores"].dtype == torch.float64 and torch.equal(out["best"].cpu(), out["scores"].cpu().argmax(1))
    assert torch.equal(out["ids"], out["candidates"][rows, out["best"]]) and torch.equal(out["cond"].cpu(), cond)
    assert torch.equal(out["image"], tr.vqgan.decode_from_ids(out["ids"], C.LAT_H, C.LAT_W))
    nll = torch.stack([tr.token_nll({"ids": out["candidates"][:, c], "cond": cond.to(DEV)}).double().sum((1, 2)) for c in range(C.SYN_CANDIDATES)], dim=1)
    assert torch.allclose(out["scores"], -nll, rtol=1e-5, atol=0)
    # a generator in place of the uniforms: the same draws as edit makes them, repeatable under a seed
    g1 = tr.synthesize(n_candidates=2, generator=torch.Generator(device=DEV).manual_seed(3), **kw)
    g2 = tr.synthesize(n_candidates=2, generator=torch.Generator(device=DEV).manual_seed(3), **kw)
    assert torch.equal(g1["candidates"], g2["candidates"])
    with pytest.raises(ValueError, match="exactly one of label and cond"):
        tr.synthesize()


# ------------------------------------------------------------------------------------------------ edit(new_label=...)
def test_edit_with_a_new_label():
    from hipops import ops
    tr = _trainer()
    ids = C.tiny_batch()[0][:2].to(DEV)
    H, W = 8 * C.LAT_H, 8 * C.LAT_W          # 24 x 40
    label = torch.zeros(2, H, W, dtype=torch.uint8)
    label[0, :12] = 1
    label[1, :, 20:] = 2
    new = label.clone()
    new[0, 15:19, 9:22] = 2          # rows 15 .. 18: cell rows 1 and 2; columns 9 .. 21: cell columns 1 and 2
    new[1, 23, 39] = 0               # one pixel, the last cell
    label, new = label.to(DEV), new.to(DEV)
    batch = {"ids": ids, "label": label}
    kw = dict(n_candidates=3, temperature=1.0, top_k=8, top_p=0.95)
    out = tr.edit(batch, new_label=new, generator=torch.Generator(device=DEV).manual_seed(9), **kw)
    changed = ops.cells_changed(label, new, C.LAT_H, C.LAT_W)
    want = np.zeros((2, C.LAT_H, C.LAT_W), dtype=np.uint8)
    want[0, 1:3, 1:3] = 1
    want[1, 2, 4] = 1
    assert np.array_equal(changed.cpu().numpy(), want) and torch.equal(out["cellmask"], changed)
    keep = ~changed.bool().reshape(2, -1)
    for c in range(3):
        assert torch.equal(out["candidates"][:, c][keep], ids[keep]), "every code outside the changed cells is the source's"
    assert torch.equal(out["source_ids"], ids) and torch.equal(out["cond"], tr.cond.tokens(new))
    assert torch.equal(out["label_cells"], ops.cell_labels(new, C.LAT_H, C.LAT_W, C.L))
    assert "composite" not in out and out["edit"].shape[0] == 2
    # a score is minus the summed conditional token_nll of the candidate, under the NEW label's prefix
    nll = torch.stack([tr.token_nll({"ids": out["candidates"][:, c], "cond": out["cond"]}).double().sum((1, 2)) for c in range(3)], dim=1)
    assert torch.allclose(out["scores"], -nll, rtol=1e-5, atol=0)
    # nothing changed: nothing redrawn
    same = tr.edit(batch, new_label=label.clone(), generator=torch.Generator(device=DEV).manual_seed(9), **kw)
    assert not bool(same["cellmask"].any()) and torch.equal(same["ids"], ids) and torch.equal(same["ids"], same["source_ids"])
    # the other selectors run under the batch's own label
    by_mask = tr.edit(batch, mask=want[0].astype(bool), generator=torch.Generator(device=DEV).manual_seed(9), **kw)
    assert torch.equal(by_mask["cond"], tr.cond.tokens(label)) and np.array_equal(by_mask["cellmask"].cpu().numpy(), np.repeat(want[:1], 2, 0))
    with pytest.raises(ValueError, match="exactly one of mask, box, nll_threshold and new_label"):
        tr.edit(batch, mask=want[0].astype(bool), new_label=new)
    with pytest.raises(ValueError, match="exactly one of mask, box, nll_threshold and new_label"):
        tr.edit(batch)
    with pytest.raises(ValueError, match="'label'"):
        tr.edit({"ids": ids, "cond": out["cond"]}, new_label=new)
    with pytest.raises(NotImplementedError, match="leak|told where"):
        tr.detect(batch, nll_threshold=1.0)
    assert tr.gpt.training


def test_edit_pastes_cell_by_cell_into_a_picture():
    """{'image', 'label'} through the tiny VQGAN: 8 x 8 pictures, a 4 x 4 latent, cells of 2 x 2 pixels."""
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer
    import prior_edit_ref as R
    torch.manual_seed(5)
    vqgan = VQGAN(**dict(P.TINY_VQGAN, dict_size=C.V))
    gpt = G.init_gpt_(GPT(vocab_size=C.V, block_size=32, n_layer=2, n_head=2, n_embed=64, n_unmasked=16), 5)
    tr = ConditionalPriorTrainer(vqgan, gpt, LabelCondition(2, 64, 4, 4), device=DEV)
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    label = torch.zeros(2, 1, 8, 8, dtype=torch.uint8)
    new = label.clone()
    new[:, 0, 2:5, 4:6] = 1          # cell rows 1 and 2, cell column 2
    out = tr.edit({"image": image, "label": label.to(DEV)}, new_label=new.to(DEV), n_candidates=2, generator=torch.Generator(device=DEV).manual_seed(1))
    want = np.zeros((2, 4, 4), dtype=np.uint8)
    want[:, 1:3, 2] = 1
    assert np.array_equal(out["cellmask"].cpu().numpy(), want)
    assert torch.equal(out["composite"].cpu(), R.paste_ref(image.cpu(), out["edit"].cpu(), out["cellmask"].cpu()))
    loss = tr.training_step({"image": image, "label": label.to(DEV)})["loss"]
    assert bool(torch.isfinite(loss)) and tr.cond.embed.weight.grad is not None
    with pytest.raises(ValueError, match="'label'"):
        tr.training_step({"image": image})
    with pytest.raises(ValueError, match="'cond'"):
        tr.training_step({"ids": tr.codes({"image": image})})


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_trains_with_a_condition_and_synthesises(tmp_path):
    import filecmp
    import glob
    import os
    from run_helpers import read_csv, run_launcher, write_config
    from utils import png
    save = os.path.join(str(tmp_path), "run")

    def raw(**run):
        r = P.prior_run_config(save, **run)
        r["model"]["prior"]["cond"] = dict(source="label", n_labels=2, labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})
        r["synth"] = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, discs=[[16, 16, 5, 1]])
        return r
    out = run_launcher(write_config(os.path.join(str(tmp_path), "run.json"), raw()), "-p")
    vdir = os.path.join(save, "study", "version_0")
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == P.PRIOR_MONITORED and len(rows) == 3 and "validation cross-entropy" in out          # two steps and the validation
    assert all(np.isfinite(float(dict(zip(header, r))["loss"])) for r in rows[:2])
    pixels, _ = png.load(os.path.join(vdir, "000000.png"))
    assert pixels.shape == (3 * 32, 2 * 32)          # slices, reconstructions, draws from the slices' label maps
    ckpt = os.path.join(vdir, "ckpt-epoch=0000-total_loss=0.00.ckpt")
    ck = torch.load(ckpt, map_location="cpu")
    assert ck["state_dict"]["cond.embed.weight"].shape == (2, 64) and ck["state_dict"]["transformer.pos_embed"].shape == (1, 512, 64)
    assert ck["vqw_run_state"]["trainer"]["prior_step"] == 2
    dirs = []
    for i in (1, 2):
        out = run_launcher(write_config(os.path.join(str(tmp_path), "synth%d.json" % i), raw(resume_checkpoint=ckpt)), "-p", "-m", "synth")
        assert "Synthesised slices are saved" in out
        dirs.append(os.path.join(save, "study", "version_%d" % i, "synth"))
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dirs[0], "*")))
    assert names == ["slice_0000.png", "slice_0001.png", "synth.csv"]
    for name in names:
        assert filecmp.cmp(os.path.join(dirs[0], name), os.path.join(dirs[1], name), shallow=False), name + " differs between two runs"
    pixels, _ = png.load(os.path.join(dirs[0], "slice_0000.png"))
    assert pixels.shape == (32, 5 * 32) and pixels.dtype == np.uint8          # label | slice | synthesis | edited label | composite
    header, rows = read_csv(os.path.join(dirs[0], "synth.csv"))
    assert header == ["slice", "winner", "score", "cells_redrawn"] and [r[0] for r in rows] == ["0", "1"]
    assert all(int(r[1]) in (0, 1) and float(r[2]) < 0 and 0 < int(r[3]) <= 49 for r in rows)          # a disc of radius 5: at most 7 x 7 cells of 2 x 2
