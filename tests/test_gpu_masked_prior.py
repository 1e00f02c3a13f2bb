"""The bidirectional masked prior on the GPU: ops.select_lowest, ops.mask_tokens and ops.unmask_step against the integer / float64
restatement of tests/masked_prior_ref.py, MaskedGPT.forward against the float64 restatement of tests/gpt_ref.py under an all-ones
mask, MaskedGPT.generate_parallel against the same loop composed from its three operators, and MaskedPriorTrainer's step, resume
and edit.

Sets are compared exactly: the select is decided on integer keys, and the kept set of unmask_step is checked against the reference
select applied to the confidences the device itself returned, so no float comparison decides a set.  The confidences are the one
float comparison: CONF_ALLOWANCE below."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, rel_err
from run_helpers import read_csv, run_launcher, write_config
import gpt_ref as G
import masked_prior_ref as R
import prior_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_ULP = 2.0 ** -23

# The confidences logp + tau g against float64, as |device - float64| / max(1, |float64|) over the inputs of test_unmask_step (two
# logf calls, each within a few ulp, of values up to about 17 in magnitude, times tau <= 4.5; where -logf(u) is near 1 the inner
# call's relative error becomes an absolute one of the outer, times tau, on a confidence of magnitude 1).  Measured on the MI355X:
# 3.87e-7 at T = 16 and 6.70e-7 at T = 257 at their largest; the allowance is four times the larger.
CONF_MEASURED = 6.70e-7
CONF_ALLOWANCE = 4 * CONF_MEASURED


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the select
def _keys(kind, B, T, rng):
    if kind == "normal":
        return rng.standard_normal((B, T)).astype(np.float32)
    if kind == "equal":
        return np.full((B, T), 0.25, dtype=np.float32)
    if kind == "two":          # long ties that straddle the threshold
        return np.where(rng.random((B, T)) < 0.5, np.float32(-1.5), np.float32(2.0)).astype(np.float32)
    special = np.array([-0.0, 0.0, -np.inf, np.inf, 1.0, -1.0, 1e-45, -1e-45], dtype=np.float32)
    return special[rng.integers(0, special.size, size=(B, T))]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_select_lowest_is_exact(T):
    from hipops import ops
    B, rng = 3, np.random.default_rng(1000 + T)
    for kind in ("normal", "equal", "two", "special"):
        keys = _keys(kind, B, T, rng)
        kd = torch.from_numpy(keys).to(DEV)
        for elig_kind in ("all", "none", "random"):
            elig = {"all": None, "none": np.zeros((B, T), dtype=np.uint8), "random": (rng.random((B, T)) < 0.6).astype(np.uint8)}[elig_kind]
            ed = None if elig is None else torch.from_numpy(elig).to(DEV)
            count = np.full(B, T) if elig is None else elig.sum(1)
            for n in (np.zeros(B), np.ones(B), count - 1, count, count + 5):
                n = n.astype(np.int32)
                nd = torch.from_numpy(n).to(DEV)
                got = _np(ops.select_lowest(kd, nd, ed))
                what = (T, kind, elig_kind, n.tolist())
                assert got.dtype == np.uint8 and np.array_equal(got, R.select_lowest(keys, n, elig)), what
                assert got.sum(1).tolist() == np.minimum(np.maximum(n, 0), count).tolist(), what
                assert np.array_equal(_np(ops.select_lowest(kd, nd, ed)), got), what          # two runs, the same bytes
    # one integer for every row, and a bool eligibility
    keys = _keys("two", B, T, rng)
    elig = rng.random((B, T)) < 0.5
    got = _np(ops.select_lowest(torch.from_numpy(keys).to(DEV), 2, torch.from_numpy(elig).to(DEV)))
    assert np.array_equal(got, R.select_lowest(keys, 2, elig))


# ------------------------------------------------------------------------------------------------ 2. the corruption of a step
@pytest.mark.parametrize("T", [16, 256, 1000])
def test_mask_tokens_bit_equal(T):
    from hipops import ops
    cases = [c for c in R.MASK_CASES if c[3] == T]
    assert len(cases) == 3
    V = 64
    for seed, call, B, _ in cases:
        ids = np.random.default_rng(T + call % 7).integers(0, V, size=(B, T))
        idd = torch.from_numpy(ids).to(DEV)
        inp, masked, n = ops.mask_tokens(idd, V, seed, call)
        assert inp.dtype == torch.long and masked.dtype == torch.uint8 and n.dtype == torch.int32
        ri, rm, rn = R.mask_tokens(ids, V, seed, call)
        assert np.array_equal(_np(n), rn) and np.array_equal(_np(masked), rm) and np.array_equal(_np(inp), ri), (seed, call, T)
        assert _np(masked).sum(1).tolist() == _np(n).tolist()                      # exactly n, no Bernoulli draw
        assert np.array_equal(_np(inp) != ids, _np(masked) != 0)                   # V is no code: inp differs exactly where masked
        again = ops.mask_tokens(idd, V, seed, call)
        assert all(torch.equal(a, b) for a, b in zip(again, (inp, masked, n)))     # a function of (seed, call) alone
        assert not torch.equal(ops.mask_tokens(idd, V, seed, call + 1)[1], masked)
        for ratio in (1.0, 0.5, 0.3):
            fi, fm, fn = ops.mask_tokens(idd, V, seed, call, ratio=ratio)
            ri, rm, rn = R.mask_tokens(ids, V, seed, call, ratio=ratio)
            assert np.array_equal(_np(fn), rn) and np.array_equal(_np(fm), rm) and np.array_equal(_np(fi), ri), (seed, call, T, ratio)
        assert bool(ops.mask_tokens(idd, V, seed, call, ratio=1.0)[1].all())


# ------------------------------------------------------------------------------------------------ 3. one decoding iteration
def _unmask_inputs(T):
    B, V, rng = 4, 50, np.random.default_rng(300 + T)
    tokens = rng.integers(0, V, size=(B, T))
    logp = (-3.0 * np.abs(rng.standard_normal((B, T)))).astype(np.float32)
    logp[:, ::5] = np.float32(-1.25)                      # ties among the confidences at tau = 0
    masked = (rng.random((B, T)) < 0.6).astype(np.uint8)
    masked[0] = 0                                         # fully known
    masked[1] = 1                                         # fully masked
    u = rng.random((B, T)).astype(np.float32)
    u[:, 1], u[:, 2], u[:, 3] = 0.0, np.float32(1.0 - 2.0 ** -24), np.float32(2.0 ** -30)          # the clamp's two ends
    return V, tokens, logp, masked, u


@pytest.mark.parametrize("T", [16, 257])
def test_unmask_step(T):
    from hipops import ops
    V, tokens, logp, masked, u = _unmask_inputs(T)
    B, was = tokens.shape[0], masked != 0
    td, ld, md, ud = (torch.from_numpy(a).to(DEV) for a in (tokens, logp, masked, u))
    m0 = np.full(B, T, dtype=np.int32)
    m0d = torch.from_numpy(m0).to(DEV)
    worst = 0.0
    for gamma in (0.0, 0.5, 0.25, 1.0 - 1e-6):
        for tau in (0.0, 1.0, 4.5):
            fixed_in = np.full((B, T), 7.5, dtype=np.float32)
            fd = torch.from_numpy(fixed_in).to(DEV)
            ids_out, masked_out, fixed, conf = ops.unmask_step(td, ld, md, m0d, gamma, tau, V, u=None if tau == 0 else ud, fixed_logp=fd,
                                                               return_conf=True)
            assert fixed is fd                                                     # in place
            ids_out, masked_out, fixed, conf = _np(ids_out), _np(masked_out), _np(fixed), _np(conf)
            what = (T, gamma, tau)
            # the confidences against float64
            c64 = R.confidence(logp, u, tau)
            dev = float((np.abs(conf.astype(np.float64) - c64) / np.maximum(1.0, np.abs(c64)))[was].max())
            worst = max(worst, dev)
            assert np.isposinf(conf[~was]).all(), what
            if tau == 0:
                assert np.array_equal(conf[was].view(np.uint32), logp[was].view(np.uint32)), what          # logp itself, bit for bit
            # the kept set: the reference select on the RETURNED confidences
            ri, rm, rf = R.unmask_step(tokens, logp, masked, m0, gamma, V, conf, fixed_in)
            assert np.array_equal(masked_out, rm) and np.array_equal(ids_out, ri), what
            assert np.array_equal(fixed.view(np.uint32), rf.view(np.uint32)), what
            # what the rules say, without the reference
            keep = masked_out != 0
            assert not (keep & ~was).any() and np.array_equal(ids_out == V, keep), what          # mask_token exactly where still masked
            assert np.array_equal(ids_out[~was], tokens[~was]) and (fixed[~was] == 7.5).all(), what          # the known are untouched
            assert (fixed[keep] == 7.5).all() and np.array_equal(fixed[was & ~keep], logp[was & ~keep]), what
            cur = was.sum(1)
            if gamma == 0.0:
                assert not keep.any(), what                                        # gamma = 0 clears the mask
            if gamma > 0.99:
                assert (cur - keep.sum(1)).tolist() == (cur > 0).astype(int).tolist(), what          # still one code per non-empty row
            assert keep.sum(1).tolist() == R.n_keep(cur, m0, gamma).tolist(), what
    print("unmask_step T=%d: the confidences deviate from float64 by at most %.3e (allowance %.3e)" % (T, worst, CONF_ALLOWANCE))
    assert worst <= CONF_ALLOWANCE
    # u=None is accepted at tau = 0 and refused otherwise; a fresh fixed_logp starts from zeros
    ids_out, masked_out, fixed = ops.unmask_step(td, ld, md, m0d, 0.5, 0.0, V)
    assert float(fixed[~torch.from_numpy(was).to(DEV)].abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="needs the uniforms"):
        ops.unmask_step(td, ld, md, m0d, 0.5, 1.0, V)
    with pytest.raises(RuntimeError, match="must be finite"):
        ops.unmask_step(td, ld, md, m0d, float("nan"), 0.0, V)


# ------------------------------------------------------------------------------------------------ 4. the model
TINY = dict(vocab_size=32, block_size=16, n_layer=2, n_head=2, n_embed=64)
_models = {}


def _tiny(cls_name="MaskedGPT", **kw):
    import networks
    key = (cls_name, tuple(sorted(kw.items())))
    if key not in _models:
        torch.manual_seed(411)
        _models[key] = G.init_gpt_(getattr(networks, cls_name)(**dict(TINY, **kw)), 411).to(DEV).eval()
    return _models[key]


def test_masked_gpt_forward_is_bidirectional(golden):
    m, causal = _tiny(), _tiny("GPT")
    idx = torch.randint(0, 33, (2, 16), generator=torch.Generator().manual_seed(412))
    idx[0, 3] = idx[1, 9] = 32                            # the mask token is a row of the table
    other = idx.clone()
    other[:, -1] = (other[:, -1] + 5) % 32
    with torch.no_grad():
        a, b = m(idx.to(DEV)), m(other.to(DEV))
        ca, cb = causal(idx.clamp(max=31).to(DEV)), causal(other.clamp(max=31).to(DEV))
    assert a.shape == (2, 16, 32)
    assert not torch.equal(a[:, 0], b[:, 0])              # position 0 sees the last token
    assert torch.equal(ca[:, :-1], cb[:, :-1]) and not torch.equal(ca[:, -1], cb[:, -1])          # a causal GPT of the same size does not
    st = {k: (v.detach().cpu() if k.endswith("mask") else v.detach().cpu().double()) for k, v in m.state_dict().items()}
    assert all(bool((v != 0).all()) for k, v in st.items() if k.endswith("mask"))
    ref = G.gpt_ref(idx, st, TINY["n_layer"], TINY["n_head"])[0]
    sp = float(golden("mingpt_gpt_gpt64.npz")["gpt64/spread.out"])          # test_gpt_fixture's bound for GPT.forward at n_unmasked > 0
    print("MaskedGPT logits: %.3e from float64 (bound 2 x %.1e)" % (rel_err(a, ref), sp))
    assert_close(a, ref, 2.0 * sp, "MaskedGPT logits")


# ------------------------------------------------------------------------------------------------ 5. parallel decoding
@pytest.mark.parametrize("n_steps", [1, 4])
def test_generate_parallel(n_steps):
    from hipops import ops
    m = _tiny()
    B, T, V = 3, 16, 32
    g = torch.Generator().manual_seed(500 + n_steps)
    ids = torch.randint(0, V, (B, T), generator=g).to(DEV)
    masked = (torch.rand(B, T, generator=g) < 0.6).to(torch.uint8)
    masked[1], masked[2] = 1, 0                           # one row fully masked, one fully known
    masked = masked.to(DEV)
    uniforms = torch.rand(n_steps, 2, B, T, generator=g).to(DEV)
    kw = dict(temperature=0.9, top_k=8, top_p=0.9, choice_temperature=4.5)
    out, fixed = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, **kw)
    # the same loop from forward, ops.sample_filtered and ops.unmask_step
    m0 = masked.sum(1, dtype=torch.int32)
    want_counts = R.masked_counts_after(_np(m0), n_steps)
    cur, mk, fx = torch.where(masked != 0, torch.full_like(ids, V), ids), masked, torch.zeros(B, T, device=DEV)
    with torch.no_grad():
        for k in range(n_steps):
            gamma, tau = R.unmask_schedule(k, n_steps, 4.5)
            forced = torch.where(mk != 0, torch.full_like(cur, -1), cur).reshape(-1)
            tokens, logp = ops.sample_filtered(m(cur).reshape(B * T, V), uniforms[k, 0].reshape(-1), forced, 0.9, 8, 0.9)
            cur, mk, fx = ops.unmask_step(tokens.view(B, T), logp.view(B, T), mk, m0, gamma, tau, V, u=uniforms[k, 1], fixed_logp=fx)
            assert _np(mk).sum(1).tolist() == want_counts[k].tolist(), k          # the reference schedule
    assert torch.equal(out, cur) and torch.equal(fixed.view(torch.int32), fx.view(torch.int32))
    known = masked == 0
    assert torch.equal(out[known], ids[known])            # known codes come back unchanged
    assert int(out.max()) < V and int(out.min()) >= 0     # no mask token is left
    assert torch.equal(out[2], ids[2]) and float(fixed[2].abs().max()) == 0.0          # a fully known row
    assert float(fixed[known].abs().max()) == 0.0 and bool((fixed[~known] < 0).all())
    again = m.generate_parallel(ids, masked, n_steps, uniforms=uniforms, **kw)
    assert torch.equal(again[0], out) and torch.equal(again[1], fixed)
    # a generator in place of the uniforms repeats under its seed
    a = m.generate_parallel(ids, masked, n_steps, generator=torch.Generator(device=DEV).manual_seed(3), **kw)
    b = m.generate_parallel(ids, masked, n_steps, generator=torch.Generator(device=DEV).manual_seed(3), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0][known], ids[known]) and not m.training


# ------------------------------------------------------------------------------------------------ 6. the trainer
def _trainer(init_seed=611, **kw):
    from networks import MaskedGPT, VQGAN
    from trainers import MaskedPriorTrainer
    torch.manual_seed(77)
    vqgan = VQGAN(**P.TINY_VQGAN)
    torch.manual_seed(init_seed)
    gpt = G.init_gpt_(MaskedGPT(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64), init_seed)
    args = dict(n_steps=4, mask_seed=21, lr=3e-3, betas=P.OPTIM["betas"], weight_decay=P.OPTIM["weight_decay"], grad_norm_clip=1.0, seed=17,
                device=DEV)
    args.update(kw)
    return MaskedPriorTrainer(vqgan, gpt, **args)


def _ids():
    return torch.randint(0, 64, (4, 16), generator=torch.Generator().manual_seed(612)).to(DEV)


def test_training_step_loss_is_the_masked_mean(golden):
    tr, ids = _trainer(), _ids()
    g = golden("prior_step_p64.npz")          # test_training_step_against_the_reference's bound for the loss
    own = max(float((np.abs(g["p64/loss32"] - g["p64/loss64"][None]) / np.abs(g["p64/loss64"][None])).max()), FP32_ULP)
    for step in range(2):
        inp, masked, n = R.mask_tokens(_np(ids), 64, 21, step)
        with torch.no_grad():
            logits = tr.gpt(torch.from_numpy(inp).to(DEV)).double().cpu()          # the device's own logits, before the update
        nll = torch.logsumexp(logits, -1) - logits.gather(-1, ids.cpu()[..., None])[..., 0]
        want = float((nll * torch.from_numpy(masked != 0)).sum() / int(n.sum()))
        out = tr.training_step({"ids": ids})
        got = float(out["loss"])
        err = abs(got - want) / abs(want)
        print("masked step %d: loss %.9g, float64 masked mean %.12g: %.2e apart (bound 2 x %.2e)" % (step, got, want, err, own))
        assert err <= 2 * own and out["ids"] is ids and out["grad_norm"].is_cuda and tr.step_count == step + 1


def test_twenty_steps_lower_the_validation_loss():
    tr, ids = _trainer(), _ids()
    before = tr.validation_step({"ids": ids})
    assert float(before["ppl"]) == pytest.approx(np.exp(float(before["loss"])), rel=1e-6) and not before["loss"].requires_grad
    assert float(tr.validation_step({"ids": ids})["loss"]) == float(before["loss"])          # ratio 0.5 under call 0: one number per batch
    for _ in range(20):
        tr.training_step({"ids": ids})
    after = tr.validation_step({"ids": ids})
    print("validation loss %.4f -> %.4f after twenty steps" % (float(before["loss"]), float(after["loss"])))
    assert float(after["loss"]) < float(before["loss"]) and tr.gpt.training


def test_resume_is_bit_exact():
    from utils.checkpoint import _to_cpu
    ids = _ids()
    full = _trainer()
    outs = [full.training_step({"ids": ids}) for _ in range(3)]
    full_bits = [(float(o["loss"]), float(o["grad_norm"])) for o in outs]
    part = _trainer()
    first = [part.training_step({"ids": ids}) for _ in range(2)]
    state = copy.deepcopy(_to_cpu(part.state_dict()))
    fresh = _trainer(init_seed=999, seed=5)               # other weights, another generator; the same mask_seed
    fresh.load_state_dict(state)
    assert fresh.step_count == 2
    nxt = fresh.training_step({"ids": ids})
    assert [(float(o["loss"]), float(o["grad_norm"])) for o in first] == full_bits[:2]
    assert (float(nxt["loss"]), float(nxt["grad_norm"])) == full_bits[2]
    for (k, a), (_, b) in zip(full.gpt.state_dict().items(), fresh.gpt.state_dict().items()):
        assert torch.equal(a, b), k
    # the mask is really a function of mask_seed: another one ends elsewhere
    assert float(_trainer(mask_seed=22).training_step({"ids": ids})["loss"]) != full_bits[0][0]


def test_edit_keeps_the_contract():
    tr = _trainer()
    image = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(78)).to(DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)          # noqa: E731
    box = (2, 6, 2, 6)                                    # the four central cells of the 4 x 4 latent
    out = tr.edit({"image": image}, box=box, n_candidates=3, n_steps=4, top_k=16, top_p=0.95, generator=gen())
    assert set(out) == {"ids", "source_ids", "candidates", "scores", "best", "cellmask", "recon", "edit", "composite"}
    cells = out["cellmask"].reshape(2, 16) != 0
    assert out["cellmask"].dtype == torch.uint8 and cells.sum(1).tolist() == [4, 4]
    src, cand = out["source_ids"], out["candidates"]
    assert cand.shape == (2, 3, 16) and out["scores"].shape == (2, 3) and out["scores"].dtype == torch.float64
    assert torch.equal(cand[~cells[:, None].expand_as(cand)], src[:, None].expand_as(cand)[~cells[:, None].expand_as(cand)])
    assert int(cand.max()) < 64 and bool((out["scores"] < 0).all())
    rows = torch.arange(2, device=DEV)
    assert torch.equal(out["best"], out["scores"].argmax(1)) and torch.equal(out["ids"], cand[rows, out["best"]])
    assert out["composite"].shape == image.shape and out["edit"].shape == image.shape and tr.gpt.training
    one = tr.edit({"image": image}, box=box, n_candidates=1, n_steps=4, top_k=16, top_p=0.95, generator=gen())
    assert torch.equal(one["candidates"][:, 0], cand[:, 0]) and torch.equal(one["scores"][:, 0], out["scores"][:, 0])
    ids_only = tr.edit({"ids": src}, mask=_np(cells).reshape(2, 4, 4), n_candidates=3, n_steps=4, top_k=16, top_p=0.95, generator=gen())
    assert "composite" not in ids_only and torch.equal(ids_only["candidates"], cand)
    with pytest.raises(NotImplementedError, match="raster-order likelihood"):
        tr.edit({"image": image}, nll_threshold=2.0)
    sample = tr.sample_ids(3, top_k=16, generator=gen())
    assert sample.shape == (3, 16) and int(sample.max()) < 64 and int(sample.min()) >= 0
    assert tr.sample_images(2, generator=gen()).shape == (2, 1, 8, 8)


def test_launcher_trains_and_edits_with_the_masked_prior(tmp_path):
    """run_vqwnet.py -p and -p -m edit pick the masked trainer from model.prior.masked: one training run (two steps, a validation, a
    picture decoded from an all-masked grid, a checkpoint) and one edit from that checkpoint in edit.n_steps passes."""
    save = os.path.join(str(tmp_path), "run")
    masked = dict(n_steps=3, choice_temperature=4.5, mask_seed=4)
    raw = P.prior_run_config(save)
    raw["model"]["prior"]["masked"] = masked
    out = run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), raw), "-p")
    vdir = os.path.join(save, "study", "version_0")
    ckpt = os.path.join(vdir, "ckpt-epoch=0000-total_loss=0.00.ckpt")
    assert "validation cross-entropy" in out and os.path.exists(ckpt) and os.path.exists(os.path.join(vdir, "000000.png"))
    assert tuple(torch.load(ckpt, map_location="cpu")["state_dict"]["transformer.tok_embed.weight"].shape) == (9, 64)          # 8 codes + the mask token
    raw = P.prior_run_config(save, resume_checkpoint=ckpt)
    raw["model"]["prior"]["masked"] = masked
    raw["edit"] = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[8, 16, 8, 24], n_steps=2)
    out = run_launcher(write_config(os.path.join(str(tmp_path), "edit.json"), raw), "-p", "-m", "edit")
    assert "Loading model from" in out and "Edited slices are saved" in out
    edir = os.path.join(save, "study", "version_1", "edit")
    assert sorted(os.listdir(edir)) == ["codes_0000.npy", "codes_0001.npy", "edit.csv", "slice_0000.png", "slice_0001.png"]
    codes = np.load(os.path.join(edir, "codes_0001.npy"))
    cells = np.zeros((16, 16), dtype=np.int64)
    cells[4:8, 4:12] = 1
    assert codes.shape == (3, 16, 16) and np.array_equal(codes[2], cells) and np.array_equal(codes[0][cells == 0], codes[1][cells == 0])
    assert codes.min() >= 0 and codes[:2].max() < 8          # no mask token (8) is left
    header, rows = read_csv(os.path.join(edir, "edit.csv"))
    assert header == ["slice", "candidate", "score", "rank", "n_resampled"] and len(rows) == 6
    assert all(int(r[4]) == 32 and float(r[2]) < 0 for r in rows)
