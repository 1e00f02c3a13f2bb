"""The GPT code prior's training on the GPU: the gradient-norm and AdamW kernels against float64 / torch.optim.AdamW on the CPU, the
input-token kernel bit for bit, the VQGAN's code side, PriorTrainer's step against the reference's fixtures
(tests/golden/prior_step_*.npz), bit-exact resume, sampling, and one -p run of the launcher with its resume.

The step's bounds.  Gradients of step 0 and parameters after step 3: helpers.grad_gate at its defaults, on the fixture's sampled
entries (helpers.sample_idx(numel, 256, seed=1) of every tensor), with the reference's fp64 values as the truth and its three fp32
evaluations as the spread.  The three losses, pre-clip norms and clip coefficients: each within twice the reference's own
fp32-to-fp64 distance for that quantity - the largest relative distance of its three fp32 evaluations from its fp64 values over
the three steps, floored at one fp32 unit in the last place (2^-23: a number held in fp32 cannot be expected closer to the truth
than its format allows); a coefficient the reference does not clip (exactly 1) must be exactly 1.

Why the distance is taken over the steps and not step by step.  The fixture's three fp32 evaluations are the same torch code and
move together: on p64 their norms sit -4.02e-6, -4.08e-6, -4.14e-6 from fp64 at step 1 and -0.46e-6, -0.18e-6, -1.48e-6 at step 2,
so a single step's spread says little about fp32.  Another mathematically identical fp32 evaluation on the CPU, prior_ref.steps_ref
in fp32 (plain torch, the optimiser written out), gives +3.63e-6 ... +4.10e-6 at step 2: beyond twice that step's 1.48e-6, within
twice the quantity's 4.14e-6.  Measured on the MI355X for p64, as relative distances (loss | norm): step 0 5.9e-9 | 6.6e-8, step 1
8.4e-7 | 2.0e-6, step 2 1.2e-6 | 3.7e-6 - a step-by-step bound is missed at the step-2 norm (3.7e-6 against 2 x 1.48e-6) exactly as
the CPU restatement misses it; every other figure of both cases is inside either bound."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, grad_gate, rel_err, sample_idx
from run_helpers import read_csv, run_launcher, write_config
import gpt_ref as G
import prior_ref as P
import vqgan_model_ref as VM

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_ULP = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ vqw_grad_norm_multi
def _norm(grads, max_norm):
    """(norm, coef) as two fp32 numbers through vqw_grad_norm_multi on the chunk table hipops.optim builds."""
    from hipops import ops, optim
    L = ops._L()
    rows = []
    for g in grads:
        rows += optim._chunk_rows(g, g, g, g)          # the kernel reads the g and n fields only
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.vqw_grad_norm_ws_bytes(len(rows)) // 8, dtype=torch.float64, device=DEV)
    out = torch.full((2,), -1.0, device=DEV)
    L.vqw_grad_norm_multi(table, len(rows), float(max_norm), ws, ws.numel() * 8, out)
    return out.cpu().numpy().copy(), len(rows)


def _expected_coef(norm32, max_norm):
    if max_norm <= 0:
        return np.float32(1.0)
    return min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


@pytest.mark.parametrize("chunk,sizes", [(None, (1, 3, 16384, 16385, 70000)), (256, (1, 3, 16384, 16385, 70000)), (256, (300000,))])
def test_grad_norm_against_float64(monkeypatch, chunk, sizes):
    from hipops import optim
    if chunk is not None:
        monkeypatch.setattr(optim, "CHUNK", chunk)
    g = torch.Generator().manual_seed(sum(sizes) + (chunk or 0))
    cpu = [torch.randn(n, generator=g) * (0.5 + i) for i, n in enumerate(sizes)]
    dev = [t.to(DEV) for t in cpu]
    want = float(torch.linalg.vector_norm(torch.cat([t.double() for t in cpu])))
    above, below = 2.0 * want, 0.25 * want
    (norm, coef), records = _norm(dev, above)
    if sizes == (300000,):
        assert records > 1024          # the second stage walks its partials more than once
    print("grad norm %s chunk %s: %d records, %.9g vs float64 %.9g (rel %.2e)" % (sizes, chunk, records, norm, want, abs(float(norm) - want) / want))
    assert abs(float(norm) - want) <= 1e-6 * want
    assert coef == np.float32(1.0) == _expected_coef(norm, above)          # a norm below max_norm is not clipped
    (norm2, coef2), _ = _norm(dev, below)
    assert norm2.tobytes() == norm.tobytes()                                # the same bits every run
    assert coef2 == _expected_coef(norm, below) and abs(float(coef2) - below / (want + 1e-6)) <= 1e-6 * 0.25
    (norm3, coef3), _ = _norm(dev, 0.0)
    assert norm3.tobytes() == norm.tobytes() and coef3 == np.float32(1.0)   # max_norm = 0: no clip
    for _ in range(2):
        again, _ = _norm(dev, below)
        assert again.tobytes() == np.array([norm2, coef2], dtype=np.float32).tobytes()


def test_grad_norm_does_not_depend_on_the_alignment():
    """A gradient that starts 4 bytes into an allocation goes through 4-byte loads, the same additions in the same order."""
    g = torch.Generator().manual_seed(7)
    base = torch.randn(40001, generator=g).to(DEV)
    for off in (1, 2, 3):
        view = base[off:]
        assert view.data_ptr() % 16 != 0
        a, _ = _norm([view], 1.0)
        b, _ = _norm([view.clone()], 1.0)
        assert a.tobytes() == b.tobytes()
        assert abs(float(a[0]) - float(view.double().norm())) <= 1e-6 * float(a[0])


# ------------------------------------------------------------------------------------------------ hipops.AdamW
ADAMW_SHAPES = [(64, 64), (64,), (1, 16, 64), (70000,)]
ADAMW_DECAYED = (0, 3)
ADAMW_KW = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8)


def _adamw_groups(ps, wd=0.01):
    return [{"params": [ps[i] for i in ADAMW_DECAYED], "weight_decay": wd},
            {"params": [p for i, p in enumerate(ps) if i not in ADAMW_DECAYED], "weight_decay": 0.0}]


def _adamw_run(max_grad_norm, steps=3, wd=0.01, reference=True):
    """Three steps on given gradients -> (reference parameters and optimiser or None, this project's, the norms torch measured)."""
    from hipops import AdamW
    g = torch.Generator().manual_seed(4)
    ref = [torch.randn(sh, generator=g).requires_grad_(True) for sh in ADAMW_SHAPES]
    mine = [p.detach().clone().to(DEV).requires_grad_(True) for p in ref]
    o_ref = torch.optim.AdamW(_adamw_groups(ref, wd), **ADAMW_KW) if reference else None
    o_mine = AdamW(_adamw_groups(mine, wd), max_grad_norm=max_grad_norm, **ADAMW_KW)
    norms = []
    for step in range(steps):
        grads = [torch.randn(p.shape, generator=g) * (0.1 + step) for p in ref]
        for q, gr in zip(mine, grads):
            q.grad = gr.clone().to(DEV)
        o_mine.step()
        for q, gr in zip(mine, grads):
            assert torch.equal(q.grad.cpu(), gr)          # p.grad keeps the unclipped values
        if reference:
            for p, gr in zip(ref, grads):
                p.grad = gr.clone()
            norms.append(float(torch.linalg.vector_norm(torch.cat([gr.double().reshape(-1) for gr in grads]))))
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(ref, max_grad_norm)
            o_ref.step()
    return ref, o_ref, mine, o_mine, norms


@pytest.mark.parametrize("route", ["multi", "per_tensor"])
@pytest.mark.parametrize("max_grad_norm", [None, 100.0])
def test_adamw_matches_torch(monkeypatch, route, max_grad_norm):
    """The tolerances of test_adam_weight_decay_matches_torch, for the same arithmetic."""
    from hipops import optim
    monkeypatch.setattr(optim, "MULTI_TENSOR", route == "multi")
    ref, o_ref, mine, o_mine, norms = _adamw_run(max_grad_norm)
    if max_grad_norm is not None:          # some steps clip and some do not
        assert min(norms) < max_grad_norm < max(norms)
        assert abs(float(o_mine.last_grad_norm) - norms[-1]) <= 1e-6 * norms[-1]
        assert abs(float(o_mine.last_clip_coef) - max_grad_norm / (norms[-1] + 1e-6)) <= 1e-6
    else:
        assert o_mine.last_grad_norm is None
    for i, (p, q) in enumerate(zip(ref, mine)):
        assert o_mine.state[q]["step"] == 3
        assert_close(q, p, 5e-6, "parameter %d after three steps" % i)
        assert_close(o_mine.state[q]["exp_avg"], o_ref.state[p]["exp_avg"], 2e-6, "exp_avg %d" % i)
        assert_close(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"], 3e-5, "exp_avg_sq %d" % i)


def test_adamw_routes_agree_bit_for_bit(monkeypatch):
    from hipops import optim
    monkeypatch.setattr(optim, "MULTI_TENSOR", True)
    _, _, multi, o_multi, _ = _adamw_run(100.0, reference=False)
    monkeypatch.setattr(optim, "MULTI_TENSOR", False)
    _, _, single, o_single, _ = _adamw_run(100.0, reference=False)
    assert torch.equal(o_multi.last_grad_norm, o_single.last_grad_norm) and torch.equal(o_multi.last_clip_coef, o_single.last_clip_coef)
    for i, (a, b) in enumerate(zip(multi, single)):
        for k in ("exp_avg", "exp_avg_sq"):
            x, y = o_multi.state[a][k], o_single.state[b][k]
            assert torch.equal(x, y), "%s %d: %d entries differ, by up to %.3e" % (k, i, int((x != y).sum()), float((x - y).abs().max()))
        assert torch.equal(a, b), "parameter %d: %d entries differ, by up to %.3e" % (i, int((a != b).sum()), float((a - b).abs().max()))


def test_adamw_decay_is_decoupled_and_per_group():
    _, _, decayed, _, _ = _adamw_run(None, reference=False)
    _, _, plain, _, _ = _adamw_run(None, wd=0.0, reference=False)
    for i, (a, b) in enumerate(zip(decayed, plain)):
        if i in ADAMW_DECAYED:          # three steps of p *= 1 - 3e-3 * 0.01: 9e-5 of the parameter
            assert 5e-5 < rel_err(a, b) < 2e-4, (i, rel_err(a, b))
        else:
            assert torch.equal(a, b), i


def test_adamw_clip_is_really_applied():
    """max_grad_norm at a tenth of the norm: exp_avg after one step is a tenth of the unclipped run's."""
    _, _, free, o_free, _ = _adamw_run(None, steps=1, reference=False)
    g = torch.Generator().manual_seed(4)
    [torch.randn(sh, generator=g) for sh in ADAMW_SHAPES]
    norm = float(torch.linalg.vector_norm(torch.cat([(torch.randn(sh, generator=g) * 0.1).double().reshape(-1) for sh in ADAMW_SHAPES])))
    _, _, clipped, o_clipped, _ = _adamw_run(norm / 10, steps=1, reference=False)
    assert abs(float(o_clipped.last_grad_norm) - norm) <= 1e-6 * norm
    for a, b in zip(free, clipped):
        assert_close(10 * o_clipped.state[b]["exp_avg"], o_free.state[a]["exp_avg"], 2e-6, "exp_avg under the clip")
        assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ ops.prior_tokens
@pytest.mark.parametrize("B,T,V", [(2, 16, 64), (2, 16, 100), (3, 1, 64), (5, 300, 100)])
@pytest.mark.parametrize("pkeep", [1.0, 0.5, 0.0])
def test_prior_tokens_bit_equal(B, T, V, pkeep):
    from hipops import ops
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + V)
    ids = torch.randint(0, V, (B, T), generator=g)
    u_keep, u_rand = torch.rand(B, T, generator=g), torch.rand(B, T, generator=g)
    if V == 100 and T > 1:          # the largest fp32 below 1 in a replaced position
        u_rand[0, 3], u_keep[0, 3] = 1 - 2.0 ** -24, 0.75
        u_rand[1, 0], u_keep[1, 0] = 1 - 2.0 ** -24, 0.99
    sos = V - 1
    want = P.tokens_ref(ids, sos, pkeep, V, u_keep, u_rand)
    if pkeep >= 1:
        got = ops.prior_tokens(ids.to(DEV), sos, pkeep, V)          # null uniforms
    else:
        got = ops.prior_tokens(ids.to(DEV), sos, pkeep, V, u_keep.to(DEV), u_rand.to(DEV))
    assert got.dtype == torch.long and torch.equal(got.cpu(), want)
    assert bool((got[:, 0] == sos).all()) and int(got.min()) >= 0 and int(got.max()) < V
    if pkeep == 0.0 and T > 1:
        assert not torch.equal(got.cpu()[:, 1:], ids[:, :-1])


def test_prior_tokens_passes_foreign_ids_through():
    from hipops import ops
    ids = torch.tensor([[-1, 70, 3, 5], [64, 2, -9, 1]])
    got = ops.prior_tokens(ids.to(DEV), 0, 1.0, 64).cpu()
    assert got.tolist() == [[0, -1, 70, 3], [0, 64, 2, -9]]


# ------------------------------------------------------------------------------------------------ the VQGAN's code side
def _small_vqgan(out_channels=1):
    from networks import VQGAN
    name = "vqgan"
    args = list(VM.CASES[name][1])
    args[2] = out_channels
    torch.manual_seed(VM.SEEDS[name])
    return VM.init_case_(VQGAN(*args), name, VM.SEEDS[name]).to(DEV).eval()


def test_encode_to_ids_and_decode_from_ids():
    vq = _small_vqgan()
    x = VM.case_input("vqgan", VM.SEEDS["vqgan"]).to(DEV)
    with torch.no_grad():
        recon = vq(x)[0]
        z = vq.encoder(x)
    seq = vq.encode_to_ids(x)
    B, _, h, w = z.shape
    assert seq.shape == (B, h * w) and seq.dtype == torch.long
    assert torch.equal(vq.decode_from_ids(seq, h, w), recon)                 # bit for bit
    # seq[b, r * w + c] is the code of latent pixel (r, c): the float64 nearest-code search on the kernel's own latent
    st = {"vq." + k: v.detach().double().cpu() for k, v in vq.vq.state_dict().items()}
    _, _, ids, gap, _ = VM.vq_ref(z.double().cpu(), st, "vq.", training=False)          # ids, gap (B, H, W) of pixel (h, w)
    clear = gap > 1e-4
    assert float(clear.float().mean()) > 0.9
    got = seq.cpu().reshape(B, h, w)
    assert torch.equal(got[clear], ids[clear])
    assert len(torch.unique(got)) > 1 and not torch.equal(got, got.transpose(1, 2))          # an order mix-up would show
    vq.train()
    with pytest.raises(RuntimeError, match="encode_to_ids: eval mode only"):
        vq.encode_to_ids(x)
    buffers = {k: v.clone() for k, v in vq.vq.state_dict().items()}
    vq.eval().encode_to_ids(x)
    assert all(torch.equal(v, vq.vq.state_dict()[k]) for k, v in buffers.items())          # no EMA update


# ------------------------------------------------------------------------------------------------ the step against the fixture
def _trainer(name, pkeep=1.0, init_seed=None, **kw):
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    vqgan = VQGAN(**P.TINY_VQGAN)
    seed = P.SEEDS[name] if init_seed is None else init_seed
    torch.manual_seed(seed)
    gpt = G.init_gpt_(GPT(**P.gpt_kwargs(name)), seed)
    o = P.OPTIM
    args = dict(pkeep=pkeep, sos_token=P.SOS, lr=o["lr"], betas=o["betas"], weight_decay=o["weight_decay"],
                grad_norm_clip=P.GRAD_NORM_CLIP[name], seed=17, device=DEV)
    args.update(kw)
    return PriorTrainer(vqgan, gpt, **args)


def _sampled(named):
    return {k: t.detach().double().cpu().reshape(-1)[sample_idx(t.numel(), 256, seed=1)] for k, t in named}


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_training_step_against_the_reference(golden, name):
    g = golden("prior_step_%s.npz" % name)
    keys = [str(k) for k in g[name + "/keys"]]
    tr = _trainer(name)
    ids = g.t(name + "/ids").to(DEV)
    got = dict(loss=[], norm=[], coef=[])
    for s in range(P.STEPS):
        out = tr.training_step({"ids": ids})
        assert out["lr"] == P.OPTIM["lr"] and out["ids"] is ids and out["loss"].is_cuda and out["grad_norm"].is_cuda
        got["loss"].append(float(out["loss"]))
        got["norm"].append(float(out["grad_norm"]))
        got["coef"].append(float(tr.optim.last_clip_coef))
        if s == 0:
            g0 = _sampled((k, p.grad) for k, p in tr.gpt.named_parameters())
    assert tr.step_count == P.STEPS and sorted(g0) == sorted(keys)
    # the scalars (module docstring)
    failures = []
    for q in ("loss", "norm", "coef"):
        t64, v32 = g["%s/%s64" % (name, q)], g["%s/%s32" % (name, q)]
        own = max(float((np.abs(v32 - t64[None]) / np.abs(t64[None])).max()), FP32_ULP)
        for s in range(P.STEPS):
            err = abs(got[q][s] - t64[s]) / abs(t64[s])
            print("%s step %d %s: %.9g, reference fp64 %.9g: %.2e apart, the reference's own fp32 distance %.2e" % (
                name, s, q, got[q][s], t64[s], err, own))
            if err > 2 * own or (q == "coef" and t64[s] == 1.0 and got[q][s] != 1.0):
                failures.append((q, s, err, own))
    # gradients of step 0 and parameters after step 3: the reference's gate on its own sampled entries
    for what, tag, test in (("gradient", "g", g0), ("parameter", "p", _sampled(tr.gpt.named_parameters()))):
        truth = {k: g.t("%s/%s64.%s" % (name, tag, k)).double() for k in keys}
        variants = [{k: g.t("%s/%s32.%s" % (name, tag, k))[i] for k in keys} for i in range(3)]
        grad_gate(truth, variants, test, what="%s %s" % (name, what))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ resume
def _everything(tr):
    out = {"p." + k: v for k, v in tr.gpt.state_dict().items()}
    for i, p in enumerate(tr.gpt.parameters()):
        st = tr.optim.state[p]
        out["m.%d" % i], out["v.%d" % i], out["t.%d" % i] = st["exp_avg"], st["exp_avg_sq"], torch.tensor(st["step"])
    out["generator"], out["step"] = tr.generator.get_state(), torch.tensor(tr.step_count)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def test_resume_is_bit_exact():
    from utils.checkpoint import _to_cpu
    name = "p64"
    ids = P.case_ids(name, P.SEEDS[name]).to(DEV)
    kw = dict(pkeep=0.5, warmup_steps=3, decay_steps=6)
    full = _trainer(name, **kw)
    losses = [float(full.training_step({"ids": ids})["loss"]) for _ in range(4)]
    part = _trainer(name, **kw)
    first = [float(part.training_step({"ids": ids})["loss"]) for _ in range(2)]
    state = copy.deepcopy(_to_cpu(part.state_dict()))          # what a checkpoint holds
    fresh = _trainer(name, init_seed=999, seed=5, **kw)          # other weights, another generator
    fresh.load_state_dict(state)
    assert fresh.step_count == 2 and fresh.current_lr() == part.current_lr()
    rest = [float(fresh.training_step({"ids": ids})["loss"]) for _ in range(2)]
    assert first + rest == losses
    a, b = _everything(full), _everything(fresh)
    assert a.keys() == b.keys()
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff[:8]
    assert int(a["step"]) == 4 and int(a["t.0"]) == 4
    # the corruption is really drawn: without it the same steps end elsewhere
    clean = _trainer(name, pkeep=1.0, warmup_steps=3, decay_steps=6)
    assert float(clean.training_step({"ids": ids})["loss"]) != losses[0]


def test_validation_step_is_clean_and_leaves_the_training_state():
    name = "p64"
    ids = P.case_ids(name, P.SEEDS[name]).to(DEV)
    tr = _trainer(name, pkeep=0.5)
    out = tr.validation_step({"ids": ids})
    assert not out["loss"].requires_grad and all(p.grad is None for p in tr.gpt.parameters())
    ref = _trainer(name, pkeep=1.0)          # pkeep = 1: the first training step's loss of the uncorrupted trainer
    assert float(out["loss"]) == float(ref.training_step({"ids": ids})["loss"])
    tr.training_step({"ids": ids})
    before = _everything(tr)
    tr.validation_step({"ids": ids})
    after = _everything(tr)
    assert tr.gpt.training and all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ sampling
def _sampling_trainer(block_size):
    from networks import GPT
    from trainers import PriorTrainer
    vq = _small_vqgan()
    torch.manual_seed(21)
    gpt = G.init_gpt_(GPT(vocab_size=8, block_size=257, n_layer=2, n_head=2, n_embed=64), 21)
    if block_size != 257:          # the same model without the position it never uses
        small = GPT(vocab_size=8, block_size=block_size, n_layer=2, n_head=2, n_embed=64)
        st = {k: v for k, v in gpt.state_dict().items() if not k.endswith("mask")}
        st["pos_embed"] = st["pos_embed"][:, :block_size]
        small.load_state_dict(st, strict=False)
        gpt = small
    return PriorTrainer(vq, gpt, device=DEV)


def test_sample_images_repeat_under_a_seed_and_follow_generate():
    tr = _sampling_trainer(257)
    gen = lambda: torch.Generator(device=DEV).manual_seed(33)  # noqa: E731
    ids = tr.sample_ids(2, temperature=1.0, top_k=4, generator=gen())
    assert ids.shape == (2, 256) and ids.dtype == torch.long and int(ids.min()) >= 0 and int(ids.max()) < 8
    start = torch.full((2, 1), tr.sos_token, dtype=torch.long, device=DEV)
    assert torch.equal(ids, tr.gpt.generate(start, 256, temperature=1.0, top_k=4, generator=gen())[:, 1:])
    assert tr.gpt.training          # put back
    a = tr.sample_images(2, temperature=1.0, top_k=4, generator=gen())
    b = tr.sample_images(2, temperature=1.0, top_k=4, generator=gen())
    assert a.shape == (2, 1, 32, 32) and torch.equal(a, b)
    assert torch.equal(a, tr.vqgan.decode_from_ids(ids, 16, 16))
    assert not torch.equal(ids, tr.sample_ids(2, temperature=1.0, top_k=4, generator=torch.Generator(device=DEV).manual_seed(34)))
    # a model whose block size is the sequence length itself draws the same codes: the last token is never fed back
    exact = _sampling_trainer(256)
    with pytest.raises(RuntimeError, match="exceeds block_size=256"):
        exact.gpt.generate(start, 256)
    assert torch.equal(exact.sample_ids(2, temperature=1.0, top_k=4, generator=gen()), ids)


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_trains_validates_checkpoints_and_resumes(tmp_path):
    from utils import png
    save = os.path.join(str(tmp_path), "run")
    cfg = write_config(os.path.join(str(tmp_path), "run.json"), P.prior_run_config(save))
    out = run_launcher(cfg, "-p")
    vdir = os.path.join(save, "study", "version_0")
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == P.PRIOR_MONITORED and len(rows) == 3          # two steps and the epoch's validation
    for i, row in enumerate(rows[:2]):
        rec = dict(zip(header, row))
        assert (int(rec["epoch"]), int(rec["iteration"])) == (0, i) and rec["val_loss"] == "" and rec["ppl"] == ""
        assert np.isfinite(float(rec["loss"])) and float(rec["grad_norm"]) > 0
        assert float(rec["lr"]) == pytest.approx(1e-3 * (i + 1) / 2)          # warm-up over two steps
    val = dict(zip(header, rows[2]))
    assert val["loss"] == "" and float(val["ppl"]) == pytest.approx(np.exp(float(val["val_loss"])), rel=1e-6)
    assert 0 < float(val["val_loss"]) < 2 * np.log(8) and "validation cross-entropy" in out
    pixels, _ = png.load(os.path.join(vdir, "000000.png"))
    assert pixels.shape == (3 * 32, 2 * 32) and pixels.dtype == np.uint8          # slices, reconstructions, draws x n_save_images
    ckpt = os.path.join(vdir, "ckpt-epoch=0000-total_loss=0.00.ckpt")
    ck = torch.load(ckpt, map_location="cpu")
    assert ck["global_step"] == 2 and ck["optimizer_indices"] == [3] and ck["vqw_run_state"]["trainer"]["prior_step"] == 2
    assert any(k.startswith("decoder.vq.") for k in ck["state_dict"]) and any(k.startswith("transformer.blocks.") for k in ck["state_dict"])
    # the second run resumes: epoch 1 behind epoch 0, the frozen first stage untouched, the transformer trained on
    raw = P.prior_run_config(save, n_epochs=2, resume_checkpoint=ckpt)
    out = run_launcher(write_config(os.path.join(str(tmp_path), "resume.json"), raw), "-p")
    assert "Loading model from" in out
    vdir1 = os.path.join(save, "study", "version_1")
    ck1 = torch.load(os.path.join(vdir1, "ckpt-epoch=0001-total_loss=0.00.ckpt"), map_location="cpu")
    assert ck1["global_step"] == 4 and ck1["vqw_run_state"]["trainer"]["prior_step"] == 4
    assert all(s["step"] == 4 for s in ck1["optimizer_states"][0]["state"].values())
    for k, v in ck["state_dict"].items():
        if k.startswith("decoder."):
            assert torch.equal(v, ck1["state_dict"][k]), k
    assert any(not torch.equal(v, ck1["state_dict"][k]) for k, v in ck["state_dict"].items() if k.startswith("transformer."))
    header, rows = read_csv(os.path.join(vdir1, "log.csv"))
    assert [(r[0], r[1]) for r in rows[:2]] == [("1", "2"), ("1", "3")] and len(rows) == 3
    assert all(float(dict(zip(header, r))["lr"]) == 1e-3 for r in rows[:2])          # behind the warm-up
    assert os.path.exists(os.path.join(vdir1, "000001.png")) and not glob.glob(os.path.join(vdir1, "ckpt-epoch=0000*"))
