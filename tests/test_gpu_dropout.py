"""GPU tests of the GPT prior's dropout: the counter-based masks of csrc/dropout.h against their numpy restatement
(tests/dropout_ref.py) bit for bit, ops.dropout / ops.add_dropout and the attention kernels' dropout policy against float64 with the
restated masks, the seeded modules against the float64 restatement, and the trainer's reproducibility and resume.  Run with
`pytest -m gpu` on an MI355X.

Tolerances: `_gate` of tests/test_gpu_mingpt_blocks.py - the kernel's relative L2 distance from the float64 restatement at most
twice the fp32 restatement's - and helpers.grad_gate at its defaults with the fp32 restatement's three evaluations as the variants.
A kernel whose passes disagree on the mask is off by O(1), not by rounding."""
import copy

import numpy as np
import pytest
import torch

import dropout_ref as D
import gpt_ref as G
import mingpt_ref as M
import prior_ref as P
from helpers import assert_close, grad_gate, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = (1234, 7, 3)          # (seed, call, site)


def _dev(t):
    return t.detach().float().contiguous().to(DEV)


def _gate(got, truth, ref32, what):
    """tests/test_gpu_mingpt_blocks.py's: |got - truth| <= 2 |ref32 - truth| (relative L2), figures printed first."""
    spread, e = rel_err(ref32, truth), rel_err(got, truth)
    print("%-52s %.3e from float64, the fp32 restatement %.3e (ratio %.2f)" % (what, e, spread, e / max(spread, 1e-300)))
    assert_close(got, truth, 2.0 * spread, what)


def _attn_inputs(B, Tq, Tk, nh, hs, seed):
    g = torch.Generator().manual_seed(seed)
    q, go = (torch.randn(B, Tq, nh * hs, generator=g) for _ in range(2))
    k, v = (torch.randn(B, Tk, nh * hs, generator=g) for _ in range(2))
    return q, k, v, go


def _np(mask):
    return torch.from_numpy(np.ascontiguousarray(mask))


# ------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("n", [1, 7, 4099, 2 ** 20 + 3])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_equals_the_restatement(n, p):
    from hipops import ops
    got = ops.dropout_keep_mask(n, p, KEY).cpu()
    assert got.dtype == torch.bool and got.shape == (n,)
    assert torch.equal(got, _np(D.keep_mask(n, p, *KEY)))
    if n > 7:
        assert not torch.equal(got, ops.dropout_keep_mask(n, p, (KEY[0], KEY[1], KEY[2] + 1)).cpu())


@pytest.mark.parametrize("B,nh,T", [(2, 3, 70), (1, 2, 129)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_keep_mask_equals_the_restatement(B, nh, T, p):
    from hipops import ops
    got = ops.attention_keep_mask(B, nh, T, T, p, KEY).cpu()
    assert got.shape == (B, nh, T, T)
    assert torch.equal(got, _np(D.attention_keep_mask(B, nh, T, T, p, *KEY)))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_of_ones_is_the_mask_times_the_scale(p):
    from hipops import ops
    n = 4099
    y = ops.dropout(torch.ones(n, device=DEV), p, KEY).cpu()
    want = _np(D.keep_mask(n, p, *KEY)).float() * float(D.scale(p))
    assert float(D.scale(p)) == float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
    assert torch.equal(y, want)


# ------------------------------------------------------------------------------------------------ ops.dropout, ops.add_dropout
@pytest.mark.parametrize("shape", [(4099,), (2, 70, 96)])
def test_dropout_and_add_dropout(shape):
    from hipops import ops
    p, n = 0.25, int(np.prod(shape))
    g = torch.Generator().manual_seed(n)
    a, b, gy = (torch.randn(shape, generator=g) for _ in range(3))
    mask = D.keep_mask(n, p, *KEY)
    res = {}
    for dtype in (torch.float64, torch.float32):
        ar, br = (t.to(dtype).requires_grad_(True) for t in (a, b))
        y1 = D.drop_ref(br, mask, p)
        y2 = ar + D.drop_ref(br, mask, p)
        g1, = torch.autograd.grad((y1 * gy.to(dtype)).sum(), br, retain_graph=True)
        ga, gb = torch.autograd.grad((y2 * gy.to(dtype)).sum(), (ar, br))
        res[dtype] = dict(drop=y1.detach(), drop_dx=g1, add=y2.detach(), add_da=ga, add_db=gb)
    ad, bd = (_dev(t).requires_grad_(True) for t in (a, b))
    y1 = ops.dropout(bd, p, KEY)
    g1, = torch.autograd.grad(y1, bd, _dev(gy))
    y2 = ops.add_dropout(ad, bd, p, KEY)
    ga, gb = torch.autograd.grad(y2, (ad, bd), _dev(gy))
    torch.cuda.synchronize()
    got = dict(drop=y1.detach(), drop_dx=g1, add=y2.detach(), add_da=ga, add_db=gb)
    for k in got:
        assert got[k].shape == tuple(shape), k
        _gate(got[k], res[torch.float64][k], res[torch.float32][k], "dropout %s %s" % (shape, k))
    assert torch.equal((y1 == 0).cpu().reshape(-1), ~_np(mask) | (b.reshape(-1) == 0))


# ------------------------------------------------------------------------------------------------ attention
# tests/test_gpu_mingpt_blocks.py's ATTN_CASES without T = 1: partial tiles, a second key step, the three key-split layouts, the
# unmasked corner
ATTN_DROP_CASES = [(2, 40, 2, 32, 5), (2, 70, 3, 32, 0), (1, 96, 1, 96, 0), (1, 129, 2, 64, 40), (1, 129, 1, 128, 129)]


def _attn_drop_ref(q, k, v, go, nh, nu, mask, p, dtype):
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    o, lse = D.causal_attention_drop_ref(q, k, v, nh, nu, mask, p)
    (o * go.to(dtype)).sum().backward()
    return dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _attn_drop_run(q, k, v, go, nh, nu, p, key):
    from hipops import ops
    qd, kd, vd = (_dev(t).requires_grad_(True) for t in (q, k, v))
    o = ops.causal_attention(qd, kd, vd, nh, n_unmasked=nu, causal=True, dropout_p=p, dropout_key=key)
    o.backward(_dev(go))
    torch.cuda.synchronize()
    return dict(o=o.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)


@pytest.mark.parametrize("B,T,nh,hs,nu", ATTN_DROP_CASES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_causal_attention_dropout(B, T, nh, hs, nu, p):
    from hipops import ops
    q, k, v, go = _attn_inputs(B, T, T, nh, hs, seed=T + hs + nu)
    mask = D.attention_keep_mask(B, nh, T, T, p, *KEY)
    truth = _attn_drop_ref(q, k, v, go, nh, nu, mask, p, torch.float64)
    ref32 = _attn_drop_ref(q, k, v, go, nh, nu, mask, p, torch.float32)
    got = _attn_drop_run(q, k, v, go, nh, nu, p, KEY)
    for key in ("o", "dq", "dk", "dv"):
        what = "attention dropout p%g B%d T%d nh%d hs%d u%d %s" % (p, B, T, nh, hs, nu, key)
        assert got[key].shape == truth[key].shape and bool(torch.isfinite(got[key]).all()), what
        _gate(got[key], truth[key], ref32[key], what)
    # lse does not know of the dropout
    L = ops._L()
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    o0, lse0 = ops.causal_attention_lse(qd, kd, vd, nh, n_unmasked=nu, causal=True)
    o1, lse1 = torch.empty_like(qd), torch.empty_like(lse0)
    L.vqw_causal_attention_drop_fwd(qd, kd, vd, o1, lse1, B, T, T, nh, hs, 1.0 / hs ** 0.5, 1, nu, p, *KEY)
    torch.cuda.synchronize()
    assert torch.equal(lse1, lse0) and torch.equal(o1, got["o"])
    # the same bits every run; another call, another mask
    again = _attn_drop_run(q, k, v, go, nh, nu, p, KEY)
    for key in got:
        assert torch.equal(got[key], again[key]), key
    other = _attn_drop_run(q, k, v, go, nh, nu, p, (KEY[0], KEY[1] + 1, KEY[2]))
    assert not torch.equal(other["o"], got["o"])
    # p = 0 with a key: today's path, today's bits
    zero = _attn_drop_run(q, k, v, go, nh, nu, 0.0, KEY)
    assert torch.equal(zero["o"], o0)


def test_causal_attention_dropout_refusals():
    from hipops import ops
    q, k, v, _ = _attn_inputs(1, 3, 40, 2, 32, seed=1)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.causal_attention(_dev(q), _dev(k), _dev(v), 2, causal=False, dropout_p=0.1, dropout_key=KEY)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.causal_attention(_dev(k), _dev(k), _dev(v), 2, dropout_p=1.0, dropout_key=KEY)
    L = ops._L()
    kd = _dev(k)
    with pytest.raises(RuntimeError, match=r"p=1 must lie in \[0, 1\)"):
        L.vqw_causal_attention_drop_fwd(kd, kd, kd, torch.empty_like(kd), torch.empty(1, 2, 40, device=DEV), 1, 40, 40, 2, 32, 0.1, 1, 0, 1.0, *KEY)


# ------------------------------------------------------------------------------------------------ modules
PD = 0.25
E, NH, T, NU, B = 64, 2, 40, 5, 2


def _flipped(masks):
    """The masks of the batch in reversed order: an element-wise mask indexes the dense (B, T, E) tensor"""
    return [None if m is None else (np.flip(m, 0) if m.ndim == 4 else np.flip(m.reshape(B, T, E), 0).reshape(-1)).copy() for m in masks]


def _ref_grads(fn, state, dtype, variant):
    """({name: gradient}, output) of fn(state in dtype, reversed batch?) through the restatement; mingpt_ref.grads_ref's three
    mathematically identical evaluations: eight threads, one thread, the batch in reversed order (fn flips its input, its masks and
    its output inside the graph, so every gradient arrives in the original order)."""
    st = {k: (v.detach().clone() if k.endswith("mask") else v.detach().clone().to(dtype).requires_grad_(True)) for k, v in state.items()}
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        out, loss = fn(st, variant == "batch_reversed")
        loss.backward()
    finally:
        torch.set_num_threads(n)
    return {k: v.grad for k, v in st.items() if not k.endswith("mask")}, out.detach()


def test_block_with_dropout():
    import networks
    from hipops import ops
    torch.manual_seed(91)
    cfg = dict(vocab_size=16, block_size=T, n_embed=E, n_head=NH, n_unmasked=NU, att_pdrop=PD, res_pdrop=PD, emb_pdrop=PD)
    m = M.init_case_(networks.Block(networks.GPTConfig(**cfg)), 91)
    x = M.round64(torch.randn(B, T, E, generator=torch.Generator().manual_seed(92)))
    seed, call = 5, 11
    masks = D.module_masks(B, T, E, NH, 1, PD, PD, PD, seed, call, with_emb=False)
    state = dict(m.state_dict(), input=x)

    def fn(st, rev):
        out = D.block_drop_ref(st["input"].flip(0) if rev else st["input"], st, "", NH, NU, _flipped(masks) if rev else masks, PD, PD)
        out = out.flip(0) if rev else out
        return out, (out * M.cotangent(out.shape, out.dtype)).sum()
    truth, out64 = _ref_grads(fn, state, torch.float64, "threads8")
    variants = [_ref_grads(fn, state, torch.float32, v) for v in M.VARIANTS]
    m = m.to(DEV).train().seed_dropout(seed, call)
    assert (m.att.dropout_site, m.dropout_site) == (0, 2)
    xin = _dev(x).requires_grad_(True)
    out = m(xin)
    (out * M.cotangent(out.shape, torch.float32).to(DEV)).sum().backward()
    ops.join_streams()
    torch.cuda.synchronize()
    assert m.dropout_call == call + 1 and m.att.dropout_call == call + 1
    _gate(out, out64, variants[0][1], "Block with dropout: output")
    test = {k: p.grad for k, p in m.named_parameters()}
    test["input"] = xin.grad
    grad_gate(truth, [v[0] for v in variants], test, what="Block with dropout")
    # eval mode of the seeded module: the bits of the same weights without dropout
    plain = networks.Block(networks.GPTConfig(**dict(cfg, att_pdrop=0.0, res_pdrop=0.0, emb_pdrop=0.0)))
    plain.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m.eval()(_dev(x)), plain.to(DEV).eval()(_dev(x)))
    assert m.dropout_call == call + 1          # an eval forward takes no call


def test_gpt_with_dropout():
    import networks
    from hipops import ops
    V, nl = 16, 2
    torch.manual_seed(93)
    kw = dict(vocab_size=V, block_size=T, n_layer=nl, n_head=NH, n_embed=E, n_unmasked=NU)
    m = G.init_gpt_(networks.GPT(emb_pdrop=PD, res_pdrop=PD, att_pdrop=PD, **kw), 93)
    g = torch.Generator().manual_seed(94)
    idx, target = torch.randint(0, V, (B, T), generator=g), torch.randint(0, V, (B, T), generator=g)
    seed, call = 6, 2
    masks = D.module_masks(B, T, E, NH, nl, PD, PD, PD, seed, call)
    state = dict(m.state_dict())

    def fn(st, rev):
        logits = D.gpt_drop_ref(idx.flip(0) if rev else idx, st, nl, NH, NU, _flipped(masks) if rev else masks, PD, PD, PD)
        logits = logits.flip(0) if rev else logits
        return logits, torch.nn.functional.cross_entropy(logits.reshape(-1, V), target.reshape(-1))
    truth, out64 = _ref_grads(fn, state, torch.float64, "threads8")
    variants = [_ref_grads(fn, state, torch.float32, v) for v in M.VARIANTS]
    m = m.to(DEV).train().seed_dropout(seed, call)
    logits = m(idx.to(DEV))
    ops.cross_entropy(logits, target.to(DEV)).backward()
    ops.join_streams()
    torch.cuda.synchronize()
    assert m.dropout_call == call + 1 and all(b.dropout_call == call + 1 and b.att.dropout_call == call + 1 for b in m.blocks)
    _gate(logits, out64, variants[0][1], "GPT with dropout: logits")
    test = {k: p.grad for k, p in m.named_parameters()}
    assert set(test) == set(truth)
    grad_gate(truth, [v[0] for v in variants], test, what="GPT with dropout")
    # the next call draws other masks; set_dropout_call brings the first ones back
    with torch.no_grad():
        second = m(idx.to(DEV))
        again = m.set_dropout_call(call)(idx.to(DEV))
    assert not torch.equal(second, logits) and torch.equal(again, logits)
    plain = networks.GPT(**kw)
    plain.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m.eval()(idx.to(DEV)), plain.to(DEV).eval()(idx.to(DEV)))


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(dropout_seed, init_seed=None, p=0.1, **kw):
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    name = "p64"
    vqgan = VQGAN(**P.TINY_VQGAN)
    seed = P.SEEDS[name] if init_seed is None else init_seed
    torch.manual_seed(seed)
    gpt = G.init_gpt_(GPT(emb_pdrop=p, res_pdrop=p, att_pdrop=p, **P.gpt_kwargs(name)), seed)
    o = P.OPTIM
    args = dict(pkeep=0.5, sos_token=P.SOS, lr=o["lr"], betas=o["betas"], weight_decay=o["weight_decay"],
                grad_norm_clip=P.GRAD_NORM_CLIP[name], seed=17, device=DEV, dropout_seed=dropout_seed)
    args.update(kw)
    return PriorTrainer(vqgan, gpt, **args)


def _params(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.gpt.state_dict().items()}


def test_trainer_with_dropout_is_reproducible_and_resumes():
    from utils.checkpoint import _to_cpu
    ids = P.case_ids("p64", P.SEEDS["p64"]).to(DEV)
    full = _trainer(3)
    outs = [full.training_step({"ids": ids}) for _ in range(3)]
    assert all(bool(torch.isfinite(o["loss"])) and bool(torch.isfinite(o["grad_norm"])) for o in outs)
    assert full.gpt.dropout_call == 3
    a = _params(full)
    # the same seed: the same bits in every parameter
    twin = _trainer(3)
    for _ in range(3):
        twin.training_step({"ids": ids})
    b = _params(twin)
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    # another dropout seed: other parameters
    other = _trainer(4)
    for _ in range(3):
        other.training_step({"ids": ids})
    c = _params(other)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    # a checkpoint after step 2, a resume, step 3
    part = _trainer(3)
    for _ in range(2):
        part.training_step({"ids": ids})
    state = copy.deepcopy(_to_cpu(part.state_dict()))
    assert state["extra"]["prior_dropout_seed"] == 3
    fresh = _trainer(3, init_seed=999, seed=5)
    fresh.load_state_dict(state)
    fresh.training_step({"ids": ids})
    d = _params(fresh)
    assert not [k for k in a if not torch.equal(a[k], d[k])]
    with pytest.raises(ValueError, match="dropout_seed"):
        _trainer(4).load_state_dict(state)
    # eval-mode routes do not know of the seed
    clean = _trainer(None, p=0.0)
    clean.gpt.load_state_dict(full.gpt.state_dict())
    assert torch.equal(full.validation_step({"ids": ids})["loss"], clean.validation_step({"ids": ids})["loss"])
    assert torch.equal(full.token_nll({"ids": ids}), clean.token_nll({"ids": ids}))
    assert full.gpt.dropout_call == 3 and full.gpt.training
