"""CPU-side checks of the GPT code prior (no GPU): the float64 restatement (tests/gpt_ref.py) against the reference's fixtures
(tests/golden/mingpt_gpt_*.npz, made by tests/golden/make_golden_mingpt_gpt.py), the model's state_dict contract and seeded
initialisation, every refusal of GPT.forward / forward_with_past / sample, the sampling rule's fp32 restatement against float64
on the GPU test's own cases, and the C ABI / operator plumbing of the embedding, cross-entropy and sampling kernels."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import checksum, sample_idx
import gpt_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(G.CASES)
NEW_SYMBOLS = ("vqw_embed_fwd", "vqw_embed_bwd", "vqw_xent_ws_bytes", "vqw_xent_fwd", "vqw_xent_bwd", "vqw_sample_topk")


def _fixture(golden, name):
    return golden("mingpt_gpt_%s.npz" % name)


def _state(g, name):
    return {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}


def _inputs(g, name):
    return g.t(name + "/in"), g.t(name + "/target"), (g.t(name + "/prefix") if name + "/prefix" in g.files else None)


def _new(name):
    import networks
    return networks.GPT(**G.gpt_kwargs(name))


def _small(**kw):
    from networks import GPT
    args = dict(vocab_size=16, block_size=8, n_layer=2, n_head=2, n_embed=64)
    args.update(kw)
    return GPT(**args)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture_in_fp64(golden, name):
    g = _fixture(golden, name)
    seed = int(g[name + "/seed"])
    idx, target, prefix = _inputs(g, name)
    ridx, rtarget, rprefix = G.case_inputs(name, seed)
    assert torch.equal(idx, ridx) and torch.equal(target, rtarget) and (prefix is None) == (rprefix is None)
    assert prefix is None or torch.equal(prefix, rprefix)
    logits, loss, grads = G.grads_ref(name, _state(g, name), idx, target, prefix, torch.float64)
    ref = g.t(name + "/logits")
    assert ref.dtype == torch.float64 and logits.shape == ref.shape
    assert float((logits - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert abs(float(loss) - float(g[name + "/loss64"])) <= 1e-12 * float(loss)
    assert float((g.t(name + "/out").double() - ref).abs().max()) <= float(g[name + "/spread.out"]) * float(ref.abs().max()) * (1 + 1e-9)
    live = [str(k) for k in g[name + "/live"]]
    nl = G.CASES[name][2]
    assert sorted(set(grads) - set(live)) == ["blocks.%d.att.k.bias" % i for i in range(nl)]
    assert ("input" in grads) == (prefix is not None)
    for k in live:
        got = grads[k].reshape(-1)[sample_idx(grads[k].numel(), 256, seed=1)]
        want = g.t("%s/g64.%s" % (name, k))
        assert float((got - want).abs().max()) <= 1e-10 * float(g["%s/gnorm64.%s" % (name, k)]), k
        assert abs(float(grads[k].norm()) - float(g["%s/gnorm64.%s" % (name, k)])) <= 1e-9 * float(grads[k].norm()), k
    # the three fp32 evaluations of the reference bracket the loss as the GPU test's bound assumes
    assert g[name + "/loss32"].shape == (3,) and float(np.abs(g[name + "/loss32"].astype(np.float64) - float(g[name + "/loss64"])).max()) < 1e-6


def test_cached_route_restatement_equals_full_sequence(golden):
    """One call on the first CACHED_PROMPT tokens, then one token per call behind the growing past: the fixture's eval logits."""
    name = G.CACHED_CASE
    g = _fixture(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    st = {k: (v if k.endswith("mask") else v.double()) for k, v in _state(g, name).items()}
    idx, _, prefix = _inputs(g, name)
    full = g.t(name + "/eval_logits")
    n0 = G.CACHED_PROMPT - Te
    with torch.no_grad():
        logits, present = G.gpt_ref(idx[:, :n0], st, nl, nh, prefix.double())
        out, past = [logits], present
        for t in range(n0, Ti):
            logits, present = G.gpt_ref(idx[:, t:t + 1], st, nl, nh, None, past=past, t0=Te + t)
            out.append(logits)
            past = torch.cat((past, present), dim=-2)
    assert tuple(past.shape) == (nl, 2, B, nh, Te + Ti, E // nh)
    got = torch.cat(out, dim=1)
    assert got.shape == full.shape and float((got - full).abs().max()) <= 1e-12 * float(full.abs().max())


def test_embedding_and_xent_restatements_are_torchs():
    g = torch.Generator().manual_seed(3)
    tok, pos = torch.randn(11, 8, generator=g).double(), torch.randn(1, 9, 8, generator=g).double()
    idx, prefix = torch.randint(0, 11, (2, 5), generator=g), torch.randn(2, 2, 8, generator=g).double()
    want = torch.cat((prefix, F.embedding(idx, tok)), dim=1) + pos[:, 1:8]
    assert torch.equal(G.embedding_ref(idx, tok, pos, prefix, t0=1), want)
    assert torch.equal(G.embedding_ref(idx, tok, pos[0]), F.embedding(idx, tok) + pos[:, :5])
    z, t = torch.randn(2, 5, 11, generator=g).double(), torch.randint(0, 11, (2, 5), generator=g)
    loss, lse = G.xent_ref(z, t)
    assert loss.shape == (2, 5) and torch.allclose(loss.reshape(-1), F.cross_entropy(z.view(-1, 11), t.view(-1), reduction="none"), rtol=1e-13, atol=0)
    assert torch.allclose(lse, torch.log(torch.exp(z).sum(-1)), rtol=1e-13, atol=0)


def test_sample_ref_rule():
    z = torch.tensor([[0.0, 1.0, 1.0, -1.0, 2.0]])
    for u, want in ((0.0, 1), (0.999, 4)):          # top-2 keeps the tie at the threshold: {1, 2, 4}
        pick, dist, kept = G.sample_ref(z, torch.tensor([u]), 1.0, 2)
        assert kept.tolist() == [[False, True, True, False, True]] and int(pick) == want
    pick, _, kept = G.sample_ref(z, torch.tensor([0.5]), 1.0, 0)
    assert bool(kept.all())
    e = torch.exp(z[0].double() - 2)
    assert int(pick) == int((torch.cumsum(e, 0) > 0.5 * e.sum()).nonzero()[0])
    assert int(G.sample_ref(z, torch.tensor([0.3]), 0.5, 1)[0]) == 4          # k = 1: the argmax for any u
    pick, dist, _ = G.sample_ref(torch.zeros(1, 4), torch.tensor([0.5]), 1.0, 0)          # u total sits exactly on a boundary
    assert int(pick) == 2 and float(dist) == 0.0


@pytest.mark.parametrize("V,k", G.SAMPLE_CASES)
def test_sampling_cases_are_decidable_in_fp32(V, k):
    """The fp32 restatement alone, against float64, on the GPU test's inputs: always in the kept set, equal wherever the float64
    decision is clear, and at most 2 % of a case's rows unclear - the cap the kernel is held to."""
    for temp in G.SAMPLE_TEMPS:
        logits, u = G.sample_inputs(V, k, temp)
        p64, dist, kept = G.sample_ref(logits, u, temp, k)
        p32, _, kept32 = G.sample_ref(logits, u, temp, k, dtype=torch.float32)
        assert torch.equal(kept, kept32)
        assert bool(kept.gather(1, p32[:, None]).all()) and bool(kept.gather(1, p64[:, None]).all())
        clear = dist > G.SAMPLE_CLEAR
        assert int((~clear).sum()) <= G.SAMPLE_UNCLEAR_CAP * G.SAMPLE_B, (V, k, temp, int((~clear).sum()))
        assert torch.equal(p32[clear], p64[clear])
        if k == 1:
            assert torch.equal(p64, logits.argmax(dim=1)) or bool((logits.gather(1, p64[:, None])[:, 0] == logits.max(dim=1).values).all())


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", CASES)
def test_state_dict_contract_and_seeded_init(golden, name):
    """Keys, their order, shapes and the parameter count equal the reference's; the same seed gives its initial values (the
    fixture's checksums of the state as seeded, and its state after gpt_ref.init_gpt_); its state loads strictly."""
    g = _fixture(golden, name)
    V, bs, nl, nh, E, nu, B, Ti, Te = G.CASES[name]
    seed = int(g[name + "/seed"])
    torch.manual_seed(seed)
    m = _new(name)
    for k, v in m.state_dict().items():
        assert np.array_equal(checksum(v), g["%s/init.%s" % (name, k)]), "seeded %s differs from the reference's" % k
    assert not bool(m.pos_embed.any()) and float(m.ln_f.weight.detach().min()) == 1.0 and not bool(m.blocks[0].att.k.bias.any())
    G.init_gpt_(m, seed)
    sd, ref = m.state_dict(), _state(g, name)
    assert list(sd) == [str(k) for k in g[name + "/keys"]]
    assert list(sd)[:2] == ["pos_embed", "tok_embed.weight"]          # a module's own parameters come before its children's
    assert list(sd)[2:7] == ["blocks.0.ln1.weight", "blocks.0.ln1.bias", "blocks.0.ln2.weight", "blocks.0.ln2.bias", "blocks.0.att.mask"]
    assert list(sd)[-3:] == ["ln_f.weight", "ln_f.bias", "head.weight"] and len(sd) == 2 + 17 * nl + 3
    assert [k for k, _ in m.named_parameters()] == [k for k in sd if not k.endswith("mask")]
    assert sum(p.numel() for p in m.parameters()) == int(g[name + "/nparams"])
    assert tuple(sd["pos_embed"].shape) == (1, bs, E) and tuple(sd["tok_embed.weight"].shape) == (V, E) and tuple(sd["head.weight"].shape) == (V, E)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
        assert torch.equal(v, ref[k]), "%s differs from the reference's under the same seed" % k
    torch.manual_seed(12345)
    other = _new(name)
    other.load_state_dict({k: v.clone() for k, v in ref.items()}, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, ref[k]), k
    assert other.blocks[0].att.n_unmasked == nu and other.block_size == bs == other.get_block_size()


def test_module_tree():
    import networks
    m = _small()
    assert networks.GPT is networks.gpt.GPT
    assert [n for n, _ in m.named_children()] == ["tok_embed", "drop", "blocks", "ln_f", "head"]
    assert isinstance(m.tok_embed, torch.nn.Embedding) and isinstance(m.pos_embed, torch.nn.Parameter) and isinstance(m.drop, torch.nn.Dropout)
    assert isinstance(m.blocks, torch.nn.Sequential) and len(m.blocks) == 2 and isinstance(m.blocks[0], networks.Block)
    assert isinstance(m.ln_f, torch.nn.LayerNorm) and m.head.bias is None and m.block_size == 8
    c = m.config
    assert (c.vocab_size, c.block_size, c.n_layer, c.n_head, c.n_embed, c.n_unmasked) == (16, 8, 2, 2, 64, 0)
    assert (c.emb_pdrop, c.res_pdrop, c.att_pdrop, m.drop.p) == (0.0, 0.0, 0.0, 0.0)
    d = networks.GPT(10, 4)          # the reference's defaults
    assert (d.config.n_layer, d.config.n_head, d.config.n_embed, len(d.blocks)) == (12, 8, 256, 12)
    assert "not built yet" not in networks.mingpt.__doc__ and "networks/gpt.py" in networks.mingpt.__doc__


def test_forward_refusals():
    idx = torch.zeros(1, 8, dtype=torch.long)
    for p in ("emb_pdrop", "res_pdrop", "att_pdrop"):
        m = _small(**{p: 0.25})
        with pytest.raises(NotImplementedError, match="dropout"):          # before any kernel: these are CPU tensors
            m.train()(idx)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.eval()(idx)
    m = _small()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train()(idx)
    with pytest.raises(RuntimeError, match="block_size=8"):
        m(torch.zeros(1, 9, dtype=torch.long))
    with pytest.raises(RuntimeError, match="block_size=8"):          # the prefix counts
        m(torch.zeros(1, 7, dtype=torch.long), embeddings=torch.zeros(1, 2, 64))


def test_forward_with_past_refusals():
    m = _small()
    one = torch.zeros(1, 1, dtype=torch.long)
    past = [torch.zeros(2, 2, 1, 2, 3, 32)]
    with pytest.raises(AssertionError):
        m.train().forward_with_past(one)
    m.eval()
    with pytest.raises(RuntimeError, match="block_size=8"):
        m.forward_with_past(torch.zeros(1, 9, dtype=torch.long))
    with pytest.raises(ValueError, match="exactly one"):
        m.forward_with_past(torch.zeros(1, 2, dtype=torch.long), past=past, past_length=3)
    with pytest.raises(ValueError, match="exactly one"):          # one token and one row of embeddings are two
        m.forward_with_past(one, embeddings=torch.zeros(1, 1, 64), past=past, past_length=3)
    with pytest.raises(ValueError, match="exactly one"):
        m.forward_with_past(torch.zeros(1, 0, dtype=torch.long), past=past, past_length=3)
    with pytest.raises(AssertionError):
        m.forward_with_past(one, past=past)          # past_length is needed
    with pytest.raises(AssertionError, match="past_length, hs"):
        m.forward_with_past(one, past=past, past_length=4)
    with pytest.raises(AssertionError, match="past_length, hs"):
        m.forward_with_past(torch.zeros(2, 1, dtype=torch.long), past=past, past_length=3)
    with pytest.raises(RuntimeError, match="past_length \\+ 1 = 9 exceeds block_size=8"):
        m.forward_with_past(one, past=[torch.zeros(2, 2, 1, 2, 8, 32)], past_length=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_with_past(one, past=past + [torch.zeros(2, 2, 1, 2, 1, 32)], past_length=4)


def test_sample_refusals():
    m = _small().train()
    with pytest.raises(RuntimeError, match="exceeds block_size=8"):
        m.sample(torch.zeros(1, 3, dtype=torch.long), 6)
    with pytest.raises(RuntimeError, match="exceeds block_size=8"):
        m.sample(torch.zeros(1, 3, dtype=torch.long), 4, embeddings=torch.zeros(1, 2, 64))
    with pytest.raises(ValueError, match="temperature"):
        m.sample(torch.zeros(1, 3, dtype=torch.long), 2, temperature=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sample(torch.zeros(1, 3, dtype=torch.long), 5)
    assert m.training          # the mode is restored
    out = m.sample(torch.ones(2, 3, dtype=torch.long), 0)
    assert torch.equal(out, torch.ones(2, 3, dtype=torch.long))


# ------------------------------------------------------------------------------------------------ operators and the C ABI
def test_operators_have_no_cpu_fallback_and_check_their_arguments():
    from hipops import ops
    idx, tok, pos = torch.zeros(2, 3, dtype=torch.long), torch.randn(5, 8), torch.randn(1, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embedding(idx, tok, pos)
    z, t = torch.randn(2, 3, 5), torch.zeros(2, 3, dtype=torch.long)
    for call in (lambda: ops.cross_entropy(z, t), lambda: ops.cross_entropy(z, t, reduction="none"), lambda: ops.cross_entropy_lse(z, t),
                 lambda: ops.sample_topk(z[0], torch.rand(3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="reduction"):
        ops.cross_entropy(z, t, reduction="sum")


def test_new_symbols_in_header_and_signatures():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
    ops = library.register()
    for s in NEW_SYMBOLS:
        assert (s in ops) == (not s.endswith("_ws_bytes")), s
    sch = str(torch.ops.vqw.embed_fwd.default._schema)
    assert "Tensor? idx" in sch and "Tensor? prefix" in sch and "Tensor(a!)? x" in sch and "int t0" in sch and "int block_size" in sch
    sch = str(torch.ops.vqw.embed_bwd.default._schema)
    assert "Tensor? gx" in sch and "Tensor(a!)? gtok" in sch and "Tensor(b!)? gpos" in sch
    sch = str(torch.ops.vqw.xent_fwd.default._schema)
    assert "Tensor? target" in sch and "Tensor(a!)? loss" in sch and "Tensor(b!)? lse" in sch and "Tensor(c!)? mean" in sch and "Tensor(d!)? ws" in sch
    sch = str(torch.ops.vqw.xent_bwd.default._schema)
    assert "Tensor? lse" in sch and "Tensor? gw" in sch and "Tensor(a!)? gz" in sch and "int mean" in sch
    sch = str(torch.ops.vqw.sample_topk.default._schema)
    assert "Tensor? logits" in sch and "Tensor? u" in sch and "Tensor(a!)? out" in sch and "float temperature" in sch and "int top_k" in sch
    L = _lib.load()
    # one partial (a double) per XE_WG_ROWS = 32 rows
    assert L.vqw_xent_ws_bytes(32) == 8 and L.vqw_xent_ws_bytes(33) == 16 and L.vqw_xent_ws_bytes(8192) == 256 * 8 and L.vqw_xent_ws_bytes(0) == 0


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """Every refusal is a non-zero status with a message that names the constraint; the pointers are never dereferenced (they are
    no device addresses) and no HIP call is made (this test runs without a device)."""
    from hipops import _lib
    L = _lib.load()
    P = 4096          # a 16-byte aligned non-null stand-in for every pointer

    def efwd(B=2, Ti=3, Te=0, E=64, V=10, bs=8, t0=0, prefix=None):
        return L.vqw_embed_fwd(P, P, P, prefix, P, B, Ti, Te, E, V, bs, t0, None)

    def ebwd(B=2, Ti=3, Te=0, E=64, V=10, bs=8, t0=0, prefix=None):
        return L.vqw_embed_bwd(P, P, P, P, B, Ti, Te, E, V, bs, t0, None)

    for call in (efwd, ebwd):
        for E in (6, 0, 2, 4100, -4):
            assert call(E=E) != 0 and b"multiple of 4" in L.vqw_last_error() and b"E=%d" % E in L.vqw_last_error()
        assert call(V=0) != 0 and b"V=0" in L.vqw_last_error()
        assert call(Ti=-1) != 0 and b"Ti=-1" in L.vqw_last_error()
        assert call(Ti=9) != 0 and b"exceeds block_size=8" in L.vqw_last_error()
        assert call(Ti=3, t0=6) != 0 and b"exceeds block_size=8" in L.vqw_last_error()
        assert call(Ti=3, Te=6, prefix=P) != 0 and b"exceeds block_size=8" in L.vqw_last_error()
        assert call(B=0) != 0 and b"B >= 1" in L.vqw_last_error()
        assert call(Ti=0) != 0 and b"Te + Ti >= 1" in L.vqw_last_error()
    assert efwd(Te=2) != 0 and b"prefix" in L.vqw_last_error()
    assert efwd(prefix=P) != 0 and b"prefix" in L.vqw_last_error()
    assert L.vqw_embed_fwd(P, P + 4, P, None, P, 2, 3, 0, 64, 10, 8, 0, None) != 0 and b"16-byte aligned" in L.vqw_last_error()
    assert L.vqw_embed_bwd(P, P, P + 8, P, 2, 3, 0, 64, 10, 8, 0, None) != 0 and b"16-byte aligned" in L.vqw_last_error()

    for V in (0, -1, 65537):
        assert L.vqw_xent_fwd(P, P, P, P, None, None, 0, 4, V, None) != 0 and b"1 <= V <= 65536" in L.vqw_last_error()
        assert L.vqw_xent_bwd(P, P, P, P, P, 4, V, 1, None) != 0 and b"1 <= V <= 65536" in L.vqw_last_error()
    assert L.vqw_xent_fwd(P, P, P, P, None, None, 0, 0, 8, None) != 0 and b"rows >= 1" in L.vqw_last_error()
    assert L.vqw_xent_bwd(P, P, P, P, P, 0, 8, 0, None) != 0 and b"rows >= 1" in L.vqw_last_error()
    assert L.vqw_xent_fwd(P, P, P, P, P, P, 8, 33, 8, None) != 0 and b"workspace of 8 bytes, 16 needed" in L.vqw_last_error()
    assert L.vqw_xent_fwd(P, P, P, P, P, None, 0, 4, 8, None) != 0 and b"workspace" in L.vqw_last_error()
    assert L.vqw_xent_fwd(P, None, P, P, None, None, 0, 4, 8, None) != 0 and b"null pointer" in L.vqw_last_error()

    def samp(B=2, V=10, temp=1.0, k=0):
        return L.vqw_sample_topk(P, P, P, B, V, temp, k, None)

    for V in (0, 65537):
        assert samp(V=V) != 0 and b"1 <= V <= 65536" in L.vqw_last_error()
    assert samp(B=0) != 0 and b"B=0" in L.vqw_last_error()
    for temp in (0.0, -1.0, float("nan")):
        assert samp(temp=temp) != 0 and b"temperature" in L.vqw_last_error() and b"positive" in L.vqw_last_error()
    assert samp(k=-1) != 0 and b"top_k=-1" in L.vqw_last_error()
    assert L.vqw_sample_topk(P, None, P, 2, 10, 1.0, 0, None) != 0 and b"null pointer" in L.vqw_last_error()


def test_fake_kernels_under_fake_tensor_mode():
    """The operators trace under FakeTensorMode without a device: results have the shapes the real ones have."""
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        idx = torch.empty(2, 37, dtype=torch.long, device="cuda")
        tok, pos = torch.empty(257, 96, device="cuda"), torch.empty(1, 70, 96, device="cuda")
        prefix = torch.empty(2, 3, 96, device="cuda")
        assert ops.embedding(idx, tok, pos).shape == (2, 37, 96)
        x = ops.embedding(idx, tok, pos, prefix, t0=4)
        assert x.shape == (2, 40, 96) and x.is_contiguous()
        z, t = torch.empty(2, 40, 257, device="cuda"), torch.empty(2, 40, dtype=torch.long, device="cuda")
        assert ops.cross_entropy(z, t).shape == () and ops.cross_entropy(z, t, reduction="none").shape == (2, 40)
        loss, lse = ops.cross_entropy_lse(z.view(80, 257), t.view(80))
        assert loss.shape == (80,) and lse.shape == (80,)
        out = ops.sample_topk(z[:, -1, :], torch.empty(2, device="cuda"), 0.5, 10)
        assert out.shape == (2,) and out.dtype == torch.long
