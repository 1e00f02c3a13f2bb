"""CPU-side checks of the minGPT blocks (no GPU): the float64 restatement (tests/mingpt_ref.py) against the reference's fixtures
(tests/golden/mingpt_blocks_*.npz, made by tests/golden/make_golden_mingpt_blocks.py), the modules' state_dict contract,
initialisation and mask handling, and the C ABI / operator plumbing of the three new kernel families."""
import os
import re

import pytest
import torch

from helpers import sample_idx
import mingpt_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(M.CASES)
NEW_SYMBOLS = ("vqw_layernorm_ws_bytes", "vqw_layernorm_fwd", "vqw_layernorm_bwd", "vqw_gelu_fwd", "vqw_gelu_bwd",
               "vqw_causal_attention_fwd", "vqw_causal_attention_bwd")


def _fixture(golden, name):
    return golden("mingpt_blocks_%s.npz" % name)


def _state(g, name):
    return {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}


def _new(name):
    import networks
    return getattr(networks, M.CASES[name][0])(networks.GPTConfig(**M.config_kwargs(name)))


def _build(name):
    torch.manual_seed(M.SEEDS[name])
    return M.init_case_(_new(name), M.SEEDS[name])


def _max_rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(golden, name):
    """Output, input gradient, present and the sampled parameter gradients within twice the fixture's own fp32-against-fp64 spread."""
    g = _fixture(golden, name)
    x = g.t(name + "/in")
    assert torch.equal(x, M.case_input(name, int(g[name + "/seed"])))
    st = _state(g, name)
    out, present, grads = M.grads_ref(name, st, x, torch.float64)
    assert _max_rel(out, g[name + "/out"]) <= 2 * float(g[name + "/spread.out"])
    assert _max_rel(grads["input"], g[name + "/gin"]) <= 2 * float(g[name + "/spread.gin"])
    live = set(str(k) for k in g[name + "/live"])
    assert "input" in live and ("k.bias" if name == "att64" else "att.k.bias") not in live
    assert len(grads) == (9 if name == "att64" else 17)
    for k, gr in grads.items():
        ref = g["%s/g64.%s" % (name, k)]
        got = gr.reshape(-1)[sample_idx(gr.numel(), 256, seed=1)]
        if k in live:
            assert _max_rel(got, ref) <= 2 * float(g[name + "/spread.gP"]), k
            assert abs(float(gr.norm()) - float(g["%s/gnorm64.%s" % (name, k)])) <= 1e-9 * float(gr.norm()), k
    if name == "att64":
        assert tuple(present.shape) == (2, 2, 2, 40, 32)
        assert _max_rel(present, g[name + "/present"]) <= 2 * float(g[name + "/spread.present"])
    if name in M.PAST_CASES:
        past, xn = M.case_past(name, int(g[name + "/seed"]))
        assert torch.equal(past, g.t(name + "/past")) and torch.equal(xn, g.t(name + "/past_in"))
        with torch.no_grad():
            o, p = M.case_ref(name, xn.double(), {k: (v if k.endswith("mask") else v.double()) for k, v in st.items()}, past.double())
        assert tuple(o.shape) == (2, M.PAST_NEW, 64) and tuple(p.shape) == (2, 2, 2, M.PAST_NEW, 32)
        assert _max_rel(o, g[name + "/past_out"]) <= 2 * float(g[name + "/spread.past_out"])
        assert _max_rel(p, g[name + "/past_present"]) <= 2 * float(g[name + "/spread.past_present"])


def test_mask_rule_is_the_reference_mask():
    """visible() - the rule the kernel implements - is tril with mask[:u, :u] = 1, as stored in the fixtures."""
    from networks.mingpt import causal_mask
    for T, u in ((1, 0), (1, 1), (40, 5), (70, 0), (129, 40), (129, 129), (7, 1)):
        ref = torch.tril(torch.ones(T, T))
        ref[:u, :u] = 1
        assert torch.equal(M.visible(T, T, u), ref != 0), (T, u)
        assert torch.equal(causal_mask(T, u), ref), (T, u)
    assert bool(M.visible(3, 41, causal=False).all())


@pytest.mark.parametrize("name", CASES)
def test_state_dict_contract_and_seeded_init(golden, name):
    """Keys, their order, shapes and the parameter count equal the reference's; the same seed gives its (rounded) initial
    values; its state loads strictly."""
    g = _fixture(golden, name)
    m = _build(name)
    sd = m.state_dict()
    ref = _state(g, name)
    E, nh, T, nu, B = M.CASES[name][1]
    pre = "" if name == "att64" else "att."
    assert list(sd) == [str(k) for k in g[name + "/keys"]]
    if name != "att64":
        assert list(sd) == ["ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias", "att.mask", "att.k.weight", "att.k.bias", "att.q.weight",
                            "att.q.bias", "att.v.weight", "att.v.bias", "att.proj.weight", "att.proj.bias", "mlp.0.weight", "mlp.0.bias",
                            "mlp.2.weight", "mlp.2.bias"]
    assert [k for k, _ in m.named_parameters()] == [k for k in sd if not k.endswith("mask")]
    assert [k for k, _ in m.named_buffers()] == [pre + "mask"]
    assert sum(p.numel() for p in m.parameters()) == int(g[name + "/nparams"])
    assert tuple(sd[pre + "mask"].shape) == (1, 1, T, T) and tuple(sd[pre + "k.weight"].shape) == (E, E)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
        assert torch.equal(v, ref[k]), "initial %s differs from the reference's under the same seed" % k
    torch.manual_seed(12345)
    other = _new(name)
    other.load_state_dict({k: v.clone() for k, v in ref.items()}, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, ref[k]), k
    att = other if name == "att64" else other.att
    assert att.n_unmasked == (nu if nu > 1 else 0) and att.n_head == nh


def test_module_tree_and_configs():
    import networks
    from networks import GPTConfig, GPT1Config, CausalSelfAttention, Block
    c = GPTConfig(100, 16, n_embed=64, n_head=2)
    assert (c.vocab_size, c.block_size, c.emb_pdrop, c.res_pdrop, c.att_pdrop) == (100, 16, 0.1, 0.1, 0.1)
    c1 = GPT1Config(100, 16)
    assert (c1.n_layer, c1.n_head, c1.n_embed) == (12, 12, 768)
    b = Block(c)
    assert isinstance(b.att, CausalSelfAttention) and isinstance(b.ln1, torch.nn.LayerNorm) and b.ln1.eps == 1e-5
    assert [type(m).__name__ for m in b.mlp] == ["Linear", "GELU", "Linear", "Dropout"]
    assert isinstance(b.att.att_drop, torch.nn.Dropout) and isinstance(b.att.res_drop, torch.nn.Dropout) and b.att.att_drop.p == 0.1
    assert b.att.n_unmasked == 0 and b.att.k.weight.dim() == 2
    assert not hasattr(networks.mingpt, "GPT")          # the model itself is a later step


def test_n_unmasked_follows_a_loaded_mask():
    from networks import GPTConfig, Block, CausalSelfAttention
    from networks.mingpt import causal_mask
    kw = dict(n_embed=64, n_head=2, att_pdrop=0.0, res_pdrop=0.0)
    src = Block(GPTConfig(16, 24, n_unmasked=7, **kw))
    dst = Block(GPTConfig(16, 24, **kw))
    assert (src.att.n_unmasked, dst.att.n_unmasked) == (7, 0)
    dst.load_state_dict(src.state_dict(), strict=True)
    assert dst.att.n_unmasked == 7 and torch.equal(dst.att.mask, src.att.mask)
    att = CausalSelfAttention(GPTConfig(16, 24, n_unmasked=24, **kw))
    assert att.n_unmasked == 24
    sd = att.state_dict()
    sd["mask"] = causal_mask(24, 0).view(1, 1, 24, 24)
    att.load_state_dict(sd, strict=True)
    assert att.n_unmasked == 0


@pytest.mark.parametrize("kind", ["hole", "upper", "band"])
def test_non_conforming_mask_raises(kind):
    from networks import GPTConfig, CausalSelfAttention
    from networks.mingpt import causal_mask, n_unmasked_of
    att = CausalSelfAttention(GPTConfig(16, 12, n_embed=64, n_head=2, n_unmasked=4))
    sd = att.state_dict()
    m = causal_mask(12, 4)
    if kind == "hole":
        m[9, 3] = 0
    elif kind == "upper":
        m[5, 8] = 1
    else:
        m[:3, :5] = 1          # a 3 x 5 corner is no square
    sd["mask"] = m.view(1, 1, 12, 12)
    before = att.mask.clone()
    with pytest.raises(ValueError, match="not tril"):
        att.load_state_dict(sd, strict=True)
    # refused before anything was stored: the buffer and n_unmasked still agree
    assert torch.equal(att.mask, before) and att.n_unmasked == 4 == n_unmasked_of(att.mask)


def test_dropout_in_training_raises_and_eval_has_no_cpu_fallback():
    from networks import GPTConfig, Block, CausalSelfAttention
    x = torch.randn(1, 8, 64)
    for cls in (Block, CausalSelfAttention):
        m = cls(GPTConfig(16, 8, n_embed=64, n_head=2))          # the class defaults: every p = 0.1
        with pytest.raises(NotImplementedError, match="dropout"):
            m.train()(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.eval()(x)
        for p in ("att_pdrop", "res_pdrop"):
            kw = dict(att_pdrop=0.0, res_pdrop=0.0)
            kw[p] = 0.25
            m = cls(GPTConfig(16, 8, n_embed=64, n_head=2, **kw))
            if cls is Block and p == "res_pdrop":
                m.att.res_drop.p = 0.0          # leave only mlp's own Dropout
            with pytest.raises(NotImplementedError, match="dropout"):
                m.train()(x)
        m = cls(GPTConfig(16, 8, n_embed=64, n_head=2, att_pdrop=0.0, res_pdrop=0.0))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.train()(x)
    b = Block(GPTConfig(16, 8, n_embed=64, n_head=2, att_pdrop=0.0, res_pdrop=0.0))
    with pytest.raises(AssertionError):
        b.train()(x, return_present=True)


def test_operators_have_no_cpu_fallback():
    from hipops import ops
    x = torch.randn(2, 8, 64)
    w, b = torch.ones(64), torch.zeros(64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.layer_norm(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gelu(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.causal_attention(x, x, x, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.causal_attention_lse(x, x, x, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(x, torch.randn(32, 64), torch.zeros(32))


def test_new_symbols_in_header_and_signatures():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
    ops = library.register()
    for s in NEW_SYMBOLS:
        assert (s in ops) == (not s.endswith("_ws_bytes")), s
    sch = str(torch.ops.vqw.causal_attention_fwd.default._schema)
    assert "Tensor? q" in sch and "Tensor? v" in sch and "Tensor(a!)? o" in sch and "Tensor(b!)? lse" in sch
    assert "int n_head" in sch and "float scale" in sch and "int causal" in sch and "int n_unmasked" in sch
    sch = str(torch.ops.vqw.layernorm_bwd.default._schema)
    assert "Tensor? gy" in sch and "Tensor(a!)? gx" in sch and "Tensor(b!)? dgamma" in sch and "Tensor(c!)? dbeta" in sch and "Tensor(d!)? ws" in sch
    sch = str(torch.ops.vqw.gelu_bwd.default._schema)
    assert "Tensor? x" in sch and "Tensor? gy" in sch and "Tensor(a!)? gx" in sch
    L = _lib.load()
    # one dgamma / dbeta partial per 32 rows: [partials][2][C] floats
    assert L.vqw_layernorm_ws_bytes(32, 64) == 2 * 64 * 4 and L.vqw_layernorm_ws_bytes(33, 64) == 2 * 2 * 64 * 4
    assert L.vqw_layernorm_ws_bytes(258, 768) == 9 * 2 * 768 * 4


def test_c_abi_refuses_bad_shapes_before_any_device_work():
    """Every refusal is a non-zero status with a message that names the constraint; the pointers are never dereferenced (they are
    no device addresses) and no HIP call is made (this test runs without a device)."""
    from hipops import _lib
    L = _lib.load()
    P = 4096          # a 16-byte aligned non-null stand-in for every pointer

    def fwd(B=1, Tq=8, Tk=8, nh=2, hs=32, causal=1, nu=0):
        return L.vqw_causal_attention_fwd(P, P, P, P, P, B, Tq, Tk, nh, hs, 0.1, causal, nu, None)

    def bwd(B=1, Tq=8, Tk=8, nh=2, hs=32, causal=1, nu=0):
        return L.vqw_causal_attention_bwd(P, P, P, P, P, P, P, P, P, P, B, Tq, Tk, nh, hs, 0.1, causal, nu, None)

    for call in (fwd, bwd):
        for hs in (48, 160, 0, 16):
            assert call(hs=hs) != 0 and b"multiple of 32" in L.vqw_last_error() and b"hs=%d" % hs in L.vqw_last_error()
        assert call(Tq=0, Tk=0) != 0 and b"1 <= T" in L.vqw_last_error()
        assert call(Tq=65537, Tk=65537) != 0 and b"<= 65536" in L.vqw_last_error()
        assert call(nu=9) != 0 and b"n_unmasked=9" in L.vqw_last_error() and b"<= T" in L.vqw_last_error()
        assert call(nu=-1) != 0 and b"n_unmasked" in L.vqw_last_error()
        assert call(Tq=8, Tk=9) != 0 and b"Tq == Tk" in L.vqw_last_error()
        assert call(B=32768, nh=2) != 0 and b"65535" in L.vqw_last_error()
        assert call(causal=0, nu=3) != 0 and b"n_unmasked" in L.vqw_last_error()
    assert bwd(Tq=3, Tk=9, causal=0) != 0 and b"forward only" in L.vqw_last_error()
    assert L.vqw_causal_attention_fwd(P, P, P + 4, P, P, 1, 8, 8, 2, 32, 0.1, 1, 0, None) != 0 and b"16-byte aligned" in L.vqw_last_error()
    for C in (6, 0, 2, 4100, -4):
        assert L.vqw_layernorm_fwd(P, P, P, P, P, P, 4, C, 1e-5, None) != 0 and b"multiple of 4" in L.vqw_last_error()
        assert L.vqw_layernorm_bwd(P, P, P, P, P, P, P, P, P, 1 << 20, 4, C, None) != 0 and b"multiple of 4" in L.vqw_last_error()
    assert L.vqw_layernorm_fwd(P, P, P, P, P, P, 0, 64, 1e-5, None) != 0 and b"row count" in L.vqw_last_error()
    assert L.vqw_layernorm_bwd(P, P, P, P, P, P, P, P, P, 16, 64, 64, None) != 0 and b"workspace" in L.vqw_last_error()
    assert L.vqw_gelu_fwd(P, P, 0, None) != 0 and b"at least 1" in L.vqw_last_error()
    assert L.vqw_gelu_bwd(P, P, P, 0, None) != 0 and b"at least 1" in L.vqw_last_error()


def test_fake_kernels_under_fake_tensor_mode():
    """The four operators trace under FakeTensorMode without a device: the kernels' fake implementations touch nothing, and the
    results have the shapes the real ones have."""
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 70, 96, device="cuda")
        w, b = torch.empty(96, device="cuda"), torch.empty(96, device="cuda")
        y = ops.layer_norm(x, w, b)
        assert y.shape == x.shape and y.is_contiguous()
        assert ops.layer_norm(torch.empty(5, 96, device="cuda"), w, b).shape == (5, 96)
        assert ops.gelu(x).shape == x.shape
        y = ops.linear(x, torch.empty(384, 96, device="cuda"), torch.empty(384, device="cuda"))
        assert y.shape == (2, 70, 384) and y.is_contiguous()
        assert ops.linear(x, torch.empty(100, 96, device="cuda")).shape == (2, 70, 100)
        o = ops.causal_attention(x, x, x, 3, n_unmasked=5)
        assert o.shape == x.shape and o.is_contiguous()
        o, lse = ops.causal_attention_lse(x[:, :3], x, x, 3, causal=False)
        assert o.shape == (2, 3, 96) and lse.shape == (2, 3, 3)
        assert torch.ops.vqw.causal_attention_fwd(x, x, x, o, lse, 2, 70, 70, 3, 32, 0.1, 1, 0) is None
        assert torch.ops.vqw.gelu_fwd(x, y, x.numel()) is None
