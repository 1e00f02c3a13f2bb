"""CPU-side checks of the VQGAN decoder blocks (no GPU): the float64 restatement (tests/vqgan_ref.py) against the reference's
fixtures (tests/golden/vqgan_blocks_*.npz, made by tests/golden/make_golden_vqgan_blocks.py), the modules' state_dict contract
and initialisation, and the C ABI / operator plumbing of the two new kernel families."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import sample_idx
import vqgan_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(V.CASES)
NEW_SYMBOLS = ("vqw_groupnorm_splits", "vqw_groupnorm_ws_bytes", "vqw_groupnorm_fwd", "vqw_groupnorm_bwd", "vqw_swish_fwd",
               "vqw_swish_bwd", "vqw_attention_fwd", "vqw_attention_bwd")


def _fixture(golden, name):
    return golden("vqgan_blocks_%s.npz" % name)


def _state(g, name):
    return {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}


def _build(name):
    import networks
    cls, kw, _, _ = V.CASES[name]
    torch.manual_seed(V.SEEDS[name])
    return V.init_case_(getattr(networks, cls)(**kw), V.SEEDS[name])


def _max_rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(golden, name):
    """Output, input gradient and the sampled parameter gradients within twice the fixture's own fp32-against-fp64 spread."""
    g = _fixture(golden, name)
    x = g.t(name + "/in")
    assert torch.equal(x, V.case_input(name, int(g[name + "/seed"])))
    out, grads = V.grads_ref(name, _state(g, name), x, torch.float64)
    assert _max_rel(out, g[name + "/out"]) <= 2 * float(g[name + "/spread.out"])
    assert _max_rel(grads["input"], g[name + "/gin"]) <= 2 * float(g[name + "/spread.gin"])
    live = set(str(k) for k in g[name + "/live"])
    assert "input" in live and (name != "attn64" or "k.bias" not in live)
    for k, gr in grads.items():
        ref = g["%s/g64.%s" % (name, k)]
        got = gr.reshape(-1)[sample_idx(gr.numel(), 256, seed=1)]
        if k in live:
            assert _max_rel(got, ref) <= 2 * float(g[name + "/spread.gP"]), k
            assert abs(float(gr.norm()) - float(g["%s/gnorm64.%s" % (name, k)])) <= 1e-9 * float(gr.norm()), k
    if name == "decoder":
        with torch.no_grad():
            e = V.decoder_ref(x.double(), {k: v.double() for k, v in _state(g, name).items()})
        assert _max_rel(e, g[name + "/eval_out"]) <= 2 * float(g[name + "/spread.eval_out"])
        assert torch.equal(e, out)              # no dropout at p = 0, no running statistics: eval is the training forward


@pytest.mark.parametrize("name", CASES)
def test_state_dict_contract_and_seeded_init(golden, name):
    """Keys, their order, shapes and the parameter count equal the reference's; the same seed gives its (rounded) initial
    values; its state loads strictly and the convolution weights stay channels_last."""
    g = _fixture(golden, name)
    m = _build(name)
    sd = m.state_dict()
    ref = _state(g, name)
    assert list(sd) == [str(k) for k in g[name + "/keys"]]
    assert [k for k, _ in m.named_parameters()] == list(sd)          # parameters only, in creation order
    assert sum(p.numel() for p in m.parameters()) == int(g[name + "/nparams"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
        assert torch.equal(v, ref[k]), "initial %s differs from the reference's under the same seed" % k
    import networks
    cls, kw, _, _ = V.CASES[name]
    torch.manual_seed(12345)
    other = getattr(networks, cls)(**kw)
    other.load_state_dict({k: v.clone().contiguous() for k, v in ref.items()}, strict=True)
    n4 = 0
    for k, v in other.state_dict().items():
        assert torch.equal(v, ref[k]), k
        if v.dim() == 4:
            assert v.is_contiguous(memory_format=torch.channels_last), k
            n4 += 1
    assert n4 >= 2


def test_decoder_tree():
    from networks import Decoder, ResnetBlock, AttnBlock, Upsample
    m = _build("decoder")
    assert isinstance(m.mid.block_1, ResnetBlock) and isinstance(m.mid.attn_1, AttnBlock) and isinstance(m.up[1].upsample, Upsample)
    assert len(m.up) == 2 and len(m.up[1].attn) == 1 and len(m.up[0].attn) == 0 and not hasattr(m.up[0], "upsample")
    assert isinstance(m.mid.block_1.norm1, torch.nn.GroupNorm) and m.mid.block_1.norm1.eps == 1e-6 and m.mid.block_1.norm1.num_groups == 32
    assert isinstance(m.mid.block_1.dropout, torch.nn.Dropout)
    assert isinstance(m, Decoder) and len(m.state_dict()) == 62
    import networks.vqgan as M
    for absent in ("Encoder", "Downsample", "VQGAN"):
        assert not hasattr(M, absent)


def test_normalize_rejects_channels_not_divisible_by_32():
    from networks import Normalize
    with pytest.raises(ValueError, match="divisible"):
        Normalize(48)
    with pytest.raises(ValueError, match="divisible"):
        torch.nn.GroupNorm(32, 48)
    from hipops import _lib
    L = _lib.load()          # the C ABI's argument check refuses it too, before any device work
    assert L.vqw_groupnorm_fwd(1, 1, 1, 1, 1, 1, 1, 1 << 20, 1, 16, 48, 1e-6, 0, None) != 0
    assert b"divisible" in L.vqw_last_error()
    assert L.vqw_attention_fwd(1, 1, 1, 1, 1, 1, 16, 48, 1.0, None) != 0 and b"multiple of 32" in L.vqw_last_error()
    assert L.vqw_attention_fwd(1, 1, 1, 1, 1, 1, 16, 544, 1.0, None) != 0


def test_new_symbols_in_header_and_signatures():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
    ops = library.register()
    for s in NEW_SYMBOLS:
        assert (s in ops) == (not s.endswith(("_splits", "_ws_bytes"))), s
    sch = str(torch.ops.vqw.groupnorm_fwd.default._schema)
    assert "Tensor? x" in sch and "Tensor(a!)? y" in sch and "Tensor(b!)? mean" in sch and "Tensor(c!)? rstd" in sch and "float eps" in sch
    sch = str(torch.ops.vqw.attention_bwd.default._schema)
    assert "Tensor? go" in sch and "Tensor(b!)? gq" in sch and "float scale" in sch
    L = _lib.load()
    # the tier choice: one workgroup up to 16384 elements per image, split above
    assert L.vqw_groupnorm_splits(512, 32) == 1 and L.vqw_groupnorm_splits(513, 32) == 2 and L.vqw_groupnorm_splits(64 * 64, 512) == 128
    assert L.vqw_groupnorm_splits(512 * 512, 32) == 256
    assert L.vqw_groupnorm_ws_bytes(2, 513, 32) == 2 * 2 * 32 * 16 + 2 * 32 * 16 + 2 * 32 * 8          # partials, totals, group means


def test_operators_have_no_cpu_fallback():
    from hipops import ops
    from networks import ResnetBlock, AttnBlock, nonlinearity
    x = torch.randn(1, 32, 4, 4)
    w, b = torch.ones(32), torch.zeros(32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.group_norm(x, w, b, swish=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.self_attention(x, x, x, 32 ** -0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nonlinearity(x)
    for m in (ResnetBlock(32), AttnBlock(32)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)


def test_fake_kernels_under_fake_tensor_mode():
    """The operators trace under FakeTensorMode without a device: the kernels' fake implementations touch nothing, and the
    results have the shapes and layout the real ones have."""
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 96, 5, 7, device="cuda").contiguous(memory_format=torch.channels_last)
        w, b = torch.empty(96, device="cuda"), torch.empty(96, device="cuda")
        y = ops.group_norm(x, w, b, swish=True)
        assert y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
        o = ops.self_attention(x, x, x, 96 ** -0.5)
        assert o.shape == x.shape and o.is_contiguous(memory_format=torch.channels_last)
        o, lse = ops.self_attention_lse(x, x, x, 96 ** -0.5)
        assert lse.shape == (2, 35)
        assert ops.swish(x).shape == x.shape
        assert torch.ops.vqw.attention_fwd(x, x, x, o, lse, 2, 35, 96, 0.1) is None
