"""CPU-side checks of the VQGAN's Downsample, Encoder and VQGAN (no GPU): the float64 restatement (tests/vqgan_model_ref.py)
against the reference's fixtures (tests/golden/vqgan_model_*.npz, made by tests/golden/make_golden_vqgan_model.py), the modules'
state_dict contract and initialisation, and the C ABI / operator plumbing of the stride-2 convolution and the wide attention."""
import importlib
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import sample_idx
from run_helpers import raw_config, write_config
import vqgan_model_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(M.CASES)
NEW_SYMBOLS = ("vqw_conv3s2_fwd", "vqw_conv3s2_dgrad_ws_bytes", "vqw_conv3s2_dgrad", "vqw_conv3s2_wgrad_ws_bytes", "vqw_conv3s2_wgrad",
               "vqw_vq_ema_update_w")


def _fixture(golden, name):
    return golden("vqgan_model_%s.npz" % name)


def _state(g, name):
    return {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}


def _build(name):
    import networks
    cls, args, _ = M.CASES[name]
    torch.manual_seed(M.SEEDS[name])
    return M.init_case_(getattr(networks, cls)(*args), name, M.SEEDS[name])


def _max_rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(golden, name):
    """Outputs, input gradient and the sampled parameter gradients within twice the fixture's own fp32-against-fp64 spread."""
    g = _fixture(golden, name)
    x = g.t(name + "/in")
    assert int(g[name + "/seed"]) == M.SEEDS[name] and torch.equal(x, M.case_input(name, M.SEEDS[name]))
    st = _state(g, name)
    res, grads = M.grads_ref(name, st, x, torch.float64)
    out = res["recon" if name == "vqgan" else "out"]
    assert _max_rel(out, g[name + "/out"]) <= 2 * float(g[name + "/spread.out"])
    assert _max_rel(grads["input"], g[name + "/gin"]) <= 2 * float(g[name + "/spread.gin"])
    live = set(str(k) for k in g[name + "/live"])
    assert "input" in live
    for k, gr in grads.items():
        if k in live:
            got = gr.reshape(-1)[sample_idx(gr.numel(), 256, seed=1)]
            assert _max_rel(got, g["%s/g64.%s" % (name, k)]) <= 2 * float(g[name + "/spread.gP"]), k
            assert abs(float(gr.norm()) - float(g["%s/gnorm64.%s" % (name, k)])) <= 1e-9 * float(gr.norm()), k
    if name == "vqgan":
        assert torch.equal(res["ids"], g.t(name + "/ids"))
        assert len(torch.unique(res["ids"])) == 8 and float(res["gap"].min()) >= 1e-4
        assert _max_rel(res["gap"], g[name + "/gap"]) <= 1e-9
        assert _max_rel(res["commit"], g[name + "/commit"]) <= 2 * float(g[name + "/spread.commit"])
        assert _max_rel(res["emb"], g[name + "/emb"]) <= 2 * float(g[name + "/spread.emb"])
        for k, v in res["buffers"].items():
            assert _max_rel(v, g["%s/buf.%s" % (name, k)]) <= 2 * float(g["%s/spread.buf.%s" % (name, k)]), k
        with torch.no_grad():
            gen = M.generate_ref(res["ids"], {k: v.double() for k, v in st.items()})
        assert _max_rel(gen, g[name + "/gen_out"]) <= 2 * float(g[name + "/spread.gen_out"])
        assert _max_rel(gen, res["recon"]) <= 1e-12      # the same codes, the same decoder: ids carry the whole quantised map


def test_embedded_4x4_identity_in_float64():
    """Downsample's convolution on an even-sized map is the 4x4 / stride 2 / pad 1 convolution of the 3x3 kernel embedded at
    [:, :, 1:, 1:] of a zero 4x4 kernel: the route the parent commit already had, and the baseline of tools/vqgan_model_bench.py."""
    g = torch.Generator().manual_seed(3)
    for (n, ci, co, h, w) in ((1, 3, 5, 4, 4), (2, 4, 2, 6, 10), (1, 2, 3, 18, 34)):
        x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64)
        wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
        b = torch.randn(co, generator=g, dtype=torch.float64)
        a = M.down2_ref(x, wt, b)
        e = F.conv2d(x, M.embed4(wt), b, stride=2, padding=1)
        assert a.shape == e.shape == (n, co, h // 2, w // 2)
        assert float((a - e).abs().max()) <= 1e-13


@pytest.mark.parametrize("name", CASES)
def test_state_dict_contract_and_seeded_init(golden, name):
    """Keys, their order, shapes and the parameter count equal the reference's; the same seed gives its (rounded) initial values;
    its state loads strictly and the convolution weights stay channels_last."""
    import networks
    g = _fixture(golden, name)
    m = _build(name)
    sd = m.state_dict()
    ref = _state(g, name)
    assert list(sd) == [str(k) for k in g[name + "/keys"]]
    assert [k for k, _ in m.named_parameters()] == [k for k in sd if M.is_param(k)]          # creation order
    assert sum(p.numel() for p in m.parameters()) == int(g[name + "/nparams"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
        assert torch.equal(v, ref[k]), "initial %s differs from the reference's under the same seed" % k
    cls, args, _ = M.CASES[name]
    torch.manual_seed(12345)
    other = getattr(networks, cls)(*args)
    other.load_state_dict({k: v.clone().contiguous() for k, v in ref.items()}, strict=True)
    n4 = 0
    for k, v in other.state_dict().items():
        assert torch.equal(v, ref[k]), k
        if v.dim() == 4:
            assert v.is_contiguous(memory_format=torch.channels_last), k
            n4 += 1
    assert n4 >= 1


def test_module_tree_and_default_parameter_count(golden):
    from networks import VQGAN, Encoder, Decoder, Downsample, AttnBlock, VQ
    m = _build("vqgan")
    assert isinstance(m.encoder, Encoder) and isinstance(m.decoder, Decoder) and isinstance(m.vq, VQ)
    assert isinstance(m.encoder.down[0].downsample, Downsample) and not hasattr(m.encoder.down[1], "downsample")
    assert len(m.encoder.down[0].attn) == 0 and len(m.encoder.down[1].attn) == 1 and isinstance(m.encoder.mid.attn_1, AttnBlock)
    conv = m.encoder.down[0].downsample.conv
    assert (conv.kernel_size, conv.stride, conv.padding) == ((3, 3), (2, 2), (0, 0))
    assert (m.vq.emb_dim, m.vq.dict_size, m.vq.momentum, m.vq.eps) == (32, 8, 0.99, 1e-5)
    # the VQGAN's quantiser follows torch's EMA weight; the class default (the U-Net models) is unchanged
    assert m.vq.torch_ema_weight is True and VQ.torch_ema_weight is False and VQ(4, 2, 0.99, 1e-5, "torch").torch_ema_weight is False
    d = VQGAN()
    assert sum(p.numel() for p in d.parameters()) == int(_fixture(golden, "vqgan")["vqgan/nparams_default"])
    assert d.encoder.mid.attn_1.in_channels == 1024 and d.vq.embed.shape == (64, 512)
    assert [b.downsample.conv.in_channels for b in d.encoder.down[:-1]] == [32, 64, 128, 256, 512]
    import networks.vqgan as blocks_module
    assert not hasattr(blocks_module, "VQGAN")


def test_downsample_without_conv_raises():
    from networks import Downsample
    d = Downsample(32, False)
    assert len(d.state_dict()) == 0
    with pytest.raises(NotImplementedError, match="average pooling"):
        d(torch.zeros(1, 32, 4, 4))


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
    sch = str(torch.ops.vqw.conv3s2_fwd.default._schema)
    assert "Tensor? x" in sch and "Tensor? w_ohwi" in sch and "Tensor? bias" in sch and "Tensor(a!)? y" in sch and "int Cout" in sch
    sch = str(torch.ops.vqw.conv3s2_wgrad.default._schema)
    assert "Tensor(a!)? dw_ohwi" in sch and "Tensor(b!)? dbias" in sch and "int accumulate" in sch
    sch = str(torch.ops.vqw.vq_ema_update_w.default._schema)
    assert "Tensor(a!)? embed" in sch and "float momentum, float new_weight, float eps" in sch
    L = _lib.load()
    assert L.vqw_conv3s2_dgrad_ws_bytes(64, 32) == 9 * 64 * 32 * 4
    assert L.vqw_conv3s2_wgrad_ws_bytes(2, 64, 64, 32, 32) > 0 and L.vqw_conv3s2_wgrad_ws_bytes(2, 18, 34, 64, 64) > 0


def test_argument_checks_return_errors_before_any_device_work():
    """Dummy pointers: a call that reached a launch would fault, these return with a message."""
    from hipops import _lib
    L = _lib.load()
    big = 1 << 30
    for H, W, Cin, Cout, msg in ((5, 4, 32, 32, b"even"), (4, 6, 48, 32, b"multiples of 32"), (4, 4, 32, 48, b"multiples of 32"),
                                 (4, 7, 32, 32, b"even"), (0, 4, 32, 32, b"even")):
        assert L.vqw_conv3s2_fwd(1, 1, 1, 1, 1, H, W, Cin, Cout, None) != 0 and msg in L.vqw_last_error(), (H, W, Cin, Cout)
        assert L.vqw_conv3s2_dgrad(1, 1, 1, 1, big, 1, H, W, Cin, Cout, None) != 0 and msg in L.vqw_last_error()
        assert L.vqw_conv3s2_wgrad(1, 1, 1, 1, 1, big, 1, H, W, Cin, Cout, 0, None) != 0 and msg in L.vqw_last_error()
    assert L.vqw_conv3s2_fwd(1, 1, 1, 1, 1 << 16, 1 << 10, 1 << 10, 32, 32, None) != 0 and b"4 GiB" in L.vqw_last_error()
    assert L.vqw_conv3s2_dgrad(1, 1, 1, 1, 16, 1, 4, 4, 32, 32, None) != 0 and b"workspace" in L.vqw_last_error()
    assert L.vqw_conv3s2_wgrad(1, 1, 1, 1, 1, 16, 1, 4, 4, 32, 32, 0, None) != 0 and b"workspace" in L.vqw_last_error()
    for C in (544, 1056, 1088, 48):
        assert L.vqw_attention_fwd(1, 1, 1, 1, 1, 1, 16, C, 1.0, None) != 0 and b"multiple of" in L.vqw_last_error(), C
        assert L.vqw_attention_bwd(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 16, C, 1.0, None) != 0 and b"multiple of" in L.vqw_last_error(), C


def test_operators_have_no_cpu_fallback():
    from hipops import ops
    from networks import Downsample
    x = torch.randn(1, 32, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv2d_down2(x, torch.randn(32, 32, 3, 3), torch.zeros(32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Downsample(32, True)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _build("encoder")(torch.randn(1, 1, 32, 32))


def test_fake_kernels_under_fake_tensor_mode():
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 64, 6, 10, device="cuda").contiguous(memory_format=torch.channels_last)
        w = torch.empty(96, 64, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last)
        y = ops.conv2d_down2(x, w, torch.empty(96, device="cuda"))
        assert y.shape == (2, 96, 3, 5) and y.is_contiguous(memory_format=torch.channels_last)
        q = torch.empty(1, 1024, 4, 4, device="cuda").contiguous(memory_format=torch.channels_last)
        assert ops.self_attention(q, q, q, 1 / 32).shape == q.shape
        assert torch.ops.vqw.conv3s2_fwd(x, w, None, y, 2, 6, 10, 64, 96) is None


def test_configure_vqgan_from_a_namespace_config():
    from trainers.config import configure_vqgan
    from networks import VQGAN
    _, args, _ = M.CASES["vqgan"]
    names = ("in_channels", "mid_channels", "out_channels", "emb_dim", "dict_size", "enc_ch_multiplier", "dec_ch_multiplier",
             "num_res_blocks", "enc_attn_resolutions", "dec_attn_resolutions", "resolution", "p_dropout", "resamp_with_conv", "knn_backend")
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(vqgan=types.SimpleNamespace(**dict(zip(names, args)))))
    torch.manual_seed(5)
    m = configure_vqgan(cfg)
    torch.manual_seed(5)
    ref = VQGAN(*args)
    assert isinstance(m, VQGAN) and list(m.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))
    del cfg.model.vqgan.knn_backend
    with pytest.raises(AttributeError):
        configure_vqgan(cfg)


def test_launcher_still_refuses_the_vqgan_flag(tmp_path):
    rv = importlib.import_module("run_vqwnet")
    cfg = write_config(tmp_path / "c.json", raw_config(tmp_path / "out"))
    with pytest.raises(NotImplementedError, match="VQGAN"):
        rv.main(["-c", cfg, "-v"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_files_stay_below_one_mib(name):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vqgan_model_%s.npz" % name)) <= 1 << 20
