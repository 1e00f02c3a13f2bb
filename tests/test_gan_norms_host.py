"""Host-side tests (no GPU) of the discriminator's ActNorm / spectral-norm configurations and of the config-driven second
step: the float64 restatement tests/gan_norm_ref.py against the reference's fixtures, the module and checkpoint contract on
CPU, trainers.config against a config file in the reference's key names, and the no-fallback rule."""
import json
import os
import re

import numpy as np
import pytest
import torch

from gan_norm_ref import discriminator_ref, hinge_d_loss_ref, adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tag -> (fixture file, normalization, n_filters, n_layers, spectral norm, training mode)
CASES = {
    "act_f16": ("gan_norms_act_f16.npz", "actnorm", 16, 3, False, True),
    "act_f8_eval": ("gan_norms.npz", "actnorm", 8, 2, False, False),
    "act_uninit_eval": ("gan_norms.npz", "actnorm", 8, 2, False, False),
    "sn_bn_f16": ("gan_norms_sn_bn_f16.npz", "batchnorm", 16, 3, True, True),
    "sn_act_f8": ("gan_norms.npz", "actnorm", 8, 2, True, True),
    "sn_bn_f8_eval": ("gan_norms.npz", "batchnorm", 8, 2, True, False),
    "gen_pass_sn": ("gan_norms.npz", "batchnorm", 8, 2, True, True),
}
NEW_SYMBOLS = ("vqw_actnorm_prepare", "vqw_actnorm_loc_grad", "vqw_spectral_norm_fwd", "vqw_spectral_norm_bwd")
F32_EPS = 2.0 ** -24          # storage rounding of a fixture value, relative to that value


def _close(a, ref, spread, what):
    """max |a - ref| <= (2 x the reference's own fp32-against-fp64 spread + fp32 storage rounding) x the largest |ref|"""
    a, ref = a.detach().double(), torch.as_tensor(ref).double()
    assert a.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(ref.shape))
    scale = float(ref.abs().max())
    err = float((a - ref).abs().max())
    bound = (2.0 * float(spread) + F32_EPS) * scale
    assert err <= bound, "%s: max |diff| %.3e > %.3e (spread %.1e, largest element %.3e)" % (what, err, bound, float(spread), scale)


def _state64(g, tag, grad=True):
    st = {}
    for k, v in g.group(tag).items():
        if k.startswith("P."):
            v = v.double() if v.is_floating_point() else v.clone()
            if grad and v.is_floating_point() and k.endswith((".weight", ".weight_orig", ".bias", ".loc", ".scale")):
                v.requires_grad_(True)
            st[k[2:]] = v
    return st


@pytest.mark.parametrize("tag", sorted(CASES))
def test_float64_restatement_reproduces_fixture(golden, tag):
    file, _, _, n_layers, _, train = CASES[tag]
    g = golden(file)
    gen_pass = tag == "gen_pass_sn"
    st = _state64(g, tag, grad=not gen_pass)
    x = g.t(tag + "/in.0").double().requires_grad_(True)
    out = discriminator_ref(x, st, n_layers, train)
    (out * g.t(tag + "/R.0").double()).sum().backward()
    sp = {k: float(g["%s/spread.%s" % (tag, k)]) for k in ("out", "gin", "gP", "after")}
    _close(out, g[tag + "/out.0"], sp["out"], tag + " out")
    _close(x.grad, g[tag + "/gin.0"], sp["gin"], tag + " gin")
    n_gp = 0
    for k in g.files:
        if k.startswith(tag + "/gP."):
            _close(st[k[len(tag) + 4:]].grad, g[k], sp["gP"], k)
            n_gp += 1
    assert (n_gp == 0) == gen_pass
    n_after = 0
    for k in g.files:
        if k.startswith(tag + "/after."):
            name = k[len(tag) + 7:]
            if st[name].is_floating_point():
                _close(st[name], g[k], sp["after"], k)
            else:
                assert int(st[name]) == int(g[k]), k
            n_after += 1
    assert n_after > 0
    if tag == "act_uninit_eval":                           # eval mode never initialises
        assert all(int(v) == 0 for k, v in st.items() if k.endswith("initialized"))
        assert all(float(v.detach().abs().max()) == 0.0 for k, v in st.items() if k.endswith(".loc"))
    if tag == "sn_bn_f8_eval":                             # eval mode: u, v unchanged
        for k, v in st.items():
            if k.endswith(("weight_u", "weight_v")):
                assert torch.equal(v.float(), g.t("%s/P.%s" % (tag, k)))


def test_float64_restatement_reproduces_discriminator_updates(golden):
    g = golden("gan_norms.npz")
    tag = "dstep_sn_act"
    st = _state64(g, tag)
    params = {k: v for k, v in st.items() if v.requires_grad}
    moments = {k: [torch.zeros_like(v), torch.zeros_like(v)] for k, v in params.items()}
    for s in range(2):
        real, fake = g.t("%s/real%d" % (tag, s)).double(), g.t("%s/fake%d" % (tag, s)).double()
        l_dis = hinge_d_loss_ref(discriminator_ref(real, st, 3, True), discriminator_ref(fake, st, 3, True))
        _close(l_dis, g["%s/loss%d" % (tag, s)], float(g[tag + "/spread.loss"]), "loss %d" % s)
        grads = dict(zip(params, torch.autograd.grad(0.8 * l_dis, list(params.values()))))
        adam_ref(params, grads, moments, s + 1, lr=1e-3, betas=(0.5, 0.999))
    for k, v in st.items():
        ref = g["%s/after.%s" % (tag, k)]
        if v.is_floating_point():
            _close(v, ref, float(g[tag + "/spread.after"]), "after." + k)
        else:
            assert int(v) == int(ref) == 1, k


def _build(normalization, n_filters, n_layers, spectral):
    from networks import NLayerDiscriminator
    from utils import apply_spectral_norm
    dis = NLayerDiscriminator(1, 1, n_filters=n_filters, n_layers=n_layers, normalization=normalization)
    if spectral:
        apply_spectral_norm(dis)
    return dis


@pytest.mark.parametrize("tag", sorted(CASES) + ["dstep_sn_act"])
def test_state_dict_matches_reference_keys_shapes_dtypes(golden, tag):
    file, norm, nf, nl, sn, _ = CASES.get(tag, ("gan_norms.npz", "actnorm", 8, 3, True, True))
    g = golden(file)
    pre = tag + "/P."
    ref = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}      # the arrays as stored (0-d stays 0-d)
    sd = _build(norm, nf, nl, sn).state_dict()
    assert list(sd) == list(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape) and v.dtype == ref[k].dtype, k


def test_constructor_signatures_and_unbuilt_paths():
    import inspect
    from networks import NLayerDiscriminator
    from networks.actnorm import ActNorm
    assert list(inspect.signature(NLayerDiscriminator.__init__).parameters)[1:] == ["in_channels", "out_channels", "n_filters",
                                                                                    "n_layers", "normalization"]
    assert list(inspect.signature(ActNorm.__init__).parameters)[1:] == ["num_features", "logdet", "affine", "allow_reverse_init"]
    with pytest.raises(NotImplementedError):
        NLayerDiscriminator(normalization='instancenorm')
    with pytest.raises(AssertionError):
        NLayerDiscriminator(normalization='batch')
    with pytest.raises(NotImplementedError):
        ActNorm(4, logdet=True)
    a = ActNorm(4)
    with pytest.raises(NotImplementedError):
        a(torch.zeros(2, 4, 3, 3), reverse=True)
    with pytest.raises(NotImplementedError):
        a(torch.zeros(2, 4))
    dis = NLayerDiscriminator(1, 1, 8, 2, 'actnorm')
    assert dis.main[2].bias is not None and dis.main[5].bias is not None          # convolutions next to an ActNorm carry a bias
    assert NLayerDiscriminator(1, 1, 8, 2).main[2].bias is None


def test_apply_spectral_norm_renames_weight_and_adds_buffers_on_convs_only():
    from networks.discriminator import SConv2d
    for norm in ("batchnorm", "actnorm"):
        plain, sn = _build(norm, 8, 2, False), _build(norm, 8, 2, True)
        want = set()
        for k in plain.state_dict():
            is_conv = isinstance(plain.get_submodule(k.rsplit(".", 1)[0]), SConv2d)
            if is_conv and k.endswith(".weight"):
                want |= {k + s for s in ("_orig", "_u", "_v")}
            else:
                want.add(k)
        assert set(sn.state_dict()) == want
        for m in sn.modules():
            if isinstance(m, SConv2d):
                assert "weight" not in dict(m.named_parameters(recurse=False))
                cout, cin, kh, kw = m.weight_orig.shape
                assert m.weight_u.shape == (cout,) and m.weight_v.shape == (cin * kh * kw,)
                assert abs(float(m.weight_u.norm()) - 1) < 1e-5 and abs(float(m.weight_v.norm()) - 1) < 1e-5
                assert m.weight_orig.is_contiguous(memory_format=torch.channels_last)
            else:
                assert not hasattr(m, "weight_orig")
        with pytest.raises(RuntimeError):
            from utils import apply_spectral_norm
            apply_spectral_norm(sn)                            # twice on the same parameter, as torch refuses it


@pytest.mark.parametrize("norm,sn", [("batchnorm", False), ("batchnorm", True), ("actnorm", False), ("actnorm", True)])
def test_checkpoint_round_trip_is_strict(tmp_path, norm, sn):
    from utils.checkpoint import load_discriminator_from_ckpt, save_lightning_style_ckpt
    torch.manual_seed(3)
    a, b = _build(norm, 8, 2, sn), _build(norm, 8, 2, sn)
    with torch.no_grad():
        for m in a.modules():
            if hasattr(m, "initialized"):
                m.loc.normal_()
                m.scale.uniform_(0.5, 2)
                m.initialized.fill_(1)
    path = str(tmp_path / "d.ckpt")
    save_lightning_style_ckpt(path, dis=a)
    load_discriminator_from_ckpt(path, b)
    for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2) and v.dtype == v2.dtype, k
    for m in b.modules():
        if hasattr(m, "initialized"):
            assert m._host_initialized is True                 # the host-side flag follows a loaded state dict
    other = _build(norm, 8, 2, not sn)
    with pytest.raises(RuntimeError):                          # strict: the other parametrisation's keys do not fit
        load_discriminator_from_ckpt(path, other)


def _config(tmp_path, dis=None, loss=None, run=None, **top):
    from utils import load_json
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["model"]["dis"].update(dis or {})
    raw["loss"].update(loss or {})
    raw["run"].update(dict(training_mode="second_step"), **(run or {}))
    raw.update(top)
    p = tmp_path / "c.json"
    p.write_text(json.dumps(raw))
    return load_json(str(p))


def test_committed_configs_name_a_normalization_the_discriminator_accepts():
    from utils import load_json
    from trainers import configure_discriminator
    for f in sorted(os.listdir(os.path.join(ROOT, "configs"))):
        if f.endswith(".json"):
            c = load_json(os.path.join(ROOT, "configs", f))
            assert c.model.dis.normalization == "batchnorm", f
    d = configure_discriminator(load_json(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    assert isinstance(d.main[3], torch.nn.BatchNorm2d) and not hasattr(d.main[0], "weight_orig")


def test_configure_discriminator(tmp_path):
    from networks.actnorm import ActNorm
    from trainers import configure_discriminator
    c = _config(tmp_path, dis=dict(n_filters=8, n_layers=2, normalization="actnorm", apply_spectral_norm=True))
    d = configure_discriminator(c)
    assert isinstance(d.main[3], ActNorm) and d.main[0].weight_orig.shape == (8, c.model.vqmodel.in_channels, 4, 4)
    assert len(d.main) == 9 and d.main[8].weight_orig.shape[0] == 1
    d = configure_discriminator(_config(tmp_path, dis=dict(n_filters=8, n_layers=3, normalization="actnorm")))
    assert len(d.main) == 12 and hasattr(d.main[0], "weight") and not hasattr(d.main[0], "weight_orig")
    with pytest.raises(NotImplementedError, match="UNetDiscriminator"):
        configure_discriminator(_config(tmp_path, dis=dict(model_name="UNetDiscriminator")))
    with pytest.raises(AssertionError):
        configure_discriminator(_config(tmp_path, dis=dict(normalization="batch")))
    with pytest.raises(NotImplementedError):
        configure_discriminator(_config(tmp_path, dis=dict(normalization="instancenorm")))


def test_gan_loss_weights(tmp_path):
    from trainers import gan_loss_weights, GanLossWeights
    assert GanLossWeights._fields == ("recon", "gen", "dis", "freq", "perceptual")
    w = gan_loss_weights(_config(tmp_path, loss=dict(loss_weight=dict(recon=2.0, gen=0.25, freq=0.5, perceptual=0.125, commit=1.0))))
    assert w == GanLossWeights(recon=2.0, gen=0.25, dis=1.0, freq=0.5, perceptual=0.125)          # no `dis` key: the default
    w = gan_loss_weights(_config(tmp_path, loss=dict(loss_weight=dict(recon=1.0, gen=1.0, dis=0.5))))
    assert w == GanLossWeights(recon=1.0, gen=1.0, dis=0.5, freq=0.0, perceptual=0.0)


def test_build_second_step_trainer_from_config(tmp_path):
    """On the CPU (nothing is launched by construction): models, checkpoints, optimiser settings, loss switches."""
    from networks.actnorm import ActNorm
    from trainers import build_second_step_trainer, build_first_step_trainer, configure_models, configure_discriminator
    from utils.checkpoint import save_lightning_style_ckpt
    kw = dict(dis=dict(n_filters=8, n_layers=2, normalization="actnorm", apply_spectral_norm=True),
              loss=dict(n_inner_loops=2, use_recon_loss=False, loss_weight=dict(recon=1.0, gen=0.5, dis=0.75)),
              dec_optim=dict(lr=2e-4, b1=0.5, b2=0.9, weight_decay=0.0), dis_optim=dict(lr=4e-4, b1=0.0, b2=0.99, weight_decay=1e-5))
    c = _config(tmp_path, **kw)
    torch.manual_seed(7)
    enc, dec = configure_models(c)
    dis = configure_discriminator(c)
    with torch.no_grad():
        for m in dis.modules():
            if isinstance(m, ActNorm):
                m.initialized.fill_(1)
    ck = str(tmp_path / "first.ckpt")
    save_lightning_style_ckpt(ck, enc, dec, dis)
    tr = build_second_step_trainer(c, device="cpu", first_stage_ckpt_path=ck, discriminator_ckpt_path=ck)
    for (k, v), (_, v2) in zip(enc.state_dict().items(), tr.encoder.state_dict().items()):
        assert torch.equal(v, v2), k
    for (k, v), (_, v2) in zip(dis.state_dict().items(), tr.dis.state_dict().items()):
        assert torch.equal(v, v2), k
    assert all(m._host_initialized for m in tr.dis.modules() if isinstance(m, ActNorm))
    gd, gs = tr.dec_optim.param_groups[0], tr.dis_optim.param_groups[0]
    assert (gd["lr"], tuple(gd["betas"]), gd["weight_decay"]) == (2e-4, (0.5, 0.9), 0.0)
    assert (gs["lr"], tuple(gs["betas"]), gs["weight_decay"]) == (4e-4, (0.0, 0.99), 1e-5)
    assert len(gs["params"]) == len(list(tr.dis.parameters()))
    assert tr.n_inner_loops == 2 and tr.use_recon_loss is False and tr.frequency_loss is None and tr.perceptual_loss is None
    assert tuple(tr.w) == (1.0, 0.5, 0.75, 0.0, 0.0)
    # the checkpoint paths of the config itself; n_inner_loops absent -> 1
    c2 = _config(tmp_path, dis=kw["dis"], run=dict(first_stage_ckpt_path=ck, discriminator_ckpt_path=ck))
    tr2 = build_second_step_trainer(c2, device="cpu")
    assert tr2.n_inner_loops == 1 and tr2.use_recon_loss is True
    assert torch.equal(tr2.dis.main[3].scale, dis.main[3].scale) and torch.equal(tr2.encoder.vq.embed, enc.vq.embed)
    with pytest.raises(NotImplementedError, match="hinge_d_loss"):
        build_second_step_trainer(_config(tmp_path, loss=dict(dis_loss_type="vanilla_d_loss")), device="cpu")
    with pytest.raises(NotImplementedError, match="UNetDiscriminator"):
        build_second_step_trainer(_config(tmp_path, dis=dict(model_name="UNetDiscriminator")), device="cpu")
    with pytest.raises(NotImplementedError, match="build_second_step_trainer"):
        build_first_step_trainer(c, device="cpu")
    with pytest.raises(NotImplementedError):
        build_second_step_trainer(_config(tmp_path, run=dict(training_mode="first_step")), device="cpu")


def test_second_step_trainer_keeps_its_signature_and_defaults():
    import inspect
    from trainers import SecondStepTrainer
    p = inspect.signature(SecondStepTrainer.__init__).parameters
    assert list(p)[1:13] == ["encoder", "decoder", "dis", "loss_weight", "n_inner_loops", "lr", "betas", "weight_decay", "device",
                             "data_parallel", "frequency_loss", "perceptual_loss"]
    assert p["dec_optim"].default is None and p["dis_optim"].default is None and p["use_recon_loss"].default is True


def test_cpu_tensors_reach_no_kernel():
    from hipops import ops
    for norm, sn in (("actnorm", False), ("batchnorm", True)):
        dis = _build(norm, 8, 2, sn)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dis(torch.zeros(2, 1, 32, 32))
    w = torch.zeros(4, 2, 4, 4).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spectral_norm_weight(w, torch.ones(4), torch.ones(32), True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.act_norm_lrelu(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 1, 1), torch.ones(1, 4, 1, 1))


def test_new_symbols_in_header_signatures_library_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    library.register()
    sch = str(torch.ops.vqw.actnorm_prepare.default._schema)
    for part in ("Tensor? sums", "Tensor(a!)? loc", "Tensor(b!)? scale", "Tensor(c!)? initialized", "Tensor(d!)? mean_rstd_beta"):
        assert part in sch, sch
    assert "Tensor? layers_dev" in str(torch.ops.vqw.spectral_norm_fwd.default._schema)


def test_fixture_files_stay_small():
    for f in ("gan_norms.npz", "gan_norms_act_f16.npz", "gan_norms_sn_bn_f16.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) <= 1 << 20, f
    z = np.load(os.path.join(ROOT, "tests", "golden", "gan_norms.npz"))
    assert all(z[k].dtype.kind in "fiub" for k in z.files)            # arrays only
