"""LPIPS perceptual loss, host side: the fp64 restatement (lpips_ref.py) against a plain torch rendering of the same
network (and against the lpips package where it is installed), the weight layouts, the no-download rule, the config
switches and the C ABI entries."""
import importlib.util
import json
import os
import re

import pytest
import torch

from lpips_ref import (he_weights, lpips_loss_ref, module_ref, params_of, features, distance, conv, unclear_pixels, LAYERS,
                       CHANNELS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_lpips_supported", "vqw_lpips_stem_fwd", "vqw_lpips_stem_bwd", "vqw_lpips_pool_fwd", "vqw_lpips_pool_bwd",
               "vqw_lpips_conv5_supported", "vqw_lpips_conv5_fwd", "vqw_lpips_ws_bytes", "vqw_lpips_dist_fwd",
               "vqw_lpips_loss_fold", "vqw_lpips_dist_bwd")


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1, torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (1, 3, 47, 61)])
@pytest.mark.parametrize("windowed", [False, True])
def test_restatement_matches_plain_torch_autograd(shape, windowed):
    sd = he_weights(1)
    sr, hr = _images(shape, 2)
    window = (1.3, 0.1, -0.8, 0.9) if windowed else None
    x = sr.clone().requires_grad_(True)
    loss = module_ref(sd)(x, hr, window)
    loss.backward()
    rl, rg, info = lpips_loss_ref(sr, hr, sd, window=window)
    assert info["zero_norm"] == 0
    assert abs(float(rl) - float(loss.detach())) <= 1e-10 * float(loss.detach())
    assert float((rg - x.grad).abs().max()) <= 1e-10 * float(x.grad.abs().max())


@pytest.mark.skipif(importlib.util.find_spec("lpips") is None, reason="the lpips package is not installed")
def test_restatement_matches_the_lpips_package():
    import lpips
    with torch.no_grad():
        net = lpips.LPIPS(net="alex", pretrained=False, pnet_rand=True, verbose=False).double().eval()
    for i in range(5):                       # the real lin weights are non-negative
        getattr(net, "lin%d" % i).model[1].weight.data.abs_()
    sd = {"loss_func." + k: v for k, v in net.state_dict().items()}
    sr, hr = _images((2, 3, 64, 64), 3)
    x = sr.clone().requires_grad_(True)
    loss = net(x, hr).mean()
    loss.backward()
    rl, rg, _ = lpips_loss_ref(sr, hr, sd, allow_zero_norm=True)
    assert abs(float(rl) - float(loss.detach())) <= 1e-10 * float(loss.detach())
    assert float((rg - x.grad).abs().max()) <= 1e-10 * float(x.grad.abs().max())
    from functions import LPIPSLoss
    assert sorted(k for k in LPIPSLoss(weights=sd).state_dict()) == sorted(k for k in sd if ".lins." not in k)


def test_distance_gradient_formula_matches_autograd():
    """(2 / n0) (w delta - a S / r) against autograd through the normalisation, on random features"""
    g = torch.Generator().manual_seed(4)
    fs = torch.rand(2, 64, 5, 7, generator=g, dtype=torch.float64)
    fh = torch.rand(2, 64, 5, 7, generator=g, dtype=torch.float64)
    w = torch.rand(64, generator=g, dtype=torch.float64)
    x = fs.clone().requires_grad_(True)
    a = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    b = fh / (fh.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = (w.view(1, -1, 1, 1) * (a - b) ** 2).sum(1).mean((1, 2))
    d.sum().backward()
    rd, rg, zeros, rmin = distance(fs, fh, w)
    assert zeros == 0 and rmin > 1
    assert torch.allclose(rd, d.detach(), rtol=1e-13, atol=0)
    assert float((rg - x.grad).abs().max()) <= 1e-13 * float(x.grad.abs().max())


def test_zero_norm_pixels_give_a_finite_gradient():
    sd = he_weights(5, bias0=-50.0)
    sr, hr = _images((1, 1, 40, 40), 6)
    rl, rg, info = lpips_loss_ref(sr, hr, sd, allow_zero_norm=True)
    assert info["zero_norm"] > 0 and bool(torch.isfinite(rg).all()) and bool(torch.isfinite(rl))
    # autograd meets inf * 0 = NaN at sqrt(0) there; the tap's ReLU backward (a select on f > 0) then discards it, so the
    # plain rendering ends finite too and must agree with the convention
    x = sr.clone().requires_grad_(True)
    module_ref(sd)(x, hr).backward()
    assert bool(torch.isfinite(x.grad).all())
    assert float((rg - x.grad).abs().max()) <= 1e-10 * float(x.grad.abs().max())
    f = torch.zeros(1, 64, 3, 3, dtype=torch.float64, requires_grad=True)      # without a ReLU behind it the NaN shows
    (f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)).sum().backward()
    assert bool(torch.isnan(f.grad).all())
    assert float(distance(f.detach(), torch.rand(1, 64, 3, 3, dtype=torch.float64), torch.ones(64, dtype=torch.float64))[1].abs().max()) == 0
    with pytest.raises(AssertionError):
        lpips_loss_ref(sr, hr, sd)


def test_folded_stem_equals_expanded_input():
    """one input channel: the three channels' weights fold into sum_c w_c / scale_c plus a constant for in-bounds taps"""
    p = params_of(he_weights(3), "cpu")
    x, _ = _images((2, 1, 43, 39), 4)
    full = conv((x.expand(2, 3, 43, 39) - p["shift"]) / p["scale"], p["w"][0], p["b"][0], 4, 2)
    wa = (p["w"][0] / p["scale"]).sum(1, keepdim=True)
    wb = -(p["w"][0] * p["shift"] / p["scale"]).sum(1, keepdim=True)
    folded = conv(x, wa, p["b"][0], 4, 2) + conv(torch.ones_like(x), wb, None, 4, 2)
    assert torch.allclose(full, folded, rtol=1e-12, atol=1e-12)


def test_restatement_is_translation_invariant():
    """equal windows give bit-equal outputs: a constant plane gives one value everywhere away from the border"""
    p = params_of(he_weights(5), "cpu")
    x = torch.full((1, 1, 264, 264), -1.0, dtype=torch.float64)
    fs, t = features(x, p)
    for f, m in zip(fs, (1, 3, 3, 4, 5)):       # how far the zero padding reaches into each map
        inner = f[:, :, m:-m, m:-m]
        assert inner.numel() > 0 and torch.equal(inner, inner[:, :, :1, :1].expand_as(inner))
    assert int((t["gap0"][:, :, 1:-1, 1:-1] != 0).sum()) == 0


def test_unclear_windows_reach_19_and_67_pixels():
    info = dict(gap0=torch.ones(1, 2, 15, 15), top0=torch.ones(1, 2, 15, 15), gap1=torch.ones(1, 2, 7, 7), top1=torch.ones(1, 2, 7, 7))
    info["gap0"][0, 1, 3, 4] = 1e-6
    m, n = unclear_pixels(info, 128, 128)
    assert n == 1 and int(m.sum()) == 19 * 19 and bool(m[0, 0, 22, 30]) and bool(m[0, 0, 40, 48]) and not bool(m[0, 0, 21, 30])
    info["gap0"][0, 1, 3, 4] = 1.0
    info["gap1"][0, 0, 2, 0] = 1e-6
    m, n = unclear_pixels(info, 128, 128)
    assert n == 1 and int(m.sum()) == 67 * 49 and bool(m[0, 0, 14, 0]) and bool(m[0, 0, 80, 48]) and not bool(m[0, 0, 81, 0])


def _cpu_lpips(**kw):
    from functions import LPIPSLoss
    return LPIPSLoss(**kw)


def test_every_weight_layout_loads_the_same_tensors(tmp_path):
    own = he_weights(7)
    alex, lins = he_weights(7, "pair")
    alex["classifier.1.weight"] = torch.zeros(8, 8)            # the rest of torchvision's alexnet: ignored
    bare = {k[len("loss_func."):]: v for k, v in own.items()}
    bare["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    bare["scaling_layer.scale"] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    newer = dict(own)
    for i in range(5):                                          # newer versions of the package save the lin layers twice
        newer["loss_func.lins.%d.model.1.weight" % i] = own["loss_func.lin%d.model.1.weight" % i]
    ckpt = {"state_dict": {"perceptual_loss." + k: v for k, v in newer.items()}, "epoch": 3}
    for k in ("shift", "scale"):                                # the package registers them as buffers: a checkpoint has them
        ckpt["state_dict"]["perceptual_loss.loss_func.scaling_layer." + k] = bare["scaling_layer." + k]
    ckpt["state_dict"]["encoder.x"] = torch.zeros(1)
    paths = {}
    for name, obj in (("own.pth", own), ("run.ckpt", ckpt), ("alexnet.pth", alex), ("alex.pth", lins)):
        torch.save(obj, str(tmp_path / name))
        paths[name] = str(tmp_path / name)
    mods = [_cpu_lpips(weights=w) for w in (own, bare, newer, ckpt, (alex, lins), [paths["alexnet.pth"], paths["alex.pth"]],
                                            paths["own.pth"], paths["run.ckpt"])]
    ref = mods[0].state_dict()
    expect = ["loss_func.net.slice%d.%d.%s" % (s, idx, k) for s, idx, *_ in LAYERS for k in ("weight", "bias")]
    expect += ["loss_func.lin%d.model.1.weight" % i for i in range(5)]
    expect += ["loss_func.scaling_layer.shift", "loss_func.scaling_layer.scale"]
    assert sorted(ref) == sorted(expect)
    assert [tuple(ref["loss_func.lin%d.model.1.weight" % i].shape) for i in range(5)] == [(1, c, 1, 1) for c in CHANNELS]
    for m in mods:
        sd = m.state_dict()
        assert all(torch.equal(sd[k], ref[k]) for k in ref)
        assert not any(p.requires_grad for p in m.parameters()) and not m.training
    assert torch.equal(ref["loss_func.net.slice2.3.weight"], alex["features.3.weight"])
    # a reference checkpoint's entries load under the prefix perceptual_loss., duplicates of the lin layers included
    holder = torch.nn.Module()
    holder.perceptual_loss = _cpu_lpips(weights=he_weights(8))
    holder.load_state_dict({k: v for k, v in ckpt["state_dict"].items() if k.startswith("perceptual_loss.")}, strict=True)
    assert torch.equal(holder.perceptual_loss.state_dict()["loss_func.lin3.model.1.weight"], ref["loss_func.lin3.model.1.weight"])


def test_wrong_shape_missing_keys_and_other_backbones_raise():
    bad = he_weights(8)
    bad["loss_func.net.slice2.3.weight"] = torch.zeros(192, 32, 5, 5)
    with pytest.raises(RuntimeError):
        _cpu_lpips(weights=bad)
    missing = he_weights(8)
    del missing["loss_func.net.slice5.10.bias"]
    with pytest.raises(KeyError, match=re.escape("net.slice5.10.bias")):
        _cpu_lpips(weights=missing)
    alex, lins = he_weights(8, "pair")
    del lins["lin2.model.1.weight"]
    with pytest.raises(KeyError, match=re.escape("lin2.model.1.weight")):
        _cpu_lpips(weights=(alex, lins))
    with pytest.raises(TypeError):
        _cpu_lpips(weights=(alex,))
    for net in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError):
            _cpu_lpips(net=net, weights=he_weights(8))


def test_default_weights_name_both_hub_files_and_never_download(tmp_path, monkeypatch):
    import urllib.request

    def no_network(*a, **k):
        raise AssertionError("LPIPSLoss tried to download")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    d = os.path.join(str(tmp_path / "hub"), "checkpoints")
    a, b = os.path.join(d, "alexnet-owt-7be5be79.pth"), os.path.join(d, "alex.pth")
    with pytest.raises(FileNotFoundError) as e:
        _cpu_lpips()
    assert a in str(e.value) and b in str(e.value)
    os.makedirs(d)
    alex, lins = he_weights(9, "pair")
    torch.save(alex, a)
    with pytest.raises(FileNotFoundError):
        _cpu_lpips()                                   # one of the two is not enough
    torch.save(lins, b)
    m = _cpu_lpips()
    assert torch.equal(m.state_dict()["loss_func.net.slice1.0.weight"], alex["features.0.weight"])
    assert torch.equal(m.state_dict()["loss_func.lin4.model.1.weight"], lins["lin4.model.1.weight"])


def test_inputs_are_checked_before_any_kernel():
    m = _cpu_lpips(weights=he_weights(0))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 2, 64, 64), torch.zeros(2, 2, 64, 64))
    with pytest.raises(RuntimeError):                  # no CPU fallback
        m(torch.zeros(2, 1, 64, 64), torch.zeros(2, 1, 64, 64))


def _config(tmp_path, **loss):
    from utils import load_json
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["loss"].update(loss)
    p = tmp_path / "c.json"
    p.write_text(json.dumps(raw))
    return load_json(str(p))


def test_config_builds_lpips_loss_from_lpips_weights(tmp_path):
    from functions import LPIPSLoss
    from trainers import configure_perceptual_loss, configure_losses
    own, (alex, lins) = he_weights(11), he_weights(11, "pair")
    w, wa, wl = str(tmp_path / "lpips.pth"), str(tmp_path / "alexnet-owt-7be5be79.pth"), str(tmp_path / "alex.pth")
    torch.save(own, w)
    torch.save(alex, wa)
    torch.save(lins, wl)
    for weights in (w, [wa, wl]):
        c = _config(tmp_path, use_perceptual_loss=True, perceptual_loss_type="lpips", lpips_weights=weights)
        m = configure_perceptual_loss(c)
        assert isinstance(m, LPIPSLoss)
        assert torch.equal(m.state_dict()["loss_func.net.slice4.8.bias"], alex["features.8.bias"])
        configure_losses(c)                                   # does not raise once the weights are named


def test_config_lpips_without_lpips_weights_raises(tmp_path):
    from trainers import configure_perceptual_loss, configure_losses
    for extra in (dict(), dict(perceptual_weights="x.pth")):      # perceptual_weights is the VGG19 file's key
        c = _config(tmp_path, use_perceptual_loss=True, perceptual_loss_type="lpips", **extra)
        with pytest.raises(NotImplementedError, match="perceptual") as e:
            configure_losses(c)
        assert "lpips_weights" in str(e.value)
        with pytest.raises(NotImplementedError, match="perceptual"):
            configure_perceptual_loss(c)


def test_multi_window_without_percep_weights_raises(tmp_path):
    from utils import load_json
    from trainers import build_first_step_trainer
    w = str(tmp_path / "lpips.pth")
    torch.save(he_weights(12), w)
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["loss"].update(use_perceptual_loss=True, perceptual_loss_type="lpips", lpips_weights=w, recon_weights=[1.0, 1.0, 1.0])
    raw["dataset"] = dict(raw.get("dataset") or {}, window_width=2000, window_center=0, window_scale=2.0)
    raw["loss"].pop("percep_weights", None)
    p = tmp_path / "mw.json"
    p.write_text(json.dumps(raw))
    with pytest.raises(ValueError, match="percep_weights"):
        build_first_step_trainer(load_json(str(p)), device="cpu")


def test_map_sizes():
    from hipops import ops
    assert ops.lpips_map_sizes(256, 256) == ((63, 63), (31, 31), (15, 15), (15, 15), (15, 15))
    assert ops.lpips_map_sizes(31, 31)[2] == (1, 1) and ops.lpips_map_sizes(512, 512)[1:3] == ((63, 63), (31, 31))
    p = params_of(he_weights(0), "cpu")
    fs, _ = features(torch.zeros(1, 1, 67, 93, dtype=torch.float64), p)
    assert tuple(tuple(f.shape[2:]) for f in fs) == ops.lpips_map_sizes(67, 93)
    assert ops.LPIPS_CHANNELS == CHANNELS


def test_new_symbols_in_header_signatures_library_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.vqw_abi_version() == _lib.ABI_VERSION == 9
    protos = library.parse_header()
    for name in NEW_SYMBOLS:
        assert len(protos[name][1]) == len(_lib.SIGNATURES[name][1]), name
    library.register()
    sch = str(torch.ops.vqw.lpips_stem_bwd.default._schema)
    for part in ("Tensor? sr", "Tensor? wp", "Tensor? win", "Tensor? g2", "Tensor? dz1", "Tensor(a!)? gsr"):
        assert part in sch, (part, sch)
    sch = str(torch.ops.vqw.lpips_dist_bwd.default._schema)
    for part in ("Tensor? f", "Tensor? lw", "Tensor? gin", "Tensor(a!)? gout"):
        assert part in sch, (part, sch)
    assert lib.vqw_lpips_supported(4, 1, 31, 31) == 1 and lib.vqw_lpips_supported(4, 3, 67, 93) == 1
    assert lib.vqw_lpips_supported(4, 2, 64, 64) == 0 and lib.vqw_lpips_supported(4, 1, 30, 64) == 0
    assert lib.vqw_lpips_supported(4, 1, 64, 30) == 0
    assert lib.vqw_lpips_conv5_supported(64, 192, 128, 31, 31) == 1 and lib.vqw_lpips_conv5_supported(3, 192, 1, 31, 31) == 0
    assert lib.vqw_lpips_ws_bytes(8, 3) >= 3 * lib.vqw_lpips_ws_bytes(8, 1)
    # argument validation before any device work
    assert lib.vqw_lpips_stem_fwd(None, None, None, None, None, None, None, None, 1, 1, 1, 64, 64, None) != 0
    assert b"vqw_lpips_stem_fwd" in lib.vqw_last_error()
    assert lib.vqw_lpips_dist_fwd(None, None, None, 0, 0, 1, 1, 9, 64, None) != 0
    assert lib.vqw_lpips_pool_bwd(None, None, None, 1, 8, 8, 64, None) != 0
