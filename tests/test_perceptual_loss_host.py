"""VGG perceptual loss, host side: the fp64 restatement (vgg_ref.py) against the reference's module stack, the weight
layouts, the no-download rule, the config switches and the C ABI entries."""
import json
import os
import re

import pytest
import torch

from vgg_ref import he_weights, vgg_loss_ref, features, sequential_ref, _sd64, conv3x3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_percep_supported", "vqw_percep_stem_fwd", "vqw_percep_diff", "vqw_percep_loss_ws_bytes",
               "vqw_percep_loss_fwd", "vqw_percep_stem_bwd")


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1, torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


@pytest.mark.parametrize("shape", [(2, 1, 12, 10), (1, 1, 9, 7), (2, 3, 8, 8)])
def test_restatement_matches_plain_sequential(shape):
    sd = _sd64(he_weights(1), "cpu")
    sr, hr = _images(shape, 2)
    seq = sequential_ref(sd)
    x = sr.clone().requires_grad_(True)
    ys = seq(x.expand(shape[0], 3, shape[2], shape[3]))
    with torch.no_grad():
        yh = seq(hr.expand(shape[0], 3, shape[2], shape[3]))
    loss = torch.nn.functional.mse_loss(ys, yh)
    loss.backward()
    rl, rg, _ = vgg_loss_ref(sr, hr, sd)
    assert abs(float(rl) - float(loss.detach())) <= 1e-12 * float(loss.detach())
    assert float((rg - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert torch.allclose(features(sr, sd), ys.detach(), rtol=1e-12, atol=1e-12)
    assert float(features(sr, sd).min()) < 0          # the output is taken before conv2_2's ReLU


def test_folded_stem_equals_expanded_input():
    sd = _sd64(he_weights(3), "cpu")
    x, _ = _images((2, 1, 10, 10), 4)
    full = conv3x3(x.expand(2, 3, 10, 10), sd["vgg.0.weight"], sd["vgg.0.bias"])
    folded = conv3x3(x, sd["vgg.0.weight"].sum(dim=1, keepdim=True), sd["vgg.0.bias"])
    assert torch.allclose(full, folded, rtol=1e-13, atol=1e-13)


def test_restatement_is_translation_invariant():
    """equal windows give bit-equal outputs: a constant plane gives one value everywhere away from the border"""
    sd = _sd64(he_weights(5), "cpu")
    x = torch.full((1, 1, 40, 40), -1.0, dtype=torch.float64)
    y = features(x, sd)
    inner = y[:, :, 5:-5, 5:-5]            # the receptive field reaches 5 pooled pixels: away from the zero padding
    assert torch.equal(inner, inner[:, :, :1, :1].expand_as(inner))


def _cpu_vgg(**kw):
    from functions import VGGLoss
    return VGGLoss(**kw)


def test_three_weight_layouts_load_the_same_tensors(tmp_path):
    tv = he_weights(7, "torchvision")
    tv["features.10.weight"] = torch.zeros(256, 128, 3, 3)    # deeper layers of the full vgg19: ignored
    own = he_weights(7, "vgg")
    ckpt = {"state_dict": {"perceptual_loss." + k: v for k, v in own.items()}, "epoch": 3}
    ckpt["state_dict"]["encoder.x"] = torch.zeros(1)
    paths = []
    for name, obj in (("tv.pth", tv), ("own.pth", own), ("run.ckpt", ckpt)):
        torch.save(obj, str(tmp_path / name))
        paths.append(str(tmp_path / name))
    mods = [_cpu_vgg(weights=w) for w in (tv, own, ckpt)] + [_cpu_vgg(weights=p) for p in paths]
    ref = mods[0].state_dict()
    assert sorted(ref) == sorted("vgg.%d.%s" % (i, k) for i in (0, 2, 5, 7) for k in ("weight", "bias"))
    for m in mods:
        sd = m.state_dict()
        assert all(torch.equal(sd[k], ref[k]) for k in ref)
        assert not any(p.requires_grad for p in m.parameters())
    from utils.checkpoint import perceptual_state_from_ckpt
    sd = perceptual_state_from_ckpt(paths[2])
    assert sorted(sd) == sorted(ref) and all(torch.equal(sd[k], ref[k]) for k in ref)


def test_wrong_shape_and_missing_layer_raise():
    bad = he_weights(8, "vgg")
    bad["vgg.5.weight"] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(RuntimeError):
        _cpu_vgg(weights=bad)
    missing = he_weights(8, "vgg")
    del missing["vgg.7.bias"]
    with pytest.raises(KeyError):
        _cpu_vgg(weights=missing)


def test_default_weights_name_the_hub_file_and_never_download(tmp_path, monkeypatch):
    import urllib.request

    def no_network(*a, **k):
        raise AssertionError("VGGLoss tried to download")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    expect = os.path.join(str(tmp_path / "hub"), "checkpoints", "vgg19-dcbb9e9d.pth")
    with pytest.raises(FileNotFoundError, match=re.escape(expect)):
        _cpu_vgg()
    os.makedirs(os.path.dirname(expect))
    torch.save(he_weights(9, "torchvision"), expect)
    m = _cpu_vgg()
    assert torch.equal(m.state_dict()["vgg.0.weight"], he_weights(9, "torchvision")["features.0.weight"])


def test_other_slices_raise():
    with pytest.raises(NotImplementedError):
        _cpu_vgg(conv_index='54', weights=he_weights(0, "vgg"))


def _config(tmp_path, **loss):
    from utils import load_json
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["loss"].update(loss)
    p = tmp_path / "c.json"
    p.write_text(json.dumps(raw))
    return load_json(str(p))


def test_config_builds_vgg_loss_from_perceptual_weights(tmp_path):
    from functions import VGGLoss
    from trainers import configure_perceptual_loss, configure_losses
    w = str(tmp_path / "vgg19.pth")
    torch.save(he_weights(11, "torchvision"), w)
    assert configure_perceptual_loss(_config(tmp_path)) is None
    c = _config(tmp_path, use_perceptual_loss=True, perceptual_loss_type="vgg", perceptual_weights=w)
    m = configure_perceptual_loss(c)
    assert isinstance(m, VGGLoss)
    assert torch.equal(m.state_dict()["vgg.7.bias"], he_weights(11, "torchvision")["features.7.bias"])
    configure_losses(c)                                   # no longer raises once the weights are named


@pytest.mark.parametrize("extra", [dict(), dict(perceptual_loss_type="lpips", perceptual_weights="x.pth"),
                                   dict(conv_index="54", perceptual_weights="x.pth")])
def test_config_unbuilt_perceptual_settings_raise(tmp_path, extra):
    from trainers import configure_perceptual_loss, configure_losses
    c = _config(tmp_path, use_perceptual_loss=True, **extra)
    with pytest.raises(NotImplementedError, match="perceptual"):
        configure_losses(c)
    with pytest.raises(NotImplementedError, match="perceptual"):
        configure_perceptual_loss(c)


def test_multi_window_without_percep_weights_raises(tmp_path):
    from utils import load_json
    from trainers import build_first_step_trainer
    w = str(tmp_path / "vgg19.pth")
    torch.save(he_weights(12, "torchvision"), w)
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["loss"].update(use_perceptual_loss=True, perceptual_weights=w, recon_weights=[1.0, 1.0, 1.0])
    raw["dataset"] = dict(raw.get("dataset") or {}, window_width=2000, window_center=0, window_scale=2.0)
    raw["loss"].pop("percep_weights", None)
    p = tmp_path / "mw.json"
    p.write_text(json.dumps(raw))
    with pytest.raises(ValueError, match="percep_weights"):
        build_first_step_trainer(load_json(str(p)), device="cpu")


def test_trainer_weight_fields():
    from trainers import GanLossWeights, LossWeights
    assert GanLossWeights(2.0, 3.0, 4.0, 5.0).perceptual == 0.0 and GanLossWeights._fields[-1] == "perceptual"
    assert LossWeights().perceptual == 0.0


def test_new_symbols_in_header_signatures_library_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.vqw_abi_version() == _lib.ABI_VERSION
    protos = library.parse_header()
    for name in NEW_SYMBOLS:
        assert len(protos[name][1]) == len(_lib.SIGNATURES[name][1]), name
    library.register()
    sch = str(torch.ops.vqw.percep_stem_bwd.default._schema)
    for part in ("Tensor? sr", "Tensor? win", "Tensor? g2", "Tensor? dz1", "Tensor(a!)? gsr"):
        assert part in sch, (part, sch)
    assert lib.vqw_percep_supported(4, 1, 33, 47) == 1 and lib.vqw_percep_supported(4, 3, 8, 8) == 1
    assert lib.vqw_percep_supported(4, 2, 8, 8) == 0 and lib.vqw_percep_supported(4, 1, 1, 8) == 0
    assert lib.vqw_percep_loss_ws_bytes(3) >= 3 * lib.vqw_percep_loss_ws_bytes(1)
    # argument validation before any device work
    assert lib.vqw_percep_stem_fwd(None, None, None, None, None, None, 1, 1, 1, 8, 8, None) != 0
    assert b"vqw_percep_stem_fwd" in lib.vqw_last_error()
    assert lib.vqw_percep_loss_fwd(None, None, None, 0, 1, 8, None) != 0
