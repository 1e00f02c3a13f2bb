"""Host-side tests (no GPU) of the multi-window second training step with the U-Net discriminator: the float64 restatement
tests/unet_dis_mw_ref.py against the reference's fixture (tests/golden/unet_dis_mw_step.npz, made by
tests/golden/make_golden_unet_dis_mw.py with the reference trainers' un-clamped re-windowing), ops.window_map with and
without the clamp, trainers.config for a config with window keys, the committed config, and the C ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import unet_dis_ref as U
import unet_dis_mw_ref as MW
from test_gan_norms_host import _config, F32_EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_window_stack_fwd", "vqw_window_stack_bwd")
UNET_KEYS = dict(model_name="UNetDiscriminator", D_ch=4, D_wide=True, D_attn="0", resolution=512)
WINDOW_KEYS = dict(window_width=2000, window_center=0, window_scale=2.0)
F32_MAX = float(np.finfo(np.float32).max)


def fixture_boxes(g):
    boxes, flips = [], []
    for i in range(3):
        y0, y1, x0, x1 = (int(v) for v in g["step/box%d" % i])
        boxes.append(((y0, y1), (x0, x1)))
        flips.append(bool(int(g["step/flip%d" % i])))
    return boxes, flips


def fixture_settings(g):
    """-> (loss weights of the two totals, dataset window, recon_weights) of the step fixture"""
    w = {k: float(g["step/cfg/w." + k]) for k in ("recon", "gen", "unet_perceptual", "dis", "cutmix", "consistency")}
    width, center, scale = (float(v) for v in g["step/cfg/dataset_window"])
    return w, (int(width), int(center), scale), tuple(float(v) for v in g["step/cfg/recon_weights"])


@pytest.fixture(scope="module")
def float64_losses(golden):
    """The restatement's ten losses of the fixture step in float64, with and without the clamp: encoder and decoder from the
    oracle (their weights regenerated from the fixture's seed and checked against its checksums), computed once."""
    from helpers import build_models, check_init
    from oracle import vqwnet_ref as O
    g = golden("unet_dis_mw_step.npz")
    cfg = {k: g["step/cfg/" + k] for k in ("enc_filters", "dec_filters", "K", "momentum", "seed")}
    enc, dec = build_models(cfg)
    check_init({k[len("step/"):]: g[k] for k in g.files if k.startswith("step/init_sum/")}, enc, dec)
    K = int(cfg["K"])
    with torch.no_grad():
        enc.vq.embed.mul_(0.7)
        enc.vq.cluster_size.fill_(512 * 512 / K)
        enc.vq.embed_avg.copy_(enc.vq.embed.t() * enc.vq.cluster_size[None, :])
    PE, PD = ({k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in m.state_dict().items()}
              for m in (enc, dec))
    image = g.t("step/image").double()
    with torch.no_grad():
        recon = O.decoder_forward(PD, O.encoder_forward(PE, image, False, float(cfg["momentum"]))[0], True)
    w, dw, rw = fixture_settings(g)
    boxes, flips = fixture_boxes(g)
    out = {}
    for clamp in (False, True):
        st = {k[2:]: v.double() for k, v in g.group("step").items() if k.startswith("P.")}
        out[clamp] = MW.step_losses_ref(image, recon, st, boxes, flips, w, dw, rw, clamp)
    return out


def _bound(g):
    ref = torch.from_numpy(g["step/loss"]).double()
    return ref, (2.0 * float(g["step/spread.loss"]) + F32_EPS) * float(ref.abs().max())


def test_float64_restatement_without_clamp_reproduces_fixture(golden, float64_losses):
    """All ten values within (2 x the fixture's own fp32-against-fp64 spread + fp32 storage rounding) of the largest."""
    g = golden("unet_dis_mw_step.npz")
    ref, bound = _bound(g)
    got = float64_losses[False]
    for k, a, r in zip(U.LOSS_NAMES, got.tolist(), ref.tolist()):
        print("%-16s %.10g  reference %.10g  |diff| %.3e  (bound %.3e)" % (k, a, r, abs(a - r), bound))
    assert float((got - ref).abs().max()) <= bound
    assert float(ref[U.LOSS_NAMES.index("freq")]) == 0.0 and float(ref[U.LOSS_NAMES.index("perceptual")]) == 0.0


def test_fixture_sees_the_windows(golden, float64_losses):
    """With the clamp at least one loss leaves that bound: the fixture tells the two re-windowings apart."""
    g = golden("unet_dis_mw_step.npz")
    ref, bound = _bound(g)
    err = (float64_losses[True] - ref).abs()
    print("with clamp: " + " ".join("%s %.3e" % kv for kv in zip(U.LOSS_NAMES, err.tolist())) + "  (bound %.3e)" % bound)
    assert float(err.max()) > bound
    image = g.t("step/image").reshape(-1)
    assert bool((image * 64 == torch.round(image * 64)).all()) and float(image.abs().max()) <= 1.0
    assert float((image > 0.2).float().mean()) >= 0.05 and float(((image < -0.18) | (image > 0.22)).float().mean()) >= 0.05


def test_window_map_with_and_without_clamp():
    """clamp=False: the float64 arithmetic of denormalize followed by t_normalize (no clip), bounds at -/+ the largest
    float32; clamp=True (and the default) is what it was: the same slope and offset, bounds at -/+ scale / 2."""
    from hipops import ops
    dw = (2000, 0, 2.0)
    x = np.linspace(-1.5, 1.5, 193)
    for tw in (MW.LUNG_WINDOW, MW.MEDIASTINAL_WINDOW, (350, 40, 1.0)):
        alpha, beta, lo, hi = ops.window_map(dw, tw, clamp=False)
        assert (lo, hi) == (-F32_MAX, F32_MAX) and np.float32(hi) == np.finfo(np.float32).max and np.isfinite(np.float32(lo))
        want = MW.to_window(torch.from_numpy(x), dw, tw, clamp=False).numpy()
        assert np.abs(alpha * x + beta - want).max() <= 1e-12 * np.abs(want).max()
        clamped = ops.window_map(dw, tw, clamp=True)
        assert clamped == ops.window_map(dw, tw) == (alpha, beta, -0.5 * tw[2], 0.5 * tw[2])
        want = MW.to_window(torch.from_numpy(x), dw, tw, clamp=True).numpy()
        assert np.abs(np.clip(alpha * x + beta, clamped[2], clamped[3]) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.allclose(ops.window_map(dw, MW.LUNG_WINDOW), (4.0 / 3.0, 11.0 / 15.0, -1.0, 1.0), rtol=1e-15, atol=0)


def test_builder_picks_the_trainer(tmp_path):
    from trainers import (build_second_step_trainer, UNetSecondStepTrainer, UNetMultiWindowSecondStepTrainer, SecondStepTrainer)
    loss = dict(recon_weights=[1.0, 0.5, 0.25], use_unet_perceptual_loss=True, n_inner_loops=2)
    c = _config(tmp_path, dis=dict(UNET_KEYS), loss=loss, dataset=dict(dataset_name="synthetic", **WINDOW_KEYS))
    tr = build_second_step_trainer(c, device="cpu")
    assert type(tr) is UNetMultiWindowSecondStepTrainer and isinstance(tr, UNetSecondStepTrainer)
    assert tr.multi_window == dict(dataset_window=(2000, 0, 2.0), recon_weights=(1.0, 0.5, 0.25))
    assert tr.clamp_windows is True and tr.use_unet_perceptual_loss and tr.n_inner_loops == 2
    assert tr.windows[0] is None and tr.windows[1][2:] == (-1.0, 1.0) and tr.windows[2][2:] == (-1.0, 1.0)
    assert set(tr.modules()) == {"encoder", "decoder", "dis"} and set(tr.optimizers()) == {"dec", "dis"}
    # the launcher without -w: the single-window step whatever keys the config carries
    assert type(build_second_step_trainer(c, device="cpu", multi_window=False)) is UNetSecondStepTrainer
    # loss.clamp_windows: absent -> true; false -> the reference trainer's affine map
    c2 = _config(tmp_path, dis=dict(UNET_KEYS), loss=dict(loss, clamp_windows=False), dataset=dict(dataset_name="synthetic", **WINDOW_KEYS))
    tr2 = build_second_step_trainer(c2, device="cpu")
    assert tr2.clamp_windows is False and tr2.windows[1][2:] == (-F32_MAX, F32_MAX) and tr2.windows[1][:2] == tr.windows[1][:2]
    # an explicit dict, as build_first_step_trainer takes it
    c3 = _config(tmp_path, dis=dict(UNET_KEYS))
    tr3 = build_second_step_trainer(c3, device="cpu", multi_window=dict(dataset_window=(2000, 0, 2.0), recon_weights=(1.0, 1.0, 1.0)))
    assert type(tr3) is UNetMultiWindowSecondStepTrainer
    assert type(build_second_step_trainer(c3, device="cpu")) is UNetSecondStepTrainer
    # the PatchGAN: multi-window raises, without -w it is the PatchGAN step
    cp = _config(tmp_path, loss=dict(recon_weights=[1.0, 1.0, 1.0]), dataset=dict(dataset_name="synthetic", **WINDOW_KEYS))
    with pytest.raises(NotImplementedError, match="U-Net discriminator"):
        build_second_step_trainer(cp, device="cpu")
    assert type(build_second_step_trainer(cp, device="cpu", multi_window=False)) is SecondStepTrainer


def test_missing_window_weights_raise(tmp_path):
    from functions import FocalFrequencyLoss
    from trainers import build_second_step_trainer, UNetMultiWindowSecondStepTrainer
    ds = dict(dataset_name="synthetic", **WINDOW_KEYS)
    loss = dict(recon_weights=[1.0, 1.0, 1.0], use_frequency_loss=True)
    with pytest.raises(ValueError, match="freq_weights"):
        build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS), loss=loss, dataset=ds), device="cpu")
    tr = build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS), loss=dict(loss, freq_weights=[1.0, 0.5, 2.0]), dataset=ds),
                                   device="cpu")
    assert tr.freq_weights == (1.0, 0.5, 2.0) and tr.frequency_loss is not None
    mw = dict(dataset_window=(2000, 0, 2.0), recon_weights=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="freq_weights"):
        UNetMultiWindowSecondStepTrainer(tr.encoder, tr.decoder, tr.dis, device="cpu", multi_window=mw,
                                         frequency_loss=FocalFrequencyLoss(loss_weight=1.0, alpha=1.0))
    with pytest.raises(ValueError, match="multi_window"):
        UNetMultiWindowSecondStepTrainer(tr.encoder, tr.decoder, tr.dis, device="cpu")


def test_trainer_signature_extends_the_single_window_one():
    import inspect
    from trainers import UNetSecondStepTrainer, UNetMultiWindowSecondStepTrainer
    base = list(inspect.signature(UNetSecondStepTrainer.__init__).parameters.values())
    new = list(inspect.signature(UNetMultiWindowSecondStepTrainer.__init__).parameters.values())
    assert [(p.name, p.default) for p in new[:len(base)]] == [(p.name, p.default) for p in base]
    assert [(p.name, p.default) for p in new[len(base):]] == [("multi_window", None), ("freq_weights", None), ("percep_weights", None),
                                                             ("clamp_windows", True)]
    # one step body: the multi-window trainer overrides the hooks, not the step
    from trainers.second_step import SecondStepBase
    assert UNetMultiWindowSecondStepTrainer.training_step is SecondStepBase.training_step


def test_committed_config_builds():
    from utils import load_json
    from trainers import build_second_step_trainer, UNetMultiWindowSecondStepTrainer, UNetSecondStepTrainer
    name = "second_step_unet_512_mw.json"
    path = os.path.join(ROOT, "configs", name)
    raw, single = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "second_step_unet_512.json")))
    assert raw["model"] == single["model"] and raw["model"]["dis"]["normalization"] == "batchnorm" and not name.startswith("baseline")
    assert (raw["dataset"]["window_width"], raw["dataset"]["window_center"], raw["dataset"]["window_scale"]) == (2000, 0, 2.0)
    assert all(len(raw["loss"][k]) == 3 for k in ("recon_weights", "freq_weights", "percep_weights"))
    assert name in open(os.path.join(ROOT, "configs", "README.md")).read()
    tr = build_second_step_trainer(load_json(path), device="cpu")
    assert type(tr) is UNetMultiWindowSecondStepTrainer and tr.clamp_windows and tr.use_unet_perceptual_loss
    assert tr.multi_window["recon_weights"] == tuple(raw["loss"]["recon_weights"])
    assert type(build_second_step_trainer(load_json(path), device="cpu", multi_window=False)) is UNetSecondStepTrainer


def test_launcher_accepts_the_committed_config_with_w():
    """check_arguments: -w needs the window keys, which the committed config carries; second_step is no longer refused."""
    import inspect
    import run_vqwnet as rv
    from utils import load_json
    args = rv.build_parser().parse_args(["-c", os.path.join(ROOT, "configs", "second_step_unet_512_mw.json"), "-w"])
    assert args.multiwindow
    cfg = load_json(args.config)
    assert all(rv._lookup(cfg, k) is not None for k in rv.WINDOW_KEYS)
    src = inspect.getsource(rv.worker)
    assert "multi_window=None if args.multiwindow else False" in src and "is not built" not in src


def test_new_symbols_in_header_library_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.vqw_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    library.register()
    sch = str(torch.ops.vqw.window_stack_fwd.default._schema)
    for part in ("Tensor? x", "Tensor? win", "Tensor(a!)? o0", "Tensor(c!)? o2", "int nwin", "int n"):
        assert part in sch, sch
    sch = str(torch.ops.vqw.window_stack_bwd.default._schema)
    for part in ("Tensor? g0", "Tensor? g2", "Tensor(a!)? gx", "int nwin"):
        assert part in sch, sch


def test_window_stack_refuses_cpu_tensors_and_bad_windows():
    from hipops import ops
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.window_stack(z, (None,))
    for bad in ((), (None,) * 4, ((1.0, 0.0, -1.0),)):
        with pytest.raises(RuntimeError, match="one to three windows"):
            ops.window_stack(z, bad)


def test_fixture_files_stay_small():
    for f in ("unet_dis_mw_step.npz", "unet_dis_mw_step_after.npz", "unet_dis_mw_step_dec.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) <= 1 << 20, f
