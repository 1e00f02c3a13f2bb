"""Host-side tests (no GPU) of the U-Net discriminator and its second training step: the float64 restatement
tests/unet_dis_ref.py against the reference's fixtures (tests/golden/unet_dis_ch4*.npz), the module and checkpoint contract on
the CPU, trainers.config for model.dis.model_name 'UNetDiscriminator', the CutMix draws, the logged row, and the C ABI."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import unet_dis_ref as U
from test_gan_norms_host import _close, _config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_unet_dtail_fwd", "vqw_unet_dtail_bwd", "vqw_unet_utail_fwd", "vqw_unet_utail_bwd", "vqw_unet_head_fwd",
               "vqw_unet_head_bwd", "vqw_cutmix_select", "vqw_unet_dis_losses_ws_bytes", "vqw_unet_dis_losses_fwd",
               "vqw_unet_dis_losses_bwd")
UNET_KEYS = dict(model_name="UNetDiscriminator", D_ch=4, D_wide=True, D_attn="0", resolution=512)


def _build(**kw):
    from networks import UNetDiscriminator
    args = dict(in_channels=1, D_ch=4, D_wide=True, D_attn="0", resolution=512, unconditional=True)
    args.update(kw)
    return UNetDiscriminator(**args)


def test_float64_restatement_reproduces_fixture(golden):
    g, gg = golden("unet_dis_ch4.npz"), golden("unet_dis_ch4_grads.npz")
    st = {}
    for k, v in g.group("mod").items():
        if k.startswith("P."):
            v = v.double()
            st[k[2:]] = v.requires_grad_(True) if k.endswith((".weight", ".bias")) else v
    before = {k: v.detach().clone() for k, v in st.items()}
    x = g.t("mod/in.0").double()
    with torch.no_grad():                                  # eval mode first: nothing is stored
        oe, be, _ = U.unet_discriminator_ref(x, st, training=False)
    sp = {k: float(g["mod/spread." + k]) for k in ("out", "bottleneck", "feat", "gin", "gP", "after")}
    _close(U.subset(oe), g["eval/out.0"], sp["out"], "eval out")
    _close(be, g["eval/bottleneck"], sp["bottleneck"], "eval bottleneck")
    for k, v in st.items():
        assert torch.equal(v, before[k]), "eval forward changed " + k
    x.requires_grad_(True)
    out, bottle, feats = U.unet_discriminator_ref(x, st, training=True)
    sum((o * U.weight_pattern(o.shape)).sum() for o in [out, bottle] + feats).backward()
    _close(U.subset(out), g["mod/out.0"], sp["out"], "out")
    _close(bottle, g["mod/bottleneck"], sp["bottleneck"], "bottleneck")
    for i, f in enumerate(feats):
        _close(U.subset(f), g["mod/feat.%d" % i], sp["feat"], "feat.%d" % i)
    _close(U.subset(x.grad), g["mod/gin.0"], sp["gin"], "gin")
    n = 0
    for k in gg.files:
        _close(st[k[len("mod/gP."):]].grad, gg[k], sp["gP"], k)
        n += 1
    assert n == 2 * 43 + 2 and st["linear.weight"].grad is None and st["linear.bias"].grad is None
    n = 0
    for k in g.files:
        if k.startswith("mod/after."):
            _close(st[k[len("mod/after."):]], g[k], sp["after"], k)
            n += 1
    assert n == 2 * 44
    assert torch.equal(st["linear.u0"], before["linear.u0"]) and not torch.equal(st["blocks.0.0.conv1.u0"], before["blocks.0.0.conv1.u0"])


def test_float64_restatement_reproduces_first_step_losses(golden):
    """The ten logged values of the step fixture's first step, in float64 on the CPU: encoder and decoder from the oracle
    (their weights regenerated from the fixture's seed and checked against its checksums), the discriminator, its spectral
    norm (u0 advances in each of the five forwards) and the losses from the restatement.  No optimiser is involved: the
    decoder's step does not touch the reconstruction the discriminator half detaches, and the discriminator has not stepped
    yet.  Bound: 2 x the fixture's fp32-against-fp64 spread of the largest value, as for the discriminator-update fixture."""
    from helpers import build_models, check_init
    from oracle import vqwnet_ref as O
    g = golden("unet_dis_step.npz")
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
    st = {k[2:]: v.double() for k, v in g.group("step").items() if k.startswith("P.")}
    image = g.t("step/image0").double()
    w = {k: float(g["step/cfg/w." + k]) for k in ("recon", "gen", "unet_perceptual", "dis", "cutmix", "consistency")}
    y0, y1, x0, x1 = (int(v) for v in g["step/box0"])
    box, flip = ((y0, y1), (x0, x1)), bool(int(g["step/flip0"]))
    with torch.no_grad():
        embed = O.encoder_forward(PE, image, False, float(cfg["momentum"]))[0]
        recon = O.decoder_forward(PD, embed, True)
        v = {"recon": torch.nn.functional.mse_loss(recon, image)}
        f_map, f_bottle, f_feat = U.unet_discriminator_ref(recon, st, True)
        v["gen"] = U.gen_loss_ref(f_map, f_bottle)
        v["unet_perceptual"] = U.unet_perceptual_ref(f_feat, U.unet_discriminator_ref(image, st, True)[2])
        v["gen_total"] = w["recon"] * v["recon"] + w["gen"] * v["gen"] + w["unet_perceptual"] * v["unet_perceptual"]
        r_map, r_bottle, _ = U.unet_discriminator_ref(image, st, True)
        f_map, f_bottle, _ = U.unet_discriminator_ref(recon, st, True)
        c_map, c_bottle, _ = U.unet_discriminator_ref(U.cutmix_images_ref(image, recon, box, flip), st, True)
        v["dis"], v["cutmix"], v["consistency"] = U.dis_losses_ref(r_map, f_map, c_map, r_bottle, f_bottle, c_bottle, box, flip)
        v["dis_total"] = w["dis"] * v["dis"] + w["cutmix"] * v["cutmix"] + w["consistency"] * v["consistency"]
    got = torch.stack([v[k].double() if k in v else torch.zeros((), dtype=torch.float64) for k in U.LOSS_NAMES])
    _close(got, g["step/loss0"], float(g["step/spread.loss"]), "step 0 losses " + str(U.LOSS_NAMES))


def test_state_dict_keys_order_and_parameter_count(golden):
    g = golden("unet_dis_ch4.npz")
    ref_keys = [k[len("mod/P."):] for k in g.files if k.startswith("mod/P.")]
    dis = _build()
    assert list(dis.state_dict()) == ref_keys and len(ref_keys) == 178
    assert sum(p.numel() for p in dis.parameters()) == 222295
    assert sum(p.numel() for p in _build(D_ch=8).parameters()) == 887051
    for k, v in dis.state_dict().items():
        assert tuple(v.shape) == tuple(g["mod/P." + k].shape), k
    w = dis.blocks[3][0].conv1.weight
    assert w.is_contiguous(memory_format=torch.channels_last) and tuple(dis.blocks[0][0].conv1.u0.shape) == (1, 4)
    assert ref_keys[:4] == ["blocks.0.0.conv1.weight", "blocks.0.0.conv1.bias", "blocks.0.0.conv1.u0", "blocks.0.0.conv1.sv0"]
    assert ref_keys[-10:-8] == ["blocks.14.weight", "blocks.14.bias"] and ref_keys[-4:] == ["linear_middle." + s for s in ("weight", "bias", "u0", "sv0")]
    narrow = _build(D_wide=False)                           # only the hidden width of the down blocks changes
    assert narrow.blocks[1][0].conv1.weight.shape == (4, 4, 3, 3) and dis.blocks[1][0].conv1.weight.shape == (8, 4, 3, 3)
    assert list(narrow.state_dict()) == ref_keys
    # orthogonal initialisation: a conv weight's rows (or columns) are orthonormal
    m = dis.blocks[2][0].conv2.weight.detach().reshape(16, -1)
    assert torch.allclose(m @ m.t(), torch.eye(16), atol=1e-5)


def test_constructor_refuses_what_is_not_built():
    for res in (128, 256):
        with pytest.raises(NotImplementedError, match=r"UNetDiscriminator.*only the 512 arch runs in the reference"):
            _build(resolution=res)
    for attn in ("64", "0_16", "256"):
        with pytest.raises(NotImplementedError, match="Attention"):
            _build(D_attn=attn)
    _build(D_attn="8")                                      # no block of the 512 arch below index 5 has resolution 8
    with pytest.raises(NotImplementedError):
        _build(unconditional=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _build()(torch.zeros(1, 1, 512, 512))


def test_checkpoint_round_trip_is_strict(tmp_path, golden):
    from trainers import configure_models
    from utils.checkpoint import save_lightning_style_ckpt, load_discriminator_from_ckpt
    c = _config(tmp_path, dis=dict(UNET_KEYS))
    enc, dec = configure_models(c)
    torch.manual_seed(5)
    dis = _build()
    path = str(tmp_path / "d.ckpt")
    save_lightning_style_ckpt(path, enc, dec, dis)
    torch.manual_seed(6)
    other = _build()
    assert not torch.equal(other.blocks[0][0].conv1.u0, dis.blocks[0][0].conv1.u0)
    load_discriminator_from_ckpt(path, other)
    for (k, v), (_, v2) in zip(dis.state_dict().items(), other.state_dict().items()):
        assert torch.equal(v, v2), k
    assert other.blocks[5][0].conv2.weight.is_contiguous(memory_format=torch.channels_last)
    # a reference checkpoint's plain contiguous tensors load too; a missing key does not
    ref = {k[2:]: v for k, v in golden("unet_dis_ch4.npz").group("mod").items() if k.startswith("P.")}
    other.load_state_dict(ref, strict=True)
    assert torch.equal(other.blocks[5][0].conv2.weight, ref["blocks.5.0.conv2.weight"])
    assert other.blocks[5][0].conv2.weight.is_contiguous(memory_format=torch.channels_last)
    sd = dis.state_dict()
    del sd["linear.sv0"]
    with pytest.raises(RuntimeError, match="linear.sv0"):
        other.load_state_dict(sd, strict=True)


def test_config_builds_the_network_and_the_trainer(tmp_path):
    from networks import UNetDiscriminator
    from trainers import (build_second_step_trainer, configure_discriminator, unet_gan_loss_weights, UNetSecondStepTrainer,
                          UNetGanLossWeights)
    assert UNetGanLossWeights._fields == ("recon", "gen", "dis", "freq", "perceptual", "unet_perceptual", "cutmix", "consistency")
    loss = dict(use_unet_perceptual_loss=True, n_inner_loops=2,
                loss_weight=dict(recon=2.0, gen=0.5, dis=1.5, unet_perceptual=0.25, cutmix=0.75, consistency=3.0))
    c = _config(tmp_path, dis=dict(UNET_KEYS), loss=loss)
    d = configure_discriminator(c)
    assert isinstance(d, UNetDiscriminator) and d.ch == 4 and d.resolution == 512
    assert unet_gan_loss_weights(c) == UNetGanLossWeights(recon=2.0, gen=0.5, dis=1.5, freq=0.0, perceptual=0.0, unet_perceptual=0.25,
                                                          cutmix=0.75, consistency=3.0)
    tr = build_second_step_trainer(c, device="cpu")
    assert isinstance(tr, UNetSecondStepTrainer) and tr.use_unet_perceptual_loss and tr.n_inner_loops == 2
    assert set(tr.modules()) == {"encoder", "decoder", "dis"} and set(tr.optimizers()) == {"dec", "dis"}
    assert len(tr.dis_optim.param_groups[0]["params"]) == len(list(tr.dis.parameters()))
    assert all(hasattr(tr, n) for n in ("state_dict", "load_state_dict", "test_step", "throttle"))
    assert build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS)), device="cpu").use_unet_perceptual_loss is False
    for missing in ("D_ch", "D_wide", "D_attn", "resolution"):
        keys = {k: v for k, v in UNET_KEYS.items() if k != missing}
        with pytest.raises(NotImplementedError, match="UNetDiscriminator"):
            configure_discriminator(_config(tmp_path, dis=keys))
    with pytest.raises(NotImplementedError, match="UNetDiscriminator"):
        build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS, resolution=256)), device="cpu")
    with pytest.raises(NotImplementedError, match="Attention"):
        build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS, D_attn="64")), device="cpu")
    with pytest.raises(NotImplementedError, match="use_l1_loss"):
        build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS), loss=dict(use_l1_loss=True)), device="cpu")
    with pytest.raises(TypeError):
        from networks import NLayerDiscriminator
        UNetSecondStepTrainer(tr.encoder, tr.decoder, NLayerDiscriminator(), device="cpu")


def test_data_parallel_reducer_leaves_out_the_unused_linear(tmp_path, monkeypatch):
    import trainers.data_parallel as DP
    from trainers import build_second_step_trainer
    seen = []
    monkeypatch.setattr(DP, "GradientAllReducer", lambda params, **kw: seen.append(list(params)) or object())
    tr = build_second_step_trainer(_config(tmp_path, dis=dict(UNET_KEYS)), device="cpu", data_parallel=True)
    unused = {id(p) for p in tr.dis.linear.parameters()}
    assert len(seen) == 2 and not any(id(p) in unused for p in seen[1])
    assert len(seen[1]) == len(list(tr.dis.parameters())) - 2


def test_committed_config_builds(tmp_path):
    from utils import load_json
    from trainers import build_second_step_trainer, UNetSecondStepTrainer
    path = os.path.join(ROOT, "configs", "second_step_unet_512.json")
    raw = json.load(open(path))
    assert raw["model"]["dis"]["model_name"] == "UNetDiscriminator" and raw["model"]["dis"]["normalization"] == "batchnorm"
    assert raw["dataset"]["image_size"] == 512 and raw["run"]["training_mode"] == "second_step"
    assert "second_step_unet_512.json" in open(os.path.join(ROOT, "configs", "README.md")).read()
    tr = build_second_step_trainer(load_json(path), device="cpu")
    assert isinstance(tr, UNetSecondStepTrainer) and tr.use_unet_perceptual_loss
    assert tuple(tr.w) == tuple(float(raw["loss"]["loss_weight"][k]) for k in type(tr.w)._fields)


def test_cutmix_draws(golden):
    """The restatement and the trainer's draw_cutmix_box reproduce the reference's rectangles under a fixed numpy seed, and
    the trainer draws rectangle then flip, from numpy then `random`, once per inner loop."""
    from trainers import draw_cutmix_box
    from trainers.second_step_unet import UNetSecondStepTrainer
    g = golden("unet_dis_ch4.npz")
    boxes = g["draws/boxes"]
    for fn in (U.cutmix_box_ref, draw_cutmix_box):
        np.random.seed(int(g["draws/seed"]))
        got = [fn(512, 512) for _ in range(len(boxes))]
        assert [[y0, y1, x0, x1] for (y0, y1), (x0, x1) in got] == boxes.tolist()
    assert all(0 <= y0 <= y1 <= 512 and 0 <= x0 <= x1 <= 512 for y0, y1, x0, x1 in boxes.tolist())
    tr = object.__new__(UNetSecondStepTrainer)
    tr.cutmix_box = None
    np.random.seed(int(g["draws/seed"]))
    random.seed(9)
    (box, flip), (box2, _) = tr._draw_box(512, 512), tr._draw_box(512, 512)
    random.seed(9)
    assert [list(box[0]) + list(box[1]), list(box2[0]) + list(box2[1])] == boxes[:2].tolist() and flip == (random.random() > 0.5)
    tr.cutmix_box = (((1, 2), (3, 4)), True)
    assert tr._draw_box(512, 512) == (((1, 2), (3, 4)), True)
    tr.cutmix_box = lambda: (((0, 0), (0, 0)), False)
    assert tr._draw_box(512, 512) == (((0, 0), (0, 0)), False)


def test_losses_restatement_matches_the_reference_formulas():
    """dis_losses_ref against the formulas of single_window_trainer.py:324-349 written out with an explicit mask tensor."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    r, f, c = (torch.randn(2, 1, 12, 20, generator=g, dtype=torch.float64) for _ in range(3))
    rb, fb, cb = (torch.randn(2, 1, generator=g, dtype=torch.float64) for _ in range(3))
    for flip in (False, True):
        mask = torch.ones_like(r)
        mask[:, :, 3:8, 5:15] = 0
        if flip:
            mask = 1 - mask
        l_dis = 0.5 * (F.relu(1 - r).mean() + F.relu(1 + f).mean()) + 0.5 * (F.relu(1 - rb).mean() + F.relu(1 + fb).mean())
        l_cut = F.relu(1 + cb).mean() + F.relu(1 - (mask * 2 - 1) * c).mean()
        l_con = F.mse_loss(c, r * mask + (1 - mask) * f)
        got = U.dis_losses_ref(r, f, c, rb, fb, cb, ((3, 8), (5, 15)), flip)
        for a, b in zip(got, (l_dis, l_cut, l_con)):
            assert abs(float(a) - float(b)) <= 1e-14
        assert torch.equal(U.cutmix_images_ref(r, f, ((3, 8), (5, 15)), flip), r * mask + (1 - mask) * f)


def test_logged_row_uses_the_reference_names():
    from trainers.fit import _second_step_row, _second_step_terms
    from trainers import UNetGanLossWeights, GanLossWeights
    w = UNetGanLossWeights(recon=2.0, gen=0.5, dis=1.5, freq=0.0, perceptual=0.0, unet_perceptual=0.25, cutmix=0.75, consistency=3.0)
    v = dict(gen_total=1.0, recon=0.5, gen=2.0, unet_perceptual=4.0, dis_total=3.0, dis=1.0, cutmix=2.0, consistency=0.5)
    row = _second_step_row(v, w)
    assert list(row) == ["total", "gen_total", "recon", "freq", "perceptual", "gen", "unet_perceptual", "dis_total", "dis", "cutmix",
                         "consistency"]
    assert (row["total"], row["recon"], row["gen"], row["unet_perceptual"], row["dis"], row["cutmix"], row["consistency"]) == \
        (4.0, 1.0, 1.0, 1.0, 1.5, 1.5, 1.5)
    assert [n for n, _ in _second_step_terms(dict(v, ids=None))] == ["gen_total", "dis_total", "recon", "gen", "unet_perceptual", "dis",
                                                                     "cutmix", "consistency"]
    # a PatchGAN run's row and terms are what they were
    pv = dict(gen_total=1.0, recon=0.5, gen=2.0, dis_total=3.0)
    assert _second_step_row(pv, GanLossWeights()) == {"total": 4.0, "gen_total": 1.0, "recon": 0.5, "freq": 0.0, "perceptual": 0.0,
                                                      "gen": 2.0, "dis_total": 3.0, "dis": 3.0}
    assert [n for n, _ in _second_step_terms(pv)] == ["gen_total", "dis_total", "recon", "gen"]


def test_new_symbols_in_header_signatures_library_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.vqw_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    library.register()
    sch = str(torch.ops.vqw.unet_dtail_fwd.default._schema)
    for part in ("Tensor? a", "Tensor? s_low", "Tensor(a!)? out", "Tensor(b!)? relu_out", "int C"):
        assert part in sch, sch
    sch = str(torch.ops.vqw.unet_dis_losses_bwd.default._schema)
    assert "Tensor? g_consistency" in sch and "Tensor(a!)? g_r_map" in sch and "Tensor(f!)? g_c_bottle" in sch and "int flip" in sch
    assert not hasattr(torch.ops.vqw, "unet_dis_losses_ws_bytes") or "unet_dis_losses_ws_bytes" not in library.SCHEMAS
    assert lib.vqw_unet_dis_losses_ws_bytes(1) == 32 and lib.vqw_unet_dis_losses_ws_bytes(10 ** 7) == 256 * 32


def test_operators_refuse_cpu_tensors():
    from hipops import ops
    z = torch.zeros(1, 4, 4, 4)
    for call in (lambda: ops.unet_down_tail(z), lambda: ops.unet_up_tail(z, torch.zeros(1, 4, 2, 2)),
                 lambda: ops.unet_bottleneck_head(z, torch.zeros(1, 4)), lambda: ops.cutmix_select(z, z, ((0, 1), (0, 1)), False),
                 lambda: ops.spectral_norm_weights([torch.zeros(1, 4)], [torch.ones(1, 1)], None, True, svs=[torch.ones(1)], biggan=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_fixture_files_stay_small():
    for f in ("unet_dis_ch4.npz", "unet_dis_ch4_grads.npz", "unet_dis_step.npz", "unet_dis_step_after.npz", "unet_dis_step_dec.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) <= 1 << 20, f
