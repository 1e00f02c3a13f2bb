"""GPU tests of the discriminator's ActNorm / spectral-norm configurations and of the config-driven second step: the HIP
path against the reference's fixtures (tests/golden/gan_norms*.npz, made by tests/golden/make_golden_dis.py) at the
tolerances the BatchNorm discriminator is held to, the spectral-norm operator alone against float64, run-to-run
bit-identity, the generator pass, trainers.build_second_step_trainer, and a one-rank process group.
Run with `pytest -m gpu` on an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close, rel_err
from gan_norm_ref import spectral_weight_ref
from test_gpu_parity import _run_block

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tag -> (fixture file, normalization, n_filters, n_layers, spectral norm, training mode)
MODULE_CASES = {
    "act_f16": ("gan_norms_act_f16.npz", "actnorm", 16, 3, False, True),
    "act_f8_eval": ("gan_norms.npz", "actnorm", 8, 2, False, False),
    "act_uninit_eval": ("gan_norms.npz", "actnorm", 8, 2, False, False),
    "sn_bn_f16": ("gan_norms_sn_bn_f16.npz", "batchnorm", 16, 3, True, True),
    "sn_act_f8": ("gan_norms.npz", "actnorm", 8, 2, True, True),
    "sn_bn_f8_eval": ("gan_norms.npz", "batchnorm", 8, 2, True, False),
}


def _build(normalization, n_filters, n_layers, spectral):
    from networks import NLayerDiscriminator
    from utils import apply_spectral_norm
    dis = NLayerDiscriminator(1, 1, n_filters=n_filters, n_layers=n_layers, normalization=normalization)
    if spectral:
        apply_spectral_norm(dis)
    return dis


def _load(dis, g, tag):
    dis.load_state_dict({k[2:]: v for k, v in g.group(tag).items() if k.startswith("P.")}, strict=True)
    return dis.to(DEV)


@pytest.mark.parametrize("tag", sorted(MODULE_CASES))
def test_discriminator_norms_golden(golden, tag):
    """Outputs, input / parameter gradients and the state after (BatchNorm buffers, loc / scale / initialized, u / v) against
    the reference module, at _run_block's default tolerances (1e-4 forward, 1e-3 gradients, 1e-5 state)."""
    from networks.actnorm import ActNorm
    file, norm, nf, nl, sn, train = MODULE_CASES[tag]
    dis = _build(norm, nf, nl, sn)
    g = golden(file)
    n_after = len([k for k in g.files if k.startswith(tag + "/after.")])
    assert n_after > 0
    _run_block(golden, tag, dis, 1, train=train, file=file)
    acts = [m for m in dis.modules() if isinstance(m, ActNorm)]
    if tag == "act_uninit_eval":                               # eval mode never initialises
        assert acts and all(int(m.initialized) == 0 and not m._host_initialized for m in acts)
        assert all(float(m.loc.detach().abs().max()) == 0.0 and float((m.scale.detach() - 1).abs().max()) == 0.0 for m in acts)
    elif acts:
        assert all(int(m.initialized) == 1 and m._host_initialized for m in acts)
    if tag == "sn_bn_f8_eval":                                 # eval mode: u, v unchanged, bit for bit
        for k, v in dis.state_dict().items():
            if k.endswith(("weight_u", "weight_v")):
                assert torch.equal(v.cpu(), g.t("%s/P.%s" % (tag, k))), k


def test_discriminator_update_golden_spectral_actnorm(golden):
    """Two discriminator updates (hinge on real / fake, Adam) with ActNorm and spectral norm against the reference run, as
    test_gpu_parity.test_discriminator_update_golden does it and at its tolerances; the first forward initialises the ActNorm
    layers, u / v advance in each of the four forwards."""
    from functions import hinge_d_loss
    from hipops import Adam, ops
    g = golden("gan_norms.npz")
    tag = "dstep_sn_act"
    dis = _load(_build("actnorm", 8, 3, True), g, tag).train()
    opt = Adam(dis.parameters(), lr=1e-3, betas=(0.5, 0.999))
    for s in range(2):
        l_dis = hinge_d_loss(dis(g.t("%s/real%d" % (tag, s), DEV)), dis(g.t("%s/fake%d" % (tag, s), DEV)))
        print("l_dis step %d: rel err %.3e" % (s, rel_err(l_dis, g["%s/loss%d" % (tag, s)])))
        assert_close(l_dis, g["%s/loss%d" % (tag, s)], 2e-4 if s else 1e-5, "l_dis step %d" % s)
        opt.zero_grad()
        ops.weighted_sum([l_dis], [0.8]).backward()
        opt.step()
    torch.cuda.synchronize()
    for k, v in dis.state_dict().items():
        ref = g["%s/after.%s" % (tag, k)]
        if k.endswith("initialized"):
            assert int(v) == int(ref) == 1
        else:
            print("after.%s: rel err %.3e" % (k, rel_err(v.float(), ref.astype(np.float32))))
            assert_close(v.float(), ref.astype(np.float32), 2e-3, "after." + k, atol=2e-4)


def test_generator_pass_golden(golden):
    """The generator pass: the discriminator's parameters have requires_grad=False, training mode.  Output and input
    gradient against the reference; no parameter receives a gradient; u, v still advance."""
    g = golden("gan_norms.npz")
    tag = "gen_pass_sn"
    dis = _load(_build("batchnorm", 8, 2, True), g, tag).train()
    for p in dis.parameters():
        p.requires_grad_(False)
    x = g.t(tag + "/in.0", DEV).requires_grad_(True)
    out = dis(x)
    (out * g.t(tag + "/R.0", DEV)).sum().backward()
    torch.cuda.synchronize()
    assert_close(out, g[tag + "/out.0"], 1e-4, "out")
    assert_close(x.grad, g[tag + "/gin.0"], 1e-3, "gin", atol=1e-6)
    assert all(p.grad is None for p in dis.parameters())
    n = 0
    for k, v in dis.state_dict().items():
        key = "%s/after.%s" % (tag, k)
        if key in g.files:
            assert_close(v.float(), g[key].astype(np.float32), 1e-5, key)
            if k.endswith(("weight_u", "weight_v")) and v.numel() > 1:      # (the last layer's u is the 1-vector +-1)
                assert not torch.equal(v.cpu(), g.t("%s/P.%s" % (tag, k))), k + " did not advance"
                n += 1
    assert n == 2 * 4 - 1


# the five matrices of the default discriminator (Cout, Cin; 4x4 taps) and one odd shape
SN_SHAPES = [(64, 1, 4), (128, 64, 4), (256, 128, 4), (512, 256, 4), (1, 512, 4), (7, 5, 3)]


def _torch_spectral_fp32(w, u, v, G, training):
    """torch.nn.utils.spectral_norm itself in fp32 on the CPU: -> (weight, u, v, d weight_orig)"""
    cout, cin, k, _ = w.shape
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, cout, k, bias=False))
    with torch.no_grad():
        conv.weight_orig.copy_(w)
        conv.weight_u.copy_(u)
        conv.weight_v.copy_(v)
    conv.train(training)
    conv(torch.zeros(1, cin, k, k))
    (conv.weight * G).sum().backward()
    return conv.weight.detach(), conv.weight_u.clone(), conv.weight_v.clone(), conv.weight_orig.grad


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", SN_SHAPES)
def test_spectral_norm_weight_vs_float64(shape, training):
    """ops.spectral_norm_weight alone against the float64 restatement: weight, updated u / v, weight_orig gradient.  Bound
    (DESIGN section 2): twice the distance of torch's own fp32 spectral_norm from float64 on the same inputs, never below the
    1e-5 that state buffers are allowed (torch's CPU sums are pairwise and can beat any other order of 8192 terms)."""
    from hipops import ops
    cout, cin, k = shape
    gen = torch.Generator().manual_seed(cout * 131 + cin)
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.2
    u = torch.nn.functional.normalize(torch.randn(cout, generator=gen), dim=0)
    v = torch.nn.functional.normalize(torch.randn(cin * k * k, generator=gen), dim=0)
    G = torch.randn(cout, cin, k, k, generator=gen)
    w64 = w.double().requires_grad_(True)
    u64, v64 = u.double(), v.double()
    out64 = spectral_weight_ref(w64, u64, v64, training)
    (out64 * G.double()).sum().backward()
    truth = dict(weight=out64.detach(), u=u64, v=v64, grad=w64.grad)
    t32 = dict(zip(("weight", "u", "v", "grad"), _torch_spectral_fp32(w, u, v, G, training)))
    wd = w.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ud, vd = u.to(DEV), v.to(DEV)
    out = ops.spectral_norm_weight(wd, ud, vd, training)
    assert out.shape == w.shape
    (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    mine = dict(weight=out.detach(), u=ud, v=vd, grad=wd.grad)
    for key in ("weight", "u", "v", "grad"):
        bound = max(2.0 * rel_err(t32[key], truth[key]), 1e-5)
        err = rel_err(mine[key], truth[key])
        print("%s %s %s: rel err %.3e, torch fp32 %.3e, bound %.3e" % (shape, "train" if training else "eval", key, err,
                                                                        rel_err(t32[key], truth[key]), bound))
        assert err <= bound, "%s %s: %.3e > %.3e" % (shape, key, err, bound)
    if not training:
        assert torch.equal(ud.cpu(), u) and torch.equal(vd.cpu(), v)


def test_spectral_norm_weights_many_layers_equal_single_calls():
    """The multi-layer call gives, bit for bit, what one call per layer gives (the table only routes workgroups)."""
    from hipops import ops
    gen = torch.Generator().manual_seed(5)
    ws, us, vs = [], [], []
    for cout, cin, k in SN_SHAPES:
        ws.append((torch.randn(cout, cin, k, k, generator=gen) * 0.2).to(DEV).contiguous(memory_format=torch.channels_last))
        us.append(torch.nn.functional.normalize(torch.randn(cout, generator=gen), dim=0).to(DEV))
        vs.append(torch.nn.functional.normalize(torch.randn(cin * k * k, generator=gen), dim=0).to(DEV))
    for training in (True, False):
        u1, v1 = [u.clone() for u in us], [v.clone() for v in vs]
        u2, v2 = [u.clone() for u in us], [v.clone() for v in vs]
        many = ops.spectral_norm_weights(ws, u1, v1, training)
        single = [ops.spectral_norm_weight(w, u, v, training) for w, u, v in zip(ws, u2, v2)]
        torch.cuda.synchronize()
        for a, b, ua, ub, va, vb in zip(many, single, u1, u2, v1, v2):
            assert torch.equal(a, b) and torch.equal(ua, ub) and torch.equal(va, vb)


def _two_updates(seed):
    from functions import hinge_d_loss
    from hipops import Adam, ops
    torch.manual_seed(seed)
    dis = _build("actnorm", 16, 3, True).to(DEV).train()
    opt = Adam(dis.parameters(), lr=1e-3, betas=(0.5, 0.999))
    gen = torch.Generator().manual_seed(seed + 1)
    losses = []
    for _ in range(2):
        real = torch.randn(4, 1, 64, 64, generator=gen).to(DEV)
        fake = torch.randn(4, 1, 64, 64, generator=gen).to(DEV)
        l_dis = hinge_d_loss(dis(real), dis(fake))
        opt.zero_grad()
        ops.weighted_sum([l_dis], [0.8]).backward()
        opt.step()
        losses.append(l_dis.detach().cpu())
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in dis.state_dict().items()}


def test_discriminator_updates_are_run_to_run_bit_identical():
    la, sa = _two_updates(21)
    lb, sb = _two_updates(21)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert all(np.isfinite(float(l)) for l in la)


def _small_config(tmp_path, name, dis=None, **top):
    from utils import load_json
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["run"]["training_mode"] = "second_step"
    raw["model"]["dis"].update(dict(n_filters=8, n_layers=3), **(dis or {}))
    raw.update(top)
    p = tmp_path / name
    p.write_text(json.dumps(raw))
    return load_json(str(p))


def test_build_second_step_trainer_actnorm_spectral(tmp_path):
    """A second-step config with actnorm + apply_spectral_norm + distinct dec_optim / dis_optim: three steps run, the losses
    are finite, `initialized` flips once, the optimisers carry their own settings, and the saved discriminator has the
    reference's keys."""
    from networks.actnorm import ActNorm
    from trainers import build_second_step_trainer, configure_models
    from utils.checkpoint import save_lightning_style_ckpt
    c = _small_config(tmp_path, "a.json", dis=dict(normalization="actnorm", apply_spectral_norm=True),
                      dec_optim=dict(lr=2e-4, b1=0.5, b2=0.9, weight_decay=0.0),
                      dis_optim=dict(lr=4e-4, b1=0.0, b2=0.99, weight_decay=1e-5))
    torch.manual_seed(11)
    enc, dec = configure_models(c)
    ck = str(tmp_path / "first.ckpt")
    save_lightning_style_ckpt(ck, enc, dec)
    tr = build_second_step_trainer(c, device=DEV, first_stage_ckpt_path=ck)
    acts = [m for m in tr.dis.modules() if isinstance(m, ActNorm)]
    assert acts and all(int(m.initialized) == 0 for m in acts)
    gd, gs = tr.dec_optim.param_groups[0], tr.dis_optim.param_groups[0]
    assert (gd["lr"], tuple(gd["betas"])) == (2e-4, (0.5, 0.9)) and (gs["lr"], tuple(gs["betas"]), gs["weight_decay"]) == (4e-4, (0.0, 0.99), 1e-5)
    gen = torch.Generator().manual_seed(2)
    scales, us = [], []
    for s in range(3):
        out = tr.training_step({"image": (torch.rand(4, 1, 32, 32, generator=gen) * 2 - 1).to(DEV)})
        torch.cuda.synchronize()
        for k in ("gen_total", "recon", "gen", "dis_total"):
            assert np.isfinite(float(out[k].detach())), (s, k)
        assert all(int(m.initialized) == 1 for m in acts)
        scales.append(acts[0].scale.detach().cpu().clone())
        us.append(tr.dis.main[0].weight_u.cpu().clone())
    assert float((scales[0] - 1).abs().max()) > 0                      # initialised from the first batch ...
    assert float((scales[1] - scales[0]).abs().max()) < 0.05 * float(scales[0].abs().max())      # ... once: then only Adam's small steps
    assert not torch.equal(us[0], us[1])
    out_ck = str(tmp_path / "dis.ckpt")
    save_lightning_style_ckpt(out_ck, dis=tr.dis)
    keys = set(torch.load(out_ck, map_location="cpu")["state_dict"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "gan_norms.npz"))
    assert keys == {"dis." + k[len("dstep_sn_act/P."):] for k in g.files if k.startswith("dstep_sn_act/P.")}


def test_config_built_default_trainer_equals_hand_built_bit_for_bit(tmp_path):
    """With the default values (batchnorm, no spectral norm, equal optimiser settings) the config route is the existing
    path: outputs and updated state equal a hand-built SecondStepTrainer's bit for bit over two steps."""
    from networks import NLayerDiscriminator
    from trainers import build_second_step_trainer, configure_models, SecondStepTrainer, gan_loss_weights
    c = _small_config(tmp_path, "d.json")
    torch.manual_seed(12)
    tr_c = build_second_step_trainer(c, device=DEV)
    enc, dec = configure_models(c)
    dis = NLayerDiscriminator(1, 1, n_filters=8, n_layers=3)
    for dst, src in ((enc, tr_c.encoder), (dec, tr_c.decoder), (dis, tr_c.dis)):
        dst.load_state_dict({k: v.cpu().clone() for k, v in src.state_dict().items()}, strict=True)
    o = c.dec_optim
    tr_h = SecondStepTrainer(enc, dec, dis, loss_weight=gan_loss_weights(c), lr=o.lr, betas=(o.b1, o.b2), weight_decay=o.weight_decay or 0.0,
                             device=DEV)
    gen = torch.Generator().manual_seed(3)
    for s in range(2):
        img = (torch.rand(4, 1, 32, 32, generator=gen) * 2 - 1).to(DEV)
        a, b = tr_c.training_step({"image": img.clone()}), tr_h.training_step({"image": img.clone()})
        torch.cuda.synchronize()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (s, k)
    for ma, mb in ((tr_c.decoder, tr_h.decoder), (tr_c.dis, tr_h.dis)):
        for (k, v), (_, v2) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, v2), k


WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "medical-image-editing_amd"))
forced = os.environ.get("VQW_DP_FORCE", "0") == "1"      # one rank, every collective issued all the same (hipops.ops)
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1)
from networks import NLayerDiscriminator
from utils import apply_spectral_norm
from functions import hinge_d_loss
from hipops import Adam, ops
torch.manual_seed(31)
dis = NLayerDiscriminator(1, 1, n_filters=8, n_layers=3, normalization='actnorm')
apply_spectral_norm(dis)
dis = dis.to("cuda:0").train()
opt = Adam(dis.parameters(), lr=1e-3, betas=(0.5, 0.999))
g = torch.Generator().manual_seed(32)
real, fake = torch.randn(4, 1, 64, 64, generator=g).cuda(), torch.randn(4, 1, 64, 64, generator=g).cuda()
l = hinge_d_loss(dis(real), dis(fake))
opt.zero_grad()
ops.weighted_sum([l], [0.8]).backward()
opt.step()
torch.cuda.synchronize()
torch.save({"loss": l.detach().cpu(), "collectives": ops.collective_calls,
            "state": {k: v.cpu() for k, v in dis.state_dict().items()}}, out)
if forced:
    dist.barrier(); dist.destroy_process_group()
'''


def test_one_rank_process_group_equals_plain_run(tmp_path):
    """ActNorm's initialisation all-reduces its sums when a process group is up; with one rank that is the identity, so the
    initialised loc / scale, a spectral step and the Adam update equal the run without a group bit for bit."""
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    res = []
    for tag, port, extra in (("plain", 29641, {}), ("group", 29642, {"VQW_DP_FORCE": "1"})):
        out = str(tmp_path / tag)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", **extra)
        p = subprocess.Popen([sys.executable, str(script), ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        o = p.communicate(timeout=500)[0].decode()
        assert p.returncode == 0, o[-3000:]
        res.append(torch.load(out))
    plain, group = res
    assert plain["collectives"] == 0 and group["collectives"] == 3          # one all-reduce per ActNorm layer, once
    assert torch.equal(plain["loss"], group["loss"])
    for k in plain["state"]:
        assert torch.equal(plain["state"][k], group["state"][k]), k
    assert all(int(v) == 1 for k, v in plain["state"].items() if k.endswith("initialized"))
