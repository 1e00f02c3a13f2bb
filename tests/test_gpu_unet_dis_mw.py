"""GPU tests of the multi-window second training step with the U-Net discriminator: the window-stack kernels and operator
against float64, one step of the reference's fixture (tests/golden/unet_dis_mw_step*.npz, made by
tests/golden/make_golden_unet_dis_mw.py with the reference trainers' un-clamped re-windowing), run-to-run bit-identity, a
one-rank process group, a run through the launcher with -w, and the step with this project's clamped windows against the
float32 restatement.  Run with `pytest -m gpu` on an MI355X.

Tolerance of the kernel tests.  A window-stack output is one fp32 fma and a clamp of fp32 table entries: relative error below
3 * 2^-24 per element; a gradient is a sum of at most three products: below 5 * 2^-24.  Both are held to 1e-6 of the tensor's
norm, as the element-wise kernels of tests/test_gpu_unet_dis.py are; an indexing error or a wrong window row is of order 1."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close, check_init
import unet_dis_ref as U
import unet_dis_mw_ref as MW

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = 2.0 ** -24
DATASET_WINDOW = (2000, 0, 2.0)
SHAPES = [(1, 1, 5, 7), (2, 1, 32, 32), (3, 2, 17, 9)]          # 35 and 918 elements: n % 4 != 0; 2048: two blocks of float4


def _windows(kind):
    from hipops import ops
    lung, med = (ops.window_map(DATASET_WINDOW, w, clamp=kind != "affine") for w in (MW.LUNG_WINDOW, MW.MEDIASTINAL_WINDOW))
    return {"identity": (None,), "lung": (lung,), "lung+identity": (lung, None), "clamped": (None, lung, med),
            "affine": (None, lung, med), "mediastinal first": (med, lung, None)}[kind]


WINDOW_SETS = ["identity", "lung", "lung+identity", "clamped", "affine", "mediastinal first"]


def _input(shape, windows, seed):
    """float32-representable values over [-1.5, 1.5] - beyond both bounds of both windows (x = -1.3 and 0.2, -0.18 and 0.22) -
    none within 1e-3 of a bound in the window's units, so that fp32 and fp64 take the same side everywhere."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g, dtype=torch.float64) * 3 - 1.5).float().double()
    x.view(-1)[:6] = torch.tensor([-1.45, 1.45, 0.0, -0.5, 0.3, -1.0], dtype=torch.float32).double()    # below, above and inside, whatever the draw
    for w in windows:
        if w is not None and abs(w[2]) < 1e30:
            for _ in range(4):
                z = w[0] * x + w[1]
                near = ((z - w[2]).abs() < 1e-3) | ((z - w[3]).abs() < 1e-3)
                x = torch.where(near, (x + 0.01).float().double(), x)
            z = w[0] * x + w[1]
            assert not bool((((z - w[2]).abs() < 1e-3) | ((z - w[3]).abs() < 1e-3)).any())
            assert bool((z < w[2]).any()) and bool((z > w[3]).any())
    return x


def _apply64(x, w):
    return x.clone() if w is None else (w[0] * x + w[1]).clamp(w[2], w[3])


def _slope64(x, w):
    if w is None:
        return torch.ones_like(x)
    z = w[0] * x + w[1]
    return torch.where((z > w[2]) & (z < w[3]), torch.full_like(x, w[0]), torch.zeros_like(x))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def _nchw(a):
    return a.permute(0, 3, 1, 2).double().cpu()


@pytest.mark.parametrize("kind", WINDOW_SETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_window_stack_kernels(shape, kind):
    from hipops import ops
    L = ops._L()
    windows = _windows(kind)
    nwin, n = len(windows), int(np.prod(shape))
    x = _input(shape, windows, seed=n + nwin)
    table = ops._window_table(windows, torch.empty(1, device=DEV))
    dx = _nhwc(x)
    N, C, H, W = shape
    outs = [torch.full((N, H, W, C), -7.0, device=DEV) for _ in range(nwin)] + [None] * (3 - nwin)
    L.vqw_window_stack_fwd(dx, table, outs[0], outs[1], outs[2], nwin, n)
    torch.cuda.synchronize()
    for i, w in enumerate(windows):
        assert_close(_nchw(outs[i]), _apply64(x, w), 1e-6, "window %d" % i)
    # a skipped output is not written; the others are what they were
    if nwin > 1:
        again = [torch.full((N, H, W, C), -7.0, device=DEV) for _ in range(nwin)] + [None] * (3 - nwin)
        L.vqw_window_stack_fwd(dx, table, again[0], None, again[2], nwin, n)
        torch.cuda.synchronize()
        assert torch.equal(again[0], outs[0]) and (nwin < 3 or torch.equal(again[2], outs[2]))
    g = torch.Generator().manual_seed(n)
    gs = [torch.randn(shape, generator=g, dtype=torch.float64).float().double() for _ in range(nwin)]
    dgs = [_nhwc(t) for t in gs]
    for present in itertools.product((True, False), repeat=nwin):          # every subset of the gradients missing
        want = sum((gs[i] * _slope64(x, windows[i]) for i in range(nwin) if present[i]), torch.zeros_like(x))
        args = [dgs[i] if i < nwin and present[i] else None for i in range(3)]
        gx, gx2 = (torch.full((N, H, W, C), -7.0, device=DEV) for _ in range(2))
        L.vqw_window_stack_bwd(dx, table, args[0], args[1], args[2], gx, nwin, n)
        L.vqw_window_stack_bwd(dx, table, args[0], args[1], args[2], gx2, nwin, n)
        torch.cuda.synchronize()
        if not any(present):
            assert not bool(gx.any()), "all gradients missing: gx must be exactly zero"
        else:
            assert_close(_nchw(gx), want, 1e-6, "gx with %s" % (present,))
        assert torch.equal(gx, gx2), "gx differs on a second call"


def test_window_stack_operator_differentiates(monkeypatch):
    """A loss over windows 0 and 2 only: x.grad equals the float64 torch gradient (torch.clamp; no input lies on a bound), the
    three outputs share one autograd node whose only differentiable input is x, and its backward is ONE launch that gets the
    unused window's gradient as None."""
    from hipops import ops
    windows = _windows("clamped")
    shape = (3, 2, 17, 9)
    x64 = _input(shape, windows, seed=3).requires_grad_(True)
    w0, w2 = (U.weight_pattern(shape) * s for s in (1.0, 0.7))
    (x64 * w0).sum().add((windows[2][0] * x64 + windows[2][1]).clamp(windows[2][2], windows[2][3]).mul(w2).sum()).backward()
    L = ops._L()
    calls, real = [], L.vqw_window_stack_bwd
    monkeypatch.setattr(L, "vqw_window_stack_bwd", lambda *a: calls.append([t is None for t in a[2:5]]) or real(*a))
    x = x64.detach().float().to(DEV).requires_grad_(True)
    outs = ops.window_stack(x, windows)
    assert len(outs) == 3 and all(o.is_contiguous(memory_format=torch.channels_last) and o.data_ptr() != x.data_ptr() for o in outs)
    assert outs[0].grad_fn is outs[1].grad_fn is outs[2].grad_fn
    assert [type(f).__name__ for f, _ in outs[0].grad_fn.next_functions if f is not None] == ["AccumulateGrad"]
    ((outs[0] * w0.float().to(DEV)).sum() + (outs[2] * w2.float().to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert calls == [[False, True, False]]
    assert_close(x.grad, x64.grad, 1e-6, "x.grad")
    for o, w in zip(outs, windows):
        assert_close(o, _apply64(x64.detach(), w), 1e-6, "output")
    # without x.requires_grad no tape is kept
    plain = ops.window_stack(x.detach(), windows)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain) and all(torch.equal(a, b) for a, b in zip(plain, outs))


# ------------------------------------------------------------------------------------------------ the step fixture
def _state(golden):
    return {k[2:]: v for k, v in golden("unet_dis_mw_step.npz").group("step").items() if k.startswith("P.")}


def _boxes(g):
    out = []
    for i in range(3):
        y0, y1, x0, x1 = (int(v) for v in g["step/box%d" % i])
        out.append((((y0, y1), (x0, x1)), bool(int(g["step/flip%d" % i]))))
    return out


def _step_trainer(golden, clamp_windows=False, **kw):
    from helpers import build_models
    from networks import UNetDiscriminator
    from trainers import UNetMultiWindowSecondStepTrainer, UNetGanLossWeights
    g = golden("unet_dis_mw_step.npz")
    cfg = {k: g["step/cfg/" + k] for k in ("enc_filters", "dec_filters", "K", "momentum", "seed")}
    enc, dec = build_models(cfg)
    check_init({k[len("step/"):]: g[k] for k in g.files if k.startswith("step/init_sum/")}, enc, dec)
    K = int(cfg["K"])
    with torch.no_grad():
        enc.vq.embed.mul_(0.7)
        enc.vq.cluster_size.fill_(512 * 512 / K)
        enc.vq.embed_avg.copy_(enc.vq.embed.t() * enc.vq.cluster_size[None, :])
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    dis.load_state_dict(_state(golden), strict=True)
    w = UNetGanLossWeights(**{k: float(g["step/cfg/w." + k]) for k in UNetGanLossWeights._fields})
    width, center, scale = (float(v) for v in g["step/cfg/dataset_window"])
    mw = dict(dataset_window=(int(width), int(center), scale), recon_weights=tuple(float(v) for v in g["step/cfg/recon_weights"]))
    it = iter(_boxes(g))
    return UNetMultiWindowSecondStepTrainer(enc, dec, dis, loss_weight=w, lr=float(g["step/cfg/lr"]),
                                            betas=tuple(float(b) for b in g["step/cfg/betas"]), device=DEV,
                                            use_unet_perceptual_loss=True, cutmix_box=lambda: next(it), multi_window=mw,
                                            clamp_windows=clamp_windows, **kw)


def _run_step(golden, **kw):
    g = golden("unet_dis_mw_step.npz")
    tr = _step_trainer(golden, **kw)
    dec_before = {k: v.detach().cpu().clone() for k, v in tr.decoder.state_dict().items()}
    out = tr.training_step({"image": g.t("step/image", DEV)})
    out = {k: v.detach().clone() for k, v in out.items()}
    torch.cuda.synchronize()
    return tr, out, dec_before


@pytest.fixture(scope="module")
def fixture_step(golden):
    """The fixture's step with clamp_windows=False, run once for the tests that only read it."""
    return _run_step(golden)


def _losses(out):
    return torch.stack([out[k].double().cpu() if k in out else torch.zeros((), dtype=torch.float64) for k in U.LOSS_NAMES])


def test_step_golden(golden, fixture_step):
    """The assertions of test_gpu_unet_dis.py::test_two_steps_golden on the one multi-window step: all ten logged losses within
    2 x the fixture's own fp32-against-fp64 spread (+ fp32 storage rounding) of the largest; the state after within 2e-3 of the
    norm (atol 2e-4); the UPDATE of the decoder and of the discriminator within twice the fixture's own fp32-against-fp64
    distance of the reference run's; `linear.*` untouched.  Every u0 and sv0 after the step is also held to 1e-5, the bound one
    forward is held to in test_gpu_unet_dis.py: the step is 15 forwards of the same weights, each a power iteration from the u0
    the one before left, whose fp32 roundings (three of 6e-8 per forward) add up to 3e-6 at most and are not amplified; one
    forward more or less moves u0 by the iteration's own progress, orders of magnitude more on these unconverged vectors."""
    g = golden("unet_dis_mw_step.npz")
    before = _state(golden)
    tr, out, dec_before = fixture_step
    sp = float(g["step/spread.loss"])
    ref, got = torch.from_numpy(g["step/loss"]).double(), _losses(out)
    scale = float(ref.abs().max())
    for k, a, r in zip(U.LOSS_NAMES, got.tolist(), ref.tolist()):
        print("%-16s %.8g  reference %.8g  |diff| / largest %.3e  (spread %.1e)" % (k, a, r, abs(a - r) / scale, sp))
    assert "freq" not in out and "perceptual" not in out
    assert set(out) == {"gen_total", "gen", "recon", "unet_perceptual", "dis_total", "dis", "cutmix", "consistency", "ids", "recon_image"}
    for file, pre, m in (("unet_dis_mw_step_after.npz", "dis", tr.dis), ("unet_dis_mw_step_dec.npz", "dec", tr.decoder)):
        ga = golden(file)
        for k, v in m.state_dict().items():
            r = ga["step/after.%s.%s" % (pre, k)]
            if v.is_floating_point():
                assert_close(v.float(), r.astype(np.float32), 2e-3, "after.%s.%s" % (pre, k), atol=2e-4)
            else:
                assert int(v) == int(r), k
    ga = golden("unet_dis_mw_step_after.npz")
    moved = 0
    for k, v in tr.dis.state_dict().items():
        if k.endswith(("u0", "sv0")) and not k.startswith("linear."):
            assert_close(v, ga["step/after.dis." + k], 1e-5, k)
            moved += not torch.equal(v.cpu(), before[k])
    assert moved == 2 * 43          # the 43 normalised layers in use (`linear` is the 44th and is never run)
    for file, pre, m, prior in (("unet_dis_mw_step_after.npz", "dis", tr.dis, before), ("unet_dis_mw_step_dec.npz", "dec", tr.decoder, dec_before)):
        ga, sd = golden(file), m.state_dict()
        names = [k for k, _ in m.named_parameters()]
        upd = torch.cat([(sd[k].cpu().double() - prior[k].double()).reshape(-1) for k in names])
        upd_ref = torch.cat([(ga.t("step/after.%s.%s" % (pre, k)).double() - prior[k].double()).reshape(-1) for k in names])
        e, bound = float((upd - upd_ref).norm() / upd_ref.norm()), 2.0 * float(g["step/spread.update_" + pre])
        print("%s update: %.3e from the reference's (norm %.3e over %d entries; bound %.3e)" % (pre, e, float(upd_ref.norm()), upd.numel(), bound))
        assert float(upd_ref.norm()) > 0 and e <= bound, "%s update %.3e > %.3e" % (pre, e, bound)
    for k in ("linear.weight", "linear.bias", "linear.u0", "linear.sv0"):
        assert torch.equal(tr.dis.state_dict()[k].cpu(), before[k]), k
    err, bound = float((got - ref).abs().max()), (2.0 * sp + F32_EPS) * scale
    assert err <= bound, "max |diff| %.3e > %.3e" % (err, bound)


def test_step_is_deterministic(golden, fixture_step):
    a, oa, _ = fixture_step
    b, ob, _ = _run_step(golden)
    assert list(oa) == list(ob)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    for ma, mb in ((a.decoder, b.decoder), (a.dis, b.dis)):
        for (k, v), (_, v2) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, v2), k


def test_clamped_step_equals_float32_restatement(golden):
    """clamp_windows=True, this project's convention: the step runs, and its ten losses equal the float32 restatement with
    clamp=True evaluated on the step's own reconstruction - two fp32 evaluations of the same losses, held to the bound the
    reference fixture sets for such a pair: (2 x its fp32-against-fp64 spread + fp32 rounding) x the largest value.  They
    differ from the un-clamped fixture's by far more."""
    g = golden("unet_dis_mw_step.npz")
    tr, out, _ = _run_step(golden, clamp_windows=True)
    assert tr.clamp_windows and tr.windows[1][2:] == (-1.0, 1.0)
    w = {k: float(g["step/cfg/w." + k]) for k in ("recon", "gen", "unet_perceptual", "dis", "cutmix", "consistency")}
    boxes = _boxes(g)
    st = {k: v.float() for k, v in _state(golden).items()}
    ref = MW.step_losses_ref(g.t("step/image").float(), out["recon_image"].float().cpu().contiguous(), st, [b for b, _ in boxes],
                             [f for _, f in boxes], w, tr.multi_window["dataset_window"], tr.multi_window["recon_weights"], True).double()
    got = _losses(out)
    scale, sp = float(ref.abs().max()), float(g["step/spread.loss"])
    for k, a, r in zip(U.LOSS_NAMES, got.tolist(), ref.tolist()):
        print("%-16s %.8g  restatement %.8g  |diff| / largest %.3e  (spread %.1e)" % (k, a, r, abs(a - r) / scale, sp))
    assert bool(torch.isfinite(got).all())
    unclamped = torch.from_numpy(g["step/loss"]).double()
    assert float((got - unclamped).abs().max()) > 1e3 * (2.0 * sp + F32_EPS) * float(unclamped.abs().max())
    err, bound = float((got - ref).abs().max()), (2.0 * sp + F32_EPS) * scale
    assert err <= bound, "max |diff| %.3e > %.3e" % (err, bound)


WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "medical-image-editing_amd")); sys.path.insert(0, os.path.join(root, "tests"))
forced = os.environ.get("VQW_DP_FORCE", "0") == "1"      # one rank, every collective issued all the same (hipops.ops)
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1)
from conftest import load_golden
import test_gpu_unet_dis_mw as T
tr, o, _ = T._run_step(load_golden, data_parallel=forced)
torch.save({"losses": {k: v.cpu() for k, v in o.items()},
            "state": {n: {k: v.cpu() for k, v in m.state_dict().items()} for n, m in (("dec", tr.decoder), ("dis", tr.dis))}}, out)
if forced:
    dist.barrier(); dist.destroy_process_group()
'''


def test_one_rank_process_group_equals_plain_run(tmp_path):
    """With one rank the gradient all-reduce is the identity: the step under a process group (reducers on, `linear.*` kept out
    of the discriminator's) equals the plain run bit for bit; each in a fresh child process."""
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    res = []
    for tag, port, extra in (("plain", 29661, {}), ("group", 29662, {"VQW_DP_FORCE": "1"})):
        out = str(tmp_path / tag)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", **extra)
        p = subprocess.Popen([sys.executable, str(script), ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        o = p.communicate(timeout=500)[0].decode()
        assert p.returncode == 0, o[-3000:]
        res.append(torch.load(out))
    plain, group = res
    assert list(plain["losses"]) == list(group["losses"])
    for k in plain["losses"]:
        assert torch.equal(plain["losses"][k], group["losses"][k]), k
    for n in plain["state"]:
        for k in plain["state"][n]:
            assert torch.equal(plain["state"][n][k], group["state"][n][k]), (n, k)


# ------------------------------------------------------------------------------------------------ through the launcher
UNET_DIS = dict(model_name="UNetDiscriminator", D_ch=4, D_wide=True, D_attn="0", resolution=512, normalization="batchnorm")
NEW_COLUMNS = ["unet_perceptual", "cutmix", "consistency"]


def _launch(tmp, name, n_epochs, resume=None):
    from run_helpers import MONITORED, raw_config, run_launcher, write_config
    save = os.path.join(str(tmp), name)
    raw = raw_config(save, None, run=dict(training_mode="second_step", n_epochs=n_epochs, monitoring_metrics=MONITORED + NEW_COLUMNS),
                     dataset=dict(dataset_name="synthetic", image_size=512, batch_size=1, n_samples_train=2, n_samples_val=1,
                                  window_width=2000, window_center=0, window_scale=2.0),
                     model=dict(dis=dict(UNET_DIS), vqmodel=dict(enc_filters=[4, 8, 16, 32, 64], dec_filters=[8, 16, 32, 64, 128])),
                     loss=dict(use_unet_perceptual_loss=True, recon_weights=[1.0, 0.5, 0.25],
                               loss_weight=dict(gen=0.5, dis=1.0, unet_perceptual=0.25, cutmix=0.75, consistency=2.0)),
                     save=dict(n_save_images=1))
    if resume:
        raw["run"]["resume_checkpoint"] = resume
    run_launcher(write_config(os.path.join(str(tmp), name + "%d.json" % n_epochs), raw), "-w")
    return save


def _ckpt(save, epoch, n=0):
    return os.path.join(save, "study", "version_%d" % n, "ckpt-epoch=%04d-total_loss=0.00.ckpt" % epoch)


def test_launcher_trains_logs_checkpoints_and_resumes(tmp_path):
    """`run_vqwnet.py -w` in second_step mode at 512 x 512 (the smallest size the 512 architecture allows), batch 1, D_ch = 4
    on two synthetic samples: one epoch of two steps writes log.csv with the ten loss keys and a checkpoint, and a second
    epoch resumed from it ends bit-identical to the uninterrupted two-epoch run (the CutMix draws, three per step, come from
    the saved generator states)."""
    from run_helpers import MONITORED, read_csv
    from test_gpu_run import _differences
    part = _launch(tmp_path, "part", 1)
    header, rows = read_csv(os.path.join(part, "study", "version_0", "log.csv"))
    assert header == MONITORED + NEW_COLUMNS and len(rows) == 2
    for row in rows:
        rec = dict(zip(header, row))
        for k in U.LOSS_NAMES:
            assert np.isfinite(float(rec[k])), (k, rec[k])
        assert float(rec["cutmix"]) > 0.0 and float(rec["unet_perceptual"]) > 0.0 and float(rec["recon"]) > 0.0
    assert os.path.isfile(_ckpt(part, 0))
    full = _launch(tmp_path, "full", 2)
    assert not _differences(_ckpt(part, 0), _ckpt(full, 0))
    _launch(tmp_path, "part", 2, resume=_ckpt(part, 0))
    diff = _differences(_ckpt(part, 1, n=1), _ckpt(full, 1))
    assert not diff, "resumed run differs from the uninterrupted one in %d tensors, e.g. %s" % (len(diff), diff[:8])
    _, rows_full = read_csv(os.path.join(full, "study", "version_0", "log.csv"))
    _, rows_resumed = read_csv(os.path.join(part, "study", "version_1", "log.csv"))
    assert rows_full[:2] == rows and rows_resumed == rows_full[2:]
