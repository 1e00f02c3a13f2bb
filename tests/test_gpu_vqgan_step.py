"""GPU tests of the VQGAN trainer (trainers/vqgan_unet_dis.py, run_vqwnet.py -v): two steps against the reference's fixture
(tests/golden/vqgan_step*.npz, made by tests/golden/make_golden_vqgan_step.py), run-to-run bit-identity, the inner loops, the term
switches, a one-rank process group, runs through the launcher (one rank with resume, two ranks on one card) and the validation
pass.  Run with `pytest -m gpu` on an MI355X.

The fixture's VQGAN is VQGAN(1, 32, 1, 32, 8, (1,1,1,1), (1,1,1,1), 1, [], [], 512, 0.0, True, 'torch') - latent 64 x 64, so the
mid attention blocks see N = 4096 - against the D_ch = 4 discriminator on one 512 x 512 image per step.  Tolerances are the
fixture's own: see test_two_steps_golden."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close
import vqgan_step_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = 2.0 ** -24


def _step_trainer(golden, **kw):
    from networks import VQGAN, UNetDiscriminator
    from trainers import VQGANUNetDisTrainer, VQGANLossWeights
    from test_vqgan_step_host import _initial_vqgan
    g = golden("vqgan_step.npz")
    vqgan = _initial_vqgan(g, VQGAN)
    dis = UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn='0', resolution=512, unconditional=True)
    dis.load_state_dict(g.group("step/P."), strict=True)
    w = VQGANLossWeights(**{k: float(g["step/cfg/w." + k]) for k in VQGANLossWeights._fields})
    boxes = []
    for s in range(2):
        y0, y1, x0, x1 = (int(v) for v in g["step/box%d" % s])
        boxes.append((((y0, y1), (x0, x1)), bool(int(g["step/flip%d" % s]))))
    boxes = boxes + boxes                    # a second inner loop draws on
    it = iter(boxes)
    kw.setdefault("use_unet_perceptual_loss", True)
    return VQGANUNetDisTrainer(vqgan, dis, loss_weight=w, lr=float(g["step/cfg/lr"]), betas=tuple(float(b) for b in g["step/cfg/betas"]),
                               device=DEV, cutmix_box=lambda: next(it), **kw)


def _run_two_steps(golden, **kw):
    g = golden("vqgan_step.npz")
    tr = _step_trainer(golden, **kw)
    outs = []
    for s in range(2):
        out = tr.training_step({"image": g.t("step/image%d" % s, DEV)})
        outs.append({k: v.detach().clone() for k, v in out.items()})
    torch.cuda.synchronize()
    return tr, outs


def test_two_steps_golden(golden):
    """All twelve logged values of both steps within (2 x the fixture's fp32-against-fp64 spread + fp32 storage rounding) of the
    largest of them - the fixture's values are the fp64 run's and its spread the worst of three fp32 evaluations of the
    reference, so a correct fp32 evaluation lies within one spread; the factor 2 is the margin tests/test_gpu_unet_dis.py
    keeps.  ids equal on every latent pixel (the fixture asserts that the reference's own fp32 evaluations all give them).  The
    state after within 2e-3 of the norm (atol 2e-4), and - because the fixture's Adam runs at lr 1e-6, which that tolerance
    does not resolve - the UPDATE of the VQGAN and of the discriminator (after - before, all parameters as one vector)
    within twice the fixture's own fp32-against-fp64 distance of that update, and non-zero.  The VQ buffers after each step,
    within 2 x spread.buf (the reference's three fp32 runs' distance from the fp64 run on those buffers) of their largest element."""
    g = golden("vqgan_step.npz")
    tr = _step_trainer(golden)
    before = {"vqgan": {k: v.detach().cpu().clone() for k, v in tr.vqgan.state_dict().items()},
              "dis": {k: v.detach().cpu().clone() for k, v in tr.dis.state_dict().items()}}
    sp, spb = float(g["step/spread.loss"]), float(g["step/spread.buf"])
    worst = []
    for s in range(2):
        out = tr.training_step({"image": g.t("step/image%d" % s, DEV)})
        torch.cuda.synchronize()
        assert "freq" not in out and "perceptual" not in out and out["recon_image"].shape == (1, 1, 512, 512)
        ref = torch.from_numpy(g["step/loss%d" % s]).double()
        got = S.logged_of({k: v.detach().cpu() for k, v in out.items()}, tr.w)
        scale = float(ref.abs().max())
        for k, a, r in zip(S.LOGGED, got.tolist(), ref.tolist()):
            print("step %d %-16s %.8g  reference %.8g  |diff| / largest %.3e  (spread %.1e)" % (s, k, a, r, abs(a - r) / scale, sp))
        worst.append((float((got - ref).abs().max()), (2.0 * sp + F32_EPS) * scale))
        ids, ref_ids = out["ids"].cpu(), torch.from_numpy(g["step/ids%d" % s])
        print("step %d: %d of %d ids differ (smallest fp64 gap %.2e)" % (s, int((ids != ref_ids).sum()), ids.numel(), float(g["step/min_gap"])))
        assert torch.equal(ids, ref_ids)
        for k in S.VQ_BUFFERS:
            ref_b = g.t("step/buf%d.%s" % (s, k)).double()
            err = float((getattr(tr.vqgan.vq, k).cpu().double() - ref_b).abs().max() / ref_b.abs().max())
            print("step %d vq.%s: %.3e of the largest element (bound %.3e)" % (s, k, err, 2 * spb + F32_EPS))
            assert err <= 2 * spb + F32_EPS, "vq.%s after step %d" % (k, s)
    files = {"encoder.": "vqgan_step_after_enc.npz", "vq.": "vqgan_step_after_enc.npz", "decoder.": "vqgan_step_after_dec.npz"}
    after = {"vqgan": {}, "dis": {}}
    for k in tr.vqgan.state_dict():
        after["vqgan"][k] = golden(files[k[:k.index(".") + 1]]).t("step/after.vqgan." + k)
    for k in tr.dis.state_dict():
        after["dis"][k] = golden("vqgan_step_after_dis.npz").t("step/after.dis." + k)
    for pre, m in (("vqgan", tr.vqgan), ("dis", tr.dis)):
        for k, v in m.state_dict().items():
            assert_close(v.float(), after[pre][k].float(), 2e-3, "after.%s.%s" % (pre, k), atol=2e-4)
        sd = m.state_dict()
        names = [k for k, _ in m.named_parameters()]
        upd = torch.cat([(sd[k].cpu().double() - before[pre][k].double()).reshape(-1) for k in names])
        upd_ref = torch.cat([(after[pre][k].double() - before[pre][k].double()).reshape(-1) for k in names])
        e, bound = float((upd - upd_ref).norm() / upd_ref.norm()), 2.0 * float(g["step/spread.update_" + pre])
        print("%s update: %.3e from the reference's (norm %.3e over %d entries; bound %.3e)" % (pre, e, float(upd_ref.norm()), upd.numel(), bound))
        assert float(upd_ref.norm()) > 0 and float(upd.norm()) > 0 and e <= bound, "%s update %.3e > %.3e" % (pre, e, bound)
    for k in ("linear.weight", "linear.bias"):
        assert torch.equal(tr.dis.state_dict()[k].cpu(), before["dis"][k]), k
    for s, (err, bound) in enumerate(worst):
        assert err <= bound, "step %d: max |diff| %.3e > %.3e" % (s, err, bound)


def test_two_steps_are_deterministic(golden):
    a, oa = _run_two_steps(golden)
    b, ob = _run_two_steps(golden)
    for x, y in zip(oa, ob):
        assert list(x) == list(y)
        for k in x:
            assert torch.equal(x[k], y[k]), k
    for ma, mb in ((a.vqgan, b.vqgan), (a.dis, b.dis)):
        for (k, v), (_, v2) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, v2), k


def test_two_inner_loops_equal_two_discriminator_updates(golden):
    """n_inner_loops = 2 is one step with a single loop followed by one more discriminator_update on the same image and
    reconstruction, bit for bit; the generator half's values are unchanged."""
    g = golden("vqgan_step.npz")
    image = g.t("step/image0", DEV)
    a, b = _step_trainer(golden, n_inner_loops=2), _step_trainer(golden)
    out_a = a.training_step({"image": image})
    out_b = b.training_step({"image": image})
    last = b.discriminator_update(image, out_b["recon_image"])
    torch.cuda.synchronize()
    for k, v in zip(("dis_total", "dis", "cutmix", "consistency"), last):
        assert torch.equal(out_a[k], v), k
        assert not torch.equal(out_a[k], out_b[k]), k + ": the second loop changed nothing"
    for k in ("gen_total", "recon", "commit", "gen", "unet_perceptual", "ids", "recon_image"):
        assert torch.equal(out_a[k], out_b[k]), k
    for ma, mb in ((a.vqgan, b.vqgan), (a.dis, b.dis)):
        for (k, v), (_, v2) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(v, v2), k
    assert all(st["step"] == 2 for st in a.dis_optim.state.values()) and all(st["step"] == 1 for st in a.dec_optim.state.values())


@pytest.mark.parametrize("off", ["use_recon_loss", "use_unet_perceptual_loss"])
def test_a_switched_off_term_is_left_out(golden, off):
    g = golden("vqgan_step.npz")
    tr = _step_trainer(golden, **{off: False})
    out = tr.training_step({"image": g.t("step/image0", DEV)})
    torch.cuda.synchronize()
    gone = {"use_recon_loss": "recon", "use_unet_perceptual_loss": "unet_perceptual"}[off]
    left = [k for k in ("recon", "commit", "gen", "unet_perceptual") if k != gone]
    assert gone not in out and all(k in out for k in left)
    # the generator total is a float32 weighted sum of three terms of order one: three roundings of 2^-24 each
    want = sum(float(getattr(tr.w, k)) * float(out[k].double()) for k in left)
    scale = sum(abs(float(getattr(tr.w, k)) * float(out[k].double())) for k in left)
    assert abs(float(out["gen_total"].double()) - want) <= 4 * F32_EPS * scale
    want = sum(float(getattr(tr.w, k)) * float(out[k].double()) for k in ("dis", "cutmix", "consistency"))
    assert abs(float(out["dis_total"].double()) - want) <= 4 * F32_EPS * abs(want)


WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "medical-image-editing_amd")); sys.path.insert(0, os.path.join(root, "tests"))
forced = os.environ.get("VQW_DP_FORCE", "0") == "1"      # one rank, every collective issued all the same (hipops.ops)
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1)
from conftest import load_golden
import test_gpu_vqgan_step as T
tr, outs = T._run_two_steps(load_golden, data_parallel=forced)
torch.save({"losses": [{k: v.cpu() for k, v in o.items()} for o in outs],
            "state": {n: {k: v.cpu() for k, v in m.state_dict().items()} for n, m in (("vqgan", tr.vqgan), ("dis", tr.dis))}}, out)
if forced:
    dist.barrier(); dist.destroy_process_group()
'''


def test_one_rank_process_group_equals_plain_run(tmp_path):
    """With one rank every all-reduce is the identity: the two steps under a process group (both reducers on, the quantiser's
    collectives issued) equal the plain run bit for bit."""
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
    for a, b in zip(plain["losses"], group["losses"]):
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for n in plain["state"]:
        for k in plain["state"][n]:
            assert torch.equal(plain["state"][n][k], group["state"][n][k]), (n, k)


# ------------------------------------------------------------------------------------------------ through the launcher
COLUMNS = ["epoch", "iteration", "total", "gen_total", "recon", "freq", "perceptual", "commit", "gen", "unet_perceptual", "dis_total",
           "dis", "cutmix", "consistency"]


def _launch(tmp, name, n_epochs, resume=None, env=None, **run):
    from run_helpers import raw_config, run_launcher, write_config
    save = os.path.join(str(tmp), name)
    raw = raw_config(save, None, **S.run_sections(n_epochs=n_epochs, monitoring_metrics=COLUMNS, training_mode="second_step", **run))
    if resume:
        raw["run"]["resume_checkpoint"] = resume
    run_launcher(write_config(os.path.join(str(tmp), name + "%d.json" % n_epochs), raw), "-v", env=env)
    return save


def _ckpt(save, epoch, n=0):
    return os.path.join(save, "study", "version_%d" % n, "ckpt-epoch=%04d-total_loss=0.00.ckpt" % epoch)


def test_launcher_trains_logs_checkpoints_and_resumes(tmp_path):
    """`run_vqwnet.py -v` at 512 x 512, batch 1, the fixture's VQGAN and D_ch = 4 on two synthetic samples, two epochs: the log
    has the trainer's columns, the picture is four tiles wide, the checkpoint loads strictly into fresh modules, and a run
    resumed from the first epoch's checkpoint ends bit-identical to the uninterrupted one."""
    from run_helpers import read_csv
    from networks import VQGAN, UNetDiscriminator
    from utils import png
    from utils.checkpoint import load_discriminator_from_ckpt
    from test_gpu_run import _differences
    full = _launch(tmp_path, "full", 2)
    vdir = os.path.join(full, "study", "version_0")
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == COLUMNS and len(rows) == 4
    for row in rows:
        rec = dict(zip(header, row))
        for k in COLUMNS[2:]:
            assert np.isfinite(float(rec[k])), (k, rec[k])
        assert float(rec["commit"]) > 0.0 and float(rec["cutmix"]) > 0.0
        assert abs(float(rec["total"]) - float(rec["gen_total"]) - float(rec["dis_total"])) <= 1e-5 * abs(float(rec["total"])) + 1e-6
    picture, _ = png.load(os.path.join(vdir, "000000.png"))
    assert tuple(picture.shape[:2]) == (512, 4 * 512) and os.path.exists(os.path.join(vdir, "000001.png"))
    sd = torch.load(_ckpt(full, 1), map_location="cpu")["state_dict"]
    assert all(k.startswith(("decoder.", "dis.")) for k in sd) and "decoder.encoder.conv_in.weight" in sd and "decoder.vq.embed" in sd
    VQGAN(*S.CASE["vqgan"]).load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    load_discriminator_from_ckpt(_ckpt(full, 1), UNetDiscriminator(in_channels=1, D_ch=4, D_wide=True, D_attn="0", resolution=512))
    part = _launch(tmp_path, "part", 1)
    assert not _differences(_ckpt(part, 0), _ckpt(full, 0))
    _launch(tmp_path, "part", 2, resume=_ckpt(part, 0))
    diff = _differences(_ckpt(part, 1, n=1), _ckpt(full, 1))
    assert not diff, "resumed run differs from the uninterrupted one in %d tensors, e.g. %s" % (len(diff), diff[:8])
    _, rows_resumed = read_csv(os.path.join(part, "study", "version_1", "log.csv"))
    assert rows_resumed == rows[2:]


def test_two_ranks_on_one_card(tmp_path):
    digest = os.path.join(str(tmp_path), "digest")
    save = _launch(tmp_path, "dp", 1, env={"VQW_DP_ONE_DEVICE": "1", "VQW_RUN_DIGEST": digest}, num_gpus=2)
    ranks = [json.load(open("%s.rank%d.json" % (digest, r))) for r in (0, 1)]
    assert ranks[0]["modules"] == ranks[1]["modules"] and set(ranks[0]["modules"]) == {"decoder", "dis"}
    seen = [set(i for _, idx in r["seen"] for i in idx) for r in ranks]
    assert not (seen[0] & seen[1]) and (seen[0] | seen[1]) == {0, 1}
    assert os.listdir(os.path.join(save, "study")) == ["version_0"]          # rank 0 alone wrote
    assert os.path.exists(_ckpt(save, 0))


def test_validation_leaves_the_state_alone(tmp_path):
    """Fit.validate runs the VQGAN and the discriminator in eval mode: the VQ buffers, every u0 / sv0 and everything else in
    the two state dicts are bit-equal before and after, the modules are back in train mode, and the picture is written."""
    from run_helpers import raw_config, write_config
    from trainers import build_vqgan_trainer, Fit
    from utils import load_json, png
    from utils.logger import Logger
    raw = raw_config(tmp_path / "out", None, **S.run_sections(n_epochs=1))
    raw["dataset"]["n_samples_val"] = 2
    raw["dataset"]["batch_size"] = 2
    raw["save"]["n_save_images"] = 2
    cfg = load_json(write_config(tmp_path / "c.json", raw))
    torch.manual_seed(3)
    tr = build_vqgan_trainer(cfg, device=DEV)
    fit = Fit(cfg, tr, Logger(save_dir=cfg.save.save_dir, config=cfg, name=cfg.save.study_name, monitoring_metrics=cfg.run.monitoring_metrics),
              device=DEV)
    before = {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in tr.modules().items()}
    assert any(k.endswith("u0") for k in before["dis"]) and "vq.embed_avg" in before["decoder"]
    path = fit.validate(0)
    torch.cuda.synchronize()
    for n, m in tr.modules().items():
        assert m.training
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[n][k]), (n, k)
    picture, _ = png.load(path)
    assert path.endswith("000000.png") and tuple(picture.shape[:2]) == (2 * 512, 4 * 512)
    # the two right-hand tiles are the discriminator's maps over their own range: each uses the whole grey scale
    for col in (2, 3):
        tile = np.asarray(picture)[:512, col * 512:(col + 1) * 512]
        assert tile.min() == 0 and tile.max() == 255
