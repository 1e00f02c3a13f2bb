"""Host side of the run_vqwnet launcher: checkpoint pruning, the logger, the PNG writer, the command line, the run
checkpoint's wire format, the synthetic dataset and the export operators' plumbing.  No GPU."""
import importlib
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from run_helpers import ROOT, SRC, raw_config, write_config


# ---------------------------------------------------------------------------------------------- 1. pruning
def _survivors(tmp_path, n):
    from utils.logger import checkpoint_name, prune_checkpoints
    d = tmp_path / ("ck%d" % n)
    d.mkdir()
    for epoch in range(n):
        (d / checkpoint_name(epoch)).write_bytes(b"")
        prune_checkpoints(str(d), limit_num=10, save_interval=10)
    return {int(f[len("ckpt-epoch="):len("ckpt-epoch=") + 4]) for f in os.listdir(d)}


def test_pruning_rule(tmp_path):
    from utils.logger import checkpoint_name
    assert checkpoint_name(7) == "ckpt-epoch=0007-total_loss=0.00.ckpt"
    assert _survivors(tmp_path, 35) == {9, 19} | set(range(25, 35))
    assert _survivors(tmp_path, 12) == set(range(2, 12))
    assert _survivors(tmp_path, 10) == set(range(10))


# ---------------------------------------------------------------------------------------------- 2. logger
def test_logger_versions_header_and_fields(tmp_path):
    from utils import load_json
    from utils.logger import Logger
    cfg = load_json(write_config(tmp_path / "c.json", raw_config(tmp_path / "out")))
    metrics = ["epoch", "total", "missing", "recon"]
    lg = Logger(str(tmp_path / "out"), cfg, metrics, name="study")
    assert lg.log_dir == str(tmp_path / "out" / "study" / "version_0")
    lg.log_metrics({"epoch": 0, "total": torch.tensor(1.5), "recon": 0.25, "unmonitored": 9})
    lg.log_metrics({"epoch": 1, "total": 2.0, "recon": torch.tensor([0.5, 0.25])})
    lines = open(os.path.join(lg.log_dir, "log.csv")).read().splitlines()
    assert lines[0] == ",".join(metrics)
    assert lines[1] == "0,1.5,,0.25" and lines[2] == "1,2.0,,0.75"
    lg.log_hyperparams([11, 12])
    saved = json.load(open(os.path.join(lg.log_dir, "config.json")))
    assert saved["seed_list"] == [11, 12] and saved["save_dir_path"] == lg.log_dir
    assert saved["model"]["vqmodel"]["dict_size"] == 10 and saved["run"]["resume_checkpoint"] is None
    second = Logger(str(tmp_path / "out"), cfg, metrics, name="study")
    assert second.version == 1 and second.log_dir.endswith("version_1")
    os.makedirs(str(tmp_path / "out" / "study" / "version_7"))
    assert Logger(str(tmp_path / "out"), cfg, metrics, name="study").version == 8


# ---------------------------------------------------------------------------------------------- 3. PNG
def _mini_decode(data):
    """Own minimal decoder: signature, chunks with CRC, zlib, filter type 0 only -> (H, W, colour type, rows, palette)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, pal, hdr = 8, b"", None, None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        pos += 12 + n
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            pal = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            idat += body
    W, H, depth, ctype, comp, filt, lace = hdr
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, -1)
    assert (raw[:, 0] == 0).all()
    return H, W, ctype, raw[:, 1:], pal


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 31), (64, 250)])
def test_png_round_trips(tmp_path, shape):
    from utils import png
    g = np.random.default_rng(sum(shape))
    grey = g.integers(0, 256, size=shape).astype(np.uint8)
    rgb = g.integers(0, 256, size=shape + (3,)).astype(np.uint8)
    pal = g.integers(0, 256, size=(11, 3)).astype(np.uint8)
    idx = g.integers(0, 11, size=shape).astype(np.uint8)
    for name, pixels, palette, ctype in (("g", grey, None, 0), ("c", rgb, None, 2), ("p", idx, pal, 3)):
        path = str(tmp_path / (name + ".png"))
        png.save(path, pixels, palette=palette)
        data = open(path, "rb").read()
        H, W, ct, rows, p = _mini_decode(data)
        assert (H, W, ct) == (shape[0], shape[1], ctype)
        assert rows.tobytes() == pixels.tobytes()
        if palette is not None:
            assert np.array_equal(p, pal)
        back, bp = png.load(path)
        assert np.array_equal(back, pixels) and (palette is None or np.array_equal(bp, pal))
        try:
            from PIL import Image
        except ImportError:
            continue
        im = Image.open(path)
        assert im.size == (shape[1], shape[0]) and im.mode == {0: "L", 2: "RGB", 3: "P"}[ctype]
        assert np.array_equal(np.asarray(im), pixels)
        if palette is not None:
            assert np.array_equal(np.asarray(im.convert("RGB")), pal[idx])


def test_png_refuses_what_it_does_not_write():
    from utils import png
    with pytest.raises(ValueError):
        png.encode(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        png.encode(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        png.encode(np.full((2, 2), 5, np.uint8), palette=np.zeros((3, 3), np.uint8))


# ---------------------------------------------------------------------------------------------- 4. command line
def _launcher():
    return importlib.import_module("run_vqwnet")


def test_command_line(tmp_path):
    rv = _launcher()
    p = rv.build_parser()
    a = p.parse_args(["-c", "x.json"])
    assert (a.mode, a.multiwindow, a.vqgan, a.rank) == ("train", False, False, None)
    a = p.parse_args(["-c", "x.json", "-m", "test", "-w", "-v"])
    assert (a.mode, a.multiwindow, a.vqgan) == ("test", True, True)
    cfg = write_config(tmp_path / "c.json", raw_config(tmp_path / "out"))
    with pytest.raises(NotImplementedError, match="VQGAN"):
        rv.main(["-c", cfg, "-v"])
    with pytest.raises(ValueError, match="'train' or 'test'"):
        rv.main(["-c", cfg, "-m", "fit"])
    inf = write_config(tmp_path / "i.json", raw_config(tmp_path / "out", run=dict(training_mode="inference")))
    with pytest.raises(ValueError, match="inference"):
        rv.main(["-c", inf, "-m", "train"])
    with pytest.raises(ValueError) as e:
        rv.main(["-c", cfg, "-w"])
    for key in ("loss.recon_weights", "dataset.window_width", "dataset.window_center", "dataset.window_scale"):
        assert key in str(e.value)
    nine = write_config(tmp_path / "n.json", raw_config(tmp_path / "out", run=dict(num_gpus=9)))
    with pytest.raises(ValueError, match="num_gpus"):
        rv.main(["-c", nine])
    assert not (tmp_path / "out").exists()          # nothing was started, nothing written


def test_parent_of_a_multi_process_run_stays_off_the_gpu(tmp_path):
    rv = _launcher()
    cfg = write_config(tmp_path / "c.json", raw_config(tmp_path / "out", run=dict(num_gpus=2)))
    marks = tmp_path / "marks"
    marks.mkdir()
    stub = ("import os, sys; a = sys.argv[1:]; "
            "open(os.path.join(%r, os.environ['RANK']), 'w').write(' '.join(a) + '|' + os.environ['WORLD_SIZE'] + '|' + "
            "os.environ['MASTER_ADDR'] + '|' + os.environ['MASTER_PORT'])" % str(marks))
    assert rv.main(["-c", cfg, "-m", "test"], child_command=[sys.executable, "-c", stub]) == 0
    assert not torch.cuda.is_initialized()
    seen = {r: open(str(marks / r)).read().split("|") for r in ("0", "1")}
    for r, (argv, world, addr, port) in seen.items():
        assert argv.split()[-2:] == ["--rank", r] and "-m test" in argv and "--seed 3" in argv
        assert world == "2" and addr and int(port) > 0
    assert seen["0"][3] == seen["1"][3]


def test_parent_stops_the_other_workers_when_one_fails(tmp_path):
    import time
    rv = _launcher()
    cfg = write_config(tmp_path / "c.json", raw_config(tmp_path / "out", run=dict(num_gpus=3)))
    stub = "import os, sys, time; sys.exit(5) if os.environ['RANK'] == '1' else time.sleep(120)"
    t0 = time.time()
    assert rv.main(["-c", cfg], child_command=[sys.executable, "-c", stub]) == 5
    assert time.time() - t0 < 60
    assert not torch.cuda.is_initialized()


def test_launcher_help_runs_as_a_script():
    out = subprocess.run([sys.executable, os.path.join(SRC, "run_vqwnet.py"), "-h"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"--multiwindow" in out.stdout and b"--vqgan" in out.stdout


# ---------------------------------------------------------------------------------------------- 5. checkpoint
def _fill_optimizer(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for p in opt.param_groups[0]["params"]:
        opt.state[p] = {"step": 3, "exp_avg": torch.randn(p.shape, generator=g).contiguous(memory_format=torch.channels_last)
                        if p.dim() == 4 else torch.randn(p.shape, generator=g),
                        "exp_avg_sq": torch.rand(p.shape, generator=g)}


def test_run_checkpoint_is_read_by_the_existing_loaders(tmp_path):
    from utils import load_json
    from utils.checkpoint import (save_run_checkpoint, load_run_checkpoint, load_first_stage_from_ckpt,
                                  load_discriminator_from_ckpt, init_from_ckpt, RUN_STATE_KEY)
    from trainers import build_first_step_trainer, build_second_step_trainer, configure_models, configure_discriminator
    c1 = load_json(write_config(tmp_path / "a.json", raw_config(tmp_path / "out")))
    c2 = load_json(write_config(tmp_path / "b.json", raw_config(tmp_path / "out", run=dict(training_mode="second_step"))))
    torch.manual_seed(1)
    tr = build_second_step_trainer(c2, device="cpu")
    _fill_optimizer(tr.dec_optim, 1)
    _fill_optimizer(tr.dis_optim, 2)
    path = str(tmp_path / "ckpt-epoch=0004-total_loss=0.00.ckpt")
    save_run_checkpoint(path, tr.state_dict(), epoch=4, global_step=55, run_state={"seed": 3, "gen": torch.get_rng_state()})
    raw = torch.load(path, map_location="cpu")            # the safe unpickler: tensors and plain containers only
    assert raw["epoch"] == 4 and raw["global_step"] == 55 and raw["optimizer_indices"] == [1, 2]
    assert len(raw["optimizer_states"]) == 2 and RUN_STATE_KEY in raw
    assert {k.split(".")[0] for k in raw["state_dict"]} == {"encoder", "decoder", "dis"}
    torch.manual_seed(2)
    enc, dec = configure_models(c2)
    dis = configure_discriminator(c2)
    load_first_stage_from_ckpt(path, enc, dec)
    load_discriminator_from_ckpt(path, dis)
    for new, old in ((enc, tr.encoder), (dec, tr.decoder), (dis, tr.dis)):
        for (k, v), (_, v2) in zip(new.state_dict().items(), old.state_dict().items()):
            assert torch.equal(v, v2), k
    enc2, dec2 = configure_models(c2)
    init_from_ckpt(path, enc2, 'encoder', 'encoder.')
    init_from_ckpt(path, dec2, 'decoder', 'decoder.')
    assert all(torch.equal(a, b) for a, b in zip(enc2.state_dict().values(), tr.encoder.state_dict().values()))
    assert all(torch.equal(a, b) for a, b in zip(dec2.state_dict().values(), tr.decoder.state_dict().values()))
    # the whole state through a second trainer, optimiser moments included (hipops.Adam.load_state_dict)
    torch.manual_seed(3)
    tr2 = build_second_step_trainer(c2, device="cpu")
    state, epoch, step, run_state = load_run_checkpoint(path)
    assert (epoch, step, run_state["seed"]) == (4, 55, 3) and torch.equal(run_state["gen"], raw[RUN_STATE_KEY]["gen"])
    tr2.load_state_dict(state)
    for o_new, o_old in ((tr2.dec_optim, tr.dec_optim), (tr2.dis_optim, tr.dis_optim)):
        for p_new, p_old in zip(o_new.param_groups[0]["params"], o_old.param_groups[0]["params"]):
            assert torch.equal(p_new, p_old)
            s_new, s_old = o_new.state[p_new], o_old.state[p_old]
            assert s_new["step"] == 3 == s_old["step"]
            assert torch.equal(s_new["exp_avg"], s_old["exp_avg"]) and torch.equal(s_new["exp_avg_sq"], s_old["exp_avg_sq"])
    # a first-step trainer owns enc and dec: positions 0 and 1 of the reference's list
    tr1 = build_first_step_trainer(c1, device="cpu")
    _fill_optimizer(tr1.enc_optim, 4)
    p1 = str(tmp_path / "first.ckpt")
    save_run_checkpoint(p1, tr1.state_dict(), 0, 3, {})
    assert torch.load(p1, map_location="cpu")["optimizer_indices"] == [0, 1]
    tr1b = build_first_step_trainer(c1, device="cpu")
    tr1b.load_state_dict(load_run_checkpoint(p1)[0])
    q, q2 = tr1.enc_optim.param_groups[0]["params"][0], tr1b.enc_optim.param_groups[0]["params"][0]
    assert torch.equal(tr1.enc_optim.state[q]["exp_avg"], tr1b.enc_optim.state[q2]["exp_avg"])
    with pytest.raises(NotImplementedError, match="build_second_step_trainer"):
        build_first_step_trainer(c2, device="cpu")


def test_trainer_state_holds_generators_and_the_dropblock_schedule(tmp_path):
    from utils import load_json
    from trainers import build_first_step_trainer
    from run_helpers import AUGMENTATION
    raw = raw_config(tmp_path / "out", augmentation=AUGMENTATION, model=dict(vqmodel=dict(use_dropblock=True, block_size=3, nr_steps=5)))
    c = load_json(write_config(tmp_path / "c.json", raw))
    tr = build_first_step_trainer(c, device="cpu")
    tr.views.t[0]._uniform(3, 0.0, 1.0)
    tr.decoder.dropblock.step()
    tr.decoder.dropblock.step()
    st = tr.state_dict()
    assert st["extra"]["dropblock"]["i"] == 2 and st["extra"]["init_embed"] is True
    nxt = tr.views.t[0]._uniform(4, 0.0, 1.0)
    tr2 = build_first_step_trainer(c, device="cpu")
    tr2.load_state_dict(st)
    assert tr2.decoder.dropblock.i == 2 and tr2.decoder.dropblock.dropblock.drop_prob == tr.decoder.dropblock.dropblock.drop_prob
    assert torch.equal(tr2.views.t[0]._uniform(4, 0.0, 1.0), nxt)


# ---------------------------------------------------------------------------------------------- 6. synthetic dataset
def test_synthetic_dataset_is_a_pure_function_of_seed_and_index(tmp_path):
    from dataio import SyntheticSliceDataset, get_data_loader
    a, b = SyntheticSliceDataset("train", 32, 20, seed=5), SyntheticSliceDataset("train", 32, 20, seed=5)
    x7 = a[7]["image"].clone()
    _ = [a[i] for i in (3, 0, 19)]
    assert torch.equal(a[7]["image"], x7) and torch.equal(b[7]["image"], x7)
    assert x7.shape == (1, 32, 32) and x7.dtype == torch.float32 and float(x7.abs().max()) <= 1.0
    assert not torch.equal(a[8]["image"], x7)
    assert not torch.equal(SyntheticSliceDataset("train", 32, 20, seed=6)[7]["image"], x7)
    assert not torch.equal(SyntheticSliceDataset("val", 32, 20, seed=5)[7]["image"], x7)
    assert len(a) == 20 and set(a[0]) == {"patient_id", "slice_num", "image"}
    with pytest.raises(IndexError):
        a[20]
    dl = get_data_loader("train", "synthetic", None, 4, 0, drop_last=True, image_size=32, n_samples=10, seed=5,
                         generator=torch.Generator().manual_seed(0))
    batches = list(dl)
    assert len(batches) == 2 and batches[0]["image"].shape == (4, 1, 32, 32)
    code = ("import sys; sys.path.insert(0, %r); import dataio, trainers.fit, run_vqwnet; "
            "bad = [m for m in sys.modules if m == 'bench' or m == 'oracle' or m.startswith('oracle.')]; "
            "sys.exit(1 if bad else 0)" % SRC)
    assert subprocess.run([sys.executable, "-c", code], timeout=120).returncode == 0


def test_get_data_loader_takes_a_sampler_and_a_generator(tmp_path):
    from torch.utils.data import SequentialSampler
    from dataio import get_data_loader, SyntheticSliceDataset
    order = lambda seed: [int(s) for b in get_data_loader(  # noqa: E731
        "train", "synthetic", None, 2, 0, image_size=8, n_samples=8, generator=torch.Generator().manual_seed(seed))
        for s in b["slice_num"]]
    assert order(1) == order(1) and sorted(order(1)) == list(range(8))
    ds = SyntheticSliceDataset("train", 8, 8)
    dl = get_data_loader("train", "synthetic", None, 2, 0, image_size=8, n_samples=8, sampler=SequentialSampler(ds))
    assert [int(s) for b in dl for s in b["slice_num"]] == list(range(8))


# ---------------------------------------------------------------------------------------------- 7. operators
def test_export_operators_are_declared_everywhere():
    from hipops import _lib, library
    header = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9 and _lib.load().vqw_abi_version() == 9
    library.register()
    for name in ("vqw_export_grey", "vqw_export_labels"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert hasattr(torch.ops.vqw, name[4:])
    sch = str(torch.ops.vqw.export_grey.default._schema)
    assert "Tensor? x, Tensor? win, Tensor(a!)? out, int nwin, int B, int H, int W, int flip" in sch
    sch = str(torch.ops.vqw.export_labels.default._schema)
    assert "Tensor? ids, Tensor? palette, Tensor(a!)? index_out, Tensor(b!)? rgb, Tensor(c!)? counts, Tensor(d!)? err" in sch
    makefile = open(os.path.join(SRC, "csrc", "Makefile")).read()
    assert "export.hip" in makefile
    # the byte-exact formula needs this file built without contraction of alpha * x + beta into one FMA
    assert "build/export.o: CXXFLAGS += -ffp-contract=off" in makefile


def test_export_arguments_are_checked_before_any_device_work():
    from hipops import ops
    ids = torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="dict_size"):
        ops.export_labels(ids, 65536)
    with pytest.raises(ValueError, match="dict_size"):
        ops.export_labels(ids, 0)
    with pytest.raises(RuntimeError, match="int64"):
        ops.export_labels(ids.int(), 10)
    with pytest.raises(RuntimeError, match=r"\(B, H, W\)"):
        ops.export_labels(ids[0], 10)
    with pytest.raises(ValueError, match="palette"):
        ops.export_labels(ids, 10, palette=np.zeros((10, 3), np.uint8))
    with pytest.raises(ValueError, match="palette"):
        ops.export_labels(ids, 10, palette=np.zeros((11, 3), np.float32))
    with pytest.raises(ValueError, match="palette"):
        ops.export_labels(ids, 10, palette=torch.zeros(11, 4, dtype=torch.uint8))
    x = torch.zeros(2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.export_grey(x.double())
    with pytest.raises(RuntimeError, match=r"\(B, 1, H, W\)"):
        ops.export_grey(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="windows"):
        ops.export_grey(x, windows=(None,) * 9)
    with pytest.raises(ValueError, match="vmax"):
        ops.export_grey(x, vmin=1.0, vmax=1.0)
    with pytest.raises(ValueError, match="window"):
        ops.export_grey(x, windows=((1.0, 0.0),))
    with pytest.raises(RuntimeError, match="ROCm device"):          # all arguments fine: a CPU tensor reaches no kernel
        ops.export_grey(x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.export_labels(ids, 10)
    pal = ops.default_palette(10)
    assert pal.shape == (11, 3) and pal.dtype == np.uint8 and ops.default_palette(1024).shape == (1025, 3)
