"""The run_vqwnet launcher end to end on the GPU: a two-epoch first-step run on a generated CRCDataset tree, bit-exact
resume, the hand-over to the second step, test-mode scoring, the inference export and two ranks on one card.  Every run is
a fresh child process of the launcher under its own time limit (run_helpers.run_launcher); nothing is tried twice."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import AUGMENTATION, MONITORED, make_crc_tree, raw_config, read_csv, run_launcher, write_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, BATCH, N_SLICES = 32, 4, 12
STEPS_PER_EPOCH = N_SLICES // BATCH
SEED = 3                                       # run.seed of run_helpers.raw_config


def _version_dir(save_dir, n=0):
    return os.path.join(str(save_dir), "study", "version_%d" % n)


def _ckpt(save_dir, epoch, n=0):
    return os.path.join(_version_dir(save_dir, n), "ckpt-epoch=%04d-total_loss=0.00.ckpt" % epoch)


def _train(tmp, name, data, timeout=400, env=None, **sections):
    save = os.path.join(str(tmp), name)
    cfg = write_config(os.path.join(str(tmp), name + ".json"), raw_config(save, data, **sections))
    out = run_launcher(cfg, timeout=timeout, env=env)
    return save, out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_crc_tree(tmp_path_factory.mktemp("crc"), n_patients=3, n_slices=N_SLICES // 3, size=SIZE, seed=1)


@pytest.fixture(scope="module")
def first_run(tmp_path_factory, data):
    """Two epochs of the first step; shared by the tests that only read its files."""
    tmp = tmp_path_factory.mktemp("first")
    save, out = _train(tmp, "run", data)
    return dict(tmp=tmp, save=save, out=out, data=data)


# ---------------------------------------------------------------------------------------------- 9
def test_two_epoch_first_step_run(first_run):
    vdir = _version_dir(first_run["save"])
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert header == MONITORED
    assert len(rows) == 2 * STEPS_PER_EPOCH              # log_every_n_steps = 1
    for i, row in enumerate(rows):
        rec = dict(zip(header, row))
        assert int(rec["epoch"]) == i // STEPS_PER_EPOCH and int(rec["iteration"]) == i
        for k in ("total", "gen_total", "commit", "cross", "dist", "reg", "recon", "freq", "perceptual"):
            assert np.isfinite(float(rec[k])), (k, rec[k])
        assert rec["gen"] == "" and rec["dis_total"] == "" and rec["dis"] == ""      # not produced by the first step
        assert float(rec["total"]) == float(rec["gen_total"]) and float(rec["freq"]) == 0.0
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(vdir, "*.ckpt"))) == \
        ["ckpt-epoch=0000-total_loss=0.00.ckpt", "ckpt-epoch=0001-total_loss=0.00.ckpt"]
    from utils import png
    for epoch in (0, 1):
        pixels, _ = png.load(os.path.join(vdir, "%06d.png" % epoch))
        assert pixels.shape == (3 * SIZE, 3 * SIZE, 3)   # n_save_images = 3 rows; CRC: image, recon, ids
        ids_tile = pixels[:SIZE, 2 * SIZE:]
        from hipops import ops
        pal = {tuple(c) for c in ops.default_palette(10)}
        assert {tuple(c) for c in ids_tile.reshape(-1, 3)} <= pal
        grey = pixels[:SIZE, :SIZE]
        assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 0] == grey[..., 2]).all()
    saved = json.load(open(os.path.join(vdir, "config.json")))
    assert saved["seed_list"] == [11] and saved["save_dir_path"].endswith("version_0")
    assert first_run["out"].count("IDs: ") == 2 * 2       # two validation batches after each epoch
    ck = torch.load(_ckpt(first_run["save"], 1), map_location="cpu")
    assert ck["epoch"] == 1 and ck["global_step"] == 2 * STEPS_PER_EPOCH and ck["optimizer_indices"] == [0, 1]


# ---------------------------------------------------------------------------------------------- 10
def _tensors(obj, prefix=""):
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _tensors(v, "%s/%s" % (prefix, k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, "%s/%d" % (prefix, i))


def _differences(path_a, path_b):
    a, b = torch.load(path_a, map_location="cpu"), torch.load(path_b, map_location="cpu")
    diff = []
    for key in ("state_dict", "optimizer_states"):
        ta, tb = dict(_tensors(a[key])), dict(_tensors(b[key]))
        assert ta.keys() == tb.keys()
        diff += ["%s%s" % (key, k) for k in ta if not torch.equal(ta[k], tb[k])]
        steps = lambda c: [s["step"] for o in c["optimizer_states"] for s in o["state"].values()]  # noqa: E731
        assert steps(a) == steps(b)
    return diff


@pytest.mark.parametrize("variant", ["flip_noise", "augmentation", "dropblock"])
def test_resume_is_bit_exact(tmp_path, data, variant):
    sections = {"flip_noise": {}, "augmentation": {"augmentation": AUGMENTATION},
                "dropblock": {"model": {"vqmodel": {"use_dropblock": True, "block_size": 3, "start_value": 0.1,
                                                    "stop_value": 0.3, "nr_steps": 4}}}}[variant]
    full_a, _ = _train(tmp_path, "full_a", data, **sections)
    full_b, _ = _train(tmp_path, "full_b", data, **sections)
    # the precondition: the run itself is bit-deterministic
    diff = _differences(_ckpt(full_a, 1), _ckpt(full_b, 1))
    assert not diff, "two identical runs differ in %d tensors, e.g. %s" % (len(diff), diff[:5])
    assert open(os.path.join(_version_dir(full_a), "log.csv")).read() == open(os.path.join(_version_dir(full_b), "log.csv")).read()
    # one epoch, stop, resume for the second
    part = os.path.join(str(tmp_path), "part")
    run1 = raw_config(part, data, **sections)
    run1["run"]["n_epochs"] = 1
    run_launcher(write_config(os.path.join(str(tmp_path), "part1.json"), run1))
    diff = _differences(_ckpt(part, 0), _ckpt(full_a, 0))
    assert not diff, "the first epoch alone differs from the first epoch of the long run: %s" % diff[:5]
    run2 = raw_config(part, data, **sections)
    run2["run"].update(n_epochs=2, resume_checkpoint=_ckpt(part, 0))
    run_launcher(write_config(os.path.join(str(tmp_path), "part2.json"), run2))
    assert os.path.isdir(_version_dir(part, 1))          # a resumed run gets a new version directory
    diff = _differences(_ckpt(part, 1, n=1), _ckpt(full_a, 1))
    assert not diff, "resumed run differs from the uninterrupted one in %d tensors, e.g. %s" % (len(diff), diff[:8])
    _, rows_full = read_csv(os.path.join(_version_dir(full_a), "log.csv"))
    _, rows_resumed = read_csv(os.path.join(_version_dir(part, 1), "log.csv"))
    assert rows_resumed == rows_full[STEPS_PER_EPOCH:]


# ---------------------------------------------------------------------------------------------- 11
def test_first_step_checkpoint_feeds_the_second_step(tmp_path, first_run):
    first = _ckpt(first_run["save"], 1)
    save, _ = _train(tmp_path, "second", first_run["data"],
                     run=dict(training_mode="second_step", n_epochs=1, first_stage_ckpt_path=first))
    ck = torch.load(_ckpt(save, 0), map_location="cpu")
    ref = torch.load(first, map_location="cpu")
    enc = [k for k in ref["state_dict"] if k.startswith("encoder.")]
    assert enc and all(torch.equal(ck["state_dict"][k], ref["state_dict"][k]) for k in enc)     # frozen encoder
    assert any(k.startswith("dis.") for k in ck["state_dict"]) and ck["optimizer_indices"] == [1, 2]
    dec = [k for k in ref["state_dict"] if k.startswith("decoder.") and k.endswith("weight")]
    assert any(not torch.equal(ck["state_dict"][k], ref["state_dict"][k]) for k in dec)         # the decoder trained
    header, rows = read_csv(os.path.join(_version_dir(save), "log.csv"))
    assert len(rows) == STEPS_PER_EPOCH
    for row in rows:
        rec = dict(zip(header, row))
        assert rec["commit"] == "" and rec["cross"] == ""
        for k in ("total", "gen_total", "recon", "gen", "dis_total", "dis"):
            assert np.isfinite(float(rec[k])), (k, rec[k])
        assert np.float32(rec["total"]) == np.float32(rec["gen_total"]) + np.float32(rec["dis_total"])


# ---------------------------------------------------------------------------------------------- 12, 13
def _loaded_models(config, ckpt):
    from trainers import InferenceModels
    from utils.checkpoint import load_run_checkpoint
    models = InferenceModels(config, device=DEV)
    state = load_run_checkpoint(ckpt)[0]
    models.load_state_dict({"modules": {k: state["modules"][k] for k in ("encoder", "decoder")}, "optimizers": {},
                            "extra": {"init_embed": True}})
    return models


def test_test_mode_writes_the_evaluators_result(tmp_path, first_run):
    from utils import load_json
    from trainers import Evaluator, build_loader
    ckpt = _ckpt(first_run["save"], 1)
    save = os.path.join(str(tmp_path), "score")
    cfg = write_config(os.path.join(str(tmp_path), "score.json"), raw_config(save, first_run["data"], run=dict(resume_checkpoint=ckpt)))
    run_launcher(cfg, "-m", "test")
    got = open(os.path.join(_version_dir(save), "result.csv")).read()
    config = load_json(cfg)
    models = _loaded_models(config, ckpt)
    direct = os.path.join(str(tmp_path), "direct")
    Evaluator(models.encoder, models.decoder, 10).run(build_loader(config, "test", SEED), direct)
    assert got == open(os.path.join(direct, "result.csv")).read()
    assert got.splitlines()[0] == ",NMSE_avg,NMSE_std,SSIM_avg,SSIM_std,PSNR_avg,PSNR_std,Entropy_avg,Entropy_std"


def test_inference_export_and_the_editing_loop(tmp_path, first_run):
    from utils import load_json, png
    from hipops import ops
    from trainers import build_loader
    import run_recon
    ckpt = _ckpt(first_run["save"], 1)
    save = os.path.join(str(tmp_path), "exp")
    raw = raw_config(save, first_run["data"], run=dict(training_mode="inference", resume_checkpoint=ckpt))
    cfg = write_config(os.path.join(str(tmp_path), "exp.json"), raw)
    run_launcher(cfg, "-m", "test")
    root = os.path.join(save, "study")
    assert sorted(os.listdir(root)) == ["patient00", "patient01", "patient02"]
    for p in os.listdir(root):
        assert sorted(os.listdir(os.path.join(root, p))) == sorted(
            "%s_%04d.%s" % (stem, s, ext) for stem in ("image", "recon", "label") for s in range(N_SLICES // 3)
            for ext in ("png", "nii.gz"))
    config = load_json(cfg)
    models = _loaded_models(config, ckpt)
    palette = ops.default_palette(10)
    checked = 0
    for batch in build_loader(config, "test", SEED):
        image = batch["image"].to(DEV)
        with torch.no_grad():
            embed, _, ids = models.encoder(image)
            recon = models.decoder(embed)
        assert int(ids.min()) >= 1 and int(ids.max()) <= 10
        grey_i = ops.export_grey(image, flip=True)[0].cpu().numpy()
        grey_r = ops.export_grey(recon, flip=True)[0].cpu().numpy()
        lab = ops.export_labels(ids, 10, palette=palette, flip=True)
        for i in range(image.shape[0]):
            d = os.path.join(root, batch["patient_id"][i])
            num = "%04d" % int(batch["slice_num"][i])
            assert np.array_equal(png.load(os.path.join(d, "image_%s.png" % num))[0], grey_i[i])
            assert np.array_equal(png.load(os.path.join(d, "recon_%s.png" % num))[0], grey_r[i])
            assert np.array_equal(png.load(os.path.join(d, "label_%s.png" % num))[0], lab.rgb[i].cpu().numpy())
            # float NIfTI = the eval forward, CRC: flipped upside down like the PNGs
            img_f = run_recon.load_from_nifti(os.path.join(d, "image_%s.nii.gz" % num))
            rec_f = run_recon.load_from_nifti(os.path.join(d, "recon_%s.nii.gz" % num))
            lab_f = run_recon.load_from_nifti(os.path.join(d, "label_%s.nii.gz" % num))
            assert np.array_equal(img_f.astype(np.float32), np.flipud(image[i, 0].cpu().numpy()))
            assert np.array_equal(rec_f.astype(np.float32), np.flipud(recon[i, 0].cpu().numpy()))
            assert np.array_equal(lab_f.astype(np.int64), np.flipud(ids[i].cpu().numpy()))
            assert np.array_equal(lab_f.astype(np.int64), lab.index[i].cpu().numpy().astype(np.int64))
            # the editing loop closed: the exported, unedited label map reconstructs the exported reconstruction
            again = run_recon.reconstruct_file(models.encoder, models.decoder, os.path.join(d, "label_%s.nii.gz" % num),
                                               flipud=True, device=DEV)
            differing = int((again != rec_f.astype(np.float32)).sum())
            print("reconstruct_file vs exported recon, %s/%s: %d differing pixels, max |diff| %.3g"
                  % (batch["patient_id"][i], num, differing, float(np.abs(again - rec_f).max())))
            assert np.array_equal(again, rec_f.astype(np.float32))
            checked += 1
    assert checked == N_SLICES


# ---------------------------------------------------------------------------------------------- 14
def test_two_ranks_on_one_card(tmp_path, data):
    digest = os.path.join(str(tmp_path), "digest")
    save, out = _train(tmp_path, "dp", data, timeout=500, env={"VQW_DP_ONE_DEVICE": "1", "VQW_RUN_DIGEST": digest},
                       run=dict(num_gpus=2, n_epochs=1))
    ranks = [json.load(open("%s.rank%d.json" % (digest, r))) for r in (0, 1)]
    assert ranks[0]["modules"] == ranks[1]["modules"] and set(ranks[0]["modules"]) == {"encoder", "decoder"}
    seen = [set(i for _, idx in r["seen"] for i in idx) for r in ranks]
    assert all(len(r["seen"]) == 1 and r["seen"][0][0] == 0 for r in ranks)
    assert not (seen[0] & seen[1]) and (seen[0] | seen[1]) == set(range(N_SLICES)) and len(seen[0]) == len(seen[1])
    assert os.listdir(os.path.join(save, "study")) == ["version_0"]          # rank 0 alone wrote
    vdir = _version_dir(save)
    header, rows = read_csv(os.path.join(vdir, "log.csv"))
    assert len(rows) == (N_SLICES // 2) // BATCH
    assert os.path.exists(_ckpt(save, 0)) and os.path.exists(os.path.join(vdir, "000000.png"))
    assert json.load(open(os.path.join(vdir, "config.json")))["seed_list"] == [11, 12]
    assert "Seed set to 11 in gpu-rank: 0" in out and "Seed set to 12 in gpu-rank: 1" in out
