"""Shared by test_run_host.py and test_gpu_run.py: a small run config on top of configs/baseline1, a generated CRCDataset
tree, and the launcher as a child process."""
import copy
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "medical-image-editing_amd")
LAUNCHER = os.path.join(SRC, "run_vqwnet.py")
MONITORED = ["epoch", "iteration", "total", "gen_total", "commit", "cross", "dist", "reg", "recon", "freq", "perceptual",
             "gen", "dis_total", "dis"]
AUGMENTATION = {
    "modules": ["RandomHorizontalFlip", "RandomAffine", "ColorJitter", "RandomGaussianNoise"],
    "RandomHorizontalFlip": {"p": 0.5},
    "RandomAffine": {"p": 0.8, "degrees": 10.0, "translate": [0.05, 0.05], "shear": 2.0},
    "ColorJitter": {"p": 0.8, "brightness": 0.1, "contrast": 0.1},
    "RandomGaussianNoise": {"p": 0.5, "std": 0.02},
}


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v
    return dst


def raw_config(save_dir, data_root=None, **sections):
    """baseline1 with small filters, every loggable key monitored, a row logged every step and four pictures per epoch;
    `sections` are merged over it section by section."""
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline1_cpu_32x32_b4.json")))
    raw["model"]["vqmodel"].update(enc_filters=[16, 32, 32, 64, 64], dec_filters=[32, 32, 64, 64, 128])
    raw["model"]["dis"].update(n_filters=8, n_layers=2)
    raw["run"].update(monitoring_metrics=list(MONITORED), log_every_n_steps=1, n_epochs=2, seed=3, seed_list=[11, 12])
    raw["save"].update(save_dir=str(save_dir), study_name="study", n_save_images=3)
    if data_root is not None:
        raw["dataset"].update(dataset_name="CRCDataset", root_dir_path=str(data_root), batch_size=4)
    return _merge(raw, copy.deepcopy(sections))


def write_config(path, raw):
    with open(path, "w") as f:
        json.dump(raw, f)
    return str(path)


def make_crc_tree(root, n_patients=3, n_slices=4, size=32, seed=0):
    """<root>/<patient>/<slice>.npy: smooth 0..255 slices as the CRC loader expects them."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    for p in range(n_patients):
        d = os.path.join(str(root), "patient%02d" % p)
        os.makedirs(d, exist_ok=True)
        for s in range(n_slices):
            a, b, c = g.uniform(1.0, 4.0, size=3)
            img = 127.5 + 100.0 * np.sin(a * xx * 3.1 + c) * np.cos(b * yy * 2.7) + g.normal(0.0, 6.0, size=(size, size))
            np.save(os.path.join(d, "%d.npy" % s), np.clip(img, 0, 255).astype(np.float32))
    return str(root)


def run_launcher(config_path, *extra, timeout=400, env=None):
    """The launcher as a fresh child process under its own time limit -> its output; a time-out or a non-zero exit fails
    the calling test with the tail of the output (nothing is tried again)."""
    p = subprocess.Popen([sys.executable, LAUNCHER, "-c", str(config_path)] + list(extra), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, env=dict(os.environ, **(env or {})))
    try:
        out = p.communicate(timeout=timeout)[0].decode(errors="replace")
    except subprocess.TimeoutExpired:
        p.kill()
        out = p.communicate()[0].decode(errors="replace")
        raise AssertionError("run_vqwnet.py %s: no exit within %d s\n%s" % (" ".join(extra), timeout, out[-3000:]))
    assert p.returncode == 0, "run_vqwnet.py %s: exit status %d\n%s" % (" ".join(extra), p.returncode, out[-3000:])
    return out


def read_csv(path):
    with open(path) as f:
        rows = [line.rstrip("\n").split(",") for line in f]
    return rows[0], rows[1:]
