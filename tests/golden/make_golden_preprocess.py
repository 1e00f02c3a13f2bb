"""Writes tests/golden/preprocess.npz: tiny synthetic volumes and the slices the reference's preprocessing makes of them.

Development container only (it needs PIL and a checkout of the reference; no test imports either):

    python tests/golden/make_golden_preprocess.py --reference <reference checkout>/src/preprocess

The expected slices come from the reference's own functions, imported under stand-ins for the packages its scripts import
at module level (nibabel, dotenv, matplotlib, tqdm): `minmax_normalize` and `parse_patient_id` of preprocess_crc.py and
make_crc_testing_dataset.py, `z_score_normalize` and `preprocess` (with IMAGE_SIZE set small) of preprocess_brats.py; the
loops under `if __name__ == '__main__'` cannot be imported, so the orientation (img[::-1], np.rot90) and the file naming
of the CRC scripts are applied here; every resize is PIL's.  This file also checks tests/preprocess_ref.py against PIL
bit for bit before it writes anything.

Keys of the fixture:
  cases            JSON list of {id, kind, vol, slope, inter, norm, orient, size, relabel}
  vol/<name>       (X, Y, Z) volume in its stored dtype
  out/<id>         (Z, size, size) expected slices (float32; int32 for kind 'label')
  wide/<id>, D/<id>   z-score cases: the same pipeline with mean and std taken in float64 and rounded once to float32, and
                   D = max |out - wide| > 0: how far float32 statistics move the slices
  commands         JSON: per command the input files (file name -> vol key, slope, inter), its arguments and the tree it
                   must write (relative path -> tree/<n> key); for the z-scored files of preprocess_brats also D (relative
                   path -> D of that file's volume, as above)
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, os.path.join(ROOT, "medical-image-editing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import preprocess_ref as R            # noqa: E402
from utils import nifti               # noqa: E402

DTYPES = ("uint8", "int16", "uint16", "int32", "float32", "float64")


def stand_ins():
    """Modules the reference's scripts import at module level and this file does not need."""
    nib = types.ModuleType("nibabel")

    class _Image:
        def __init__(self, path):
            self.raw, self.slope, self.inter, _ = nifti.load_raw(path)

        def get_data(self):
            if self.slope not in (0.0, 1.0) or self.inter != 0.0:
                return R.scaled(self.raw, self.slope, self.inter)
            return self.raw.copy()

        def get_fdata(self):
            return R.scaled(self.raw, self.slope, self.inter)

    nib.load = _Image
    sys.modules["nibabel"] = nib
    dotenv = types.ModuleType("dotenv")
    dotenv.load_dotenv = lambda *a, **k: None
    sys.modules["dotenv"] = dotenv
    for name in ("matplotlib", "matplotlib.pyplot", "tqdm"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.tqdm = lambda x, *a, **k: x
            sys.modules[name] = m
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]


def reference_module(directory, name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(directory, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def volume(g, dtype, shape):
    """Smooth-ish positive and negative values with a background of zeros, in the range of the dtype."""
    x = g.standard_normal(shape) * 300.0 + 200.0
    x[g.random(shape) < 0.25] = 0.0
    if dtype == "uint8":
        x = np.clip(np.abs(x) / 4.0, 0, 255)
    elif dtype == "uint16":
        x = np.abs(x) * 40.0
    elif dtype == "int32":
        x = x * 70000.0
    elif dtype in ("float32", "float64"):
        x = x * 1.2345678
    return np.asfortranarray(x.astype(dtype))


def pil_resize(slices, size, resample):
    return np.stack([np.array(Image.fromarray(s).resize((size, size), resample=resample)) for s in slices])


def oriented(vol, how):
    out = []
    for i in range(vol.shape[2]):
        s = vol[..., i]
        if how == "crc":
            s = np.rot90(s[::-1, ...])
        elif how == "brats":
            s = np.rot90(s, k=3)
        out.append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's src/preprocess directory")
    ap.add_argument("--out", default=os.path.join(HERE, "preprocess.npz"))
    args = ap.parse_args()
    stand_ins()
    crc = reference_module(args.reference, "preprocess_crc")
    heldout = reference_module(args.reference, "make_crc_testing_dataset")
    brats = reference_module(args.reference, "preprocess_brats")

    g = np.random.default_rng(20261017)
    z, cases = {}, []

    def add(kind, vol, size, norm=None, orient=None, slope=1.0, inter=0.0, relabel=False):
        cid = "%s-%s-%s-%s-%d%s" % (kind, vol, norm, orient, size, "-relabel" if relabel else "")
        cases.append(dict(id=cid, kind=kind, vol=vol, slope=slope, inter=inter, norm=norm, orient=orient, size=size,
                          relabel=relabel))
        return cid

    # the restatement against PIL itself, at the sizes of the issue and at odd ones
    for h, w, s in [(240, 240, 256), (600, 600, 512), (512, 512, 512), (287, 333, 512), (768, 1024, 512), (37, 53, 50)]:
        a = (g.standard_normal((h, w)) * 100).astype(np.float32)
        assert np.array_equal(pil_resize([a], s, Image.BILINEAR)[0].view(np.uint32), R.resize_bilinear(a, s).view(np.uint32))
        lab = g.integers(0, 5, size=(h, w)).astype(np.int32)
        assert np.array_equal(pil_resize([lab], s, Image.NEAREST)[0], R.resize_nearest(lab, s))

    # ---- bilinear, exact: non-square 20 x 14 x 2 up to 24 and down to 9 (20 / 9, 14 / 9), square 12 x 12 x 2 kept at 12
    scalings = {d: (1.0, 0.0) for d in DTYPES}
    scalings["int16s"] = (float(np.float32(0.0123)), -3.5)
    for d in DTYPES + ("int16s",):
        z["vol/rect_" + d] = volume(g, d[:5] if d == "int16s" else d, (20, 14, 2))
        z["vol/square_" + d] = volume(g, d[:5] if d == "int16s" else d, (12, 12, 2))
        slope, inter = scalings[d]
        for how in (None, "crc", "brats"):
            for vol, size in (("rect_" + d, 24), ("rect_" + d, 9), ("square_" + d, 12)):
                v = R.scaled(z["vol/" + vol], slope, inter)
                cid = add("bilinear", vol, size, "minmax", how, slope, inter)
                z["out/" + cid] = pil_resize(oriented(crc.minmax_normalize(v.copy()), how), size, Image.BILINEAR)
        cid = add("bilinear", "rect_" + d, 9, None, None, slope, inter)
        z["out/" + cid] = pil_resize(oriented(R.scaled(z["vol/rect_" + d], slope, inter), None), 9, Image.BILINEAR)

    # ---- z-score: 40 x 32 x 3, volumes drawn until float32 statistics move the slices (D > 0)
    for d in DTYPES + ("int16s",):
        slope, inter = scalings[d]
        for size in ((44, 21) if d == "int16" else (21,)):
            while True:
                raw = volume(g, d[:5] if d == "int16s" else d, (40, 32, 3))
                v = R.scaled(raw, slope, inter) if d == "int16s" else raw
                ref = pil_resize(oriented(brats.z_score_normalize(v), "brats"), size, Image.BILINEAR)
                wide = pil_resize(oriented(R.z_score_normalize(v, wide_statistics=True), "brats"), size, Image.BILINEAR)
                D = float(np.max(np.abs(ref.astype(np.float64) - wide.astype(np.float64))))
                if D > 0:
                    break
            name = "z%d_%s" % (size, d)
            z["vol/" + name] = raw
            cid = add("zscore", name, size, "zscore", "brats", slope, inter)
            z["out/" + cid], z["wide/" + cid], z["D/" + cid] = ref, wide, np.float64(D)

    # ---- labels, nearest
    z["vol/lab_rect"] = np.asfortranarray(g.choice(np.array([0, 1, 2, 4], dtype=np.int32), size=(20, 14, 2)))
    z["vol/lab_square"] = np.asfortranarray(g.choice(np.array([0, 1, 2, 4], dtype=np.int32), size=(12, 12, 2)))
    for how in (None, "crc", "brats"):
        for vol, size in (("lab_rect", 24), ("lab_rect", 9), ("lab_square", 12)):
            for relabel in (False, True):
                lab = z["vol/" + vol].copy()
                if relabel:
                    lab[lab == 4] = 3
                cid = add("label", vol, size, None, how, relabel=relabel)
                z["out/" + cid] = pil_resize(oriented(lab, how), size, Image.NEAREST)
                assert z["out/" + cid].dtype == np.int32

    # ---- the commands
    commands, trees = {}, []

    def tree_key(array):
        trees.append(array)
        z["tree/%d" % (len(trees) - 1)] = array
        return "tree/%d" % (len(trees) - 1)

    crc_files = {"CRC_0001_image.nii.gz": ("rect_int16", 1.0, 0.0), "CRC_0002_image.nii.gz": ("rect_float32", 1.0, 0.0),
                 "CRC_0003_image.nii.gz": ("rect_int16s",) + scalings["int16s"], "CRC_0004_mask.nii.gz": ("lab_rect", 1.0, 0.0)}
    size = 16
    for name, module, train in (("preprocess_crc", crc, None), ("make_crc_testing_dataset", heldout, ["CRC_0001", "OTHER_7"])):
        tree = {}
        for fname, (vol, slope, inter) in sorted(crc_files.items()):
            if not fname.endswith("_image.nii.gz"):
                continue
            patient = module.parse_patient_id(os.path.join("/somewhere", fname))
            if train is not None and patient in train:
                continue
            image = module.minmax_normalize(R.scaled(z["vol/" + vol], slope, inter))
            for i, s in enumerate(pil_resize(oriented(image, "crc"), size, Image.BILINEAR)):
                tree[patient + "/" + str(i).zfill(4) + ".npy"] = tree_key(s)
        commands[name] = dict(files={k: list(v) for k, v in crc_files.items()}, image_size=size, train=train, tree=tree)

    # BraTS: the reference's own `preprocess`, reading files this script writes, IMAGE_SIZE set small
    brats.IMAGE_SIZE = 20
    brats_files, tree, brats_D = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for group, patient in (("MICCAI_BraTS_Training_HGG", "BraTS19_AAA_1"), ("held_back_LGG", "BraTS19_BBB_1")):
            os.makedirs(os.path.join(tmp, "src", group, patient))
            for m in ("t1", "t1ce", "t2", "flair", "seg"):
                key = "brats_%s_%s" % (patient, m)
                if m == "seg":
                    z["vol/" + key] = np.asfortranarray(g.choice(np.array([0, 1, 2, 4], dtype=np.uint8), size=(24, 24, 3)))
                else:                                  # drawn until float32 statistics move the slices, as above
                    while True:
                        raw = volume(g, "int16", (24, 24, 3))
                        ref = pil_resize(oriented(brats.z_score_normalize(raw), "brats"), 20, Image.BILINEAR)
                        wide = pil_resize(oriented(R.z_score_normalize(raw, wide_statistics=True), "brats"), 20, Image.BILINEAR)
                        D = float(np.max(np.abs(ref.astype(np.float64) - wide.astype(np.float64))))
                        if D > 0:
                            break
                    z["vol/" + key] = raw
                    for i in range(3):
                        brats_D["%s/%s_%s_%s.npy" % (patient, patient, m, str(i).zfill(4))] = D
                rel = os.path.join(group, patient, "%s_%s.nii.gz" % (patient, m))
                brats_files[rel] = [key, 1.0, 0.0]
                R.save_nifti(os.path.join(tmp, "src", rel), z["vol/" + key])
            config = dict(src_dir_path=os.path.join(tmp, "src", group), dst_dir_path=os.path.join(tmp, "dst"),
                          modalities=brats.train_dataset_config_1["modalities"])
            brats.preprocess(patient, config)
        for dirpath, _, names in os.walk(os.path.join(tmp, "dst")):
            for n in sorted(names):
                rel = os.path.relpath(os.path.join(dirpath, n), os.path.join(tmp, "dst"))
                tree[rel] = tree_key(np.load(os.path.join(dirpath, n)))
    commands["preprocess_brats"] = dict(files=brats_files, image_size=20, tree=tree, D=brats_D,
                                        srcs=["MICCAI_BraTS_Training_HGG", "held_back_LGG"])

    z["cases"] = np.array(json.dumps(cases))
    z["commands"] = np.array(json.dumps(commands))
    np.savez_compressed(args.out, **z)
    print("%s: %d cases, %d tree files, %d bytes" % (args.out, len(cases), len(trees), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
