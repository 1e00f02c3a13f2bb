"""The preprocess kernels (hipops.ops.volume_stats / volume_to_slices / label_volume_to_slices, csrc/resample.hip) and the
three commands on the device, against the fixture made with the reference's functions and PIL.

Bilinear and nearest outputs are compared bit for bit: every operation of the kernels is one IEEE double or float
multiply, add, subtract or divide in PIL's order, so there is no tolerance.  The statistics are sums in another order than
numpy's: the masked mean and deviation are held to n * 2^-53 relative, the worst case of any summation order of n terms;
z-scored slices to 2 D, D being how far the reference's float32 statistics move them (stored with the fixture)."""
import json
import os

import numpy as np
import pytest
import torch

import preprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(raw):
    """(X, Y, Z) as the file holds it -> the (Z, Y, X) device tensor the operators take."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(raw).T)).to(DEV)


def _cases(golden, kind):
    z = golden("preprocess.npz")
    return z, [c for c in json.loads(str(z["cases"])) if c["kind"] == kind]


def test_bilinear_is_bit_equal_under_every_orientation_and_dtype(golden):
    from hipops import ops
    z, cases = _cases(golden, "bilinear")
    seen = set()
    for c in cases:
        raw = z["vol/" + c["vol"]]
        got = ops.volume_to_slices(_dev(raw), c["size"], norm=c["norm"], orient=c["orient"], slope=c["slope"],
                                   inter=c["inter"]).cpu().numpy()
        want = z["out/" + c["id"]]
        assert got.dtype == np.float32 and got.shape == want.shape, c["id"]
        bad = int((_bits(got) != _bits(want)).sum())
        print(c["id"], "differing", bad, "max abs", float(np.abs(got.astype(np.float64) - want).max()))
        assert bad == 0, c["id"]
        kind = "keep" if raw.shape[0] == raw.shape[1] == c["size"] else "up" if c["size"] > raw.shape[0] else "down"
        seen.add((str(raw.dtype), c["orient"], kind))
    for d in ("uint8", "int16", "uint16", "int32", "float32", "float64"):
        for o in (None, "crc", "brats"):
            for kind in ("up", "down", "keep"):
                assert (d, o, kind) in seen, (d, o, kind)


def test_labels_are_bit_equal_and_relabelled(golden):
    from hipops import ops
    z, cases = _cases(golden, "label")
    assert {(c["orient"], c["relabel"]) for c in cases} == {(o, r) for o in (None, "crc", "brats") for r in (False, True)}
    for c in cases:
        got = ops.label_volume_to_slices(_dev(z["vol/" + c["vol"]]), c["size"], orient=c["orient"], relabel=c["relabel"])
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, z["out/" + c["id"]]), c["id"]
    lab = z["vol/lab_rect"].copy()
    lab[3, 2, 1] = 3
    with pytest.raises(ValueError, match="label 3"):
        ops.label_volume_to_slices(_dev(lab), 9, orient="brats", relabel=True)
    kept = ops.label_volume_to_slices(_dev(lab), 24, orient="brats", relabel=False).cpu().numpy()
    assert 3 in kept and 4 in kept


def _check_stats(raw, slope, inter, name):
    from hipops import ops
    s1 = ops.volume_stats(_dev(raw), slope, inter).cpu().numpy()
    s2 = ops.volume_stats(_dev(raw), slope, inter).cpu().numpy()
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64)), name          # the same bits every run
    v = R.scaled(raw, slope, inter)
    assert s1[0] == v.min() and s1[1] == v.max(), (name, s1[:2], v.min(), v.max())
    f = v.astype(np.float32)
    sel = f[f > 0].astype(np.float64)
    mean, std = float(np.mean(sel)), float(np.std(sel))
    bound = raw.size * 2.0 ** -53
    print(name, "n", raw.size, "mean rel", abs(s1[3] - mean) / abs(mean), "std rel", abs(s1[4] - std) / std, "bound", bound)
    assert s1[2] == sel.size, name
    assert abs(s1[3] - mean) <= bound * abs(mean), name
    assert abs(s1[4] - std) <= bound * std, name


def test_statistics(golden):
    z = golden("preprocess.npz")
    cases = json.loads(str(z["cases"]))
    done = set()
    for c in cases:
        if c["kind"] != "label" and c["vol"] not in done:
            done.add(c["vol"])
            _check_stats(z["vol/" + c["vol"]], c["slope"], c["inter"], c["vol"])
    assert len(done) >= 7 * 2 + 8


def test_zscore_slices_are_within_twice_the_statistics_effect(golden):
    from hipops import ops
    z, cases = _cases(golden, "zscore")
    assert {str(z["vol/" + c["vol"]].dtype) for c in cases} == {"uint8", "int16", "uint16", "int32", "float32", "float64"}
    for c in cases:
        D = float(z["D/" + c["id"]])
        got = ops.volume_to_slices(_dev(z["vol/" + c["vol"]]), c["size"], norm="zscore", orient="brats", slope=c["slope"],
                                   inter=c["inter"]).cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - z["out/" + c["id"]]).max())
        wide = int((_bits(got) != _bits(z["wide/" + c["id"]])).sum())
        print(c["id"], "D", D, "max abs", err, "pixels differing from the float64-statistics pipeline", wide)
        assert D > 0 and err <= 2 * D, c["id"]


def _command(golden, name):
    z = golden("preprocess.npz")
    return z, json.loads(str(z["commands"]))[name]


def test_preprocess_crc_on_the_device(golden, tmp_path):
    from preprocess import preprocess_crc
    z, spec = _command(golden, "preprocess_crc")
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    R.write_sources(z, spec, src)
    preprocess_crc.main(["--src", src, "--dst", dst, "--image-size", str(spec["image_size"])])
    R.assert_tree(z, spec, dst)


def test_make_crc_testing_dataset_on_the_device(golden, tmp_path):
    from preprocess import make_crc_testing_dataset
    z, spec = _command(golden, "make_crc_testing_dataset")
    cand, train, dst = str(tmp_path / "cand"), str(tmp_path / "train"), str(tmp_path / "dst")
    R.write_sources(z, spec, cand)
    for p in spec["train"]:
        os.makedirs(os.path.join(train, p))
    make_crc_testing_dataset.main(["--train", train, "--candidates", cand, "--dst", dst, "--image-size",
                                   str(spec["image_size"]), "--expect-train-patients", "2"])
    R.assert_tree(z, spec, dst)


def test_preprocess_brats_on_the_device(golden, tmp_path):
    from preprocess import preprocess_brats
    z, spec = _command(golden, "preprocess_brats")
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    R.write_sources(z, spec, src)
    argv = ["--dst", dst, "--image-size", str(spec["image_size"])]
    for s in spec["srcs"]:
        argv += ["--src", os.path.join(src, s)]
    preprocess_brats.main(argv)
    R.assert_tree(z, spec, dst)


def test_full_size_volume_is_reproducible_and_equals_the_restatement():
    """A 512 x 512 x 64 int16 CT-like volume to 512^2 (both passes keep their size) and to 256^2."""
    from hipops import ops
    g = np.random.default_rng(11)
    raw = np.empty((512, 512, 64), dtype=np.int16, order="F")
    for k in range(64):                                # smooth structure plus noise, in the range of CT numbers
        yy, xx = np.meshgrid(np.arange(512), np.arange(512))
        raw[..., k] = (600.0 * np.sin(xx / 37.0 + k / 5.0) * np.cos(yy / 53.0) + g.standard_normal((512, 512)) * 150.0 - 300.0)
    vol = _dev(raw)
    _check_stats(raw, 1.0, 0.0, "full size")
    for size in (512, 256):
        a = ops.volume_to_slices(vol, size, norm="minmax", orient="crc").cpu().numpy()
        b = ops.volume_to_slices(vol, size, norm="minmax", orient="crc").cpu().numpy()
        assert a.shape == (64, size, size) and np.array_equal(_bits(a), _bits(b)), size
        assert float(a.min()) >= 0.0 and float(a.max()) <= 255.0
        want = R.image_slices(raw, 1.0, 0.0, size, "minmax", "crc", only=(5, 63))
        assert np.array_equal(_bits(a[[5, 63]]), _bits(want)), size
    lab = (np.abs(raw) // 400).astype(np.int32)        # labels 0..3: 3 is present, so no relabel here
    got = ops.label_volume_to_slices(_dev(lab), 256, orient="brats").cpu().numpy()
    assert np.array_equal(got[[0, 40]], R.label_slices(np.asfortranarray(lab[..., [0, 40]]), 256, "brats", False))
    z = ops.volume_to_slices(vol, 256, norm="zscore", orient="brats").cpu().numpy()
    z2 = ops.volume_to_slices(vol, 256, norm="zscore", orient="brats").cpu().numpy()
    assert np.array_equal(_bits(z), _bits(z2)) and np.isfinite(z).all()
