"""Time of the preprocess kernels (csrc/resample.hip) on a full-size volume, of a whole command, and of the numpy
restatement of the same work on the host.

    python tools/preprocess_bench.py [--iters 50] [--out FILE.json]

Volume: 512 x 512 x 64 int16 (a CT series of the CRC set).  Device: device events around `iters` back-to-back calls of
volume_stats (4 launches: two streaming passes over the volume and two one-workgroup folds), volume_to_slices to 512^2
(k_rows alone: both passes keep their size) and to 256^2 (k_rows + k_cols), label_volume_to_slices to 256^2.  Bytes: what
the algorithm reads and writes, from the shapes (stored voxels in, float32 slices out, the float32 intermediate of the
horizontal pass written and read once).  Command: preprocess_crc on one gzip-compressed volume in a temporary directory,
with the time of reading the file (gunzip), of the producer (upload, kernels, download) and of np.save taken separately
on the same data.  Host: tests/preprocess_ref.py on the same volume.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "medical-image-editing_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def volume(X=512, Y=512, Z=64, seed=11):
    g = np.random.default_rng(seed)
    raw = np.empty((X, Y, Z), dtype=np.int16, order="F")
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X))
    for k in range(Z):
        raw[..., k] = 600.0 * np.sin(xx / 37.0 + k / 5.0) * np.cos(yy / 53.0) + g.standard_normal((X, Y)) * 150.0 - 300.0
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true", help="leave out the numpy restatement (it takes a while)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "preprocess_bench needs a GPU"
    from hipops import ops
    from preprocess import preprocess_crc
    from preprocess.producers import DeviceProducer
    from utils import nifti
    import preprocess_ref as R

    raw = volume()
    X, Y, Z = raw.shape
    n = raw.size
    vol = torch.from_numpy(np.ascontiguousarray(raw.T)).to("cuda")
    lab = torch.from_numpy(np.ascontiguousarray((np.abs(raw) // 400).astype(np.int32).T)).to("cuda")
    stats = ops.volume_stats(vol)
    rows = []

    def row(name, seconds, nbytes, launches):
        rows.append(dict(kernel=name, seconds=seconds, bytes=nbytes, bytes_per_second=nbytes / seconds, launches=launches))

    row("volume_stats", timed(lambda: ops.volume_stats(vol), args.iters), 2 * 2 * n, 4)
    row("volume_to_slices_512_minmax_crc", timed(lambda: ops.volume_to_slices(vol, 512, "minmax", "crc", stats), args.iters),
        2 * n + 4 * Z * 512 * 512, 1)
    row("volume_to_slices_256_minmax_crc", timed(lambda: ops.volume_to_slices(vol, 256, "minmax", "crc", stats), args.iters),
        2 * n + 2 * 4 * Z * Y * 256 + 4 * Z * 256 * 256, 2)
    row("volume_to_slices_256_zscore_brats", timed(lambda: ops.volume_to_slices(vol, 256, "zscore", "brats", stats), args.iters),
        2 * n + 2 * 4 * Z * Y * 256 + 4 * Z * 256 * 256, 2)
    row("volume_to_slices_256_none_none", timed(lambda: ops.volume_to_slices(vol, 256), args.iters),
        2 * n + 2 * 4 * Z * X * 256 + 4 * Z * 256 * 256, 2)
    row("label_volume_to_slices_256_brats", timed(lambda: ops.label_volume_to_slices(lab, 256, "brats"), args.iters),
        4 * Z * 256 * 256 * 2, 1)
    for r in rows:
        print("%-36s %9.1f us  %7.3f TB/s  (%d launches)" % (r["kernel"], r["seconds"] * 1e6, r["bytes_per_second"] / 1e12,
                                                             r["launches"]))

    res = dict(device=torch.cuda.get_device_name(0), volume=[X, Y, Z], dtype="int16", rows=rows)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "src"), os.path.join(tmp, "dst")
        os.makedirs(src)
        path = os.path.join(src, "CRC_0001_image.nii.gz")
        nifti.save(raw, path)
        producer = DeviceProducer()
        preprocess_crc.run(src, os.path.join(tmp, "warm"), 512, producer)
        t0 = time.perf_counter()
        preprocess_crc.run(src, dst, 512, producer)
        whole = time.perf_counter() - t0
        t0 = time.perf_counter()
        loaded, slope, inter, _ = nifti.load_raw(path)
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        slices = producer.image_slices(loaded, slope, inter, 512, "minmax", "crc")
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        os.makedirs(os.path.join(tmp, "again"))
        for i in range(slices.shape[0]):
            np.save(os.path.join(tmp, "again", "%04d.npy" % i), slices[i])
        t_save = time.perf_counter() - t0
        res["command"] = dict(name="preprocess_crc, one volume to 512^2", seconds=whole, read_gunzip_seconds=t_read,
                              producer_seconds=t_dev, save_seconds=t_save, file_io_share=(t_read + t_save) / whole,
                              compressed_bytes=os.path.getsize(path))
        print("preprocess_crc one volume: %.3f s (read + gunzip %.3f, producer %.3f, np.save %.3f; file I/O share %.2f)"
              % (whole, t_read, t_dev, t_save, (t_read + t_save) / whole))
    if not args.skip_host:
        for size in (512, 256):
            t0 = time.perf_counter()
            R.image_slices(raw, 1.0, 0.0, size, "minmax", "crc")
            t = time.perf_counter() - t0
            res["host_restatement_%d_seconds" % size] = t
            print("numpy restatement, minmax + crc + %d^2: %.3f s" % (size, t))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
