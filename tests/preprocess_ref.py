"""Restatement of the preprocess pipelines in numpy for the tests (not imported by the product package).

The reference's scripts (src/preprocess/) normalise a volume with numpy and resize every slice with PIL's Image.resize.
PIL is not a dependency of the tests, so its resampler is written out here from its documented arithmetic (Resample.c,
mode F, and the affine NEAREST path of Geometry.c); tests/golden/make_golden_preprocess.py checks this file against PIL
itself when it writes the fixture.

Bilinear, mode F (32-bit float pixels), per axis with in != out (an axis that keeps its size is skipped):
- scale = in / out, filterscale = max(scale, 1), support = 1 * filterscale, ksize = ceil(support) * 2 + 1;
- for output xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
  xmax = min(int(center + support + 0.5), in) - xmin, w[x] = triangle((x + xmin - center + 0.5) * (1.0 / filterscale)),
  the reciprocal taken once; w /= sum(w), the sum a running double sum in index order;
- out = float32(sum_x double(pixel[xmin + x]) * w[x]), a double accumulator starting at 0.0, in index order;
- the horizontal pass (along the columns) comes first and is stored as float32, then the vertical pass.
Nearest: the source coordinate is a double stepped from 0.5 * scale by scale per output pixel and truncated.
"""
import numpy as np

f32 = np.float32


def bilinear_coefficients(in_size, out_size):
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_size, ksize), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    return k, bounds


def _pass_columns(img, out_size):
    """img (..., rows, cols) float32 -> (..., rows, out_size) float32: one resampling pass along the last axis."""
    in_size = img.shape[-1]
    if in_size == out_size:
        return img
    k, bounds = bilinear_coefficients(in_size, out_size)
    ss = np.zeros(img.shape[:-1] + (out_size,), dtype=np.float64)
    for t in range(k.shape[1]):                            # tap by tap: the accumulation order of the C loop
        live = t < bounds[:, 1]
        src = np.minimum(bounds[:, 0] + t, in_size - 1)
        term = img[..., src].astype(np.float64) * k[:, t]  # one rounding
        ss = np.where(live, ss + term, ss)                 # one rounding
    return ss.astype(f32)


def resize_bilinear(img, size):
    """Image.fromarray(img).resize((size, size), BILINEAR) for float32 img (..., H, W): bit for bit."""
    img = np.asarray(img)
    assert img.dtype == f32
    h = _pass_columns(img, size)
    v = _pass_columns(np.swapaxes(h, -1, -2), size)
    return np.ascontiguousarray(np.swapaxes(v, -1, -2))


def nearest_indices(in_size, out_size):
    scale = float(in_size) / float(out_size)
    idx = np.empty(out_size, dtype=np.int64)
    xo = 0.0 + scale * 0.5
    for i in range(out_size):
        idx[i] = min(int(xo), in_size - 1)
        xo += scale
    return idx


def resize_nearest(img, size):
    """Image.fromarray(img).resize((size, size), NEAREST) for img (..., H, W)."""
    img = np.asarray(img)
    return np.ascontiguousarray(img[..., nearest_indices(img.shape[-2], size), :][..., nearest_indices(img.shape[-1], size)])


def scaled(raw, slope, inter):
    """nibabel's get_fdata(): float64, array * slope + inter unless they are the identity (slope 0: not set)."""
    out = np.asarray(raw).astype(np.float64)
    if slope not in (0.0, 1.0) or inter != 0.0:
        out = out * (slope if slope != 0.0 else 1.0) + inter
    return out


def orient(vol, how):
    """vol (X, Y, Z) -> (Z, rows, cols): every slice vol[..., i] as the scripts turn it."""
    s = np.moveaxis(vol, 2, 0)
    if how == 'crc':
        return np.rot90(s[:, ::-1, :], axes=(1, 2))
    if how == 'brats':
        return np.rot90(s, k=3, axes=(1, 2))
    assert how is None
    return s


def minmax_normalize(image, scale=255.0):
    image = image.copy()
    a_min, a_max = image.min(), image.max()
    image -= a_min
    image /= (a_max - a_min)
    image *= scale
    return image


def z_score_normalize(array, wide_statistics=False):
    """wide_statistics: mean and std taken in float64 and rounded once to float32 (the reference takes them in float32)."""
    array = array.astype(f32)
    mask = array > 0
    if wide_statistics:
        mean, std = f32(np.mean(array[mask], dtype=np.float64)), f32(np.std(array[mask], dtype=np.float64))
    else:
        mean, std = np.mean(array[mask]), np.std(array[mask])
    array -= mean
    array /= std
    return array


def image_slices(raw, slope, inter, size, norm, how, wide_statistics=False, only=None):
    """only: the slice indices to orient and resize (the statistics are the whole volume's either way)."""
    v = scaled(raw, slope, inter)
    if norm == 'minmax':
        v = minmax_normalize(v).astype(f32)                # PIL's F;64F unpack: one rounding
    elif norm == 'zscore':
        v = z_score_normalize(v, wide_statistics)
    else:
        assert norm is None
        v = v.astype(f32)
    if only is not None:
        v = v[..., list(only)]
    return resize_bilinear(np.ascontiguousarray(orient(v, how)), size)


def label_slices(labels, size, how, relabel):
    labels = np.asarray(labels)
    assert labels.dtype == np.int32
    if relabel:
        if (labels == 3).any():
            raise ValueError("label 3 is already present")
        labels = np.where(labels == 4, np.int32(3), labels)
    return resize_nearest(np.ascontiguousarray(orient(labels, how)), size)


class Producer:
    """The slice producer the preprocess commands take, on the host (tests only)."""

    def image_slices(self, raw, slope, inter, size, norm, orient):
        return image_slices(raw, slope, inter, size, norm, orient)

    def label_slices(self, labels, size, orient, relabel):
        return label_slices(labels, size, orient, relabel)


_NIFTI_CODES = {'u1': 2, 'i2': 4, 'i4': 8, 'f4': 16, 'f8': 64, 'i1': 256, 'u2': 512, 'u4': 768, 'i8': 1024, 'u8': 1280}


def save_nifti(path, array, slope=1.0, inter=0.0, big_endian=False):
    """A single-file NIfTI-1 (.nii or .nii.gz) with the given scl_slope / scl_inter and byte order: what the tests feed the
    reader and the commands (the product's writer stores neither a scaling nor big-endian data)."""
    import gzip
    import struct
    a = np.asarray(array)
    e = '>' if big_endian else '<'
    hdr = bytearray(348)
    struct.pack_into(e + 'i', hdr, 0, 348)
    struct.pack_into(e + '8h', hdr, 40, a.ndim, *(list(a.shape) + [1] * (7 - a.ndim)))
    struct.pack_into(e + 'h', hdr, 70, _NIFTI_CODES[a.dtype.str[1:]])
    struct.pack_into(e + 'h', hdr, 72, a.dtype.itemsize * 8)
    struct.pack_into(e + '8f', hdr, 76, *([1.0] * 8))
    struct.pack_into(e + 'f', hdr, 108, 352.0)
    struct.pack_into(e + 'f', hdr, 112, slope)
    struct.pack_into(e + 'f', hdr, 116, inter)
    struct.pack_into(e + 'h', hdr, 254, 2)
    for row, off in enumerate((280, 296, 312)):
        struct.pack_into(e + '4f', hdr, off, *np.eye(4)[row])
    hdr[344:348] = b'n+1\x00'
    body = bytes(hdr) + b'\x00' * 4 + a.astype(a.dtype.newbyteorder(e)).tobytes(order='F')
    with (gzip.open(path, 'wb') if str(path).endswith('.gz') else open(path, 'wb')) as f:
        f.write(body)


# ---- the command fixtures: tests/golden/preprocess.npz 'commands' ----------------------------------------------------

def write_sources(z, spec, root):
    """The .nii.gz files of a command's fixture under `root`."""
    import os
    for rel, (vol, slope, inter) in spec["files"].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        save_nifti(path, z["vol/" + vol], slope=slope, inter=inter)


def assert_tree(z, spec, dst):
    """`dst` holds exactly the fixture's files with its dtypes and shapes; values are bit-equal, z-scored files within 2 D
    of the reference's (D: how far float32 statistics move that volume's slices; the factor 2 lets a statistic round to the
    other neighbouring float32)."""
    import os
    found = sorted(os.path.relpath(os.path.join(d, n), dst) for d, _, names in os.walk(dst) for n in names)
    assert found == sorted(spec["tree"])
    for rel, key in spec["tree"].items():
        got, want = np.load(os.path.join(dst, rel)), z[key]
        assert got.dtype == want.dtype and got.shape == want.shape, rel
        D = spec.get("D", {}).get(rel)
        if D is None:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), rel
        else:
            assert D > 0 and np.abs(got.astype(np.float64) - want).max() <= 2 * D, rel
