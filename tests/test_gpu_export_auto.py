"""The per-image auto-ranged export kernel (hipops.ops.export_grey_auto, csrc/export.hip) against its restatement in numpy
float32: bytes and ranges are EQUAL, there is no tolerance in this file (one float32 rounding per operation, no fused
multiply-add, is the kernel's contract, as it is export_grey's in tests/test_gpu_export.py).

The range pass is what can go wrong: the shapes put an image's extreme at its first element and at the one or two elements
behind the last full group of four, use planes smaller than one workgroup's stride and planes spread over several
workgroups, and the contents cover mixed signs, all-negative data (a maximum that starts from 0 would be wrong), +-0, a
constant image, NaN / inf among finite values and an image without a finite value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32

SHAPES = [(1, 1, 1, 1), (2, 1, 5, 7), (3, 1, 64, 64), (1, 1, 3, 513), (2, 1, 512, 512)]
CONTENTS = ["mixed", "negative", "zeros", "constant", "nan_inf", "no_finite"]


def auto_ref(x, flip=False):
    """x (B, 1, H, W) float32 -> ((B, H, W) uint8, (B, 2) float32 ranges), operation by operation in float32."""
    x = np.asarray(x, dtype=f32)[:, 0]
    out = np.zeros(x.shape, np.uint8)
    rng = np.zeros((x.shape[0], 2), f32)
    for b, img in enumerate(x):
        fin = np.isfinite(img)
        vmin = img[fin].min() if fin.any() else f32(np.inf)
        vmax = img[fin].max() if fin.any() else f32(-np.inf)
        rng[b] = (vmin, vmax)
        with np.errstate(all="ignore"):
            d = f32(vmax) - f32(vmin)                # one rounding
            if not d > 0:                            # a constant image, or none of its values finite
                continue
            q = (img - f32(vmin)) / d                # two roundings
            q = np.minimum(np.maximum(q, f32(0)), f32(1))
            level = np.minimum(np.floor(f32(256) * q), f32(255))
            assert q.dtype == f32
        out[b] = np.where(fin, level, f32(0)).astype(np.uint8)
    return (out[:, ::-1, :] if flip else out), rng


def images(shape, content, seed):
    B, _, H, W = shape
    HW = H * W
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, HW)).astype(f32)
    for b in range(B):
        x[b] = x[b] * f32(0.5 + b) + f32(b - 0.75)             # a different range per image
    if content == "negative":
        x = -np.abs(x) - f32(0.125)
    elif content == "zeros":
        x = np.where(g.integers(0, 2, size=x.shape) > 0, f32(0.0), f32(-0.0)).astype(f32)
    elif content == "constant":
        x[:] = (f32(1.5) - np.arange(B, dtype=f32))[:, None]
    elif content == "nan_inf":
        x[:, g.integers(0, HW)] = np.nan
        x[:, g.integers(0, HW)] = np.inf
        if HW > 2:
            x[0, HW // 2] = -np.inf
    elif content == "no_finite":
        x[0] = np.where(g.integers(0, 2, size=HW) > 0, np.nan, np.inf)
        if B > 1:
            x[1:, 0] = np.nan                                   # the other images keep finite values
    if content in ("mixed", "negative"):
        # the extremes at the first element, the last and the one before it, in turn over the images
        for b in range(B):
            lo, hi = ((0, HW - 1), (HW - 1, max(HW - 2, 0)), (max(HW - 2, 0), 0))[b % 3]
            x[b, hi] = x[b].max() + f32(0.5)
            x[b, lo] = x[b].min() - f32(0.5)
    return x.reshape(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("content", CONTENTS)
def test_bytes_and_ranges_equal_numpy_float32(shape, content):
    from hipops import ops
    x = images(shape, content, seed=sum(shape) + len(content))
    for channels_last in (False, True):
        t = torch.from_numpy(x).to(DEV)
        if channels_last:
            t = t.contiguous(memory_format=torch.channels_last)
        for flip in (False, True):
            ref, rng = auto_ref(x, flip)
            got, got_rng = ops.export_grey_auto(t, flip=flip, return_range=True)
            got, got_rng = got.cpu().numpy(), got_rng.cpu().numpy()
            assert got.shape == ref.shape and got.dtype == np.uint8
            diff = int((got != ref).sum())
            print("auto %s %s flip %d cl %d: %d differing bytes, %d levels, ranges %s" % (shape, content, flip, channels_last, diff,
                                                                                        len(np.unique(ref)), got_rng.tolist()))
            assert np.array_equal(got_rng, rng), "ranges %s, expected %s" % (got_rng.tolist(), rng.tolist())
            assert np.array_equal(got, ref), "%d bytes differ" % diff
            assert np.array_equal(ops.export_grey_auto(t, flip=flip).cpu().numpy(), ref)        # without the range output


def test_extreme_at_each_of_the_three_places_of_a_64x64_plane():
    from hipops import ops
    HW = 64 * 64
    for where_min, where_max in ((0, HW - 1), (HW - 1, HW - 2), (HW - 2, 0)):
        x = np.random.default_rng(where_min + 1).uniform(-1, 1, size=(3, 1, 64, 64)).astype(f32)
        flat = x.reshape(3, HW)
        flat[:, where_min] = (-7.0, -2.5, -1.25)
        flat[:, where_max] = (3.0, -0.5, 9.75)
        flat[1] = -np.abs(flat[1]) - f32(0.5)
        flat[1, where_min], flat[1, where_max] = -2.5, -0.25                # all-negative: the maximum is -0.25
        got, rng = ops.export_grey_auto(torch.from_numpy(x).to(DEV), return_range=True)
        assert rng.cpu().numpy().tolist() == [[-7.0, 3.0], [-2.5, -0.25], [-1.25, 9.75]]
        assert np.array_equal(got.cpu().numpy(), auto_ref(x)[0])
        g = got.cpu().numpy().reshape(3, HW)
        assert (g[:, where_min] == 0).all() and (g[:, where_max] == 255).all()


@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (3, 1, 64, 64), (2, 1, 512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_equals_export_grey_over_each_images_own_range(shape):
    from hipops import ops
    x = images(shape, "mixed", seed=11)
    t = torch.from_numpy(x).to(DEV)
    for flip in (False, True):
        got = ops.export_grey_auto(t, flip=flip).cpu().numpy()
        for b in range(shape[0]):
            fixed = ops.export_grey(t[b:b + 1], vmin=float(x[b].min()), vmax=float(x[b].max()), flip=flip)[0, 0].cpu().numpy()
            assert np.array_equal(got[b], fixed)


def test_refuses_what_export_grey_refuses():
    from hipops import ops
    x = torch.zeros(2, 1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.export_grey_auto(x.double())
    with pytest.raises(RuntimeError, match=r"\(B, 1, H, W\)"):
        ops.export_grey_auto(x[:, 0])
    with pytest.raises(RuntimeError, match="empty"):
        ops.export_grey_auto(x[:0])
