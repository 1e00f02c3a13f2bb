"""The 8-bit export kernels (hipops.ops.export_grey / export_labels, csrc/export.hip) against their restatement in numpy
float32, byte for byte.

The grey formula is restated operation by operation: every numpy float32 operation below rounds once, exactly what the
kernel's round-to-nearest intrinsics do (no fused multiply-add), so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32

DATASET_WINDOW = (4096, 0, 2.0)              # configs/baseline4: window_width / window_center / window_scale


def grey_ref(x, window, vmin=-1.0, vmax=1.0, flip=False):
    """x (B, 1, H, W) float32 -> (B, H, W) uint8."""
    alpha, beta, lo, hi = (f32(v) for v in (window if window is not None else (1.0, 0.0, -np.inf, np.inf)))
    x = np.asarray(x, dtype=f32)[:, 0]
    t = alpha * x                            # one rounding
    t = t + beta                             # one rounding
    t = np.minimum(np.maximum(t, lo), hi)
    rng = f32(vmax) - f32(vmin)
    q = (t - f32(vmin)) / rng                # two roundings
    q = np.minimum(np.maximum(q, f32(0)), f32(1))
    level = np.floor(f32(256) * q)           # exact product
    out = np.minimum(level, f32(255)).astype(np.uint8)
    assert t.dtype == f32 and q.dtype == f32
    return out[:, ::-1, :] if flip else out


def _windows():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW, MEDIASTINAL_WINDOW
    return (None, ops.window_map(DATASET_WINDOW, LUNG_WINDOW), ops.window_map(DATASET_WINDOW, MEDIASTINAL_WINDOW))


def _images(B, S, seed):
    """Smooth values in about [-1.3, 1.3] (so some lie outside [vmin, vmax]) with exact level boundaries k / 128 - 1,
    the two ends and values one float32 step to either side of a boundary written over part of them."""
    g = np.random.default_rng(seed)
    x = (1.3 * np.tanh(g.standard_normal((B, 1, S, S)))).astype(f32)
    flat = x.reshape(-1)
    n = flat.size
    k = g.integers(0, 257, size=n // 4)
    edges = (k.astype(f32) / f32(128) - f32(1)).astype(f32)
    pos = g.choice(n, size=n // 4, replace=False)
    flat[pos] = edges
    third = pos[: len(pos) // 3]
    flat[third] = np.nextafter(flat[third], f32(-2))
    third = pos[len(pos) // 3: 2 * (len(pos) // 3)]
    flat[third] = np.nextafter(flat[third], f32(2))
    flat[:4] = (-1.0, 1.0, 0.0, -0.0)
    return x


@pytest.mark.parametrize("size,batch", [(32, 3), (250, 2), (512, 2)])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
def test_grey_matches_numpy_float32_bytes(size, batch, flip, channels_last):
    from hipops import ops
    x = _images(batch, size, seed=size + batch)
    wins = _windows()
    t = torch.from_numpy(x).to(DEV)
    if channels_last:
        t = t.contiguous(memory_format=torch.channels_last)
    got = ops.export_grey(t, windows=wins, flip=flip).cpu().numpy()
    assert got.shape == (3, batch, size, size) and got.dtype == np.uint8
    for i, w in enumerate(wins):
        ref = grey_ref(x, w, flip=flip)
        diff = int((got[i] != ref).sum())
        print("grey %dx%d window %d flip %d: %d differing bytes, %d levels used" % (size, size, i, flip, diff, len(np.unique(ref))))
        assert np.array_equal(got[i], ref), "window %d: %d bytes differ" % (i, diff)
    single = ops.export_grey(t, flip=flip).cpu().numpy()
    assert np.array_equal(single[0], grey_ref(x, None, flip=flip))


def test_grey_plane_size_not_a_multiple_of_four_and_other_range():
    from hipops import ops
    x = _images(3, 33, seed=7)[:, :, :, :31].copy()           # 33 x 31 planes: the one-pixel form
    t = torch.from_numpy(x).to(DEV)
    for flip in (False, True):
        got = ops.export_grey(t, windows=(None, _windows()[1]), vmin=-0.5, vmax=1.25, flip=flip).cpu().numpy()
        for i, w in enumerate((None, _windows()[1])):
            assert np.array_equal(got[i], grey_ref(x, w, vmin=-0.5, vmax=1.25, flip=flip))


def _ids(B, H, W, K, seed):
    g = np.random.default_rng(seed)
    ids = g.integers(0, K + 1, size=(B, H, W)).astype(np.int64)
    ids[0, 0, :4] = (0, K, 1, K - 1)
    return ids


def _palette(K, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(K + 1, 3)).astype(np.uint8)


@pytest.mark.parametrize("K", [10, 1024, 5000])
@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 250, 250), (2, 512, 512), (2, 33, 31)])
@pytest.mark.parametrize("flip", [False, True])
def test_labels_match_numpy(K, shape, flip):
    from hipops import ops
    ids = _ids(*shape, K, seed=K + shape[1])
    pal = _palette(K)
    res = ops.export_labels(torch.from_numpy(ids).to(DEV), K, palette=pal, flip=flip)
    ref = ids[:, ::-1, :] if flip else ids
    index, rgb, counts = res.index.cpu().numpy(), res.rgb.cpu().numpy(), res.counts.cpu().numpy()
    assert index.dtype == (np.uint8 if K <= 255 else np.uint16)
    assert np.array_equal(index.astype(np.int64), ref)
    assert rgb.shape == shape + (3,) and np.array_equal(rgb, pal[ref])
    assert counts.dtype == np.int32
    for b in range(shape[0]):
        assert np.array_equal(counts[b], np.bincount(ids[b].ravel(), minlength=K + 1))


def test_labels_accept_the_encoder_style_transposed_view_and_the_default_palette():
    from hipops import ops
    K = 10
    ids = _ids(2, 32, 48, K, seed=1)
    t = torch.from_numpy(np.ascontiguousarray(ids.transpose(0, 2, 1))).to(DEV).transpose(1, 2)    # a (B, H, W) view
    assert not t.is_contiguous()
    res = ops.export_labels(t, K)
    assert np.array_equal(res.index.cpu().numpy(), ids)
    assert np.array_equal(res.rgb.cpu().numpy(), ops.default_palette(K)[ids])
    only = ops.export_labels(t, K, rgb=False, counts=False)
    assert only.rgb is None and only.counts is None and np.array_equal(only.index.cpu().numpy(), ids)


@pytest.mark.parametrize("K", [10, 1024])
def test_id_above_dict_size_raises(K):
    from hipops import ops
    ids = _ids(2, 32, 32, K, seed=2)
    ids[1, 5, 7] = K + 1
    with pytest.raises(ValueError, match="outside"):
        ops.export_labels(torch.from_numpy(ids).to(DEV), K)
    ids[1, 5, 7] = -1
    with pytest.raises(ValueError, match="outside"):
        ops.export_labels(torch.from_numpy(ids).to(DEV), K)
    ids[1, 5, 7] = 3
    ops.export_labels(torch.from_numpy(ids).to(DEV), K)          # the flag is cleared by the next call


@pytest.mark.parametrize("K", [10, 1024])
def test_counts_summed_over_the_batch_equal_code_entropy_counts(K):
    from hipops import ops
    ids = torch.from_numpy(_ids(4, 64, 64, K, seed=K)).to(DEV)
    _, counts = ops.code_entropy(ids, K)
    res = ops.export_labels(ids, K, rgb=False, index=False)
    assert torch.equal(res.counts.sum(dim=0).to(torch.int64), counts)
