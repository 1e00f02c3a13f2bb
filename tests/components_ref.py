"""Restatements in numpy of the connected-component operators (csrc/components.hip): labelling by a union-find with numbering by
first pixel, areas, the matching of predicted against ground-truth components and the scores derived from its eight integers.
Plain and slow on purpose; nothing here imports the package or scipy."""
import math

import numpy as np

ACC = ("slices", "gt_lesions", "gt_detected", "pred_components", "pred_false", "inter", "pred_pixels", "gt_pixels")


def cap(H, W, connectivity):
    """The most components an H x W image can hold."""
    return ((H + 1) // 2) * ((W + 1) // 2) if connectivity == 8 else (H * W + 1) // 2


def _label_one(fg, connectivity):
    H, W = fg.shape
    parent = list(range(H * W))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    near = ((0, -1), (-1, 0)) + (((-1, -1), (-1, 1)) if connectivity == 8 else ())
    ys, xs = np.nonzero(fg)
    for y, x in zip(ys.tolist(), xs.tolist()):
        for dy, dx in near:
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and fg[v, u]:
                union(y * W + x, v * W + u)
    out = np.zeros(H * W, dtype=np.int32)
    number = {}
    for y, x in zip(ys.tolist(), xs.tolist()):          # raster order: a root is its component's first pixel
        r = find(y * W + x)
        if r not in number:
            number[r] = len(number) + 1
        out[y * W + x] = number[r]
    return out.reshape(H, W), len(number)


def label(x, threshold=None, connectivity=8):
    """x (N, H, W): foreground = non-zero, or x >= threshold (a NaN is background) -> (labels (N, H, W) int32, counts (N,) int32)."""
    assert connectivity in (4, 8)
    x = np.asarray(x)
    assert x.ndim == 3
    with np.errstate(invalid="ignore"):
        fg = (x != 0) if threshold is None else (x >= np.float32(threshold))
    pairs = [_label_one(f, connectivity) for f in fg]
    return np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int32)


def areas(labels, counts, connectivity=8):
    """(N, cap) int32: [n][l - 1] = the pixels of component l; zeros past counts[n]."""
    N, H, W = labels.shape
    c = cap(H, W, connectivity)
    out = np.zeros((N, c), dtype=np.int32)
    for n in range(N):
        b = np.bincount(labels[n].reshape(-1), minlength=c + 1)
        assert len(b) == c + 1 and b[counts[n] + 1:].sum() == 0
        out[n] = b[1:]
    return out


def match(pred_labels, gt_labels, min_size):
    """The eight integers of lesion_match, by set arithmetic on the label maps."""
    assert pred_labels.shape == gt_labels.shape and min_size >= 1
    acc = dict.fromkeys(ACC, 0)
    for p, g in zip(pred_labels, gt_labels):
        size = np.bincount(p.reshape(-1))
        kept = {l for l in range(1, len(size)) if size[l] >= min_size}
        keep_px = np.isin(p, sorted(kept)) if kept else np.zeros_like(p, dtype=bool)
        gt_px = g > 0
        both = keep_px & gt_px
        acc["slices"] += 1
        acc["gt_lesions"] += len(set(g[gt_px].tolist()))
        acc["gt_detected"] += len(set(g[both].tolist()))
        acc["pred_components"] += len(kept)
        acc["pred_false"] += len(kept - set(p[both].tolist()))
        acc["inter"] += int(both.sum())
        acc["pred_pixels"] += int(keep_px.sum())
        acc["gt_pixels"] += int(gt_px.sum())
    return [acc[k] for k in ACC]


def scores(acc):
    """{sensitivity, fp_per_slice, precision, f1, dice_filtered} in double from the eight integers; NaN where a denominator is 0."""
    a = dict(zip(ACC, (int(v) for v in acc)))
    div = lambda num, den: num / den if den else math.nan  # noqa: E731
    sens = div(a["gt_detected"], a["gt_lesions"])
    prec = div(a["pred_components"] - a["pred_false"], a["pred_components"])
    f1 = math.nan if math.isnan(sens) or math.isnan(prec) else div(2.0 * sens * prec, sens + prec)
    return {"sensitivity": sens, "fp_per_slice": div(a["pred_false"], a["slices"]), "precision": prec, "f1": f1,
            "dice_filtered": div(2 * a["inter"], a["pred_pixels"] + a["gt_pixels"])}


def lesion_scores(maps, gt, thresholds, min_size, connectivity):
    """LesionScores restated: rows of eight integers, one per threshold."""
    gl, _ = label(gt, None, connectivity)
    return [match(label(maps, t, connectivity)[0], gl, min_size) for t in thresholds]


# ---------------------------------------------------------------------------------------------- patterns for the tests
def spiral(H, W):
    """A one-pixel rectangular spiral from the corner inwards, one pixel of background between its arms: one component under either
    connectivity, and the longest parent chains a picture of this size can make."""
    m = np.zeros((H, W), dtype=np.uint8)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = d = 0
    m[0, 0] = 1

    def free(d):
        v, u = y + dirs[d][0], x + dirs[d][1]
        if not (0 <= v < H and 0 <= u < W) or m[v, u]:
            return False
        v2, u2 = v + dirs[d][0], u + dirs[d][1]
        return not (0 <= v2 < H and 0 <= u2 < W and m[v2, u2])

    while True:
        if not free(d):
            d = (d + 1) % 4
            if not free(d):
                return m
        y, x = y + dirs[d][0], x + dirs[d][1]
        m[y, x] = 1


def comb(H, W):
    """Teeth in every second column, joined only by the last row."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[:, ::2] = 1
    m[H - 1, :] = 1
    return m


def rings(H, W):
    """Two nested rectangular rings, not joined: the outer one begins first."""
    m = np.zeros((H, W), dtype=np.uint8)
    for k in (0, 3):
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = 1
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = 1
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) % 2 == 0).astype(np.uint8)
