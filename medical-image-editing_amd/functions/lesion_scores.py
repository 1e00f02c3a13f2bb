"""Lesion-wise detection scores: how many lesions were found, how many false alarms a slice carries, and the Dice once specks are
thrown away.  LesionScores accumulates, per threshold, the eight integers of ops.lesion_match on the device (connected components
of the thresholded map against those of the ground truth, csrc/components.hip) and reads them once, in result()."""
import math

import torch

from hipops import ops

LESION_SCORES = ("sensitivity", "fp_per_slice", "precision", "f1", "dice_filtered")
LESION_CSV = ("threshold", "slices", "gt_lesions", "gt_detected", "sensitivity", "pred_components", "pred_false", "fp_per_slice",
              "precision", "f1", "dice_filtered")


def _div(num, den):
    return num / den if den else math.nan


def derived_scores(acc):
    """The scores of one row of eight integers (ops.LESION_ACC), in double; NaN where a denominator is 0 (the definition, not an
    error): sensitivity = gt_detected / gt_lesions; fp_per_slice = pred_false / slices; precision = (pred_components - pred_false) /
    pred_components; f1 = the harmonic mean of sensitivity and precision; dice_filtered = 2 inter / (pred_pixels + gt_pixels)."""
    a = dict(zip(ops.LESION_ACC, (int(v) for v in acc)))
    sens = _div(a["gt_detected"], a["gt_lesions"])
    prec = _div(a["pred_components"] - a["pred_false"], a["pred_components"])
    f1 = math.nan if math.isnan(sens) or math.isnan(prec) else _div(2.0 * sens * prec, sens + prec)
    return {"sensitivity": sens, "fp_per_slice": _div(a["pred_false"], a["slices"]), "precision": prec, "f1": f1,
            "dice_filtered": _div(2 * a["inter"], a["pred_pixels"] + a["gt_pixels"])}


class LesionScores:
    """update(maps, labels): maps (N, H, W) fp32 scores, labels (N, H, W) (or (N, 1, H, W)) torch.uint8 / torch.bool ground truth,
    both on the device.  The ground truth is labelled once per batch; each threshold then takes one label_components, one
    component_areas and one lesion_match call into its row of a (K, 8) accumulator.  update makes no host read; result() makes the
    single one and returns one dict per threshold: the threshold, the eight integers, the derived scores, and `err`, the kernels'
    error word (0 on every valid run)."""

    def __init__(self, thresholds, min_size=1, connectivity=8):
        thresholds = [float(t) for t in thresholds]
        if not thresholds or any(not (t == t and 0.0 <= t < math.inf) for t in thresholds):
            raise ValueError("LesionScores: thresholds=%r must be at least one finite number >= 0" % (thresholds,))
        if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1:
            raise ValueError("LesionScores: min_size=%r must be an integer >= 1" % (min_size,))
        if connectivity not in (4, 8):
            raise ValueError("LesionScores: connectivity=%r must be 4 or 8" % (connectivity,))
        self.thresholds, self.min_size, self.connectivity = thresholds, min_size, connectivity
        self.acc = self.err = None

    def update(self, maps, labels):
        if labels.dim() == 4 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if maps.dim() != 3 or maps.shape != labels.shape:
            raise ValueError("LesionScores.update: maps (N, H, W) and labels of the same shape expected, got %s and %s" % (tuple(maps.shape), tuple(labels.shape)))
        if labels.dtype not in (torch.uint8, torch.bool):
            raise ValueError("LesionScores.update: labels torch.uint8 or torch.bool expected, got %s" % labels.dtype)
        if self.acc is None:
            self.acc = ops.new_lesion_acc(maps.device, len(self.thresholds))
            self.err = torch.zeros(1, dtype=torch.int32, device=maps.device)
        gt_labels, gt_counts, _ = ops.label_components(labels, None, self.connectivity, self.err)
        for k, t in enumerate(self.thresholds):
            pl, pc, _ = ops.label_components(maps, t, self.connectivity, self.err)
            areas = ops.component_areas(pl, pc, self.connectivity, self.err)
            ops.lesion_match(pl, pc, areas, gt_labels, gt_counts, self.min_size, self.acc[k])

    def result(self):
        if self.acc is None:
            rows, err = [[0] * len(ops.LESION_ACC)] * len(self.thresholds), 0
        else:
            both = torch.cat([self.acc.reshape(-1), self.err.long()]).cpu().tolist()          # the one read
            n = len(ops.LESION_ACC)
            rows, err = [both[k * n:(k + 1) * n] for k in range(len(self.thresholds))], int(both[-1])
        out = []
        for t, row in zip(self.thresholds, rows):
            r = {"threshold": t}
            r.update(zip(ops.LESION_ACC, (int(v) for v in row)))
            r.update(derived_scores(row))
            r["err"] = err
            out.append(r)
        return out


def lesion_csv_row(r):
    """One line of detect_lesions.csv (LESION_CSV): the threshold as %.9g, integers as they are, floats as %.17g."""
    cells = []
    for key in LESION_CSV:
        v = r[key]
        cells.append("%.9g" % v if key == "threshold" else ("%d" % v if isinstance(v, int) else "%.17g" % v))
    return ",".join(cells)
