"""Drop-ins for the torchmetrics 0.6.2 metrics the reference scores a model with (trainers/base.py:9-11, 75-77:
MeanSquaredError, StructuralSimilarityIndexMeasure, PeakSignalNoiseRatio, all with default arguments), and the code-usage
entropy of its test step (single_window_trainer.py:794-797).  The arithmetic is the HIP kernels behind
hipops.ops.recon_metrics.

What follows restates the package's 0.6.2 sources (the package itself is not a dependency):
- Metric.forward(*args) updates the accumulated state and, with compute_on_step, returns the value of that batch alone.
- MeanSquaredError keeps sum_squared_error and total; compute() = sum_squared_error / total (its sqrt with squared=False).
- PeakSignalNoiseRatio(data_range=None) keeps sum_squared_error, total and min_target / max_target, both seeded with
  tensor(0.0), so the range is max(max target, 0) - min(min target, 0).  compute() = (2 ln(range) - ln(sse / total)) *
  10 / ln(base).
- StructuralSimilarityIndexMeasure keeps every (preds, target) pair it is given and computes SSIM over their
  concatenation: range = max(range preds, range target), C1 = (k1 range)^2, C2 = (k2 range)^2, a Gaussian window
  (11 x 11, sigma 1.5), reflect padding by 5 and a crop of 5, which cancel: the mean runs over the valid windows.

Results are 0-d float64 device tensors.  Distributed state synchronisation, `dim`, reductions other than
'elementwise_mean' and non-square SSIM windows are not built and raise NotImplementedError.
"""
import math

import torch
import torch.nn as nn

from hipops import ops


def _slot(out, name):
    return out[ops.METRIC_SLOTS.index(name)]


class _Metric(nn.Module):
    """The part of torchmetrics.Metric these three use: forward (update + the batch's own value), update, compute, reset."""

    def __init__(self, compute_on_step=True, dist_sync_on_step=False, process_group=None, dist_sync_fn=None):
        super().__init__()
        if dist_sync_on_step or process_group is not None or dist_sync_fn is not None:
            raise NotImplementedError("%s: distributed state synchronisation is not built (the reference scores on rank 0)"
                                      % type(self).__name__)
        self.compute_on_step = compute_on_step
        self.reset()

    def forward(self, preds, target):
        out = self._stats(preds, target)
        self._accumulate(preds, target, out)
        return self._batch_value(out) if self.compute_on_step else None

    def update(self, preds, target):
        self._accumulate(preds, target, self._stats(preds, target))

    def _stats(self, preds, target):
        return ops.image_metrics_raw(preds, target, kernel_size=0)


class MeanSquaredError(_Metric):
    def __init__(self, compute_on_step=True, dist_sync_on_step=False, process_group=None, dist_sync_fn=None, squared=True):
        self.squared = squared
        super().__init__(compute_on_step, dist_sync_on_step, process_group, dist_sync_fn)

    def reset(self):
        self.sum_squared_error = None
        self.total = 0

    def _accumulate(self, preds, target, out):
        sse = _slot(out, "sse")
        self.sum_squared_error = sse if self.sum_squared_error is None else self.sum_squared_error + sse
        self.total += target.numel()

    def _batch_value(self, out):
        mse = _slot(out, "mse")
        return mse if self.squared else torch.sqrt(mse)

    def compute(self):
        if self.sum_squared_error is None:
            raise RuntimeError("MeanSquaredError.compute() before any update")
        mse = self.sum_squared_error / self.total
        return mse if self.squared else torch.sqrt(mse)


class PeakSignalNoiseRatio(_Metric):
    def __init__(self, data_range=None, base=10.0, reduction="elementwise_mean", dim=None, compute_on_step=True,
                 dist_sync_on_step=False, process_group=None, dist_sync_fn=None):
        if dim is not None:
            raise NotImplementedError("PeakSignalNoiseRatio(dim=...) is not built (the reference uses dim=None)")
        if reduction != "elementwise_mean":
            raise NotImplementedError("PeakSignalNoiseRatio(reduction=%r) is not built" % (reduction,))
        if data_range is not None and not float(data_range) > 0:
            raise ValueError("PeakSignalNoiseRatio: data_range must be > 0 (got %r)" % (data_range,))
        self.data_range = None if data_range is None else float(data_range)
        self.base = float(base)
        self.reduction, self.dim = reduction, dim
        super().__init__(compute_on_step, dist_sync_on_step, process_group, dist_sync_fn)

    def reset(self):
        self.sum_squared_error = None
        self.total = 0
        self.min_target = None         # tensor(0.0) in the package: folded in by compute()
        self.max_target = None

    def _stats(self, preds, target):
        return ops.image_metrics_raw(preds, target, data_range=self.data_range, kernel_size=0)

    def _accumulate(self, preds, target, out):
        sse, lo, hi = _slot(out, "sse"), _slot(out, "target_min"), _slot(out, "target_max")
        if self.sum_squared_error is None:
            self.sum_squared_error, self.min_target, self.max_target = sse, lo, hi
        else:
            self.sum_squared_error = self.sum_squared_error + sse
            self.min_target = torch.minimum(self.min_target, lo)
            self.max_target = torch.maximum(self.max_target, hi)
        self.total += target.numel()

    def _rescale(self, psnr10):
        return psnr10 if self.base == 10.0 else psnr10 * (math.log(10.0) / math.log(self.base))

    def _batch_value(self, out):
        return self._rescale(_slot(out, "psnr"))

    def compute(self):
        if self.sum_squared_error is None:
            raise RuntimeError("PeakSignalNoiseRatio.compute() before any update")
        if self.data_range is not None:
            rng = torch.full_like(self.sum_squared_error, self.data_range)
        else:
            rng = self.max_target.clamp(min=0.0) - self.min_target.clamp(max=0.0)
        psnr_e = 2.0 * torch.log(rng) - torch.log(self.sum_squared_error / self.total)
        return psnr_e * (10.0 / math.log(self.base))


class StructuralSimilarityIndexMeasure(_Metric):
    def __init__(self, kernel_size=(11, 11), sigma=(1.5, 1.5), reduction="elementwise_mean", data_range=None, k1=0.01,
                 k2=0.03, compute_on_step=True, dist_sync_on_step=False, process_group=None):
        if reduction != "elementwise_mean":
            raise NotImplementedError("StructuralSimilarityIndexMeasure(reduction=%r) is not built" % (reduction,))
        ks, sg = tuple(kernel_size), tuple(sigma)
        if len(ks) != 2 or len(sg) != 2:
            raise ValueError("StructuralSimilarityIndexMeasure: kernel_size and sigma take two values each")
        if ks[0] != ks[1] or sg[0] != sg[1]:
            raise NotImplementedError("StructuralSimilarityIndexMeasure: only square windows are built "
                                      "(kernel_size=%r, sigma=%r)" % (kernel_size, sigma))
        if ks[0] < 1 or ks[0] % 2 == 0 or not sg[0] > 0:
            raise ValueError("StructuralSimilarityIndexMeasure: kernel_size must be odd and positive, sigma positive")
        if data_range is not None and not float(data_range) > 0:
            raise ValueError("StructuralSimilarityIndexMeasure: data_range must be > 0 (got %r)" % (data_range,))
        self.kernel_size, self.sigma = ks, sg
        self.reduction, self.data_range, self.k1, self.k2 = reduction, data_range, float(k1), float(k2)
        super().__init__(compute_on_step, dist_sync_on_step, process_group, None)

    def reset(self):
        self.preds, self.target = [], []

    def _ssim(self, preds, target):
        return ops.image_metrics_raw(preds, target, data_range=self.data_range, kernel_size=self.kernel_size[0],
                                     sigma=self.sigma[0], k1=self.k1, k2=self.k2)

    def _stats(self, preds, target):
        return self._ssim(preds, target) if self.compute_on_step else None

    def _accumulate(self, preds, target, out):
        self.preds.append(preds.detach())
        self.target.append(target.detach())

    def _batch_value(self, out):
        return _slot(out, "ssim")

    def update(self, preds, target):
        self._accumulate(preds, target, None)

    def compute(self):
        if not self.preds:
            raise RuntimeError("StructuralSimilarityIndexMeasure.compute() before any update")
        return _slot(self._ssim(torch.cat(self.preds), torch.cat(self.target)), "ssim")


def label_entropy(ids, dict_size):
    """scipy.stats.entropy(np.bincount(ids.ravel(), minlength=dict_size + 1)[1:], base=2) as a Python float, computed on
    the device (single_window_trainer.py:794-797).  ids outside [0, dict_size] raise ValueError; nan when no id is
    in 1..dict_size."""
    return float(ops.code_entropy(ids, dict_size)[0])
