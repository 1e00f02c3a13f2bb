"""Drop-in for the third-party `focal_frequency_loss.FocalFrequencyLoss` (package v0.3.0; Jiang et al., "Focal Frequency
Loss for Image Reconstruction and Synthesis", ICCV 2021) that the reference builds as FFL(loss_weight=1.0, alpha=1.0)
(trainers/base.py:277-278).  Same constructor; the arithmetic is the HIP kernels behind hipops.ops.frequency_loss."""
import torch.nn as nn

from hipops import ops


class FocalFrequencyLoss(nn.Module):
    def __init__(self, loss_weight=1.0, alpha=1.0, patch_factor=1, ave_spectrum=False, log_matrix=False, batch_matrix=False):
        super().__init__()
        if ave_spectrum:
            raise NotImplementedError("FocalFrequencyLoss(ave_spectrum=True) is not built (the reference does not use it)")
        self.loss_weight = loss_weight
        self.alpha = alpha
        self.patch_factor = patch_factor
        self.ave_spectrum = ave_spectrum
        self.log_matrix = log_matrix
        self.batch_matrix = batch_matrix

    def forward(self, pred, target, matrix=None, window=None, **kwargs):
        """pred, target: (N, C, H, W).  window: optional (alpha, beta, lo, hi) of ops.window_map, applied to both images
        inside the kernel (the lung / mediastinal terms of the multi-window step)."""
        if matrix is not None:
            raise NotImplementedError("FocalFrequencyLoss: an explicit spectrum weight matrix is not built "
                                      "(the reference does not pass one)")
        return ops.frequency_loss(pred, target, alpha=self.alpha, patch_factor=self.patch_factor, log_matrix=self.log_matrix,
                                  batch_matrix=self.batch_matrix, loss_weight=self.loss_weight, window=window)
