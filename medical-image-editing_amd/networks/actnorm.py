"""ActNorm of the discriminator (reference: networks/actnorm.py:11-70, the taming-transformers module) on the HIP kernels.

Same constructor, parameters `loc`, `scale` of shape (1, C, 1, 1) and uint8 scalar buffer `initialized`.  Only the path
the discriminator uses is built: 4-d input, forward direction, logdet=False; anything else raises.

The reference reads `initialized.item()` in every forward, one host synchronisation per layer per forward.  Here the
module keeps a host-side copy of the flag (`_host_initialized`), refreshed whenever a state dict is loaded, so a
steady-state step enqueues without waiting for the GPU.  Code that writes the `initialized` buffer by hand must call
`refresh_initialized()`.
"""
import torch
import torch.nn as nn

from hipops import ops


class ActNorm(nn.Module):
    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        if logdet:
            raise NotImplementedError("ActNorm(logdet=True) is not on the discriminator's path and is not built")
        self.logdet = logdet
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.allow_reverse_init = allow_reverse_init
        self.register_buffer('initialized', torch.tensor(0, dtype=torch.uint8))
        self._host_initialized = False

    def refresh_initialized(self):
        """Re-read the flag buffer (one host synchronisation)."""
        self._host_initialized = bool(self.initialized.item())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self.refresh_initialized()

    def forward(self, input, reverse=False, slope=1.0):
        if reverse:
            raise NotImplementedError("ActNorm reverse is not on the discriminator's path and is not built")
        if input.dim() != 4:
            raise NotImplementedError("ActNorm is built for 4-d (N, C, H, W) inputs only")
        init = self.training and not self._host_initialized
        y = ops.act_norm_lrelu(input, self.loc, self.scale, self.initialized if init else None, slope=slope)
        if init:
            self._host_initialized = True
        return y
