"""Drop-in for the reference's `functions.perceptual_loss.VGGLoss` (trainers/base.py:271-275 builds it as VGGLoss()):
F.mse_loss(vgg(sr), vgg(hr)) with vgg = torchvision's vgg19(pretrained=True).features[:8] - conv1_1, ReLU, conv1_2, ReLU,
MaxPool2d(2), conv2_1, ReLU, conv2_2, the output taken before conv2_2's ReLU - on the inputs expanded to 3 channels.  The
arithmetic is the HIP kernels behind hipops.ops.perceptual_loss.

The reference downloads the weights.  This build never does: `weights` is a path or a state dict in torchvision's vgg19
layout (`features.N.*`), VGGLoss's own (`vgg.N.*`) or a reference Lightning checkpoint's (`perceptual_loss.vgg.N.*` under
'state_dict'); weights=None reads the file torchvision's pretrained=True would have cached,
torch.hub.get_dir()/checkpoints/vgg19-dcbb9e9d.pth, and raises naming that path when it is absent.

One deliberate difference: the reference's `self.vgg.requires_grad = False` sets a plain attribute and freezes nothing, so
it also computes the VGG weight gradients, which no optimiser holds (base.py:164-181).  Here the parameters have
requires_grad=False and no weight gradient is computed; nothing in training can observe the difference.
"""
import os

import torch
import torch.nn as nn

from hipops import ops

VGG19_FILE = "vgg19-dcbb9e9d.pth"          # the file name torchvision's vgg19(pretrained=True) downloads to
_LAYERS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128))      # (features index, in, out) of the '22' slice


def default_weights_path():
    """Where torchvision's vgg19(pretrained=True) keeps its download: the torch hub cache."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", VGG19_FILE)


def vgg_slice_state_dict(weights):
    """{'vgg.N.weight' / 'vgg.N.bias': tensor} for N in 0, 2, 5, 7 from a path or a dict in any of the three layouts."""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(os.fspath(weights), map_location="cpu")
    if not isinstance(weights, dict):
        raise TypeError("VGGLoss weights: expected a path or a state dict, got %s" % type(weights).__name__)
    if "state_dict" in weights and isinstance(weights["state_dict"], dict):
        weights = weights["state_dict"]
    out = {}
    for idx, _, _ in _LAYERS:
        for kind in ("weight", "bias"):
            for prefix in ("vgg.", "features.", "perceptual_loss.vgg."):
                key = "%s%d.%s" % (prefix, idx, kind)
                if key in weights:
                    out["vgg.%d.%s" % (idx, kind)] = weights[key]
                    break
            else:
                raise KeyError("VGGLoss weights: no entry for layer %d %s (looked for vgg.%d.%s, features.%d.%s and "
                               "perceptual_loss.vgg.%d.%s)" % (idx, kind, idx, kind, idx, kind, idx, kind))
    return out


class VGGLoss(nn.Module):
    def __init__(self, conv_index='22', weights=None):
        super().__init__()
        if conv_index != '22':
            raise NotImplementedError("VGGLoss(conv_index=%r): only the '22' slice (vgg19.features[:8]) that trainers/base.py "
                                      "builds is implemented" % (conv_index,))
        self.conv_index = conv_index
        layers = []
        for i in range(8):
            spec = next((s for s in _LAYERS if s[0] == i), None)
            layers.append(nn.Conv2d(spec[1], spec[2], 3, padding=1) if spec else
                          nn.MaxPool2d(2) if i == 4 else nn.ReLU(inplace=True))
        self.vgg = nn.Sequential(*layers)
        for p in self.vgg.parameters():
            p.requires_grad_(False)
        if weights is None:
            path = default_weights_path()
            if not os.path.isfile(path):
                raise FileNotFoundError(
                    "VGGLoss: no VGG19 weights at %s (torchvision's pretrained=True cache file); nothing is downloaded - pass "
                    "weights=<path or state dict> (config.loss.perceptual_weights)" % path)
            weights = path
        self.load_state_dict(vgg_slice_state_dict(weights), strict=True)

    def forward(self, sr, hr, window=None, windows=None):
        """sr, hr: (N, C, H, W) with C = 1 or 3 (expanded to 3 as the reference does).  window: optional (alpha, beta, lo,
        hi) of ops.window_map applied to both images inside the kernels (the lung / mediastinal terms of the multi-window
        step).  windows: a tuple of such windows (None = the identity) evaluated in one batch: returns one loss each."""
        if sr.dim() != 4 or sr.shape[1] not in (1, 3):
            raise ValueError("VGGLoss: expected (N, 1 or 3, H, W) inputs, got %s" % (tuple(sr.shape),))
        v = self.vgg
        return ops.perceptual_loss(sr, hr, v[0].weight, v[0].bias, v[2].weight, v[2].bias, v[5].weight, v[5].bias, v[7].weight,
                                   v[7].bias, window=window, windows=windows)
