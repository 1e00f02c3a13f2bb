"""Drop-in for the reference's `functions.lpips_loss.LPIPSLoss` (trainers/base.py:271-275 builds it as LPIPSLoss() for
perceptual_loss_type 'lpips'): torch.mean(lpips.LPIPS(net='alex')(sr, hr)) on the inputs expanded to 3 channels.  The
arithmetic is the HIP kernels behind hipops.ops.lpips_loss; the `lpips` package is not needed.

What is computed (lpips.LPIPS(net='alex'), version 0.1, with its defaults: linear layers on, spatial=False, eval mode,
normalize=False) - written from the package's published definition, which is this module's specification:
  1. scaling layer, per channel: (x - shift) / scale, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450); the
     first convolution's zero padding applies after it;
  2. torchvision's alexnet.features[0:12]: Conv(3->64, 11, stride 4, pad 2), ReLU, MaxPool(3, 2), Conv(64->192, 5, pad 2),
     ReLU, MaxPool(3, 2), Conv(192->384, 3, pad 1), ReLU, Conv(384->256, 3, pad 1), ReLU, Conv(256->256, 3, pad 1), ReLU,
     tapped after each of the five ReLUs;
  3. per tap: a = f / (|f| + 1e-10) along channels, b likewise from hr, d = sum_c w_c (a_c - b_c)^2 with the 1x1 "lin"
     weights w (no bias), mean over the tap's pixels; the five taps summed per image; the mean over the batch.

The module tree mirrors the package's so that a reference checkpoint's `perceptual_loss.*` entries load:
loss_func.net.slice{1..5}.{0,3,6,8,10}.{weight,bias}, loss_func.lin{0..4}.model.1.weight, loss_func.scaling_layer.shift /
.scale (buffers).  Newer versions of the package also save the lin layers a second time as loss_func.lins.{i}.model.1.weight:
those entries are accepted and ignored.

The package downloads torchvision's AlexNet and carries its own lin weights.  This build never downloads: `weights` is an
LPIPS state dict or a path to one (keys as above, with or without the `loss_func.` / `perceptual_loss.loss_func.` prefix,
optionally under 'state_dict'), or a pair (alexnet, lins) of torchvision's alexnet state dict (`features.N.*`, the file
alexnet-owt-7be5be79.pth) and the package's weights/v0.1/alex.pth (`lin{i}.model.1.weight`), each a dict or a path.
weights=None looks for those two file names in torch.hub.get_dir()/checkpoints and raises naming both when one is absent.

Two deliberate conventions:
  - At a pixel whose tap features are all zero, autograd through sqrt(sum f^2) gives the reference inf * 0 = NaN, which only
    the select in the backward of the ReLU behind the tap discards again.  Here that pixel's normalisation contributes zero
    gradient outright (its forward value, 0, is exact); the end result is the same, without a NaN in between.
  - No weight gradients are computed: the parameters have requires_grad=False (as the package sets them) and the operator
    returns a gradient for sr only; hr is the clear image.
"""
import os

import torch
import torch.nn as nn

from hipops import ops

ALEXNET_FILE = "alexnet-owt-7be5be79.pth"    # the file name torchvision's alexnet(pretrained=True) downloads to
LINS_FILE = "alex.pth"                       # the package's weights/v0.1/alex.pth
_LAYERS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
           (5, 10, 256, 256, 3, 1, 1))      # (slice, features index, in, out, kernel, stride, padding)
_SHIFT = (-0.030, -0.088, -0.188)
_SCALE = (0.458, 0.448, 0.450)
_PREFIXES = ("loss_func.", "", "perceptual_loss.loss_func.")


def default_weights_paths():
    """(alexnet, lins): where torchvision keeps its AlexNet download, and where this build looks for the package's lin
    weights: the torch hub cache."""
    d = os.path.join(torch.hub.get_dir(), "checkpoints")
    return os.path.join(d, ALEXNET_FILE), os.path.join(d, LINS_FILE)


def _load(src, what):
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(os.fspath(src), map_location="cpu")
    if not isinstance(src, dict):
        raise TypeError("LPIPSLoss weights: expected a path or a state dict for %s, got %s" % (what, type(src).__name__))
    if "state_dict" in src and isinstance(src["state_dict"], dict):
        src = src["state_dict"]
    return src


def _find(src, names, what):
    for k in names:
        if k in src:
            return src[k]
    raise KeyError("LPIPSLoss weights: no entry for %s (looked for %s)" % (what, ", ".join(names)))


def lpips_state_dict(weights):
    """The module's own state dict ({'loss_func.net.slice1.0.weight': ..., 'loss_func.lin0.model.1.weight': ...,
    'loss_func.scaling_layer.shift': ...}) from any accepted form of `weights` (see the module docstring)."""
    out = {}
    if isinstance(weights, (tuple, list)):
        if len(weights) != 2:
            raise TypeError("LPIPSLoss weights: a pair must be (alexnet, lins), got %d elements" % len(weights))
        alex, lins = _load(weights[0], "the AlexNet state dict"), _load(weights[1], "the lin weights")
        for s, idx, *_ in _LAYERS:
            for kind in ("weight", "bias"):
                out["loss_func.net.slice%d.%d.%s" % (s, idx, kind)] = _find(
                    alex, ["features.%d.%s" % (idx, kind)], "AlexNet layer %d %s" % (idx, kind))
        for i in range(5):
            out["loss_func.lin%d.model.1.weight" % i] = _find(
                lins, ["lin%d.model.1.weight" % i, "lins.%d.model.1.weight" % i], "lin layer %d" % i)
        return out
    src = _load(weights, "the LPIPS state dict")
    for s, idx, *_ in _LAYERS:
        for kind in ("weight", "bias"):
            tail = "net.slice%d.%d.%s" % (s, idx, kind)
            out["loss_func." + tail] = _find(src, [p + tail for p in _PREFIXES], "AlexNet layer %d %s" % (idx, kind))
    for i in range(5):
        tails = ("lin%d.model.1.weight" % i, "lins.%d.model.1.weight" % i)
        out["loss_func.lin%d.model.1.weight" % i] = _find(src, [p + t for t in tails for p in _PREFIXES], "lin layer %d" % i)
    for name in ("shift", "scale"):          # buffers: saved by the package, constants of version 0.1 otherwise
        tail = "scaling_layer." + name
        for p in _PREFIXES:
            if p + tail in src:
                out["loss_func." + tail] = src[p + tail]
                break
    return out


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(_SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(_SCALE).view(1, 3, 1, 1))


class _AlexTaps(nn.Module):
    """alexnet.features[0:12] cut into the package's five slices; module names = torchvision's feature indices."""

    def __init__(self):
        super().__init__()
        for s, idx, cin, cout, k, stride, pad in _LAYERS:
            seq = nn.Sequential()
            if s in (2, 3):
                seq.add_module(str(idx - 1), nn.MaxPool2d(3, 2))
            seq.add_module(str(idx), nn.Conv2d(cin, cout, k, stride=stride, padding=pad))
            seq.add_module(str(idx + 1), nn.ReLU(inplace=True))
            setattr(self, "slice%d" % s, seq)


class _Lin(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(cin, 1, 1, bias=False))


class _LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _AlexTaps()
        for i, c in enumerate(ops.LPIPS_CHANNELS):
            setattr(self, "lin%d" % i, _Lin(c))


class LPIPSLoss(nn.Module):
    def __init__(self, net='alex', weights=None):
        super().__init__()
        if net != 'alex':
            raise NotImplementedError("LPIPSLoss(net=%r): only the 'alex' backbone that trainers/base.py builds is "
                                      "implemented" % (net,))
        self.loss_func = _LPIPS()
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        if weights is None:
            paths = default_weights_paths()
            if not all(os.path.isfile(p) for p in paths):
                raise FileNotFoundError(
                    "LPIPSLoss: no LPIPS weights at %s (torchvision's AlexNet) and %s (the lpips package's weights/v0.1/alex.pth); "
                    "nothing is downloaded - pass weights=<state dict, path or (alexnet, lins) pair> "
                    "(config.loss.lpips_weights)" % paths)
            weights = paths
        sd = lpips_state_dict(weights)
        for name in ("shift", "scale"):
            sd.setdefault("loss_func.scaling_layer." + name, getattr(self.loss_func.scaling_layer, name))
        self.load_state_dict(sd, strict=True)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # newer versions of the package save the lin layers twice (lin{i} and lins.{i}): the duplicates carry nothing new
        for k in [k for k in state_dict if k.startswith(prefix + "loss_func.lins.")]:
            del state_dict[k]
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def params(self):
        """The 17 tensors of ops.lpips_loss: (w1, b1, ..., w5, b5, lin0 .. lin4, shift, scale)."""
        lf = self.loss_func
        out = []
        for s, idx, *_ in _LAYERS:
            conv = getattr(getattr(lf.net, "slice%d" % s), str(idx))
            out += [conv.weight, conv.bias]
        out += [getattr(lf, "lin%d" % i).model[1].weight for i in range(5)]
        return tuple(out) + (lf.scaling_layer.shift, lf.scaling_layer.scale)

    def forward(self, sr, hr, window=None, windows=None):
        """sr, hr: (N, C, H, W) in [-1, 1] with C = 1 or 3 (expanded to 3 as the reference does), H, W >= 31.  window:
        optional (alpha, beta, lo, hi) of ops.window_map applied to both images inside the kernels (the lung /
        mediastinal terms of the multi-window step).  windows: a tuple of such windows (None = the identity) evaluated in
        one batch: returns one loss each."""
        if sr.dim() != 4 or sr.shape[1] not in (1, 3):
            raise ValueError("LPIPSLoss: expected (N, 1 or 3, H, W) inputs, got %s" % (tuple(sr.shape),))
        return ops.lpips_loss(sr, hr, self.params(), window=window, windows=windows)
