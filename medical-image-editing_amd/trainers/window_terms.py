"""The multi-window loss terms both training steps assemble (trainers/multi_window_trainer.py:93-126, 229-257): per loss
kind the full / lung / mediastinal terms and their weights, `weights[i] / 3` of a mean over the three windows.

Every function returns [(loss term, weight)] in the order ops.weighted_sum adds them (the order is part of a total's bits);
`scale` multiplies every weight (the first step folds loss_weight.recon / freq / perceptual in here, the second step takes
the window mean first).  multi_window = dict(dataset_window=(width, center, scale), recon_weights=(w_full, w_lung,
w_mediastinal)) or None for the single term of a single-window step.  clamp=False re-windows by the pure affine map
(ops.window_map).
"""
from hipops import ops

LUNG_WINDOW = (1500, -550, 2.0)             # trainers/base.py:33-43
MEDIASTINAL_WINDOW = (400, 20, 2.0)
WINDOWS = (None, LUNG_WINDOW, MEDIASTINAL_WINDOW)        # the order of recon_weights / freq_weights / percep_weights


def window_maps(dataset_window, clamp=True):
    """The three windows as ops take them: None (the identity), then the lung and mediastinal (alpha, beta, lo, hi)."""
    return tuple(None if w is None else ops.window_map(dataset_window, w, clamp=clamp) for w in WINDOWS)


def recon_terms(recon, clear, multi_window, scale, clamp=True):
    """Plain MSE, or the multi-window recon_weights[i] / 3 * MSE on the full / lung / mediastinal windows
    (multi_window_trainer.py:93-118)."""
    if multi_window is None:
        return [(ops.mse_loss(recon, clear), scale)]
    dw, rw = multi_window["dataset_window"], multi_window["recon_weights"]
    terms = [ops.mse_loss(recon, clear), ops.window_mse_loss(recon, clear, dw, LUNG_WINDOW, clamp=clamp),
             ops.window_mse_loss(recon, clear, dw, MEDIASTINAL_WINDOW, clamp=clamp)]
    return [(t, scale * float(r) / 3.0) for t, r in zip(terms, rw)]


def freq_terms(ffl, recon, clear, multi_window, freq_weights, scale, clamp=True):
    """The focal frequency loss (single_window_trainer.py:117-136): none without the loss; FFL(recon, clear); or,
    multi-window, freq_weights[i] / 3 * FFL on the three windows with the window map applied inside the kernel
    (multi_window_trainer.py:100-126)."""
    if ffl is None:
        return []
    if multi_window is None:
        return [(ffl(recon, clear), scale)]
    dw = multi_window["dataset_window"]
    terms = [ffl(recon, clear), ffl(recon, clear, window=ops.window_map(dw, LUNG_WINDOW, clamp=clamp)),
             ffl(recon, clear, window=ops.window_map(dw, MEDIASTINAL_WINDOW, clamp=clamp))]
    return [(t, scale * float(f) / 3.0) for t, f in zip(terms, freq_weights)]


def percep_terms(vgg, recon, clear, multi_window, percep_weights, scale, clamp=True):
    """The perceptual loss (single_window_trainer.py:124-137): none without the loss; VGGLoss(recon, clear); or,
    multi-window, percep_weights[i] / 3 * VGGLoss on the three windows (multi_window_trainer.py:101-119), all three in
    one batch with the window map applied inside the kernels.  The first term is the full-window (or only) loss."""
    if vgg is None:
        return []
    if multi_window is None:
        return [(vgg(recon, clear), scale)]
    dw = multi_window["dataset_window"]
    terms = vgg(recon, clear, windows=(None, ops.window_map(dw, LUNG_WINDOW, clamp=clamp),
                                       ops.window_map(dw, MEDIASTINAL_WINDOW, clamp=clamp)))
    return [(t, scale * float(p) / 3.0) for t, p in zip(terms, percep_weights)]
