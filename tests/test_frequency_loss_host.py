"""Focal frequency loss, CPU side (no GPU): the drop-in module and its config wiring, the C ABI / dispatcher entries, the
refusal to run on CPU tensors, and the fp64 restatement of the contract (focal-frequency-loss 0.3.0) that the GPU tests
compare the kernels against, checked on its own known answers."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_freq_loss_ws_bytes", "vqw_freq_twiddles", "vqw_freq_loss_fwd", "vqw_freq_loss_bwd")


def _patches(x, pf):
    """(N, C, H, W) -> (N, pf^2, C, h, w): the package's tensor2freq stacking order."""
    N, C, H, W = x.shape
    h, w = H // pf, W // pf
    return x.reshape(N, C, pf, h, pf, w).permute(0, 2, 4, 1, 3, 5).reshape(N, pf * pf, C, h, w)


def _unpatch(y, pf, shape):
    N, C, H, W = shape
    h, w = H // pf, W // pf
    return y.reshape(N, pf, pf, C, h, w).permute(0, 3, 1, 4, 2, 5).reshape(N, C, H, W)


def _win(x, window):
    if window is None:
        return x, torch.ones_like(x)
    a, b, lo, hi = window
    z = a * x + b
    return z.clamp(lo, hi), torch.where((z > lo) & (z < hi), torch.full_like(z, a), torch.zeros_like(z))


def ffl_weight(D, alpha, log_matrix, batch_matrix):
    """Steps 3-4: the detached spectrum weight of D (N, p^2, C, h, w)."""
    m = D.abs() ** alpha
    if log_matrix:
        m = torch.log(m + 1.0)
    m = m / (m.max() if batch_matrix else m.amax(dim=(-2, -1), keepdim=True))
    m = torch.where(torch.isnan(m), torch.zeros_like(m), m)
    return m.clamp(0.0, 1.0)


def ffl_ref(pred, target, alpha=1.0, patch_factor=1, log_matrix=False, batch_matrix=False, loss_weight=1.0, window=None):
    """fp64 restatement: -> (loss, dL/dpred, dL/dtarget) for gL = 1, as CPU float64 tensors."""
    p = pred.detach().double().cpu()
    t = target.detach().double().cpu()
    wp, sp = _win(p, window)
    wt, st = _win(t, window)
    D = torch.fft.fft2(_patches(wp - wt, patch_factor), norm="ortho")
    w = ffl_weight(D, alpha, log_matrix, batch_matrix)
    loss = loss_weight * torch.mean(w * (D.real ** 2 + D.imag ** 2))
    g = (2.0 * loss_weight / p.numel()) * torch.fft.ifft2(w * D, norm="ortho").real
    g = _unpatch(g, patch_factor, p.shape)
    return loss, g * sp, -g * st


def ffl_autograd(pred, target, alpha=1.0, patch_factor=1, log_matrix=False, batch_matrix=False, loss_weight=1.0):
    """Steps 1-5 literally as the package writes them (real / imaginary stacked), differentiated by autograd."""
    p = pred.detach().double().clone().requires_grad_(True)
    fp = torch.fft.fft2(_patches(p, patch_factor), norm="ortho")
    ft = torch.fft.fft2(_patches(target.double(), patch_factor), norm="ortho")
    fp, ft = torch.stack([fp.real, fp.imag], -1), torch.stack([ft.real, ft.imag], -1)
    tmp = (fp - ft) ** 2
    m = torch.sqrt(tmp[..., 0] + tmp[..., 1]) ** alpha
    if log_matrix:
        m = torch.log(m + 1.0)
    m = m / (m.max() if batch_matrix else m.max(-1).values.max(-1).values[:, :, :, None, None])
    m[torch.isnan(m)] = 0.0
    w = torch.clamp(m, min=0.0, max=1.0).clone().detach()
    loss = torch.mean(w * (tmp[..., 0] + tmp[..., 1])) * loss_weight
    loss.backward()
    return loss.detach(), p.grad


def _pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1, torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1


# ---- the restatement's known answers ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,pf", [((2, 1, 16, 16), 1), ((2, 3, 12, 20), 2), ((1, 1, 15, 9), 3)])
def test_restatement_alpha0_is_mse(shape, pf):
    """alpha = 0: w == 1, and by Parseval the loss is mse_loss(pred, target) with gradient 2 (pred - target) / M."""
    p, t = _pair(shape)
    loss, gp, gt = ffl_ref(p, t, alpha=0.0, patch_factor=pf)
    assert abs(float(loss) - float(torch.mean((p - t) ** 2))) <= 1e-14 * float(loss)
    assert float((gp - 2 * (p - t) / p.numel()).abs().max()) <= 1e-15
    assert torch.equal(gt, -gp)


def test_restatement_equal_images_give_zero():
    p, _ = _pair((2, 1, 8, 8))
    for kw in (dict(), dict(alpha=2.0), dict(log_matrix=True), dict(batch_matrix=True), dict(patch_factor=2)):
        loss, gp, _ = ffl_ref(p, p, **kw)
        assert float(loss) == 0.0 and not torch.isnan(gp).any() and float(gp.abs().max()) == 0.0, kw


@pytest.mark.parametrize("kw", [dict(), dict(alpha=0.5), dict(alpha=2.0, patch_factor=2), dict(log_matrix=True),
                                dict(batch_matrix=True, patch_factor=2), dict(loss_weight=3.0)])
def test_restatement_gradient_is_autograd_of_the_package_formulation(kw):
    """Step 6 (one inverse DFT) against autograd of steps 1-5 written as the package writes them."""
    p, t = _pair((2, 2, 12, 16), seed=1)
    loss, gp, _ = ffl_ref(p, t, **kw)
    la, ga = ffl_autograd(p, t, **kw)
    assert abs(float(loss - la)) <= 1e-13 * float(la)
    assert float((gp - ga).abs().max()) <= 1e-12 * float(ga.abs().max())


# ---- module, config, ABI -------------------------------------------------------------------------------------------

def test_module_import_and_package_defaults():
    from functions import FocalFrequencyLoss
    f = FocalFrequencyLoss()
    assert (f.loss_weight, f.alpha, f.patch_factor, f.ave_spectrum, f.log_matrix, f.batch_matrix) == (1.0, 1.0, 1, False, False, False)
    with pytest.raises(NotImplementedError):
        FocalFrequencyLoss(ave_spectrum=True)
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError):
        f(x, x, matrix=torch.ones(1, 1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        f(x, x)
    from hipops import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.frequency_loss(x, x)


def _config(tmp_path, mutate):
    from utils import load_json
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json")))
    mutate(raw)
    path = tmp_path / "c.json"
    path.write_text(json.dumps(raw))
    return load_json(str(path))


def test_config_builds_the_frequency_loss(tmp_path):
    from functions import EmbeddingLoss, FocalFrequencyLoss
    from trainers import configure_frequency_loss, configure_losses
    off = _config(tmp_path, lambda r: None)
    assert configure_frequency_loss(off) is None
    on = _config(tmp_path, lambda r: r["loss"].update(use_frequency_loss=True))
    f = configure_frequency_loss(on)
    assert isinstance(f, FocalFrequencyLoss) and f.alpha == 1.0 and f.loss_weight == 1.0
    assert isinstance(configure_losses(on), EmbeddingLoss)        # no longer refused


def test_multi_window_config_needs_freq_weights(tmp_path):
    from trainers import build_first_step_trainer

    def mw(r):
        r["loss"].update(use_frequency_loss=True, recon_weights=[1.0, 1.0, 1.0])
        r["dataset"].update(window_width=2000, window_center=0, window_scale=2.0)
    with pytest.raises(ValueError, match="freq_weights"):
        build_first_step_trainer(_config(tmp_path, mw), device="cpu")


def test_second_step_weights_keep_positional_construction():
    from trainers import GanLossWeights
    w = GanLossWeights(2.0, 3.0, 4.0)
    assert (w.recon, w.gen, w.dis, w.freq) == (2.0, 3.0, 4.0, 0.0)


def test_new_symbols_in_header_signatures_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 9 and _lib.load().vqw_abi_version() == 9
    library.register()
    for short in ("freq_twiddles", "freq_loss_fwd", "freq_loss_bwd"):
        assert hasattr(torch.ops.vqw, short), short
    sch = str(torch.ops.vqw.freq_loss_bwd.default._schema)
    assert "Tensor? pred" in sch and "Tensor(a!)? gpred" in sch and "Tensor(b!)? gtarget" in sch
    L = _lib.load()
    assert L.vqw_freq_loss_ws_bytes(64, 1, 256, 256, 1) >= 64 * 256 * 256 * 16
    # argument validation before any device work
    assert L.vqw_freq_loss_fwd(None, None, None, None, None, None, 0, 1, 1, 8, 8, 1, 1.0, 0, 0, 1.0, 0, 1.0, 0.0, 0.0, 0.0, None) != 0
    assert b"vqw_freq_loss_fwd" in L.vqw_last_error()
