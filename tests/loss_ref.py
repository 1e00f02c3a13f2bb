"""Restatement of the loss and optional-path operations for the tests (not imported by the product package).

Plain torch on the CPU, written from the formulas of the reference; every function works in the dtype of its inputs
(the tests pass float64, and float32 where they measure the rounding error of a correct fp32 evaluation) and is
differentiable by autograd: the tests take gradients from `.backward()` on these, never from a derivative written by hand.

- cross_loss_dense / cross_loss_labels: functions/embed_loss.py:46-66 (`_calc_cross_loss`).
- soft_dice / focal: functions/seg_loss.py:15-62.
- dropblock_keep: networks/dropblock.py:70-91.
- onehot: functions/onehot.py:11-20; pixel_shuffle2: blocks.py:100-104; flip_labels: the flip views' id map
  (single_window_trainer.py:91-96 with a horizontal flip).

tests/test_loss_ref_host.py pins these to the recorded outputs of the reference modules.
"""
import torch
import torch.nn.functional as F

CROSS_EPS = 1e-6      # EmbeddingLoss.epsilon (embed_loss.py:8)


def _cross_mean(num, cnt):
    """embed_loss.py:60-64: per (b, k) num / (cnt + eps), mean over the (b, k) with cnt != 0 (NaN when there is none)."""
    per = num / (cnt + CROSS_EPS)
    return per[cnt != 0].mean()


def cross_loss_dense(embed, r, cb_kd):
    """embed_loss.py:46-66 without the (b, D, K, n_loc) broadcast.  embed (B, D, H, W), r (B, K, H, W) weights,
    cb_kd (K, D) (the reference holds the codebook as (D, K) and detaches it).  Per (b, k):
    sum_p r |e_p - c_k|^2 / (sum_p r + 1e-6)."""
    B, D = embed.shape[:2]
    K = cb_kd.shape[0]
    e = embed.reshape(B, D, -1)                       # (B, D, P)
    w = r.reshape(B, K, -1).to(e.dtype)               # (B, K, P)
    c = cb_kd.detach().to(e.dtype)
    cols = []
    for k in range(K):                                # one class at a time: (B, D, P) temporaries only
        d2 = ((e - c[k].view(1, D, 1)) ** 2).sum(1)   # (B, P)
        cols.append((d2 * w[:, k]).sum(1))
    num = torch.stack(cols, 1)
    return _cross_mean(num, w.sum(2))


def cross_loss_labels(embed, labels, cb_kd):
    """The same loss for hard assignments: labels (B, H, W) integers in [0, K], 0 = out of frame (no class), label l >= 1
    standing for the one-hot plane l - 1.  Written as a gather of each pixel's own centre."""
    B, D = embed.shape[:2]
    K = cb_kd.shape[0]
    e = embed.reshape(B, D, -1).permute(0, 2, 1)      # (B, P, D)
    lab = labels.reshape(B, -1).long()
    valid = (lab >= 1) & (lab <= K)
    idx = (lab - 1).clamp(0, K - 1)
    c = cb_kd.detach().to(e.dtype)[idx]               # (B, P, D)
    d2 = ((e - c) ** 2).sum(2) * valid.to(e.dtype)    # (B, P)
    num = torch.zeros(B, K, dtype=e.dtype).scatter_add(1, idx, d2)
    cnt = torch.zeros(B, K, dtype=e.dtype).scatter_add(1, idx, valid.to(e.dtype))
    return _cross_mean(num, cnt)


def _flatten(t):
    """seg_loss.py:8-12: (B, C, *spatial) -> (C, B * prod(spatial))"""
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def soft_dice(logits, target, ignore_index=None, smooth=1e-6):
    """seg_loss.py:15-43.  ignore_index None or negative: no class is left out (the package's ops use -1 for None)."""
    p = _flatten(torch.softmax(logits, dim=1))
    t = _flatten(target).to(p.dtype)
    inter = (p * t).sum(-1)
    den = p.sum(-1) + t.sum(-1)
    if ignore_index is not None and ignore_index >= 0:
        kept = [c for c in range(p.shape[0]) if c != ignore_index]
        inter, den = inter[kept], den[kept]
    return 1.0 - 2.0 * inter.sum() / den.sum().clamp(min=smooth)


def focal(logits, target, gamma=2.0, eps=1e-6):
    """seg_loss.py:46-62 (alpha unused upstream): mean over pixels of sum_c -t log_softmax(z) (1 - clamp(p, eps, 1 - eps))^gamma"""
    p = torch.softmax(logits, dim=1).clamp(min=eps, max=1 - eps)
    log_p = torch.log_softmax(logits, dim=1)
    return ((-target.to(p.dtype) * log_p) * (1.0 - p) ** gamma).sum(1).mean()


def dropblock_keep(seed, block):
    """dropblock.py:80-91 and :73: keep = 1 - max_pool2d(seed, block, stride 1, pad block // 2), even sizes cropped at the
    end; scale = numel(keep) / sum(keep).  seed (B, H, W) of {0, 1}."""
    m = F.max_pool2d(seed[:, None], kernel_size=(block, block), stride=(1, 1), padding=block // 2)
    if block % 2 == 0:
        m = m[:, :, :-1, :-1]
    keep = 1 - m.squeeze(1)
    return keep, keep.numel() / keep.sum()


def dropblock_apply(x, keep, scale):
    """dropblock.py:70-73: x (B, C, H, W) * keep (B, H, W) * scale"""
    return x * keep[:, None].to(x.dtype) * scale


def pixel_shuffle2(x):
    return F.pixel_shuffle(x, 2)


def onehot(labels, n_classes):
    """onehot.py:11-20 as (B, n_classes, *spatial) float; a label outside [0, n_classes) gives an all-zero column (the
    reference's index_select would raise there; the package defines it as no class)."""
    lab = labels.long()
    ok = (lab >= 0) & (lab < n_classes)
    oh = F.one_hot(lab.clamp(0, n_classes - 1), n_classes) * ok[..., None]
    return oh.movedim(-1, 1).contiguous().to(torch.float64)


def flip_labels(ids, border=0):
    """Id map of the horizontally flipped view: out[b, h, w] = ids[b, h, W - 1 - w], zero within `border` pixels of the frame."""
    out = torch.flip(ids, dims=(2,)).to(torch.int32).clone()
    H, W = out.shape[1:]
    if border > 0:
        b = min(border, H, W)
        out[:, :b] = 0
        out[:, H - b:] = 0
        out[:, :, :b] = 0
        out[:, :, W - b:] = 0
    return out
