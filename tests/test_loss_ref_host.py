"""tests/loss_ref.py against the recorded outputs of the reference modules (tests/golden/losses.npz, extras.npz): the
float64 restatement the GPU tests compare the kernels with is pinned to the reference here, at 1e-6 relative (the
fixtures hold the reference's fp32 results).  Runs without a GPU."""
import numpy as np
import pytest
import torch

import loss_ref as LR
from helpers import assert_close

TOL = 1e-6


def _t64(g, k):
    return g.t(k).double()


@pytest.mark.parametrize("tag", ["full", "cross_only"])
@pytest.mark.parametrize("form", ["dense", "labels"])
def test_cross_loss_matches_reference(golden, tag, form):
    g = golden("losses.npz")
    cb_kd = _t64(g, tag + "/cb").t().contiguous()          # the fixture holds the reference's (D, K)
    K = cb_kd.shape[0]
    e1 = _t64(g, tag + "/e1").requires_grad_(True)
    e2 = _t64(g, tag + "/e2").requires_grad_(True)
    ids1, ids2 = g.t(tag + "/ids1"), g.t(tag + "/ids2")
    if form == "dense":
        r1, r2 = (LR.onehot(i, K + 1)[:, 1:] for i in (ids1, ids2))
        lc = LR.cross_loss_dense(e1, r2, cb_kd) + LR.cross_loss_dense(e2, r1, cb_kd)      # embed_loss.py:31-34
    else:
        lc = LR.cross_loss_labels(e1, ids2, cb_kd) + LR.cross_loss_labels(e2, ids1, cb_kd)
    lc.backward()
    assert_close(lc, g[tag + "/l_cross"], TOL, "l_cross")
    assert_close(e1.grad, g[tag + "/ge1"], TOL, "ge1")
    assert_close(e2.grad, g[tag + "/ge2"], TOL, "ge2")


@pytest.mark.parametrize("tag", ["full", "cross_only"])
def test_onehot_matches_reference(golden, tag):
    g = golden("losses.npz")
    K = g[tag + "/cb"].shape[1]
    assert np.array_equal(LR.onehot(g.t(tag + "/ids1"), K + 1).numpy(), g[tag + "/onehot1"])


@pytest.mark.parametrize("name", ["dice", "dice_ign", "focal"])
def test_seg_losses_match_reference(golden, name):
    g = golden("losses.npz")
    z = _t64(g, "seg/logits").requires_grad_(True)
    t = _t64(g, "seg/target")
    l = {"dice": lambda: LR.soft_dice(z, t), "dice_ign": lambda: LR.soft_dice(z, t, ignore_index=0),
         "focal": lambda: LR.focal(z, t)}[name]()
    l.backward()
    assert_close(l, g["seg/" + name], TOL, name)
    assert_close(z.grad, g["seg/g_" + name], TOL, "g_" + name)


def test_dropblock_matches_reference(golden):
    g, ge = golden("losses.npz"), golden("extras.npz")
    for block, key in ((4, "keep4"), (5, "keep5")):
        keep, _ = LR.dropblock_keep(_t64(g, "dropblock/seed4"), block)
        assert np.array_equal(keep.numpy(), g["dropblock/" + key])
    keep, scale = LR.dropblock_keep(_t64(ge, "dropblock/seed"), 4)
    assert_close(LR.dropblock_apply(_t64(ge, "dropblock/x"), keep, scale), ge["dropblock/y"], TOL, "dropblock y")


def test_exact_maps_are_self_consistent():
    """flip_labels has no recorded fixture: check it against its definition element by element on a tiny map."""
    ids = torch.arange(1, 2 * 5 * 4 + 1).reshape(2, 5, 4)
    out = LR.flip_labels(ids, 1)
    for b in range(2):
        for h in range(5):
            for w in range(4):
                inside = 1 <= h < 4 and 1 <= w < 3
                assert int(out[b, h, w]) == (int(ids[b, h, 3 - w]) if inside else 0)
    assert int(LR.flip_labels(ids, 3).abs().sum()) == 0
    assert np.array_equal(LR.flip_labels(ids, 0).numpy(), ids.numpy()[:, :, ::-1])
