"""Test-mode metrics on the GPU: hipops.ops.recon_metrics / code_entropy, the torchmetrics drop-ins and the Evaluator
against the float64 restatement in metrics_ref.  Each image metric must lie within twice the distance of the package's
own fp32 arithmetic (the fp32 ATen restatement on the CPU, per case) from float64, with a floor of 1e-6."""
import math

import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tanh_pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.tanh(torch.randn(shape, generator=g))
    p = torch.tanh(torch.atanh(t.clamp(-0.999, 0.999)) + 0.2 * torch.randn(shape, generator=g))
    return p, t


def _check(pred, target, got, data_range=None, **kw):
    ref64 = R.package_form(pred, target, data_range, dtype=torch.float64, **kw)
    ref32 = R.package_form(pred, target, data_range, dtype=torch.float32, **kw)
    for k in ("mse", "ssim", "psnr"):
        g = float(got[k])
        dist = abs(ref32[k] - ref64[k]) if math.isfinite(ref32[k] - ref64[k]) else 0.0
        tol = max(2.0 * dist, 1e-6)
        assert R.close(g, ref64[k], tol), "%s: %r vs float64 %r (tol %.3g, fp32 form %r)" % (k, g, ref64[k], tol, ref32[k])


def _run(p, t, **kw):
    from hipops import ops
    return ops.recon_metrics(p.to(DEV), t.to(DEV), **kw)


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (3, 1, 37, 53), (64, 1, 256, 256), (2, 1, 512, 512), (2, 3, 40, 48)])
def test_metrics_match_float64(shape):
    p, t = _tanh_pair(shape, seed=sum(shape))
    _check(p, t, _run(p, t))


def test_channels_last_input_with_three_channels():
    p, t = _tanh_pair((2, 3, 33, 35), seed=5)
    got = _run(p.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last))
    _check(p, t, got)


def test_given_data_range():
    p, t = _tanh_pair((4, 1, 64, 64), seed=1)
    _check(p, t, _run(p, t, data_range=2.0), data_range=2.0)


def test_other_window():
    p, t = _tanh_pair((2, 1, 40, 40), seed=2)
    _check(p, t, _run(p, t, kernel_size=7, sigma=1.0), kernel_size=7, sigma=1.0)


def test_all_positive_target_uses_the_zero_seeded_range():
    p, t = _tanh_pair((4, 1, 64, 64), seed=3)
    p, t = 0.5 + 0.25 * (p + 1), 0.5 + 0.25 * (t + 1)
    got = _run(p, t)
    _check(p, t, got)
    mse = float(((p.double() - t.double()) ** 2).mean())
    assert abs(float(got["psnr"]) - 10 * math.log10(float(t.max()) ** 2 / mse)) < 1e-6


def test_equal_images():
    p, _ = _tanh_pair((2, 1, 48, 48), seed=4)
    got = _run(p, p)
    # MSE exactly 0 and PSNR +inf as in the package; SSIM 1 within the suite's 1e-6 floor (measured: 1 - 2.4e-10)
    assert float(got["mse"]) == 0.0 and abs(float(got["ssim"]) - 1.0) <= 1e-6 and float(got["psnr"]) == math.inf


def test_constant_batch_is_nan():
    p = torch.full((2, 1, 32, 32), 0.25)
    got = _run(p, p * 2)       # range 0: C1 = C2 = 0, zero variance -> 0 / 0 as in the package's exact arithmetic
    assert math.isnan(float(got["ssim"]))
    mse = 0.25 ** 2
    assert abs(float(got["mse"]) - mse) < 1e-12
    assert abs(float(got["psnr"]) - 10 * math.log10(0.5 ** 2 / mse)) < 1e-9


def test_low_contrast_plane():
    g = torch.Generator().manual_seed(6)
    t = 0.3 + 1e-3 * torch.randn((8, 1, 256, 256), generator=g)
    p = t + 3e-4 * torch.randn((8, 1, 256, 256), generator=g)
    _check(p, t, _run(p, t))


@pytest.mark.parametrize("K", [10, 64, 1024])
def test_entropy_and_counts(K):
    from hipops import ops
    g = torch.Generator().manual_seed(K)
    ids = torch.randint(0, K // 2 + 1, (16, 64, 64), generator=g)      # id-0 pixels; bins above K/2 empty
    want, counts = R.entropy(ids, K)
    H, c = ops.code_entropy(ids.to(DEV), K)
    assert torch.equal(c.cpu(), torch.from_numpy(counts).to(torch.int64))
    assert abs(float(H) - want) <= 1e-12 * max(1.0, abs(want))
    p, t = _tanh_pair((16, 1, 64, 64), seed=K)
    got = ops.recon_metrics(p.to(DEV), t.to(DEV), ids.to(DEV), K)
    assert float(got["entropy"]) == float(H)
    assert math.isnan(float(ops.code_entropy(torch.zeros(5, dtype=torch.int64, device=DEV), K)[0]))


def test_out_of_range_ids_raise():
    from hipops import ops
    ids = torch.ones(4, 16, 16, dtype=torch.int64)
    for bad in (11, -1):
        ids[1, 2, 3] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.code_entropy(ids.to(DEV), 10)
        p, t = _tanh_pair((4, 1, 16, 16))
        with pytest.raises(ValueError, match="outside"):
            ops.recon_metrics(p.to(DEV), t.to(DEV), ids.to(DEV), 10)


def test_two_calls_are_bit_identical():
    from hipops import ops
    p, t = _tanh_pair((64, 1, 256, 256), seed=7)
    ids = torch.randint(1, 11, (64, 256, 256), generator=torch.Generator().manual_seed(7)).to(DEV)
    p, t = p.to(DEV), t.to(DEV)
    a = ops._recon_metrics_out(p, t, ids, 10, None, 11, 1.5, 0.01, 0.03).cpu()
    b = ops._recon_metrics_out(p, t, ids, 10, None, 11, 1.5, 0.01, 0.03).cpu()
    assert torch.equal(a[:11].view(torch.int64), b[:11].view(torch.int64))


def test_transposed_ids_view_counts_without_a_copy():
    from hipops import ops
    base = torch.randint(0, 11, (4, 40, 24), generator=torch.Generator().manual_seed(8)).to(DEV)
    view = base.transpose(1, 2)                                # as the encoder returns ids (unet_encoder.py:86)
    assert not view.is_contiguous()
    assert ops._dense_storage(view).data_ptr() == base.data_ptr()
    H1, c1 = ops.code_entropy(view, 10)
    H2, c2 = ops.code_entropy(view.contiguous(), 10)
    assert torch.equal(c1, c2) and float(H1) == float(H2)


def test_drop_in_classes_forward_update_compute():
    from functions import MeanSquaredError, PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure, label_entropy
    p1, t1 = _tanh_pair((2, 1, 32, 32), seed=9)
    p2, t2 = _tanh_pair((3, 1, 32, 32), seed=10)
    t2 = 0.5 * (t2 + 1.0)                              # changes the zero-seeded target range between batches
    mse, psnr, ssim = MeanSquaredError(), PeakSignalNoiseRatio(), StructuralSimilarityIndexMeasure()
    for m, key in ((mse, "mse"), (psnr, "psnr"), (ssim, "ssim")):
        v1 = float(m(p1.to(DEV), t1.to(DEV)))
        assert R.close(v1, R.package_form(p1, t1)[key], 1e-6), key          # forward: that batch alone
        m.update(p2.to(DEV), t2.to(DEV))
    P = torch.cat([p1, p2]).double()
    T = torch.cat([t1, t2]).double()
    assert R.close(float(mse.compute()), float(R.mse(P, T)), 1e-9)
    assert R.close(float(psnr.compute()), float(R.psnr(P, T)), 1e-6)
    assert R.close(float(ssim.compute()), float(R.ssim_padded(P, T)), 1e-6)
    rmse = MeanSquaredError(squared=False)
    assert R.close(float(rmse(p1.to(DEV), t1.to(DEV))), math.sqrt(R.package_form(p1, t1)["mse"]), 1e-9)
    ids = torch.randint(0, 11, (2, 32, 32), generator=torch.Generator().manual_seed(11))
    assert R.close(label_entropy(ids.to(DEV), 10), R.entropy(ids, 10)[0], 1e-12)


def _small_models(K):
    from networks import UNetEncoder, UNetDecoder
    torch.manual_seed(0)
    enc = UNetEncoder(1, [16, 32, 64, 128, 256], K, 0.999, 'torch', False, 1, True).to(DEV)
    dec = UNetDecoder(16, 1, [32, 64, 128, 256, 512], use_dropblock=False, dropped_skip_layers=[],
                      use_pixel_shuffle=False).to(DEV)
    return enc, dec


def test_evaluator_end_to_end(tmp_path):
    import numpy as np
    from trainers import Evaluator
    K = 10
    enc, dec = _small_models(K)
    g = torch.Generator().manual_seed(12)
    loader = [{"image": torch.tanh(torch.randn(4, 1, 64, 64, generator=g))} for _ in range(2)]
    ev = Evaluator(enc, dec, K, keep_outputs=True)
    outputs = []
    for batch in loader:
        o = ev.test_step(batch)
        assert list(o) == ["NMSE", "SSIM", "PSNR", "Entropy"]
        last = ev.last
        want = R.package_form(last["recon"], last["image"])
        _check(last["recon"], last["image"], dict(mse=o["NMSE"], ssim=o["SSIM"], psnr=o["PSNR"]))
        assert R.close(o["SSIM"], want["ssim"], 1e-6)
        H, _ = R.entropy(last["ids"], K)
        assert R.close(o["Entropy"], H, 1e-12)
        outputs.append(o)
    res = ev.test_epoch_end(outputs, str(tmp_path))
    for key in ("NMSE", "SSIM", "PSNR", "Entropy"):
        vals = np.array([o[key] for o in outputs])
        assert res[key + "_avg"] == float(np.mean(vals)) and res[key + "_std"] == float(np.std(vals))
    lines = (tmp_path / "result.csv").read_text().splitlines()
    assert lines[0] == "," + ",".join(res)
    assert [float(x) for x in lines[1].split(",")[1:]] == list(res.values())
    assert enc.training and dec.training                     # modes restored
    again = ev.run(loader, str(tmp_path / "run"))
    for k, v in res.items():
        assert R.close(again[k], v, 1e-6 * max(1.0, abs(v))), k


def test_first_step_trainer_test_step_leaves_training_state():
    from trainers import FirstStepTrainer, FlipViews
    K = 10
    enc, dec = _small_models(K)
    tr = FirstStepTrainer(dict_size=K, views=FlipViews(border=2), encoder=enc, decoder=dec, device=DEV)
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    o = tr.test_step({"image": torch.tanh(torch.randn(2, 1, 32, 32))})
    assert set(o) == {"NMSE", "SSIM", "PSNR", "Entropy"} and all(math.isfinite(v) for v in o.values())
    after = enc.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
