"""Test-mode metrics, CPU side (no GPU): the float64 restatement of the torchmetrics 0.6.2 / scipy contract on its own
known answers, result.csv in pandas' layout, the C ABI and dispatcher entries, argument validation, and the drop-in
classes' signatures."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqw_recon_metrics_ws_bytes", "vqw_recon_metrics", "vqw_code_entropy")


def _pair(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    t = torch.tanh(torch.randn(shape, generator=g, dtype=dtype))
    p = torch.tanh(torch.atanh(t.clamp(-0.999, 0.999)) + 0.2 * torch.randn(shape, generator=g, dtype=dtype))
    return p, t


@pytest.mark.parametrize("shape,ks,sigma", [((2, 1, 23, 31), 11, 1.5), ((1, 3, 16, 16), 7, 1.0), ((1, 1, 11, 11), 11, 1.5)])
def test_padded_and_cropped_equals_valid_windows(shape, ks, sigma):
    p, t = _pair(shape)
    a = R.ssim_padded(p, t, ks, sigma)
    b = R.ssim_valid(p, t, ks, sigma)
    assert abs(float(a) - float(b)) <= 1e-14, (float(a), float(b))


def test_gaussian_window_matches_the_package_definition():
    g = R.gaussian(11, 1.5)
    d = np.arange(-5, 6, dtype=np.float64)
    e = np.exp(-(d / 1.5) ** 2 / 2)
    assert np.allclose(g.numpy(), e / e.sum(), rtol=0, atol=1e-16)


def test_psnr_all_positive_target_uses_the_zero_seeded_range():
    p, t = _pair((2, 1, 16, 16))
    t = 0.5 + 0.25 * (t + 1)                    # in [0.5, 1]: min(t) > 0
    p = t + 0.01 * torch.sin(torch.arange(t.numel(), dtype=t.dtype)).reshape(t.shape)
    mse = float(((p - t) ** 2).mean())
    want = 10 * math.log10(float(t.max()) ** 2 / mse)              # range = max(t) - 0
    naive = 10 * math.log10(float(t.max() - t.min()) ** 2 / mse)
    got = float(R.psnr(p, t))
    assert abs(got - want) <= 1e-10 and abs(got - naive) > 1.0
    assert abs(float(R.psnr(p, t, data_range=2.0)) - 10 * math.log10(4.0 / mse)) <= 1e-10


def test_constant_batch_gives_nan_ssim():
    # range 0 -> C1 = C2 = 0 and a zero variance: 0 / 0.  (With a non-zero constant the rounding of E[x^2] - mu^2 in
    # either precision leaves a residue instead; the kernel's shifted moments are exact there and give nan too.)
    x = torch.zeros((1, 1, 16, 16), dtype=torch.float64)
    assert math.isnan(float(R.ssim_padded(x, x))) and math.isnan(float(R.psnr(x, x)))


def test_entropy_matches_scipy_or_the_numpy_formula():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 8, (4, 32, 32), generator=g)             # id 0 present; bins 8..10 empty
    H, counts = R.entropy(ids, 10)
    assert counts.shape == (11,) and counts[9] == 0 and counts[0] > 0
    try:
        from scipy.stats import entropy
        want = float(entropy(counts[1:], base=2))
    except ImportError:
        c = counts[1:][counts[1:] > 0] / counts[1:].sum()
        want = float(-(c * np.log2(c)).sum())
    assert abs(H - want) <= 1e-12
    assert math.isnan(R.entropy(torch.zeros(5, dtype=torch.int64), 10)[0])


def _result():
    return {"NMSE_avg": 0.0123456789, "NMSE_std": 1e-05, "SSIM_avg": 0.75, "SSIM_std": 0.0, "PSNR_avg": 21.3,
            "PSNR_std": float("inf"), "Entropy_avg": 3.1, "Entropy_std": float("nan")}


def test_result_csv_has_pandas_layout(tmp_path):
    from trainers.evaluation import write_result_csv
    res = _result()
    path = tmp_path / "result.csv"
    write_result_csv(res, str(path))
    text = path.read_text()
    try:
        import pandas as pd
    except ImportError:
        pd = None
    if pd is not None:
        want = pd.DataFrame.from_dict({k: [v] for k, v in res.items()}).to_csv()
        assert text == want, (text, want)
        back = pd.read_csv(str(path), index_col=0)
        assert list(back.columns) == list(res)
        for k, v in res.items():
            assert R.close(float(back[k][0]), v, 0.0), k
    else:
        assert text == (",NMSE_avg,NMSE_std,SSIM_avg,SSIM_std,PSNR_avg,PSNR_std,Entropy_avg,Entropy_std\n"
                        "0,0.0123456789,1e-05,0.75,0.0,21.3,inf,3.1,\n")


def test_test_epoch_end_mean_and_population_std(tmp_path):
    from trainers import Evaluator
    outs = [dict(NMSE=0.1, SSIM=0.8, PSNR=20.0, Entropy=3.0), None, dict(NMSE=0.3, SSIM=0.6, PSNR=24.0, Entropy=2.0)]
    res = Evaluator(None, None, 10).test_epoch_end(outs, str(tmp_path))
    assert list(res) == ["NMSE_avg", "NMSE_std", "SSIM_avg", "SSIM_std", "PSNR_avg", "PSNR_std", "Entropy_avg",
                         "Entropy_std"]
    assert abs(res["NMSE_avg"] - 0.2) < 1e-15 and abs(res["NMSE_std"] - 0.1) < 1e-15
    assert res["PSNR_avg"] == 22.0 and res["PSNR_std"] == 2.0
    head = (tmp_path / "result.csv").read_text().splitlines()
    assert head[0] == "," + ",".join(res) and head[1].startswith("0,")


def test_new_symbols_in_header_signatures_and_dispatcher():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    declared = set(re.findall(r"\b(vqw_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 9 and lib.vqw_abi_version() == 9
    library.register()
    sch = str(torch.ops.vqw.recon_metrics.default._schema)
    for part in ("Tensor? pred", "Tensor? target", "Tensor? ids", "Tensor(a!)? out", "Tensor(b!)? counts", "Tensor(c!)? ws"):
        assert part in sch, (part, sch)
    sch = str(torch.ops.vqw.code_entropy.default._schema)
    assert "Tensor? ids" in sch and "Tensor(a!)? out" in sch and "Tensor(b!)? counts" in sch
    assert lib.vqw_recon_metrics_ws_bytes(64, 1, 256, 256, 10) >= 64 * 4 * 8 * 8
    assert lib.vqw_recon_metrics_ws_bytes(-1, 1, 8, 8, 10) == 0


def _call(lib, pred=None, target=None, ids=None, out=1, ws=1, ws_bytes=1 << 30, N=1, C=1, H=16, W=16, n_ids=0, K=10,
          ks=11, sigma=1.5, dr=0.0):
    return lib.vqw_recon_metrics(pred, target, ids, out, None, ws, ws_bytes, N, C, H, W, n_ids, K, ks, sigma, 0.01, 0.03,
                                 dr, None)


def test_argument_validation_before_device_work():
    from hipops import _lib
    L = _lib.load()
    fake = 4096                               # never dereferenced: every call below fails validation first
    assert _call(L, out=None) != 0 and b"vqw_recon_metrics" in L.vqw_last_error()
    assert _call(L) != 0 and b"nothing to compute" in L.vqw_last_error()
    assert _call(L, pred=fake) != 0 and b"together" in L.vqw_last_error()
    assert _call(L, pred=fake, target=fake, ks=10) != 0 and b"odd" in L.vqw_last_error()
    assert _call(L, pred=fake, target=fake, H=10) != 0 and b"at least" in L.vqw_last_error()
    assert _call(L, pred=fake, target=fake, ws_bytes=16) != 0 and b"workspace" in L.vqw_last_error()
    assert _call(L, ids=fake, n_ids=5, K=0) != 0 and b"K=0" in L.vqw_last_error()
    assert _call(L, ids=fake, n_ids=0) != 0 and b"no ids" in L.vqw_last_error()
    assert L.vqw_code_entropy(None, fake, None, fake, 1 << 20, 5, 10, None) != 0
    assert b"vqw_code_entropy" in L.vqw_last_error()


def test_ops_argument_errors_come_before_the_device():
    from hipops import ops
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match="odd"):
        ops.recon_metrics(x, x, kernel_size=10)
    with pytest.raises(ValueError, match="at least"):
        ops.recon_metrics(x[..., :10, :], x[..., :10, :])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.recon_metrics(x, x[:1])
    with pytest.raises(NotImplementedError, match="square"):
        ops.recon_metrics(x, x, kernel_size=(11, 7))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.recon_metrics(x, x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.code_entropy(torch.ones(4, dtype=torch.int64), 10)


def _params(cls):
    return [(p.name, p.default) for p in inspect.signature(cls.__init__).parameters.values() if p.name != "self"]


def test_drop_in_signatures_and_refusals():
    from functions import MeanSquaredError, PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure, label_entropy
    assert _params(MeanSquaredError) == [("compute_on_step", True), ("dist_sync_on_step", False), ("process_group", None),
                                         ("dist_sync_fn", None), ("squared", True)]
    assert _params(PeakSignalNoiseRatio) == [("data_range", None), ("base", 10.0), ("reduction", "elementwise_mean"),
                                             ("dim", None), ("compute_on_step", True), ("dist_sync_on_step", False),
                                             ("process_group", None), ("dist_sync_fn", None)]
    assert _params(StructuralSimilarityIndexMeasure) == [
        ("kernel_size", (11, 11)), ("sigma", (1.5, 1.5)), ("reduction", "elementwise_mean"), ("data_range", None),
        ("k1", 0.01), ("k2", 0.03), ("compute_on_step", True), ("dist_sync_on_step", False), ("process_group", None)]
    with pytest.raises(NotImplementedError):
        PeakSignalNoiseRatio(dim=(1, 2))
    with pytest.raises(NotImplementedError):
        PeakSignalNoiseRatio(reduction="sum")
    with pytest.raises(NotImplementedError):
        StructuralSimilarityIndexMeasure(reduction="none")
    with pytest.raises(NotImplementedError):
        StructuralSimilarityIndexMeasure(kernel_size=(11, 9))
    with pytest.raises(NotImplementedError):
        StructuralSimilarityIndexMeasure(sigma=(1.5, 1.0))
    with pytest.raises(NotImplementedError):
        MeanSquaredError(dist_sync_on_step=True)
    with pytest.raises(ValueError):
        StructuralSimilarityIndexMeasure(kernel_size=(10, 10))
    x = torch.zeros(1, 1, 16, 16)
    for m in (MeanSquaredError(), PeakSignalNoiseRatio(), StructuralSimilarityIndexMeasure()):
        with pytest.raises(RuntimeError, match="ROCm device"):
            m(x, x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        label_entropy(torch.ones(3, dtype=torch.int64), 10)


def test_trainers_expose_the_evaluator(tmp_path):
    import json
    from utils import load_json
    from trainers import FirstStepTrainer, SecondStepTrainer, Evaluator, build_evaluator
    assert callable(FirstStepTrainer.test_step) and callable(SecondStepTrainer.test_step)
    raw = json.load(open(os.path.join(ROOT, "configs", "baseline2_256x256_b32_1gpu.json")))
    path = tmp_path / "c.json"
    path.write_text(json.dumps(raw))
    ev = build_evaluator(load_json(str(path)), None, None)
    assert isinstance(ev, Evaluator) and ev.dict_size == raw["model"]["vqmodel"]["dict_size"]
