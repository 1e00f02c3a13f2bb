"""The sample scores on the GPU: ops.feature_moments, ops.knn_radius and ops.ball_counts against the float64 restatement of
tests/sample_scores_ref.py, and functions.sample_scores composed from them.

Bounds.  u = 2^-24.  Every bound is against float64 arithmetic over the same fp32 centred rows y = fp32(x - shift).
  moments   |sum - ref| <= 2 N 2^-53 sum_n |y| and |outer - ref| <= 2 N 2^-53 |Y|^T |Y| elementwise (R.moments_bounds).
  radii     |r2 - ref| <= max_j e(i, j), e(q, a) = (D + 4) u (|q|^2 + |a|^2 + 2 sum_i |q_i a_i|) (R.dist_err).
  counts    exact: tests/test_sample_scores_host.py asserts that every decision of these fixtures is clear of e + u r2.
  Frechet   FRECHET_RTOL below.
"""
import numpy as np
import pytest
import torch

import sample_scores_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# The Frechet distance of the composed case against the restatement, relative to tr S_a + tr S_b.  Both sides evaluate the same
# formula in float64 from moments that differ by the moment bounds above: relative 2 N 2^-53 = 5.7e-14 at N = 257 on sums of
# non-negative squares (the traces), and on the covariances' off-diagonal entries absolute 5.7e-14 |Y|^T |Y| / (N - 1), about
# 5.7e-14 E|y_i y_j| N / (N - 1) ~ 4e-14 of a unit variance.  The distance is Lipschitz in the covariances except through the
# square roots, whose condition is 1 / (2 sqrt(lambda_min)); the fixtures' covariances at N = 257, 193 and D = 48 have
# lambda_min ~ (1 - sqrt(D / N))^2 >= 0.25, so the condition is at most 1, and the perturbation of a trace of D = 48 eigenvalues is at
# most D times the entry bound: 48 * 5.7e-14 * 2 (two covariances) * 2 (eigh's own backward error on either side) ~ 1.1e-11
# absolute on a trace sum of ~ 100, i.e. 1.1e-13 relative.  The tolerance is that rounded up to 1e-12.
FRECHET_RTOL = 1e-12


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ moments
def _moment_rows(N, D, shifted):
    rng = np.random.default_rng(100 + N + D)
    x = rng.standard_normal((N, D)).astype(np.float32)
    shift = None
    if shifted:
        shift = (R.SHIFT_SIGMA * rng.standard_normal(D)).astype(np.float32)
        x = x + shift[None, :]
    return x, shift


def _run_moments(batches, shift, D):
    from hipops import ops
    s = torch.zeros(D, dtype=torch.float64, device=DEV)
    o = torch.zeros((D, D), dtype=torch.float64, device=DEV)
    for b in batches:
        assert ops.feature_moments(_dev(b), s, o, _dev(shift)) is None
    return _np(s), _np(o)


def _check_moments(s, o, x, shift):
    y = R.centred(x, shift)
    rs, ro = R.moments(y)
    bs, bo = R.moments_bounds(y)
    es, eo = np.abs(s - rs), np.abs(o - ro)
    print("moments %s: sum err / bound %.3g, outer err / bound %.3g" % (x.shape, (es / np.maximum(bs, 1e-300)).max(),
                                                                      (eo / np.maximum(bo, 1e-300)).max()))
    assert (es <= bs).all()
    assert (eo <= bo).all()
    assert np.array_equal(o, o.T), "outer is not exactly symmetric"


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("N,D", R.MOMENT_CASES)
def test_feature_moments(N, D, shifted):
    x, shift = _moment_rows(N, D, shifted)
    s, o = _run_moments([x], shift, D)
    _check_moments(s, o, x, shift)
    s2, o2 = _run_moments([x], shift, D)
    assert s.tobytes() == s2.tobytes() and o.tobytes() == o2.tobytes(), "two runs differ"


@pytest.mark.parametrize("shifted", [False, True])
def test_feature_moments_accumulate_over_unequal_batches(shifted):
    x, shift = _moment_rows(1000, 100, shifted)
    s, o = _run_moments([x[:7], x[7:400], x[400:]], shift, 100)
    _check_moments(s, o, x, shift)
    s2, o2 = _run_moments([x[:7], x[7:400], x[400:]], shift, 100)
    assert s.tobytes() == s2.tobytes() and o.tobytes() == o2.tobytes(), "two runs of one call sequence differ"


# ------------------------------------------------------------------------------------------------ radii
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("N,D,k", R.KNN_CASES + R.KNN_WIDE_CASES)
def test_knn_radius(N, D, k, shifted):
    from hipops import ops
    a, _, shift = R.fixture_sets(N, 1, D, seed=N + D, shifted=shifted)
    got = _np(ops.knn_radius(_dev(a), k, _dev(shift))).astype(np.float64)
    y = R.centred(a, shift)
    ref, bound = R.knn_radius(y, k), R.knn_radius_bound(y)
    err = np.abs(got - ref)
    print("knn_radius (%d, %d, %d): err / bound %.3g" % (N, D, k, (err / bound).max()))
    assert got.shape == (N,) and (err <= bound).all()


@pytest.mark.parametrize("k", [1, 2])
def test_knn_radius_of_bit_identical_rows_is_exactly_zero(k):
    from hipops import ops
    a, _, shift = R.fixture_sets(70, 1, 48, seed=3, shifted=True)
    a[5] = a[40]
    a[69] = a[40]               # three copies, in two different centre tiles and both halves of a wave's block
    got = _np(ops.knn_radius(_dev(a), k, _dev(shift)))
    assert (got[[5, 40, 69]] == 0.0).all(), got[[5, 40, 69]]
    others = np.delete(got, [5, 40, 69])
    assert (others > 0).all()


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("N,M,D,k", R.BALL_CASES)
def test_ball_counts(N, M, D, k, shifted):
    from hipops import ops
    a, q, shift, r2 = R.ball_fixture(N, M, D, k, shifted)
    ya, yq = R.centred(a, shift), R.centred(q, shift)
    assert R.ball_margin(yq, ya, r2) > 0, "the fixture has an unclear decision: take another seed"
    cnt_q, hit_a = ops.ball_counts(_dev(q), _dev(a), _dev(r2), _dev(shift))
    rc, rh = R.ball_counts(yq, ya, r2)
    assert cnt_q.dtype == torch.int32 and hit_a.dtype == torch.int32
    assert np.array_equal(_np(cnt_q), rc) and np.array_equal(_np(hit_a), rh)
    cnt2, hit2 = ops.ball_counts(_dev(q), _dev(a), _dev(r2), _dev(shift))
    assert torch.equal(cnt2, cnt_q) and torch.equal(hit2, hit_a)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("N,M,D,k", R.NEAR_CASES)
def test_ball_counts_at_512_columns_with_pairs_inside(N, M, D, k, shifted):
    from hipops import ops
    a, q, shift, r2 = R.near_fixture(N, M, D, k, shifted)
    ya, yq = R.centred(a, shift), R.centred(q, shift)
    assert R.ball_margin(yq, ya, r2) > 0, "the fixture has an unclear decision: take another seed"
    rc, rh = R.ball_counts(yq, ya, r2)
    assert rc.sum() >= 1 and (rc == 0).sum() >= (1 if M > 1 else 0)          # the case decides something
    cnt_q, hit_a = ops.ball_counts(_dev(q), _dev(a), _dev(r2), _dev(shift))
    assert np.array_equal(_np(cnt_q), rc) and np.array_equal(_np(hit_a), rh)


def test_ball_counts_duplicate_row_is_inside_and_nan_radius_holds_nobody():
    from hipops import ops
    a, q, shift, r2 = R.ball_fixture(130, 67, 20, 1, shifted=True)
    q[11] = a[77]               # a row shared by Q and A: distance exactly 0 <= any radius
    r2[3] = np.nan
    r2[77] = 0.0                # the inclusive rule at the distance-0 row itself
    cnt_q, hit_a = ops.ball_counts(_dev(q), _dev(a), _dev(r2), _dev(shift))
    assert int(hit_a[77]) == 1 and int(cnt_q[11]) >= 1
    assert int(hit_a[3]) == 0


# ------------------------------------------------------------------------------------------------ composed
@pytest.mark.parametrize("shifted", [False, True])
def test_sample_scores_composed(shifted):
    from functions import FeatureStats, sample_scores
    from hipops import ops
    N, M, D, k = R.COMPOSED_CASE
    real, fake, shift = R.fixture_sets(N, M, D, seed=R.COMPOSED_SEED, shifted=shifted)
    yr, yf = R.centred(real, shift), R.centred(fake, shift)
    # the kernel's own radii, and the CPU's word that every decision under them is clear of e + max_j e(i, j) + u r2
    r2_real = _np(ops.knn_radius(_dev(real), k, _dev(shift))).astype(np.float64)
    r2_fake = _np(ops.knn_radius(_dev(fake), k, _dev(shift))).astype(np.float64)
    assert R.ball_margin(yf, yr, R.knn_radius(yr, k), R.knn_radius_bound(yr)) > 0
    assert R.ball_margin(yr, yf, R.knn_radius(yf, k), R.knn_radius_bound(yf)) > 0
    sr, sf = FeatureStats(D, _dev(shift), keep=N), FeatureStats(D, _dev(shift), keep=M)
    sr.add(_dev(real[:100]))
    sr.add(_dev(real[100:]))
    sf.add(_dev(fake))
    got = sample_scores(sr, sf, k)
    ref = R.manifold_scores(yr, yf, k, r2_real, r2_fake)
    for key in ("precision", "recall", "density", "coverage"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert ref == R.manifold_scores(yr, yf, k), "the kernel's radii decide a pair differently from the restatement's"
    (_, mr, cr), (_, mf, cf) = R.mean_cov(yr, shift), R.mean_cov(yf, shift)
    fd = R.frechet(mr, cr, mf, cf)
    scale = np.trace(cr) + np.trace(cf)
    print("frechet %.12g vs %.12g: |diff| / traces %.3g" % (got["frechet"], fd, abs(got["frechet"] - fd) / scale))
    assert abs(got["frechet"] - fd) <= FRECHET_RTOL * scale
    assert (got["n_real"], got["n_fake"], got["D"], got["k"], got["rank_deficient"]) == (N, M, D, k, 0)
    assert np.abs(sr.mean().numpy() - mr).max() <= 1e-12 * (1 + np.abs(mr).max())


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_features_and_score():
    """PriorTrainer.features is the pooled encoder output; score() is a function of the generator's seed, counts what it was given,
    splits the floor by arrival parity across batch boundaries, takes top_p (the generate_masked route) and encodes a held-out slice once."""
    import gpt_ref as G
    import prior_ref as P
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    torch.manual_seed(77)
    vqgan = VQGAN(**P.TINY_VQGAN)
    gpt = G.init_gpt_(GPT(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64), 611)
    tr = PriorTrainer(vqgan, gpt, seed=17, device=DEV)
    images = torch.rand((21, 1, 8, 8), generator=torch.Generator().manual_seed(5)) * 2 - 1
    f = tr.features(images[:5])
    assert f.shape == (5, 32) and f.dtype == torch.float32
    assert torch.equal(f, tr.vqgan.encoder(images[:5].to(DEV)).mean(dim=(2, 3)))
    batches = [images[0:7], {"image": images[7:21]}]
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)  # noqa: E731
    kw = dict(n_samples=9, batch_size=4, k=2, top_k=16)
    a = tr.score(batches, top_p=0.9, generator=gen(), **kw)
    assert a == tr.score(batches, top_p=0.9, generator=gen(), **kw)
    assert (a["scores"]["n_real"], a["scores"]["n_fake"], a["scores"]["D"], a["scores"]["k"]) == (21, 9, 32, 2)
    assert (a["floor"]["n_real"], a["floor"]["n_fake"]) == (11, 10)          # even arrival indices 0, 2, .., 20 against the odd ones
    b = tr.score(batches, generator=gen(), against="recon", **kw)
    # against='image' takes codes and features from ONE encoder pass: the same rows as features() of the slices
    from functions import FeatureStats, sample_scores
    f = tr.features(images)
    st = [FeatureStats(32, f[:7].mean(dim=0), keep=21) for _ in range(2)]
    st[0].add(f[0::2])
    st[1].add(f[1::2])
    want = sample_scores(st[0], st[1], 2, tr.codes(images)[0::2], tr.codes(images)[1::2], 64)
    # (other batch sizes and another order of the double sums; the sets are rank deficient, n <= D, where a perturbation eps of a
    # covariance moves the Frechet distance by sqrt(eps) of the traces: fp32 features, eps ~ 1e-7, so 1e-3 is what can be asked)
    got = dict(a["floor"])
    assert got.pop("frechet") == pytest.approx(want.pop("frechet"), rel=1e-3)
    assert got == pytest.approx(want, rel=1e-9, abs=1e-12)
    for res in (a, b):
        for part in ("scores", "floor"):
            assert all(np.isfinite(v) for v in res[part].values()), res[part]
            assert all(0.0 <= res[part][key] <= 1.0 for key in ("precision", "recall", "coverage"))
    with pytest.raises(ValueError, match="k \\+ 1"):
        tr.score(batches, n_samples=2, k=2)
    with pytest.raises(ValueError, match="each half"):
        tr.score([images[:4]], n_samples=9, k=2)
    with pytest.raises(ValueError, match="against"):
        tr.score(batches, n_samples=9, against="reconstruction")


def test_conditional_trainer_scores_one_sample_per_slice():
    """ConditionalPriorTrainer.score: the held-out slices' own label maps condition the draws, one per slice, with and without
    guidance; a seed repeats the result; another n_samples is refused."""
    import gpt_ref as G
    import prior_ref as P
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer
    torch.manual_seed(5)
    vqgan = VQGAN(**P.TINY_VQGAN)
    gpt = G.init_gpt_(GPT(vocab_size=64, block_size=32, n_layer=2, n_head=2, n_embed=64, n_unmasked=16), 5)
    tr = ConditionalPriorTrainer(vqgan, gpt, LabelCondition(2, 64, 4, 4, null_token=True), device=DEV)
    g = torch.Generator().manual_seed(6)
    images = torch.rand((14, 1, 8, 8), generator=g) * 2 - 1
    labels = (torch.rand((14, 1, 8, 8), generator=g) < 0.4).to(torch.uint8)
    batches = [{"image": images[i:i + 7], "label": labels[i:i + 7].to(DEV)} for i in (0, 7)]
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)  # noqa: E731
    kw = dict(n_samples=14, batch_size=4, k=2, top_k=16)
    plain = tr.score(batches, generator=gen(), **kw)
    assert plain == tr.score(batches, generator=gen(), **kw)
    guided = tr.score(batches, generator=gen(), guidance_scale=2.0, **kw)
    for res in (plain, guided):
        assert (res["scores"]["n_real"], res["scores"]["n_fake"]) == (14, 14) and (res["floor"]["n_real"], res["floor"]["n_fake"]) == (7, 7)
        assert all(np.isfinite(v) for part in res.values() for v in part.values())
    assert plain["floor"] == guided["floor"]          # the floor does not see the samples
    with pytest.raises(ValueError, match="one sample is drawn per held-out slice"):
        tr.score(batches, generator=gen(), **dict(kw, n_samples=9))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("masked", [False, True])
def test_launcher_scores_a_trained_prior(tmp_path, masked):
    """run_vqwnet.py -p trains a tiny prior for two steps; -p -m score, run twice with one seed, writes the same bytes; every score
    is finite, the floor's shares lie in [0, 1] and the counts are what the config asked for."""
    import json
    import math
    import os
    import prior_ref as P
    from run_helpers import read_csv, run_launcher, write_config
    save = os.path.join(str(tmp_path), "run")

    def config(**run):
        raw = P.prior_run_config(save, **run)
        raw["dataset"]["n_samples_test"] = 16
        if masked:
            raw["model"]["prior"]["masked"] = dict(n_steps=3, choice_temperature=4.5, mask_seed=4)
        return raw

    run_launcher(write_config(os.path.join(str(tmp_path), "train.json"), config()), "-p")
    ckpt = os.path.join(save, "study", "version_0", "ckpt-epoch=0000-total_loss=0.00.ckpt")
    assert os.path.exists(ckpt)
    raw = config(resume_checkpoint=ckpt)
    raw["score"] = dict(n_slices=12, n_samples=8, batch_size=4, k=2, temperature=1.0, top_k=4, top_p=0.9 if masked else False,
                        against="recon", seed=5, guidance_scale=False)
    if masked:
        raw["score"]["n_steps"] = 2
    path = write_config(os.path.join(str(tmp_path), "score.json"), raw)
    files = []
    for version in (1, 2):
        out = run_launcher(path, "-p", "-m", "score")
        assert "Loading model from" in out and "Scores are saved" in out
        sdir = os.path.join(save, "study", "version_%d" % version, "score")
        assert sorted(os.listdir(sdir)) == ["score.csv", "score.json"]
        files.append([open(os.path.join(sdir, name), "rb").read() for name in ("score.csv", "score.json")])
    assert files[0] == files[1], "one seed, two runs: the files differ"
    header, rows = read_csv(os.path.join(sdir, "score.csv"))
    assert header == ["score", "value", "floor"]
    value, floor = {r[0]: float(r[1]) for r in rows}, {r[0]: float(r[2]) for r in rows}
    for key in ("frechet", "precision", "recall", "density", "coverage", "code_js_bits", "code_entropy_real", "code_entropy_fake",
                "code_usage_real", "code_usage_fake"):
        assert math.isfinite(value[key]) and math.isfinite(floor[key]), key
    for key in ("precision", "recall", "coverage"):
        assert 0.0 <= floor[key] <= 1.0 and 0.0 <= value[key] <= 1.0, key
    assert (value["n_real"], value["n_fake"], value["k"], value["D"]) == (12, 8, 2, 32)
    assert (floor["n_real"], floor["n_fake"]) == (6, 6)
    js = json.load(open(os.path.join(sdir, "score.json")))
    assert js["scores"]["frechet"] == value["frechet"] and js["floor"]["frechet"] == floor["frechet"]
    assert js["config"]["seed"] == 5 and js["config"]["n_slices"] == 12 and js["config"]["against"] == "recon"
    assert js["config"].get("n_steps") == (2 if masked else None)
