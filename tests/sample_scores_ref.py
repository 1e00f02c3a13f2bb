"""The sample scores (csrc/sample_scores.hip, functions/sample_scores.py) restated in numpy float64: the centred rows, the double
moments, the pairwise squared distances as sums of squared differences (no Gram form: nothing cancels), the k-th neighbour radii,
the ball counts, the Frechet distance by eigendecompositions, precision / recall / density / coverage and the code scores.  Also
the error model the GPU tests take their bounds from, and the fixtures they share with the host tests."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32


def centred(x, shift=None):
    """The rows the kernels use: fp32(x - shift), one fp32 subtraction per element -> float64."""
    x = np.asarray(x, dtype=np.float32)
    if shift is not None:
        x = x - np.asarray(shift, dtype=np.float32)[None, :]
    assert x.dtype == np.float32
    return x.astype(np.float64)


def moments(y):
    """(sum (D,), outer (D, D)) of float64 rows y."""
    return y.sum(axis=0), y.T @ y


def moments_bounds(y):
    """Elementwise bounds of |sum - ref| and |outer - ref| for double accumulation in any order: N 2^-53 sum |terms| covers
    one order (the products of fp32 values are exact in double), the factor 2 covers numpy's own order on the reference side."""
    n = y.shape[0]
    a = np.abs(y)
    return 2.0 * n * 2.0 ** -53 * a.sum(axis=0), 2.0 * n * 2.0 ** -53 * (a.T @ a)


def sqdist(q, a):
    """(M, N) float64: sum_i (q_i - a_i)^2, row by row."""
    out = np.empty((q.shape[0], a.shape[0]), dtype=np.float64)
    for m in range(q.shape[0]):
        d = a - q[m][None, :]
        out[m] = (d * d).sum(axis=1)
    return out


def dist_err(q, a):
    """e(q, a) = (D + 4) u (|q|^2 + |a|^2 + 2 sum_i |q_i a_i|): the worst case of two fp32 fmaf chains of length D (the norms),
    a third (the product, doubled) and the three-term combination."""
    D = q.shape[1]
    return (D + 4) * U * ((q * q).sum(1)[:, None] + (a * a).sum(1)[None, :] + 2.0 * (np.abs(q) @ np.abs(a).T))


def knn_radius(a, k):
    """r2[i] = the k-th smallest sqdist(i, j) over j != i, self excluded by index."""
    d = sqdist(a, a)
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, k - 1]


def knn_radius_bound(a):
    """max_j e(i, j) per row: an order statistic moves by at most the largest perturbation of its inputs."""
    e = dist_err(a, a)
    np.fill_diagonal(e, 0.0)
    return e.max(axis=1)


def ball_counts(q, a, r2):
    """(cnt_q (M,), hit_a (N,)) int64 with the inclusive rule d2 <= r2[i]; a NaN radius contains nobody."""
    inside = sqdist(q, a) <= np.asarray(r2, dtype=np.float64)[None, :]
    return inside.sum(axis=1), inside.sum(axis=0)


def ball_margin(q, a, r2, radius_err=None):
    """min over all pairs of |d2 - r2_i| - (e(q, a_i) + u r2_i [+ radius_err_i]): positive means every decision is clear."""
    r2 = np.asarray(r2, dtype=np.float64)
    slack = dist_err(q, a) + U * np.abs(r2)[None, :]
    if radius_err is not None:
        slack = slack + np.asarray(radius_err, dtype=np.float64)[None, :]
    return float((np.abs(sqdist(q, a) - r2[None, :]) - slack).min())


def mean_cov(y, shift=None):
    """(n, mean, unbiased covariance) of float64 rows y (the mean has the shift added back)."""
    n = y.shape[0]
    s, o = moments(y)
    m = s / n
    cov = (o - n * np.outer(m, m)) / (n - 1)
    return n, (m if shift is None else m + np.asarray(shift, dtype=np.float64)), cov


def _psd_sqrt(s):
    w, u = np.linalg.eigh((s + s.T) / 2)
    return (u * np.sqrt(np.clip(w, 0.0, None))[None, :]) @ u.T


def frechet(mu_a, cov_a, mu_b, cov_b):
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2, negative eigenvalues clipped to 0."""
    ra = _psd_sqrt(cov_a)
    m = ra @ cov_b @ ra
    w = np.linalg.eigvalsh((m + m.T) / 2)
    d = np.asarray(mu_a, dtype=np.float64) - np.asarray(mu_b, dtype=np.float64)
    return float(d @ d + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.sqrt(np.clip(w, 0.0, None)).sum())


def manifold_scores(real, fake, k, r2_real=None, r2_fake=None):
    """precision, recall, density, coverage of float64 rows (Kynkaanniemi et al. 2019; Naeem et al. 2020).  r2_*: radii to use in
    place of the restatement's own (the composed GPU test passes the kernel's)."""
    r2_real = knn_radius(real, k) if r2_real is None else r2_real
    r2_fake = knn_radius(fake, k) if r2_fake is None else r2_fake
    cnt_f, hit_r = ball_counts(fake, real, r2_real)
    cnt_r, _ = ball_counts(real, fake, r2_fake)
    return {"precision": float((cnt_f > 0).sum()) / fake.shape[0], "recall": float((cnt_r > 0).sum()) / real.shape[0],
            "density": float(cnt_f.sum()) / (k * fake.shape[0]), "coverage": float((hit_r > 0).sum()) / real.shape[0]}


def _entropy_bits(p):
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def code_scores(real_ids, fake_ids, V):
    """Jensen-Shannon divergence (bits) of the unigram code histograms, each side's entropy (bits) and codebook usage."""
    cr = np.bincount(np.asarray(real_ids).reshape(-1), minlength=V).astype(np.float64)
    cf = np.bincount(np.asarray(fake_ids).reshape(-1), minlength=V).astype(np.float64)
    p, q = cr / cr.sum(), cf / cf.sum()
    js = _entropy_bits((p + q) / 2) - 0.5 * _entropy_bits(p) - 0.5 * _entropy_bits(q)
    return {"code_js_bits": max(js, 0.0), "code_entropy_real": _entropy_bits(p), "code_entropy_fake": _entropy_bits(q),
            "code_usage_real": float((cr > 0).sum()) / V, "code_usage_fake": float((cf > 0).sum()) / V}


# ---------------------------------------------------------------------------------------------------------------------
# fixtures shared by tests/test_sample_scores_host.py (which asserts their margins) and tests/test_gpu_sample_scores.py
MOMENT_CASES = [(1, 4), (63, 16), (257, 48), (1000, 100), (513, 512)]
KNN_CASES = [(2, 3, 1), (9, 20, 8), (64, 48, 3), (65, 48, 3), (257, 48, 3), (130, 512, 5)]
BALL_CASES = [(257, 193, 48, 3), (130, 67, 20, 1), (300, 300, 8, 5), (64, 1, 512, 3)]
COMPOSED_CASE = (257, 193, 48, 3)
# the composed case's margin is wider (e + max_j e(i, j) + u r2): of the seeds 0 .. 11 the restatement finds 0, 1, 3, 7 and 10 with a
# pair inside it; seed 2 leaves 3.5e-3 beyond a margin of about 1e-3 (a choice made on the CPU, from the restatement alone)
COMPOSED_SEED = 2
SHIFT_SIGMA = 5.0


def fixture_sets(N, M, D, seed=0, shifted=False):
    """(real (N, D), fake (M, D), shift (D,) or None) fp32: standard-normal rows against rows of scale 1.1 offset by 0.1; with
    `shifted` both sit SHIFT_SIGMA sigma from the origin and the shift takes them back."""
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((N, D)).astype(np.float32)
    fake = (1.1 * rng.standard_normal((M, D)) + 0.1).astype(np.float32)
    if not shifted:
        return real, fake, None
    shift = np.full(D, SHIFT_SIGMA, dtype=np.float32)
    return real + shift[None, :], fake + shift[None, :], shift


# At D = 512 independent normal rows never fall into each other's balls (BALL_CASES' (64, 1, 512, 3) has no pair inside: it would
# pass for a kernel that returns zeros).  These cases put query m at a[m mod N] + t_m noise with t_m cycling through NEAR_STEPS:
# squared distance about 512 t^2 to its own centre against k-th neighbour radii of about 900 - 1000, so the steps 0.25, 0.5 and 1.0
# land inside their centre's ball (and now and then a neighbour's) and 1.6 and 2.0 outside, over 16 column chunks.  No step is 0: a
# query that IS centre j sits exactly on the sphere of every centre whose k-th neighbour is j - a tie no margin clears; the
# bit-identical row has a test of its own.
NEAR_CASES = [(130, 67, 512, 3), (64, 1, 512, 3), (70, 9, 600, 2)]          # the last: beyond the columns a resident query tile holds
KNN_WIDE_CASES = [(70, 600, 2)]
NEAR_STEPS = (0.5, 0.25, 1.0, 1.6, 2.0)


def near_fixture(N, M, D, k, shifted=False, seed=0):
    """centres a (N, D), queries q (M, D) near them (above), shift, and r2 (N,) fp32: the reference's radii rounded to fp32."""
    a, _, shift, r2 = ball_fixture(N, 1, D, k, shifted, seed)
    rng = np.random.default_rng(seed + 1)
    t = np.asarray(NEAR_STEPS, dtype=np.float32)[np.arange(M) % len(NEAR_STEPS)]
    q = (a[np.arange(M) % N] + t[:, None] * rng.standard_normal((M, D)).astype(np.float32)).astype(np.float32)
    return a, q, shift, r2


def ball_fixture(N, M, D, k, shifted=False, seed=0):
    """centres a (N, D), queries q (M, D), shift, and r2 (N,) fp32: the reference's k-th neighbour radii rounded to fp32."""
    a, q, shift = fixture_sets(N, M, D, seed, shifted)
    r2 = knn_radius(centred(a, shift), k).astype(np.float32)
    return a, q, shift, r2
