"""Scores of a generative prior's samples in a feature space: the Frechet distance between feature distributions, precision /
recall on k-nearest-neighbour manifolds (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and the divergence of
the unigram code histograms.  The reference has nothing of this.

The feature space is the project's own frozen first stage (PriorTrainer.features), not Inception: the numbers rank priors trained
on ONE first stage against each other and against the floor PriorTrainer.score reports.  They are not comparable with published
FID values.

The heavy parts run in csrc/sample_scores.hip (hipops.ops.feature_moments, knn_radius, ball_counts): the D x D second moments in
double, and the two N x M nearest-neighbour problems on a tile engine that never writes the distances.  What is left here is
float64 on the host: the mean and covariance from the raw sums, and the matrix square roots through torch.linalg.eigh."""
import torch

from hipops import ops


class FeatureStats:
    """Streams feature batches (B, D) fp32 on the device into double moments and keeps the first `keep` rows, in arrival order,
    for the manifold scores.  shift (D,) fp32 or None: the centring every kernel subtracts while staging (the caller's, e.g. the
    pooled mean of the first real batch); it keeps the distances' Gram form from cancelling on features far from the origin.
    n, mean() and cov() come from the raw sums in float64 on the host: one device-to-host read of D + D^2 doubles, cached until
    the next add()."""

    def __init__(self, D, shift=None, keep=0):
        self.D, self.keep = int(D), int(keep)
        if not 1 <= self.D <= ops.FEATURE_MAX_D:
            raise ValueError("FeatureStats: D=%d out of [1, %d]" % (self.D, ops.FEATURE_MAX_D))
        if self.keep < 0:
            raise ValueError("FeatureStats: keep=%d must not be negative" % self.keep)
        if shift is not None and (shift.dtype != torch.float32 or tuple(shift.shape) != (self.D,)):
            raise ValueError("FeatureStats: shift (%d,) fp32 expected, got %s of %s" % (self.D, tuple(shift.shape), shift.dtype))
        self.shift = None if shift is None else shift.detach().clone()
        self.n = 0
        self._sum = self._outer = self._host = None
        self._rows, self._kept = [], 0

    def add(self, x):
        if x.dim() != 2 or x.shape[1] != self.D:
            raise ValueError("FeatureStats.add: (B, %d) expected, got %s" % (self.D, tuple(x.shape)))
        if x.shape[0] == 0:
            return
        if self._sum is None:
            self._sum = torch.zeros(self.D, dtype=torch.float64, device=x.device)
            self._outer = torch.zeros((self.D, self.D), dtype=torch.float64, device=x.device)
            if self.shift is not None:
                self.shift = self.shift.to(x.device)
        ops.feature_moments(x, self._sum, self._outer, self.shift)
        self.n += int(x.shape[0])
        self._host = None
        if self._kept < self.keep:
            rows = x.detach()[:self.keep - self._kept].clone()
            self._rows.append(rows)
            self._kept += int(rows.shape[0])

    def rows(self):
        """The kept rows (min(keep, n), D) fp32 on the device."""
        if not self._rows:
            raise ValueError("FeatureStats.rows: no rows kept (keep=%d, n=%d)" % (self.keep, self.n))
        return self._rows[0] if len(self._rows) == 1 else torch.cat(self._rows, dim=0)

    def _moments(self):
        if self.n < 1:
            raise ValueError("FeatureStats: no rows added")
        if self._host is None:
            host = torch.cat([self._sum, self._outer.reshape(-1)]).cpu()            # the one read
            self._host = (host[:self.D].clone(), host[self.D:].reshape(self.D, self.D).clone())
        return self._host

    def mean(self):
        """(D,) float64 on the host: shift + sum / n."""
        m = self._moments()[0] / self.n
        return m if self.shift is None else m + self.shift.double().cpu()

    def cov(self):
        """(D, D) float64 on the host, unbiased: (outer - n m m^T) / (n - 1) over the centred rows (a covariance does not see
        the shift)."""
        if self.n < 2:
            raise ValueError("FeatureStats.cov: at least 2 rows are needed (n=%d)" % self.n)
        s, o = self._moments()
        m = s / self.n
        return (o - self.n * torch.outer(m, m)) / (self.n - 1)


class Moments:
    """Given statistics with FeatureStats's reading side: n, mean(), cov() (float64 on the host)."""

    def __init__(self, n, mean, cov):
        self.n, self._mean, self._cov = int(n), torch.as_tensor(mean, dtype=torch.float64), torch.as_tensor(cov, dtype=torch.float64)
        self.D = int(self._mean.numel())

    def mean(self):
        return self._mean

    def cov(self):
        return self._cov


def _psd_sqrt(s):
    w, u = torch.linalg.eigh((s + s.T) / 2)
    return (u * w.clamp_min(0.0).sqrt()[None, :]) @ u.T


def frechet_distance(a, b):
    """(distance, rank_deficient) between two sets of statistics (FeatureStats or Moments):
    |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2 in float64 on the host, both square roots through
    torch.linalg.eigh with negative eigenvalues clipped to 0.  rank_deficient = min(n_a, n_b) <= D: a covariance of n rows has rank
    at most n - 1, the clipped null eigenvalues then leave an error of the size of the square root of the rounding unit times the
    traces, and the estimate itself is biased - compare it with a floor taken at the same n."""
    mu_a, mu_b, sa, sb = a.mean().double(), b.mean().double(), a.cov().double(), b.cov().double()
    if mu_a.shape != mu_b.shape:
        raise ValueError("frechet_distance: D=%d against D=%d" % (mu_a.numel(), mu_b.numel()))
    ra = _psd_sqrt(sa)
    m = ra @ sb @ ra
    w = torch.linalg.eigvalsh((m + m.T) / 2)
    d = mu_a - mu_b
    fd = float(d @ d) + float(torch.trace(sa)) + float(torch.trace(sb)) - 2.0 * float(w.clamp_min(0.0).sqrt().sum())
    return fd, bool(min(a.n, b.n) <= mu_a.numel())


def manifold_scores(real, fake, k=3, shift=None):
    """{'precision', 'recall', 'density', 'coverage'} of feature rows real (N, D) and fake (M, D), fp32 on the device.
    precision: the share of fake rows inside at least one real ball (the ball of a real row reaches to its k-th nearest other
    real row); recall: the same with the roles swapped; density: sum_m #{real balls around fake m} / (k M); coverage: the share
    of real balls that hold a fake row.  Four kernel calls and one device-to-host read of four integers."""
    k = int(k)
    if min(real.shape[0], fake.shape[0]) < k + 1:
        raise ValueError("manifold_scores: both sets need at least k + 1 = %d rows (got %d real, %d fake)" % (k + 1, real.shape[0], fake.shape[0]))
    cnt_f, hit_r = ops.ball_counts(fake, real, ops.knn_radius(real, k, shift), shift)
    cnt_r, _ = ops.ball_counts(real, fake, ops.knn_radius(fake, k, shift), shift)
    n_prec, n_dens, n_cov, n_rec = torch.stack([(cnt_f > 0).sum(), cnt_f.sum(dtype=torch.int64), (hit_r > 0).sum(),
                                                (cnt_r > 0).sum()]).tolist()
    N, M = int(real.shape[0]), int(fake.shape[0])
    return {"precision": n_prec / M, "recall": n_rec / N, "density": n_dens / (k * M), "coverage": n_cov / N}


def _entropy_bits(p):
    p = p[p > 0]
    return float(-(p * torch.log2(p)).sum())


def code_scores(real_ids, fake_ids, V):
    """The unigram code histograms of two sets of code sequences (torch.long, any shape, codes in [0, V)): their Jensen-Shannon
    divergence in bits (0: equal histograms, 1: disjoint supports), each side's entropy in bits and the share of the codebook
    each side uses.  torch.bincount on the tensors' device, the rest in float64 on the host."""
    V = int(V)
    counts = []
    for name, ids in (("real_ids", real_ids), ("fake_ids", fake_ids)):
        ids = ids.reshape(-1)
        if ids.dtype != torch.long or ids.numel() == 0:
            raise ValueError("code_scores: %s must be a non-empty torch.long tensor" % name)
        if int(ids.min()) < 0 or int(ids.max()) >= V:
            raise ValueError("code_scores: %s has codes outside [0, %d)" % (name, V))
        counts.append(torch.bincount(ids, minlength=V).double().cpu())
    p, q = counts[0] / counts[0].sum(), counts[1] / counts[1].sum()
    js = _entropy_bits((p + q) / 2) - 0.5 * _entropy_bits(p) - 0.5 * _entropy_bits(q)
    return {"code_js_bits": max(js, 0.0), "code_entropy_real": _entropy_bits(p), "code_entropy_fake": _entropy_bits(q),
            "code_usage_real": float((counts[0] > 0).sum()) / V, "code_usage_fake": float((counts[1] > 0).sum()) / V}


def _stats_of(x, shift, what):
    if isinstance(x, FeatureStats):
        return x
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("sample_scores: %s must be a FeatureStats or feature rows (N, D)" % what)
    st = FeatureStats(x.shape[1], shift, keep=x.shape[0])
    st.add(x)
    return st


def sample_scores(real, fake, k=3, real_ids=None, fake_ids=None, dict_size=None):
    """Every score as one dict of Python floats and ints.  real, fake: FeatureStats that kept rows (the moments over everything
    added, the manifold scores over the kept rows), or feature rows (N, D) fp32 on the device, which are centred on the fp32 mean
    of the real rows.  Both sides must use one shift.  Keys: frechet, rank_deficient, precision, recall, density, coverage, n_real,
    n_fake, D, k; with real_ids, fake_ids and dict_size also code_scores's."""
    shift = None
    if not isinstance(real, FeatureStats):
        shift = fake.shift if isinstance(fake, FeatureStats) else real.detach().mean(dim=0)
    real = _stats_of(real, shift, "real")
    fake = _stats_of(fake, real.shift, "fake")
    if real.D != fake.D:
        raise ValueError("sample_scores: D=%d against D=%d" % (real.D, fake.D))
    if (real.shift is None) != (fake.shift is None) or (real.shift is not None and not torch.equal(real.shift.cpu(), fake.shift.cpu())):
        raise ValueError("sample_scores: real and fake must be centred on the same shift")
    fd, deficient = frechet_distance(real, fake)
    out = {"frechet": fd, "rank_deficient": int(deficient)}
    out.update(manifold_scores(real.rows(), fake.rows(), k, real.shift))
    if real_ids is not None or fake_ids is not None:
        if real_ids is None or fake_ids is None or dict_size is None:
            raise ValueError("sample_scores: real_ids, fake_ids and dict_size go together")
        out.update(code_scores(real_ids, fake_ids, dict_size))
    out.update(n_real=int(real.n), n_fake=int(fake.n), D=int(real.D), k=int(k))
    return out
