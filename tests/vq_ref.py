"""Float64 restatement of the vector quantiser (csrc/vq.hip) and the a-priori bounds its tests use.  Plain torch on the host:
nothing here knows how a kernel walks its data.  tests/test_vq_ref_host.py checks this file against the oracle and the recorded
reference module on the CPU; tests/test_gpu_vq.py holds the kernels to it.

Layout: pixels are rows, x[Npix][D]; the codebook is embed[K][D]; statistics are counts[K] and sums[D][K] (the layout of
embed_avg).  `to_map` turns rows into the (B, D, H, W) channels-last map the operators take.  u = 2^-24 is the unit roundoff
of float32 throughout.
"""
import numpy as np
import torch

U = 2.0 ** -24
_CHUNK_ELEMS = 1 << 22          # score elements per row chunk: 32 MiB in float64


def _chunks(n, K):
    rows = max(1, _CHUNK_ELEMS // max(1, K))
    return [(a, min(n, a + rows)) for a in range(0, n, rows)]


def scores(x, embed):
    """s[p][k] = 2 x_p . e_k - |e_k|^2 - |x_p|^2 (= -|x_p - e_k|^2) in the dtype of x, rows of x in chunks."""
    e = embed.to(x.dtype)
    en = (e * e).sum(1)
    out = torch.empty(x.shape[0], e.shape[0], dtype=x.dtype)
    for a, b in _chunks(x.shape[0], e.shape[0]):
        xc = x[a:b]
        out[a:b] = (2 * (xc @ e.t()) - en[None, :]) - (xc * xc).sum(1, keepdim=True)
    return out


def search64(x, embed):
    """Float64 arg-max of the score with ties to the LOWEST index -> (ids int64 [Npix], gap float64 [Npix]); gap is the top-1
    minus the top-2 score (0 on an exact tie), +inf for K = 1.  The score matrix only ever exists one row chunk at a time."""
    x64, e64 = x.double(), embed.double()
    n, K = x64.shape[0], e64.shape[0]
    ids = torch.empty(n, dtype=torch.int64)
    gap = torch.full((n,), float("inf"), dtype=torch.float64)
    for a, b in _chunks(n, K):
        s = scores(x64[a:b], e64)
        best = s.max(1, keepdim=True).values
        # the first maximal entry, spelled out: the library's argmax does not promise which of several maxima it returns
        first = torch.where(s == best, torch.arange(K)[None, :], torch.full((1, 1), K)).min(1).values
        ids[a:b] = first
        if K > 1:
            top2 = s.topk(2, dim=1).values
            gap[a:b] = top2[:, 0] - top2[:, 1]
    return ids, gap


def clear_bound(x, embed):
    """2 (D + 3) u (|x_p| + max_k |e_k|)^2 per pixel, float64 [Npix]; see clear()."""
    D = x.shape[1]
    xn = x.double().norm(dim=1)
    en = embed.double().norm(dim=1).max()
    return 2.0 * (D + 3) * U * (xn + en) ** 2


def clear(x, embed, gap):
    """A pixel is CLEAR iff gap > 2 (D + 3) u (|x| + max_k |e_k|)^2: no float32 evaluation of the score, in any order of its
    additions, with or without fused multiply-adds, can then prefer another code than the float64 arg-max.

    Derivation.  A kernel computes s^_k = fl(fl(2 dot^ - n^_k) - x2^) with dot^ ~ e_k . x, n^_k ~ |e_k|^2, x2^ ~ |x|^2.
      * An fp32 dot product of length D, in any order, is off by at most gamma_D sum_d |a_d b_d| <= gamma_D |a| |b|
        (gamma_D = D u / (1 - D u); Cauchy-Schwarz).  So |dot^ - e.x| <= gamma_D |e||x|, |n^ - |e|^2| <= gamma_D |e|^2,
        |x2^ - |x|^2| <= gamma_D |x|^2.  Doubling is exact.  Together: gamma_D (2 |e||x| + |e|^2 + |x|^2) = gamma_D (|e| + |x|)^2.
      * The first subtraction rounds a value of magnitude <= 2 |e||x| + |e|^2 <= (|e| + |x|)^2: at most u (|e| + |x|)^2.
      * The second rounds a value of magnitude |s| = |x - e|^2 <= (|e| + |x|)^2: at most u (|e| + |x|)^2.
    Per code that is (gamma_D + 2 u) (|e| + |x|)^2 <= (D + 3) u (|e| + |x|)^2 (the third unit absorbs the second-order terms
    while D u < 1e-3, i.e. D < 16000).  A wrong pick needs s^_j >= s^_i although s_i - s_j >= gap, so the two errors together
    must reach the gap: with |e| <= max_k |e_k| for both codes, 2 (D + 3) u (|x| + max_k |e_k|)^2 >= gap.  Above that the pick
    is forced, the tie rule included (an exact tie has gap 0 and is never clear)."""
    return gap > clear_bound(x, embed)


def commit64(x, embed, ids):
    """mean((x - embed[ids])^2) over all Npix * D elements, float64 scalar."""
    d = x.double() - embed.double()[ids]
    return (d * d).mean()


def commit_bound(D):
    """Relative error of the kernels' commitment loss at their own ids: (D + 4) u.  Per pixel: one rounding for x - e, two for
    the square (gamma_2; one with a fused multiply-add), gamma_D for the chain of D non-negative terms (no cancellation, so the
    bound is relative); per-pixel values are then summed in double (error ~ Npix 2^-53, nothing) and the mean is rounded to
    float once: (1 + 2 + D + 1) u."""
    return (D + 4) * U


def stats64(x, ids, K):
    """counts[K] and sums[D][K] of the pixels of every code, float64, by index_add_."""
    x64 = x.double()
    counts = torch.bincount(ids, minlength=K).double()
    sums = torch.zeros(K, x64.shape[1], dtype=torch.float64).index_add_(0, ids, x64).t().contiguous()
    return counts, sums


def sums_bound(x, ids, K):
    """Elementwise bound [D][K] for fp32 member sums in ANY order of additions: (n_k + 1) u sum_{p in k} |x_pd|.  n_k - 1
    additions give gamma_{n_k - 1}; the two spare units cover one rounding from a double partial to float and the second-order
    terms (n_k u < 2e-2 at every size used here)."""
    counts, asum = stats64(x.abs(), ids, K)
    return (counts[None, :] + 1.0) * U * asum


def ema_weights(momentum, torch_ema_weight=False):
    """(m, om, eps) as the float32 values the launcher hands to k_vq_ema, returned as Python doubles.  om, the weight of the new
    statistics, is 1.f - m formed in float32, or with torch_ema_weight the double 1 - momentum rounded once."""
    m = np.float32(momentum)
    om = np.float32(1.0 - float(momentum)) if torch_ema_weight else np.float32(1.0) - m
    return float(m), float(om), float(np.float32(1e-5))


def ema64(counts, sums, cluster_size, embed_avg, m, om, eps, sum_scale=1.0):
    """The formulas of k_vq_ema / k_vq_ema_cs in float64 -> dict(cluster_size [K], embed_avg [D][K], embed [K][D], csn [K]):
         c_k  = cs_k m + om counts_k                        a_dk = ea_dk m + om (sums_dk sum_scale)
         n    = sum_k c_k                                   csn_k = n (c_k + eps) / (n + K eps)      (Laplace smoothing)
         embed_kd = a_dk / csn_k"""
    c = cluster_size.double() * m + om * counts.double()
    a = embed_avg.double() * m + om * (sums.double() * sum_scale)
    K = c.shape[0]
    n = c.sum()
    csn = n * (c + eps) / (n + K * eps)
    return dict(cluster_size=c, embed_avg=a, embed=(a / csn[None, :]).t().contiguous(), csn=csn)


def ema_bounds(counts, sums, cluster_size, embed_avg, m, om, eps, sum_scale=1.0):
    """Elementwise a-priori bounds of k_vq_ema / k_vq_ema_cs against ema64, from their operation count (inputs exact in fp32:
    counts < 2^24, and the tests that use this feed integer-valued sums).
      cluster_size  c = fl(fl(cs m) + fl(om cnt)): three roundings of non-negative terms -> relative 3 u; bound 4 u c.
      embed_avg     a = fl(fl(ea m) + fl(om fl(S scale))): product, product, product, sum (a fused multiply-add saves one) ->
                    at most 2 u |m ea| + 4 u |om S scale| to first order; bound 5 u (|m ea| + |om S scale|).  Absolute: the two
                    terms may cancel.
      embed         fl(a / csn).  csn = n (c + eps) / (n + K eps) in fp32: n is a double sum of the c_k rounded once (4 u),
                    c + eps (3 u c / (c + eps) + u <= 4 u), the product (u), K eps (u), the denominator's sum (n's 4 u and K eps'
                    u weigh at most 4 u together, + u), the division (u): 4 + 4 + 1 + 5 + 1 = 15 u relative on csn, then the
                    quotient's own rounding, 16 u; bound |a - a64| / csn + 18 u |embed64| (two units for the second-order terms).
    -> dict of float64 tensors shaped like ema64's."""
    r = ema64(counts, sums, cluster_size, embed_avg, m, om, eps, sum_scale)
    b_ea = 5.0 * U * ((embed_avg.double() * m).abs() + (om * sums.double() * sum_scale).abs())
    b_e = (b_ea / r["csn"][None, :]).t() + 18.0 * U * r["embed"].abs()
    return dict(cluster_size=4.0 * U * r["cluster_size"].abs(), embed_avg=b_ea, embed=b_e)


def bwd64(x, q, gq, gc):
    """vqw_vq_bwd: gx = gq + gc * 2 (x - q) / numel (straight-through + commitment), float64; gq / gc may be None.
    -> (gx, bound) with the elementwise bound 2^-22 (|gq| + |s| |x - q|), s = 2 gc / numel: s is formed with two roundings,
    x - q with one, the fused multiply-add with one -> 4 u on the product term and u on gq."""
    x64, q64 = x.double(), q.double()
    s = 0.0 if gc is None else 2.0 * float(gc) / x64.numel()
    g = torch.zeros_like(x64) if gq is None else gq.double()
    gx = g + s * (x64 - q64)
    return gx, 2.0 ** -22 * (g.abs() + abs(s) * (x64 - q64).abs())


# ---- inputs: one source for the host and the GPU tests, so both see the same bits --------------------------------------------
def gauss(K, D, Npix, seed, offset=0.0):
    """-> (x [Npix][D], embed [K][D]) float32: unit-normal codes, features 1.1 x unit normal, both shifted by `offset` (the state
    after a ReLU encoder: features and codes share a mean, and the score cancels heavily)."""
    g = torch.Generator().manual_seed(int(seed))
    embed = torch.randn(K, D, generator=g) + offset
    x = torch.randn(Npix, D, generator=g) * 1.1 + offset
    return x.float().contiguous(), embed.float().contiguous()


def integer_valued(K, D, Npix, seed):
    """-> (x, embed) with small integer values, as test_vq_statistics_skewed_and_exact draws them: codes in 8 * {-3..3} with code
    0 at the origin, features in {-2..2} (nearest to code 0) except min(97, Npix / 4) pixels that sit exactly on other codes.
    Every score and every sum is an integer far below 2^24: ids, counts and sums are exact in fp32 whatever the order."""
    g = torch.Generator().manual_seed(int(seed))
    embed = torch.randint(-3, 4, (K, D), generator=g).float() * 8.0
    embed[0] = 0.0
    x = torch.randint(-2, 3, (Npix, D), generator=g).float()
    n_on = min(97, Npix // 4)
    if n_on > 0 and K > 1:
        pick = torch.randperm(Npix, generator=g)[:n_on]
        x[pick] = embed[torch.randint(1, K, (n_on,), generator=g)]
    return x.contiguous(), embed.contiguous()


def with_counts(K, D, counts, seed):
    """-> (x [sum(counts)][D], embed [K][D]): pixels sitting exactly on integer-valued, pairwise distinct codes, counts[k] of
    them on code k, shuffled.  Channel 0 of code k is k - K / 2 (distinct by construction), the others are in {-3..3}."""
    counts = [int(c) for c in counts]
    assert len(counts) == K
    g = torch.Generator().manual_seed(int(seed))
    embed = torch.randint(-3, 4, (K, D), generator=g).float()
    embed[:, 0] = torch.arange(K).float() - float(K // 2)
    owner = torch.repeat_interleave(torch.arange(K), torch.tensor(counts))
    owner = owner[torch.randperm(owner.numel(), generator=g)]
    return embed[owner].contiguous(), embed.contiguous()


def duplicate_rows(embed, pairs):
    """embed with row j overwritten by row i for every (i, j): bit-identical rows, exact score ties."""
    e = embed.clone()
    for i, j in pairs:
        assert i < j
        e[j] = e[i]
    return e


def tie_inputs(K, D, i, j, Npix, seed):
    """-> (x, embed, seeded): a gauss codebook with embed[j] = embed[i]; the first half of the pixels are embed[i] + 0.05 randn
    (`seeded` marks them), the rest are gauss features."""
    x, embed = gauss(K, D, Npix, seed)
    embed = duplicate_rows(embed, [(i, j)])
    g = torch.Generator().manual_seed(int(seed) + 1)
    half = Npix // 2
    x[:half] = embed[i][None, :] + 0.05 * torch.randn(half, D, generator=g)
    seeded = torch.zeros(Npix, dtype=torch.bool)
    seeded[:half] = True
    return x.contiguous(), embed, seeded


def to_map(x, B, H, W):
    """Rows [B*H*W][D] -> (B, D, H, W) view in channels-last memory: the form the operators take without a copy."""
    return x.reshape(B, H, W, x.shape[1]).permute(0, 3, 1, 2)


def to_rows(t):
    """(B, D, H, W) -> rows [B*H*W][D] on the host."""
    return t.detach().cpu().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
