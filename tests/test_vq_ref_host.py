"""tests/vq_ref.py, the float64 reference of the vector quantiser, checked on the CPU; and the case tables of
tests/test_gpu_vq.py walked without a GPU: the share of clear pixels per case and seed (the 0.97 cap), the share of seeded pixels
that take the lower index of every tie case (the 0.20 cap), the plan every row expects.  Run with -s to see the shares.

The EMA formulas are held to two restatements of the reference module's torch path: the oracle's (oracle.vqwnet_ref.vq_quantize,
run here in float64) and the recorded run of the reference VQModule(knn_backend="torch") in tests/golden/vq.npz (float32).  The
project's own networks.vq.VQ has no host path to compare with: its forward is the HIP operator, which refuses CPU tensors.
"""
import numpy as np
import pytest
import torch

import test_gpu_vq as T
import vq_ref as R
from helpers import assert_close


def _oracle_inputs(K, D, B, S):
    """The inputs of test_vq_routes_vs_oracle (tests/test_gpu_parity.py) for one of its VQ_ROUTES rows."""
    g = torch.Generator().manual_seed(K * 1000 + D)
    embed = torch.randn(K, D, generator=g)
    x = torch.randn(B, D, S, S, generator=g) * 1.1
    return x, embed


@pytest.mark.parametrize("K,D,B,S", [(10, 16, 3, 40), (96, 40, 1, 23), (50, 7, 1, 21)])
def test_search_and_commit_vs_oracle(K, D, B, S):
    from oracle import vqwnet_ref as O
    x, embed = _oracle_inputs(K, D, B, S)
    V = dict(embed=embed.clone(), cluster_size=torch.zeros(K), embed_avg=embed.t().contiguous())
    q, commit, ids, gap = O.vq_forward(V, x, False, 0.9)
    rows = R.to_rows(x)
    ids64, gap64 = R.search64(rows, embed)
    clear = (gap > 1e-4 * (1 + gap.abs())).reshape(-1)          # the oracle's own rule on its own fp32 gap
    assert float(clear.float().mean()) > 0.97
    assert torch.equal(ids64[clear], ids.reshape(-1)[clear])
    assert float((gap64 - gap.reshape(-1).double()).abs().max()) <= 1e-4 * float(gap64.max())
    c64 = float(R.commit64(rows, embed, ids.reshape(-1)))
    assert abs(float(commit) - c64) <= 1e-6 * c64
    assert torch.equal(R.to_rows(q), embed[ids.reshape(-1)])


def test_ema64_vs_oracle_float64():
    """One training call of the oracle in float64 (momentum and 1 - momentum as doubles) against stats64 + ema64."""
    from oracle import vqwnet_ref as O
    K, D, B, S = 50, 7, 2, 12
    x, embed = _oracle_inputs(K, D, B, S)
    x, embed = x.double(), embed.double()
    embed[5] += 40.0                                               # a code nobody picks: the Laplace term decides its row
    V = dict(embed=embed.clone(), cluster_size=torch.full((K,), 3.0, dtype=torch.float64), embed_avg=(3.0 * embed).t().contiguous())
    cs0, ea0 = V["cluster_size"].clone(), V["embed_avg"].clone()
    _, ids, _ = O.vq_quantize(V, x, True, 0.9)
    rows = R.to_rows(x)
    ids64, _ = R.search64(rows, embed)
    assert torch.equal(ids64, ids.reshape(-1))
    counts, sums = R.stats64(rows, ids64, K)
    assert int(counts[5]) == 0 and int(counts.sum()) == B * S * S
    ref = R.ema64(counts, sums, cs0, ea0, 0.9, 1 - 0.9, O.VQ_EPS)
    for k in ("cluster_size", "embed_avg", "embed"):
        assert float((ref[k] - V[k]).abs().max()) <= 1e-13 * float(V[k].abs().max()), k
    half = R.ema64(counts, sums, cs0, ea0, 0.9, 1 - 0.9, O.VQ_EPS, sum_scale=0.5)
    assert torch.allclose(half["embed_avg"], ea0 * 0.9 + (1 - 0.9) * 0.5 * sums, rtol=1e-14, atol=0)
    assert torch.equal(half["cluster_size"], ref["cluster_size"])


@pytest.mark.parametrize("tag", ["k10", "k64", "k1024"])
def test_ema64_vs_recorded_reference_module(golden, tag):
    """tests/golden/vq.npz holds one training call of the reference VQModule(knn_backend="torch") in float32."""
    g = golden("vq.npz")
    embed0 = g.t(tag + "/embed0")
    K, D = embed0.shape
    mom = float(g[tag + "/momentum"])
    rows = R.to_rows(g.t(tag + "/x1"))
    ids = g.t(tag + "/ids1").reshape(-1).long()
    ids64, gap = R.search64(rows, embed0)
    clr = R.clear(rows, embed0, gap)
    assert torch.equal(ids64[clr], ids[clr]) and float(clr.float().mean()) > 0.97
    counts, sums = R.stats64(rows, ids, K)
    ref = R.ema64(counts, sums, torch.zeros(K), embed0.t(), mom, 1 - mom, 1e-5)
    for k in ("cluster_size", "embed_avg", "embed"):
        assert_close(g.t("%s/%s_after1" % (tag, k)), ref[k], 1e-5, "%s %s" % (tag, k))
    assert_close(g.t(tag + "/commit1"), R.commit64(rows, embed0, ids), 1e-6, "commit")


def test_ema_weights_are_the_launchers():
    m, om, eps = R.ema_weights(0.99)
    assert m == float(np.float32(0.99)) and om == float(np.float32(1) - np.float32(0.99)) and eps == float(np.float32(1e-5))
    assert R.ema_weights(0.99, True)[1] == float(np.float32(1 - 0.99)) != om
    assert R.ema_weights(0.0) == (0.0, 1.0, eps)


def test_bwd64_vs_autograd():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(30, 8, generator=g).double().requires_grad_(True)
    q = torch.randn(30, 8, generator=g).double()
    r = torch.randn(30, 8, generator=g).double()
    ste = q + (x - x.detach())
    ((ste * r).sum() + 3.0 * ((x - q) ** 2).mean()).backward()
    gx, bound = R.bwd64(x.detach(), q, r, 3.0)
    assert torch.allclose(gx, x.grad, rtol=1e-13, atol=1e-15) and bool((bound > 0).all())
    assert torch.equal(R.bwd64(x.detach(), q, r, None)[0], r)
    assert torch.allclose(R.bwd64(x.detach(), q, None, 3.0)[0], 6.0 * (x.detach() - q) / x.numel(), rtol=1e-14, atol=0)


def _cap(K, D, n, seed, offset, what):
    x, embed = R.gauss(K, D, n, seed, offset)
    ids, gap = R.search64(x, embed)
    clr = R.clear(x, embed, gap)
    share = float(clr.double().mean())
    ids32 = torch.cat([R.scores(x[a:b], embed).argmax(1) for a, b in R._chunks(n, K)])
    wrong32 = int((clr & (ids32 != ids)).sum())
    print("%s K %d D %d: clear %.4f, fp32 torch differs on %d clear and %d other pixels" % (
        what, K, D, share, wrong32, int((~clr & (ids32 != ids)).sum())))
    assert share >= T.CLEAR_CAP, "%s K %d D %d: clear share %.4f" % (what, K, D, share)
    assert wrong32 == 0, "the bound is too tight for the fp32 reference itself"
    return clr


@pytest.mark.parametrize("K,D,plan,form", T.FORMS)
def test_clear_cap_centred(K, D, plan, form):
    _cap(K, D, T.NPIX_FORM, T.seed_of(K, D), 0.0, "centred")


@pytest.mark.parametrize("K,D,plan", T.OFF_ZERO)
def test_clear_cap_off_zero(K, D, plan):
    assert D <= 128, "offset cases are restricted to D <= 128: beyond, the bound leaves too few pixels clear"
    _cap(K, D, T.NPIX_FORM, T.seed_of(K, D), T.OFFSET, "offset %.1f" % T.OFFSET)


@pytest.mark.parametrize("K,D,plan,form", T.SECOND_TRIP)
def test_clear_cap_second_trip(K, D, plan, form):
    clr = _cap(K, D, T.SECOND_TRIP_NPIX, T.seed_of(K, D), 0.0, "second trip")
    assert int(clr[-65:].sum()) >= 60, "the last 65 pixels must mostly be clear for their check to mean something"


def test_tables_expect_the_librarys_plans():
    plan = T._plan
    rows = [(K, D, p) for K, D, p, _ in T.FORMS] + list(T.OFF_ZERO) + [(K, D, p) for K, D, p, _, _, _ in T.TIES]
    rows += list(T.EDGE_SHAPES) + list(T.SEGMENT_SHAPES) + [(K, D, p) for K, D, p, _ in T.SECOND_TRIP]
    for K, D, p in rows:
        assert plan(D, K) == p, "vqw_vq_plan(%d, %d) = %d, the table says %d" % (D, K, plan(D, K), p)
    for D, k1, k2 in T.CAPACITY_SWITCHES:
        assert k2 == k1 + 1 and k1 * (D + 1) <= 15360 < k2 * (D + 1)
        assert plan(D, k1) == 1 and plan(D, k2) == 2
    assert {p for _, _, p, _ in T.FORMS} == {0, 1, 2, 3} and len(T.FORMS) == 41
    # every tile form (DT, NT) and every MFMA form (DT, FULL) is named by a row
    forms = " ".join(f for _, _, _, f in T.FORMS)
    for dt, nts in ((16, (0, 1, 2, 4, 8)), (32, (0, 1, 2, 4)), (64, (0, 1, 2))):
        for nt in nts:
            assert "k_vq_tile<%d,%d>" % (dt, nt) in forms
    for dt in (32, 64, 128, 256):
        for full in ("true", "false"):
            assert "k_vq_mfma<%d,%s>" % (dt, full) in forms
    for f in ("k_vq_fwd<0,true,0>", "k_vq_fwd<0,false,0>", "k_vq_segsum<true>", "k_vq_segsum<false>"):
        assert f in forms


@pytest.mark.parametrize("K,D,plan,i,j,what", T.TIES)
def test_tie_cases_for_the_reference(K, D, plan, i, j, what):
    x, embed, seeded = R.tie_inputs(K, D, i, j, T.NPIX_TIE, T.seed_of(K, D) + 17 * j)
    assert torch.equal(embed[i], embed[j]) and int(seeded.sum()) == T.NPIX_TIE // 2
    others = [k for k in range(K) if k not in (i, j)]
    assert not bool((embed[others] == embed[i]).all(1).any())
    s = R.scores(x.double(), embed.double())
    assert torch.equal(s[:, i], s[:, j]), "identical rows must tie exactly"
    ids, gap = R.search64(x, embed)
    assert not bool((ids == j).any())
    share = float((ids[seeded] == i).double().mean())
    print("K %d D %d (%d, %d) %s: %.3f of the seeded pixels take %d; gap 0 on %d pixels" % (K, D, i, j, what, share, i, int((gap == 0).sum())))
    assert share >= T.TIE_SHARE
    assert bool((gap[ids == i] == 0).all()) and not bool(R.clear(x, embed, gap)[ids == i].any())


@pytest.mark.parametrize("K,D,plan", T.SEGMENT_SHAPES)
def test_with_counts_yields_the_counts(K, D, plan):
    want = T.segment_counts(K)
    x, embed = R.with_counts(K, D, want, T.seed_of(K, D))
    assert x.shape == (sum(want), D) and bool((embed == embed.round()).all())
    assert len({tuple(r.tolist()) for r in embed}) == K, "codes must be pairwise distinct"
    ids, gap = R.search64(x, embed)
    assert torch.bincount(ids, minlength=K).tolist() == want
    assert torch.equal(x, embed[ids]) and float(gap.min()) >= 1.0
    assert not torch.equal(ids, ids.sort().values), "shuffled"
    counts, sums = R.stats64(x, ids, K)
    assert torch.equal(sums, (embed.double() * counts[:, None]).t())


@pytest.mark.parametrize("K,D,plan", T.EDGE_SHAPES)
def test_integer_valued_inputs_are_exact_in_fp32(K, D, plan):
    for n in T.EDGE_NPIX:
        x, embed = R.integer_valued(K, D, n, T.seed_of(K, D) + n)
        assert x.shape == (n, D) and bool((x == x.round()).all()) and bool((embed == embed.round()).all())
        s32, s64 = R.scores(x, embed), R.scores(x.double(), embed.double())
        assert torch.equal(s32.double(), s64) and float(s64.abs().max()) < 2 ** 24
        ids, _ = R.search64(x, embed)
        assert torch.equal(ids, (-s64).argmin(1)) or torch.equal(s64.gather(1, ids[:, None]), s64.max(1, keepdim=True).values)
        counts, sums = R.stats64(x, ids, K)
        assert float(sums.abs().max()) < 2 ** 24
        if n >= 2047:
            assert int(counts[0]) > n - 98 and int((counts > 0).sum()) > 1
