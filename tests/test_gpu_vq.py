"""The vector quantiser (csrc/vq.hip) against float64 on every plan and template form: nearest-code search, gather, commitment
loss, EMA statistics and codebook update, the straight-through backward, vq_lookup and mask_scale.  Run with
`pytest -m gpu tests/test_gpu_vq.py -s` on an MI355X; -s shows the measured error / bound ratio of every comparison.  The module
imports without a GPU: tests/test_vq_ref_host.py walks the case tables below on the CPU (the share of clear pixels per case, the
tie cases, the expected plans) and checks tests/vq_ref.py, the float64 reference, against the oracle.

Calls go through hipops.ops; the plan comes from vqw_vq_plan.  Raw statistics are read with momentum = 0, cluster_size = 0,
embed_avg = 0: after the call cluster_size holds the counts and embed_avg the sums.

No bound here is taken from a kernel's output.  Each is an exact equality, a cap checked for the reference on the CPU, or one of
the a-priori bounds derived in tests/vq_ref.py (u = 2^-24):
  ids .......... equal to the float64 arg-max on every CLEAR pixel, gap > 2 (D + 3) u (|x| + max_k |e_k|)^2 (vq_ref.clear); at
                 least 0.97 of a case's pixels are clear.  Integer-valued inputs: equal on every pixel.
  q ............ torch.equal(q, embed[ids]) on all pixels: a gather is bit-exact whatever was picked.
  commit ....... relative (D + 4) u against float64 at the kernel's own ids (vq_ref.commit_bound).
  counts ....... exactly the bincount of the kernel's ids.
  sums ......... elementwise (n_k + 1) u sum_{p in k} |x_pd| against float64 at the kernel's ids (vq_ref.sums_bound).
  EMA .......... elementwise, from the operation count of k_vq_ema (vq_ref.ema_bounds): cluster_size 4 u c, embed_avg
                 5 u (|m ea| + |om S|), embed that over cs_n plus 18 u |embed|.
  backward ..... elementwise 2^-22 (|g| + |s| |x - q|) (vq_ref.bwd64).
  A second identical call gives identical bits in every output.

Which template form a case reaches (restating vq_plan / vq_small_nt / vq_mfma_dt of vq.hip; FORMS names it per row):
  plan 0  k_vq_tile<D, NT>, NT = pow2 >= ceil(K / 16) while (D / 16 + 1) NT <= 16: matrix-core statistics
  plan 1  k_vq_tile<D, 0> + sorted statistics: D in {16, 32, 64}, K (D + 1) <= 15360 (903 / 465 / 236 codes at most)
  plan 2  k_vq_mfma<DT, FULL>: D % 4 == 0, 8 <= D <= 256, K >= 32; DT = 32 / 64 / 128 / 256, FULL iff D == DT
  plan 3  k_vq_fwd<0, LDS_CB, 0>: codebook in LDS iff K (D + 1) <= 15360; k_vq_segsum<V4> with V4 iff D % 4 == 0

Measured on an MI355X (largest error / bound over all cases; 1.0 would be the bound):
  ids .......... 0 differ on clear pixels in all 53 gauss cases, and none on any pixel of the 1500-pixel cases; smallest clear share 0.9840
                 centred (K 20, D 1024), 0.9827 at offset 4 (K 160, D 128); 0 of the integer-valued and tie cases differ anywhere
  commit ....... 0.095 (K 1, D 1); 0.048 at most on every other case
  sums ......... 0.447 (K 465, D 32, sorted statistics); matrix-core statistics 0.310 at most; 0.056 on the second trip
  EMA .......... cluster_size 0.357, embed_avg 0.217, embed 0.129
  backward ..... 0.604 (commit only), 0.264 (q and commit), 0 (q only: a copy)
  All 76 cases pass on vq.hip as it stands: no kernel change was needed.  Wrong builds the suite was run against (scratch copies):
  `>=` in one arg-max compare of each kernel fails exactly the tie cases of that kernel ((10,16) and (180,16) tile, (50,7) generic,
  (8,10) for the third compare of the MFMA group); the half merge without `oi < bi` fails ties (12,40), (5,1000) and (7,299);
  VQ_CH - 1 members per k_vq_segsum item fails test_vq_segment_boundaries, test_vq_pixel_count_edges on the three sorted plans and
  the sums of 18 gauss cases; a tile prefetch that zero-fills the last row fails test_vq_second_trip on both tile cases (the
  `Npix - 1` prefetch clamp of k_vq_fwd sits in its DT > 0 branch, which no instantiation compiles any more).
"""
import pytest
import torch

import vq_ref as R

DEV = "cuda"
NPIX_FORM, H_FORM, W_FORM = 1500, 30, 50          # ragged against 64, 128 and 256
CLEAR_CAP = 0.97
TIE_SHARE = 0.20

# (K, D, expected plan, the form it reaches)
FORMS = [
    (10, 16, 0, "k_vq_tile<16,1>"), (17, 16, 0, "k_vq_tile<16,2>"), (33, 16, 0, "k_vq_tile<16,4>"), (100, 16, 0, "k_vq_tile<16,8>"),
    (5, 32, 0, "k_vq_tile<32,1>"), (20, 32, 0, "k_vq_tile<32,2>"), (33, 32, 0, "k_vq_tile<32,4>"),
    (16, 64, 0, "k_vq_tile<64,1>"), (32, 64, 0, "k_vq_tile<64,2>"),
    (129, 16, 1, "k_vq_tile<16,0>"), (903, 16, 1, "k_vq_tile<16,0>, last K that fits LDS"),
    (65, 32, 1, "k_vq_tile<32,0>"), (465, 32, 1, "k_vq_tile<32,0>, last K that fits LDS"),
    (33, 64, 1, "k_vq_tile<64,0>, > 64 KiB LDS opt-in"), (236, 64, 1, "k_vq_tile<64,0>, last K that fits LDS, 128 KiB"),
    (904, 16, 2, "k_vq_mfma<32,false>, first K past LDS"), (466, 32, 2, "k_vq_mfma<32,true>"), (237, 64, 2, "k_vq_mfma<64,true>"),
    (32, 8, 2, "k_vq_mfma<32,false>, narrowest D, smallest K"), (40, 12, 2, "k_vq_mfma<32,false>"),
    (32, 20, 2, "k_vq_mfma<32,false>"), (64, 28, 2, "k_vq_mfma<32,false>"),
    (130, 36, 2, "k_vq_mfma<64,false>, D just above 32"), (96, 60, 2, "k_vq_mfma<64,false>"),
    (70, 68, 2, "k_vq_mfma<128,false>, D just above 64"), (70, 100, 2, "k_vq_mfma<128,false>"), (160, 128, 2, "k_vq_mfma<128,true>"),
    (33, 132, 2, "k_vq_mfma<256,false>, D just above 128"), (40, 200, 2, "k_vq_mfma<256,false>"), (64, 252, 2, "k_vq_mfma<256,false>"),
    (1024, 256, 2, "k_vq_mfma<256,true>, 32 stages"), (3000, 12, 2, "k_vq_mfma<32,false>, 12 stages of 256 codes, last one ragged"),
    (20, 20, 3, "k_vq_fwd<0,true,0>, k_vq_segsum<true>"), (31, 128, 3, "k_vq_fwd<0,true,0>, K just under the MFMA threshold"),
    (50, 7, 3, "k_vq_fwd<0,true,0>, k_vq_segsum<false>"), (700, 30, 3, "k_vq_fwd<0,false,0>, codebook in global memory"),
    (40, 260, 3, "k_vq_fwd<0,true,0>, D > 256"), (8, 1024, 3, "k_vq_fwd<0,true,0>, VQ_MAX_D: k_vq_segfinal at 64 KiB"),
    (20, 1024, 3, "k_vq_fwd<0,false,0>, VQ_MAX_D, global codebook"), (2, 3, 3, "k_vq_fwd<0,true,0>"), (1, 1, 3, "k_vq_fwd<0,true,0>, K = 1"),
]
# LDS-capacity switches K (D + 1) <= 15360: (D, last K of plan 1, first K of plan 2)
CAPACITY_SWITCHES = [(16, 903, 904), (32, 465, 466), (64, 236, 237)]
OFFSET = 4.0
OFF_ZERO = [(33, 16, 0), (129, 16, 1), (904, 16, 2), (466, 32, 2), (237, 64, 2), (70, 100, 2), (160, 128, 2), (20, 20, 3), (50, 7, 3)]
# (K, D, plan, i, j, what): embed[j] == embed[i] bit for bit, i < j
TIES = [
    (10, 16, 0, 3, 7, "tile, matrix-core statistics"), (180, 16, 1, 3, 7, "tile, sorted statistics"), (50, 7, 3, 3, 7, "generic"),
    # K = 1024, D = 256: 32 codes per stage, lane half h owns code rows 8 g + 4 h + r
    (1024, 256, 2, 8, 9, "same lane, next register"), (1024, 256, 2, 8, 10, "same lane, third register of the group"),
    (1024, 256, 2, 8, 12, "other lane half"), (1024, 256, 2, 8, 40, "next stage"), (1024, 256, 2, 5, 1000, "far stage"),
    (1024, 256, 2, 12, 40, "the higher lane half holds the lower code"),
    # K = 300, D = 64: TR = 128, four 32-code blocks per stage
    (300, 64, 2, 3, 35, "next block of the same stage"), (300, 64, 2, 3, 131, "next stage"), (300, 64, 2, 7, 299, "last code"),
]
NPIX_TIE, H_TIE, W_TIE = 600, 20, 30
EDGE_NPIX = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049]
EDGE_SHAPES = [(10, 16, 0), (180, 16, 1), (96, 40, 2), (50, 7, 3)]
SEGMENT_SHAPES = [(180, 16, 1), (96, 40, 2), (50, 7, 3)]
SEGMENT_COUNTS = [0, 127, 128, 129, 0, 1, 257, 2048, 0, 2049, 64]       # VQ_CH = 128 and VQ_SB = 2048 straddled; the rest empty
SECOND_TRIP_NPIX = 262144 + 65
SECOND_TRIP = [(10, 16, 0, "k_vq_tile<16,1>"), (129, 16, 1, "k_vq_tile<16,0>"), (50, 7, 3, "k_vq_fwd<0,true,0>")]


def seed_of(K, D):
    return K * 1000 + D


def segment_counts(K):
    return SEGMENT_COUNTS + [0] * (K - len(SEGMENT_COUNTS))


def _ops():
    from hipops import ops
    return ops


def _plan(D, K):
    from hipops import _lib
    return _lib.load().vqw_vq_plan(D, K)


def run_vq(x, embed, B, H, W, id_base=0, momentum=0.0, cs0=0.0, ea0=None, torch_ema_weight=False):
    """One training call on rows x [B*H*W][D] -> host tensors: q rows, commit, ids (flat), cluster_size, embed_avg, embed."""
    K, D = embed.shape
    e = embed.to(DEV).clone()
    cs = torch.full((K,), float(cs0), device=DEV)
    ea = torch.zeros(D, K, device=DEV) if ea0 is None else ea0.to(DEV).clone().contiguous()
    q, commit, ids = _ops().vq_quantize(R.to_map(x, B, H, W).to(DEV), e, cs, ea, True, momentum, 1e-5, id_base=id_base,
                                        torch_ema_weight=torch_ema_weight)
    torch.cuda.synchronize()
    return dict(q=R.to_rows(q), commit=commit.cpu(), ids=ids.reshape(-1).cpu(), cs=cs.cpu(), ea=ea.cpu(), embed=e.cpu())


def _ratio(err, bound):
    """max of err / bound over the elements; an element with bound 0 must have err 0."""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an element whose bound is 0 (no members, or all-zero members) is off"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


def check_raw(x, embed, out, id_base, what, exact=False):
    """The checks of one raw-statistics call (momentum 0, zeroed buffers) -> dict of error / bound ratios."""
    K, D = embed.shape
    n = x.shape[0]
    ids = out["ids"]
    assert ids.dtype == torch.int64 and ids.numel() == n
    assert int(ids.min()) >= id_base and int(ids.max()) < id_base + K, "%s: ids outside [%d, %d)" % (what, id_base, id_base + K)
    ids0 = ids - id_base
    ref_ids, gap = R.search64(x, embed)
    if exact:
        wrong = ids0 != ref_ids
        assert not bool(wrong.any()), "%s: %d of %d ids differ from the exact arg-max, first at pixel %d" % (
            what, int(wrong.sum()), n, int(wrong.nonzero()[0]))
        clear_share = 1.0
    else:
        clr = R.clear(x, embed, gap)
        clear_share = float(clr.double().mean())
        assert clear_share >= CLEAR_CAP, "%s: only %.4f of the pixels are clear" % (what, clear_share)
        wrong = clr & (ids0 != ref_ids)
        assert not bool(wrong.any()), "%s: %d ids differ on clear pixels (smallest gap / bound among them %.2f)" % (
            what, int(wrong.sum()), float((gap[wrong] / R.clear_bound(x, embed)[wrong]).min()))
    assert torch.equal(out["q"], embed[ids0]), "%s: q is not the gather of the kernel's ids" % what
    c64 = float(R.commit64(x, embed, ids0))
    c_err = abs(float(out["commit"].double()) - c64)
    r_commit = c_err / (R.commit_bound(D) * c64) if c64 > 0 else 0.0
    counts, sums = R.stats64(x, ids0, K)
    assert torch.equal(out["cs"].double(), counts), "%s: counts differ from the bincount of the kernel's ids" % what
    if exact:
        assert torch.equal(out["ea"].double(), sums), "%s: sums of integer-valued members are not exact" % what
        r_sums = 0.0
    else:
        r_sums = _ratio((out["ea"].double() - sums).abs(), R.sums_bound(x, ids0, K))
    print("%s: clear %.4f, agreement with float64 %.5f, commit err/bound %.3f, sums err/bound %.3f" % (
        what, clear_share, float((ids0 == ref_ids).double().mean()), r_commit, r_sums))
    assert c_err <= R.commit_bound(D) * c64, "%s: commit %.9g vs %.9g, err / bound %.2f" % (what, float(out["commit"]), c64, r_commit)
    assert r_sums <= 1.0, "%s: sums err / bound %.2f" % (what, r_sums)
    return dict(commit=r_commit, sums=r_sums, clear=clear_share)


def check_same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs between two identical calls" % (what, k)


def _form_case(K, D, plan, what, offset, B=1, H=H_FORM, W=W_FORM):
    assert _plan(D, K) == plan, "%s: vqw_vq_plan(%d, %d) = %d, expected %d" % (what, D, K, _plan(D, K), plan)
    x, embed = R.gauss(K, D, B * H * W, seed_of(K, D), offset)
    id_base = K % 2
    out = run_vq(x, embed, B, H, W, id_base=id_base)
    res = check_raw(x, embed, out, id_base, "K %d D %d plan %d %s" % (K, D, plan, what))
    check_same_bits(out, run_vq(x, embed, B, H, W, id_base=id_base), what)
    return res, out, x, embed, id_base


@pytest.mark.gpu
def test_vq_capacity_switches():
    for D, k1, k2 in CAPACITY_SWITCHES:
        assert _plan(D, k1) == 1 and _plan(D, k2) == 2, "D %d: plans %d / %d at K %d / %d" % (D, _plan(D, k1), _plan(D, k2), k1, k2)


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan,form", FORMS)
def test_vq_every_form(K, D, plan, form):
    """Every template instantiation of the search and the statistics once, on 1500 centred gauss pixels (30 x 50)."""
    _form_case(K, D, plan, form, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan", OFF_ZERO)
def test_vq_off_zero(K, D, plan):
    """Features and codes share an offset of 4: the score (2 e.x - |e|^2) - |x|^2 cancels heavily."""
    _form_case(K, D, plan, "offset %.1f" % OFFSET, OFFSET)


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan,i,j,what", TIES)
def test_vq_ties_to_lowest_index(K, D, plan, i, j, what):
    """embed[j] == embed[i] bit for bit: identical rows go through identical arithmetic, the scores tie exactly, and i < j must
    win - inside a lane's compare chain, across the two lane halves, across blocks and stages."""
    assert _plan(D, K) == plan
    x, embed, seeded = R.tie_inputs(K, D, i, j, NPIX_TIE, seed_of(K, D) + 17 * j)
    out = run_vq(x, embed, 1, H_TIE, W_TIE)
    ids = out["ids"]
    assert not bool((ids == j).any()), "%s: %d pixels took the duplicate %d instead of %d" % (what, int((ids == j).sum()), j, i)
    share = float((ids[seeded] == i).double().mean())
    print("K %d D %d (%d, %d) %s: %.3f of the seeded pixels take %d" % (K, D, i, j, what, share, i))
    assert share >= TIE_SHARE, "%s: only %.3f of the seeded pixels take %d" % (what, share, i)
    assert float(out["cs"][j]) == 0.0, "%s: the duplicate %d has %g members" % (what, j, float(out["cs"][j]))
    ref_ids, gap = R.search64(x, embed)
    clr = R.clear(x, embed, gap)
    assert torch.equal(ids[clr], ref_ids[clr])
    assert torch.equal(out["q"], embed[ids])
    assert torch.equal(out["cs"].double(), torch.bincount(ids, minlength=K).double())


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan", EDGE_SHAPES)
def test_vq_pixel_count_edges(K, D, plan):
    """One pixel; one wave's tile, the MFMA workgroup tile, a full workgroup and the sort block, each +- 1.  Integer-valued inputs:
    ids, counts and sums are exact."""
    assert _plan(D, K) == plan
    for n in EDGE_NPIX:
        x, embed = R.integer_valued(K, D, n, seed_of(K, D) + n)
        id_base = n % 2
        out = run_vq(x, embed, 1, 1, n, id_base=id_base)
        check_raw(x, embed, out, id_base, "K %d D %d Npix %d" % (K, D, n), exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan", SEGMENT_SHAPES)
def test_vq_segment_boundaries(K, D, plan):
    """Member counts that straddle a segment item (VQ_CH = 128) and a sort block (VQ_SB = 2048), empty codes between populated
    ones; then the EMA update of the same data against ema64 within vq_ref.ema_bounds (derived there from the operation count of
    k_vq_ema: cluster_size 4 u c; embed_avg 5 u (|m ea| + |om S|); embed that over cs_n plus 18 u |embed|)."""
    assert _plan(D, K) == plan
    want = segment_counts(K)
    x, embed = R.with_counts(K, D, want, seed_of(K, D))
    n = x.shape[0]
    out = run_vq(x, embed, 1, 1, n)
    check_raw(x, embed, out, 0, "K %d D %d segments" % (K, D), exact=True)
    assert out["cs"].tolist() == [float(c) for c in want]
    assert float(out["commit"]) == 0.0
    counts, sums = R.stats64(x, out["ids"], K)
    cs0 = torch.full((K,), 3.0)
    ea0 = (3.0 * embed).t().contiguous()
    for tew in (False, True):
        m, om, eps = R.ema_weights(0.9, tew)
        got = run_vq(x, embed, 1, 1, n, momentum=0.9, cs0=3.0, ea0=ea0, torch_ema_weight=tew)
        assert torch.equal(got["ids"], out["ids"])
        ref = R.ema64(counts, sums, cs0, ea0, m, om, eps)
        bnd = R.ema_bounds(counts, sums, cs0, ea0, m, om, eps)
        ratios = {}
        for key, name in (("cs", "cluster_size"), ("ea", "embed_avg"), ("embed", "embed")):
            assert bool(torch.isfinite(got[key]).all()), "%s is not finite (empty codes)" % name
            ratios[name] = _ratio((got[key].double() - ref[name]).abs(), bnd[name])
        print("K %d D %d EMA torch_ema_weight %s: err / bound %s" % (K, D, tew, {k: round(v, 3) for k, v in ratios.items()}))
        for name, r in ratios.items():
            assert r <= 1.0, "%s: err / bound %.2f" % (name, r)
    # the two weights differ (0.1f - ulp vs the rounded double): the switch must reach the kernel
    assert R.ema_weights(0.9, False)[1] != R.ema_weights(0.9, True)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,plan,form", SECOND_TRIP)
def test_vq_second_trip(K, D, plan, form):
    """Npix = 262144 + 65: the 1024-workgroup grid strides a second time for 65 pixels, served by the prefetch of the first trip."""
    n = SECOND_TRIP_NPIX
    res, out, x, embed, id_base = _form_case(K, D, plan, form + ", second trip", 0.0, 1, 1, n)
    tail = slice(n - 65, n)
    ref_ids, gap = R.search64(x[tail], embed)
    clr = R.clear(x[tail], embed, gap)
    ids0 = out["ids"][tail] - id_base
    assert int(clr.sum()) >= 60 and torch.equal(ids0[clr], ref_ids[clr]), "ids of the last 65 pixels"
    assert torch.equal(out["q"][tail], embed[ids0]), "q rows of the last 65 pixels"


@pytest.mark.gpu
@pytest.mark.parametrize("K,D", [(64, 32), (96, 40)])
def test_vq_backward_branches(K, D):
    """vqw_vq_bwd with both gradients, with gq only, with gcommit only; a loss that uses neither leaves x.grad None."""
    ops = _ops()
    B, H, W = 2, 5, 7
    x, embed = R.gauss(K, D, B * H * W, seed_of(K, D))
    r = R.to_map(torch.randn(B * H * W, D, generator=torch.Generator().manual_seed(3)), B, H, W).to(DEV)

    def call():
        dx = R.to_map(x, B, H, W).to(DEV).requires_grad_(True)
        q, commit, _ = ops.vq_quantize(dx, embed.to(DEV), torch.zeros(K, device=DEV), torch.zeros(D, K, device=DEV), False, 0.9, 1e-5)
        return dx, q, commit

    for name, use_q, gc in (("q and commit", True, 3.0), ("q only", True, None), ("commit only", False, 3.0)):
        dx, q, commit = call()
        loss = ((q * r).sum() if use_q else 0.0) + (gc * commit if gc is not None else 0.0)
        loss.backward()
        ref, bound = R.bwd64(x, R.to_rows(q), R.to_rows(r) if use_q else None, gc)
        ratio = _ratio((R.to_rows(dx.grad).double() - ref).abs(), bound)
        print("K %d D %d backward, %s: err / bound %.3f" % (K, D, name, ratio))
        assert ratio <= 1.0, "%s: err / bound %.2f" % (name, ratio)
    dx, q, commit = call()
    w = torch.ones((), device=DEV, requires_grad=True)
    (w * float(q.detach().sum())).backward()
    assert dx.grad is None and w.grad is not None


@pytest.mark.gpu
def test_vq_lookup_and_mask_scale():
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    for K, D in ((10, 16), (50, 7)):
        embed = torch.randn(K, D, generator=g)
        ids = torch.randint(0, K, (2, 5, 7), generator=g)
        ids[0, 0, 0], ids[1, 4, 6], ids[0, 2, 3], ids[1, 1, 1] = -1, K, 0, K - 1
        inside = (ids >= 0) & (ids < K)
        gather = torch.where(inside[..., None], embed[ids.clamp(0, K - 1)], torch.zeros(()))        # (B, H, W, D)
        out = ops.vq_lookup(ids.to(DEV), embed.to(DEV))
        assert tuple(out.shape) == (2, D, 5, 7)
        got = out.cpu().permute(0, 2, 3, 1)
        assert torch.equal(got, gather), "vq_lookup K %d D %d" % (K, D)
        assert bool((got[~inside] == 0).all())
        assert torch.equal(ops.vq_lookup(ids.int().to(DEV), embed.to(DEV)).cpu().permute(0, 2, 3, 1), gather), "int32 ids"
        mask = (torch.rand(2, 5, 7, generator=g) < 0.6).to(torch.uint8)
        mask[0, 2, 3], mask[1, 1, 1] = 1, 0
        scale = torch.tensor([1.7], dtype=torch.float32)
        got = ops.vq_lookup(ids.to(DEV), embed.to(DEV), mask.to(DEV), scale.to(DEV)).cpu().permute(0, 2, 3, 1)
        assert bool((got[mask == 0] == 0).all()), "masked-out rows"
        assert torch.equal(got, torch.where(mask[..., None] != 0, gather * scale, torch.zeros(()))), "embed * scale, one rounding"
    for n in (1, 1023, 1024, 1025, 5000):
        lab = torch.tensor([0, 1, 2, 7])[torch.randint(0, 4, (n,), generator=g)]
        lab[0] = 7
        mask, ids0, scale = ops.mask_scale(lab.to(DEV))
        assert torch.equal(mask.cpu(), (lab != 0).to(torch.uint8)), "mask at n = %d" % n
        assert torch.equal(ids0.cpu(), lab.clamp(min=1) - 1), "ids0 at n = %d" % n
        want = torch.tensor(float(n), dtype=torch.float32) / torch.tensor(float((lab != 0).sum()), dtype=torch.float32)
        assert scale.dtype == torch.float32 and float(scale.cpu()[0]) == float(want), "scale at n = %d: %r vs %r" % (n, float(scale.cpu()[0]), float(want))
