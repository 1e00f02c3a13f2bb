"""The case table of tests/test_gpu_patchgan.py, checked without a GPU: the library loads on a CPU-only machine and its
`*_ws_bytes` queries are host code.  Every row is legal geometry, reaches the routes it claims (by the restated predicates, and
by the size queries where those can tell), every route of the list is claimed by a row, the float64 reference of the LeakyReLU
rows leaves at most MASK_FRACTION of the outputs inside the band with the seeds in use, and the hinge inputs hold their
planted kink values."""
import pytest
import torch

import test_gpu_patchgan as T


def _lib():
    from hipops import _lib
    return _lib.load()


def test_rows_are_legal_and_distinct():
    rows = T.ROUTE_CASES + T.MISALIGNED_CASES
    assert all(T.legal(c) for c in rows), [c for c in rows if not T.legal(c)]
    assert len(set(c[:10] for c in T.ROUTE_CASES)) == len(T.ROUTE_CASES)
    L = _lib()
    fake = 4096                                     # never dereferenced: geometry is validated before any device work
    for c in rows:
        N, H, W, Cin, Cout, ks, stride, pad = c[:8]
        assert T.out_dim(H, ks, stride, pad) >= 1 and T.out_dim(W, ks, stride, pad) >= 1
    # check_sconv itself refuses what legal() refuses (the first two) and the library says why
    for bad in ((1, 2, 2, 3, 3, 4, 1, 0), (1, 8, 8, 3, 3, 3, 3, 1), (1, 8, 8, 3, 3, 8, 1, 1), (1, 8, 8, 3, 3, 3, 1, 3)):
        assert not T.legal(bad + (False, 1.0))
        assert L.vqw_sconv_fwd(fake, fake, None, fake, fake, 16, *bad, 1.0, None) != 0
        assert b"bad geometry" in L.vqw_last_error()


@pytest.mark.parametrize("case", T.ROUTE_CASES, ids=T.case_id)
def test_row_reaches_the_routes_it_claims(case):
    r = T.routes(case)
    claimed = case[10].split()
    assert claimed, "a row names what it is there for"
    for name in claimed:
        assert name in T.ROUTES, "unknown route %r" % name
        assert T.ROUTES[name](case, r), "%s does not reach %s: %r" % (T.case_id(case), name, r)
    T.size_query_facts(_lib(), case)


def test_every_route_is_claimed():
    claimed = set(name for c in T.ROUTE_CASES for name in c[10].split())
    assert claimed == set(T.ROUTES), sorted(set(T.ROUTES) ^ claimed)


def test_no_row_is_larger_than_the_wrap_rows():
    """The largest tensors of the table are those of the rows that must wrap a grid."""
    def floats(c):
        N, H, W, Cin, Cout, ks, stride, pad = c[:8]
        return N * H * W * Cin + N * T.out_dim(H, ks, stride, pad) * T.out_dim(W, ks, stride, pad) * Cout
    wraps = [c for c in T.ROUTE_CASES if "wrap" in c[10]]
    assert len(wraps) >= 4
    assert max(map(floats, T.ROUTE_CASES)) == max(map(floats, wraps)) <= 3_000_000


@pytest.mark.parametrize("case", [c for c in T.ROUTE_CASES + T.MISALIGNED_CASES if c[9] != 1.0], ids=T.case_id)
def test_slope_rows_stay_clear_of_the_mask_band(case):
    z, _ = T.pre_activation(case)
    share = float(T.band(z).double().mean())
    assert share <= T.MASK_FRACTION, "%s: %.2e of the float64 pre-activations inside the band; change the row" % (T.case_id(case), share)
    assert float((z.detach() > 0).double().mean()) > 0.2 and float((z.detach() < 0).double().mean()) > 0.2      # both branches taken


def test_misaligned_rows_reach_the_guards():
    """One row per guard: the Cout = 1 shape (x, w, gx), the Cin = 1 shape (y, gy), and a generic float4 shape (x, w)."""
    fwd = [T.routes(c)["fwd"] for c in T.MISALIGNED_CASES]
    assert fwd == ["o1", "c1", "generic"] and T.MISALIGNED_CASES[2][3] % 4 == 0
    assert not any(T.routes(c)["mfma"] for c in T.MISALIGNED_CASES)


def test_hinge_inputs_hold_the_planted_kinks():
    assert sorted(T.HINGE_SHAPES) == [1, 1023, 1025, 30752, 524288 + 3]
    for n, shape in T.HINGE_SHAPES.items():
        assert len(shape) == 4 and shape[0] * shape[1] * shape[2] * shape[3] == n
        if n == 1:
            assert [float(T.hinge_input(1, v)) for v in range(3)] == [1.0, -1.0, 0.0]
            continue
        x = T.hinge_input(n)
        assert shape[1] > 1, "channels_last must differ from contiguous"
        for v in T.KINKS:
            assert int((x == v).sum()) >= 3, (n, v)
        cl = x.contiguous(memory_format=torch.channels_last)
        for v in T.KINKS:
            assert int((cl == v).sum()) >= 3
        assert float((x > 1).double().mean()) > 0.1 and float((x < -1).double().mean()) > 0.1      # both sides of both kinks


def test_actnorm_inputs():
    for C in (3, 4, 64, 260):
        far, const = T.actnorm_input(C, "far").double(), T.actnorm_input(C, "const")
        m, s = far[:, 1].mean(), far[:, 1].std()
        assert 800 < float(m / s) < 1250, float(m / s)
        assert bool((const[:, 1] == const[0, 1, 0, 0]).all()) and float(const[0, 1, 0, 0]) != 0.0
    assert {c[0] for c in T.ACTNORM_CASES} == {3, 4, 64, 260} and {c[1] for c in T.ACTNORM_CASES} == {0.2, 1.0}
    assert {c[3] for c in T.ACTNORM_CASES} == {"randn", "far", "const"}


@pytest.mark.parametrize("case", T.ACTNORM_CASES, ids=lambda c: "C%d-slope%g-%s-%s" % (c[0], c[1], "init" if c[2] else "given", c[3]))
def test_actnorm_cases_stay_clear_of_the_mask_band(case):
    x, r, loc0, scale0, x64, loc64, scale64 = T.actnorm_setup(case)
    share = float(T.actnorm_band(case, scale64 * (x64 + loc64)).double().mean())
    assert share <= T.MASK_FRACTION, "%.2e of the float64 pre-activations inside the band; change the seed of the case" % share
