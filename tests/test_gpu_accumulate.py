"""The ACCUMULATING forms of the gradient kernels against float64.

Every layer of the first-step trainer is used twice per step (once per view) and both uses share one gradient buffer: the
first weight-gradient launch overwrites `weight.grad`, the second runs with accumulate = 1.  The branches of a gradient group
(ops.GradGroup) do the same for input gradients: y += conv(...) in a kernel epilogue.  test_conv2d back-propagates once into
fresh parameters, so it never sees those paths; the tests here do, on every route, against torch on the CPU in float64
(F.conv2d on the virtual input [up2x(x0) | x1], test_gpu_parity._conv_ref; device inputs = the float32 roundings).

1. k uses of one layer plus a preset gradient G0 (RMS of G0 = RMS of the float64 gradient, so a lost or doubled preset or view
   is a 100 % error): per tensor  |got - (G0 + sum g_i)|_2 <= 2e-5 |sum g_i|_2 + 2^-23 |G0 + sum g_i|_2  - test_conv2d's
   single-kernel bound on the gradient part plus the one fp32 rounding of adding the preset; the preset buys no slack.
2. m convolutions of one tensor in a GradGroup: x.grad against the float64 sum of the m input gradients at 2e-5.
3. vqw_sconv_wgrad / vqw_bn_affine_bwd_apply with accumulate = 1 (ops.py always passes 0) into preset buffers.

Every test prints the relative errors it measured ("ACC <route> | <tensor> <error>"; run with -s to see them).

Where the accumulate lives, per route (read from the predicates of conv.hip / conv_mfma.hip / conv_thin.hip):
  own finalize ............ k_stem_wgrad_finalize, k_head_wgrad_finalize (dW and db), k_reduce_wgup (dW; its db goes through
                            reduce_rows)
  reduce_rows ............. everything else: the direct kernel, bias_grad, the per-tap kernel (launch_wgrad, which switches to
                            the workspace when splits == 1 and accumulate is set), the all-taps and block-tile kernels, the
                            row-chain kernel (conv_dil_wgrad), the Winograd forms, the nine-product up-sampled form
                            (conv_wino_up_wgrad) and the streaming 1x1 (conv_pw_wgrad).  Immediate folds run k_reduce_rows
                            (n < 4096 or unaligned) or k_reduce_rows_few; deferred ones are records of k_fold_multi (vec /
                            non-vec, one or two segments).
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, rel_err
from test_gpu_parity import CONV_CASES, SCONV_CASES, _conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
TOL = 2e-5                  # the project's single-kernel bound (test_conv2d)
EPS32 = 2.0 ** -23          # one fp32 rounding of (preset + gradient)


def _ops():
    from hipops import ops
    return ops


def _lib():
    from hipops import _lib
    return _lib.load()


@contextlib.contextmanager
def _fold_hygiene(ops):
    """No deferred fold may outlive the backward pass of a test; whatever a failed test left is dropped so that it cannot poison
    the next one."""
    lib = _lib()
    try:
        yield
    finally:
        lib.vqw_fold_discard()
        try:
            torch.cuda.synchronize()
            assert lib.vqw_fold_pending() == 0 and not ops._fold_keep
        finally:
            ops.begin_step()
            ops.join_streams()      # (begin_step() opens a trainer step: close it, the tests after this file are not inside one)


def _report(route, what, got, want, part, tol=TOL):
    """|got - want|_2 <= tol |part|_2 + 2^-23 |want|_2 where `part` is the gradient part of `want` (want = preset + part)."""
    got = got.detach().double().cpu().reshape(-1)
    want, part = want.reshape(-1), part.reshape(-1)
    assert got.numel() == want.numel(), "%s: %d vs %d elements" % (what, got.numel(), want.numel())
    d, gn = float((got - want).norm()), float(part.norm())
    print("ACC %s | %s %.3e" % (route, what, d / (gn + 1e-30)))
    bound = tol * gn + EPS32 * float(want.norm())
    assert d <= bound, "%s, %s: |diff| %.3e > bound %.3e (%.3e of the gradient part)" % (route, what, d, bound, d / (gn + 1e-30))


# --------------------------------------------------------------------------------------------------
# 1. weight and bias gradients
# --------------------------------------------------------------------------------------------------
# (route, case, folds, each): case = N, H, W, C0, C1, up, Cout, ks, dil, bias, relu as in CONV_CASES; folds: some gradient of the
# layer goes through reduce_rows (a third deferred fold into it then needs the flush-and-retry of ops._run_wgrad).
# P = N H W, Cin = C0 + C1.  Dispatch order of vqw_conv2d_wgrad: conv_stem_wgrad_ok, conv_head_ok, conv_pw_wgrad_ok,
# conv_mfma_wgrad_ok (C0 % 4 == C1 % 4 == Cout % 4 == 0, Cin >= 8, Cout >= 8), else bias_grad + conv_direct_wgrad; inside
# conv_mfma_wgrad: Winograd form (dilation-2 phase form | ks 3, dil 1, P >= 32, Cin % 16 == 0, Cout % 32 == 0, W % 16 == 0),
# wg9_ok (ks 3, W % 32 == 0) -> conv_dil_wgrad (C0 == 32, Cout <= 32, dil >= 2) | block tiles (dil 1) | k_conv_wgrad9, else the
# per-tap kernel (launch_wgrad).
WG_CASES = [
    # k_stem_wgrad_finalize: C0 == 1 and Cout == 16 (k_stem_wgrad<16>), 3x3 with bias and 1x1 (taps = 1) without
    ("stem16", (2, 16, 16, 1, 0, False, 16, 3, 1, True, False), False, True),
    ("stem16", (2, 24, 16, 1, 0, False, 16, 1, 1, False, False), False, False),
    # k_stem_wgrad_finalize behind k_stem_wide_wgrad: Cout % 64 == 0, 64 <= Cout <= 256; dilated without bias
    ("stem-wide", (2, 24, 20, 1, 0, False, 256, 3, 1, True, False), False, True),
    ("stem-wide", (1, 20, 12, 1, 0, False, 192, 3, 2, False, False), False, False),
    # 1 -> 32 is no stem weight gradient (Cout not 16, not a multiple of 64) and C0 % 4 != 0: bias_grad + conv_direct_wgrad,
    # nout = 288 (2 slabs: P / 1024), db n = 32 with 4 rows; ReLU
    ("direct", (1, 32, 64, 1, 0, False, 32, 3, 1, True, True), True, False),
    # k_head_wgrad_finalize: Cout == 1, ks == 1, C0 = 32; db[0] accumulates too
    ("head", (2, 16, 16, 32, 0, False, 1, 1, 1, True, False), False, True),
    ("head", (2, 8, 64, 32, 0, False, 1, 1, 1, True, False), False, False),
    # C0 = 3: bias_grad + conv_direct_wgrad, one slab (P / 1024 = 0); nout = 135 and C = 5 are no multiples of 4: non-vec branch of
    # k_fold_multi, partial last 64-column block of k_reduce_rows (135 = 2 * 64 + 7)
    ("direct-nonvec", (2, 10, 10, 3, 0, False, 5, 3, 1, True, False), True, True),
    # per-tap kernel: P = 4 < 32 (no Winograd form, no all-taps kernel); wgrad_splits(32, 64, 3, 4): tiles = 9, 6 workgroups per
    # CU -> 170, capped by max(P / 256, 1) = 1: splits == 1, so the accumulating launch writes its slab to the workspace
    # (nout = 18 432 floats, what conv_mfma_wgrad_ws_floats sizes) and folds one row
    ("per-tap-splits1", (1, 2, 2, 32, 0, False, 64, 3, 1, True, False), True, True),
    # per-tap kernel, W = 10 (no multiple of 16): 128 x 64 tile, ragged in both; P = 360 -> splits == 1 as well
    ("per-tap-splits1", (3, 12, 10, 48, 0, False, 80, 3, 1, True, False), True, False),
    # per-tap kernel, 1x1 below the streaming kernel's P: 32 x 32 tile, splits = min(2560, P / 256) = 2; n = 512: k_reduce_rows
    ("per-tap", (2, 16, 16, 16, 0, False, 32, 1, 1, False, False), True, True),
    # per-tap kernel, 128-wide tiles.  CONV_CASES' (2, 16, 16, 128 -> 160) has W % 16 == 0, Cin % 16 == 0, Cout % 32 == 0 and takes
    # the Winograd form (it runs below); the same layer at W = 20 (smallest width above 16 that neither form nor the all-taps kernel
    # serves, P = 640 -> 2 splits) is the 128 x 128 tile; (3, 24, 40, 16 -> 96, dil 2) is the 128 x 32 tile with 11 splits
    ("per-tap-128", (2, 16, 20, 128, 0, False, 160, 3, 1, True, False), True, False),
    ("per-tap-128", (3, 24, 40, 16, 0, False, 96, 3, 2, True, False), True, False),
    # all-taps kernel k_conv_wgrad9: W % 32 == 0, dil 2 (no block tiles), Cout = 80 (no phase form: Cout % 32 != 0), C0 != 32
    # (no row chains); 8 slabs, n = 69 120: k_reduce_rows_few
    ("all-taps", (2, 32, 32, 96, 0, False, 80, 3, 2, True, False), True, True),
    # block-shared tile form (conv_wgrad_tile_ok: dil 1, W % 32 == 0) where the Winograd form does not apply (Cout % 32 != 0 or
    # Cin % 16 != 0): ragged H; two sources (C0 % 32 == 0); (1, 23, 64, 24 -> 48) is CONV_CASES' ragged-H Winograd row:
    # its FORWARD has a Winograd form, its weight gradient is this one (Cin % 16 != 0)
    ("block-tile", (3, 12, 32, 48, 0, False, 80, 3, 1, True, False), True, False),
    ("block-tile", (2, 32, 32, 32, 16, True, 16, 3, 1, True, False), True, False),
    ("block-tile", (1, 23, 64, 24, 0, False, 48, 3, 1, True, False), True, False),
    # conv_dil_wgrad (C0 == 32, Cout <= 32, W % 32 == 0, W + 2 dil <= 320; Cout % 32 != 0 or dil != 2 keeps the phase form away):
    # 24 couts; dilation == H.  Its slabs fold through reduce_rows (no epilogue of its own), db through bias_grad
    ("row-chain", (3, 40, 64, 32, 0, False, 24, 3, 2, True, False), True, False),
    ("row-chain", (1, 8, 32, 32, 0, False, 32, 3, 8, True, False), True, True),
    # Winograd form, generic kernel (C0 % 32 != 0 / H % 4 != 0 / W % 32 != 0 keep the block kernels away): ReLU; ragged odd H;
    # the 128 -> 160 layer at W = 16; two sources with a 16-channel first source
    ("wino", (2, 16, 32, 16, 0, False, 32, 3, 1, True, True), True, True),
    ("wino", (2, 7, 32, 32, 0, False, 96, 3, 1, True, False), True, False),
    ("wino", (2, 16, 16, 128, 0, False, 160, 3, 1, True, False), True, False),
    ("wino", (1, 24, 32, 16, 32, False, 32, 3, 1, True, False), True, False),
    # Winograd form, (64 x 32)-block kernel: Cout % 64 == 0, C0 % 32 == 0, W % 32 == 0, H % 4 == 0
    ("wino64", (2, 16, 32, 64, 0, False, 64, 3, 1, True, False), True, False),
    # ... with an odd number of regions in a workgroup's run (the skipped second region of the last pair, a short last run).
    # wg9_split_blocks caps the slabs at max(P / 256, 1), a region is 128 pixels, one (co, ci) block:
    # W = 32, H = 20: 5 regions of 4 x 32, cap 640 / 256 = 2 -> kt = ceil(5 / 2) = 3: runs of 3 and 2 regions;
    # W = 16, H = 24 (H % 8 == 0): 3 regions of 8 x 16, cap 384 / 256 = 1 -> kt = 3: one run of 3 regions
    ("wino64", (1, 20, 32, 32, 0, False, 64, 3, 1, True, False), True, False),
    ("wino64", (1, 24, 16, 32, 0, False, 64, 3, 1, True, False), True, False),
    # Winograd form, (32 x 32)-block kernel: Cout % 64 == 32, sources % 32 == 0, W % 32 == 0, H % 4 == 0; two sources, the first
    # up-sampled; three co blocks; no bias
    ("wino32", (2, 32, 32, 64, 32, True, 32, 3, 1, True, False), True, False),
    ("wino32", (3, 64, 64, 32, 0, False, 96, 3, 1, True, False), True, False),
    ("wino32", (2, 12, 96, 64, 0, False, 32, 3, 1, False, False), True, False),
    # dilation 2 on the four phase images (conv_wino_blk_wgrad_dil2_ok: the (32 x 32)-block predicate at H / 2, W / 2)
    ("wino-dil2", (2, 16, 64, 32, 0, False, 32, 3, 2, True, False), True, False),
    # vqw_conv3x3_up2_wgrad, k_conv_wgrad_up + k_reduce_wgup: Cout = 16 / 48 keeps the nine-product form away (Cout % 32 != 0).
    # (CONV_CASES lists (1, 40, 32, 64 -> 16) with the nine-product FORWARD; its weight gradient is this kernel, and (2, 32, 32,
    # 128 -> 64), "collapsed" there, has the nine-product weight gradient.)  With a bias db folds through reduce_rows; without, nothing does; ReLU
    ("up2-collapsed", (1, 40, 32, 64, 0, True, 16, 3, 1, True, False), True, True),
    ("up2-collapsed", (1, 64, 32, 32, 0, True, 48, 3, 1, False, True), False, True),
    # vqw_conv3x3_up2_wgrad, conv_wino_up_wgrad (Cin % 32 == Cout % 32 == 0, w % 16 == 0, h % 4 == 0): folds through reduce_rows; ReLU
    ("up2-nine-product", (2, 32, 32, 128, 0, True, 64, 3, 1, True, False), True, False),
    ("up2-nine-product", (3, 16, 96, 128, 0, True, 32, 3, 1, True, True), True, True),
    # conv_pw_wgrad: 1x1, 16 -> 32, P = 131 072 (the smallest it serves); n = 512 folds through reduce_rows
    ("streaming-1x1", (2, 256, 256, 16, 0, False, 32, 1, 1, False, False), True, False),
]
# (b) - (d): one case per accumulate implementation (the last field of its row)
WG_EACH = [e for e in WG_CASES if e[3]]
_listed = set(CONV_CASES)
assert all(c in _listed for _, c, _, _ in WG_CASES if c != (2, 16, 20, 128, 0, False, 160, 3, 1, True, False))
assert sum(1 for _, c, _, _ in WG_CASES if c[10]) >= 3          # ReLU epilogues: the gradient is masked before it is accumulated


def _id(entry):
    return "%s-%s" % (entry[0], "x".join(str(int(v)) for v in entry[1]))


_ref_cache = {}


def _reference(case, k):
    """float64 inputs and gradients of k uses of one layer; one entry is kept (the parametrisation runs a case's variants back to back)."""
    key = (case, k)
    if key in _ref_cache:
        return _ref_cache[key]
    _ref_cache.clear()
    N, H, W, C0, C1, up, Cout, ks, dil, bias, relu = case
    g = torch.Generator().manual_seed((hash(case) + 977 * k) & 0xFFFF)
    hs, wsz = (H // 2, W // 2) if up else (H, W)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    xs = [rnd(N, C0, hs, wsz).requires_grad_(True) for _ in range(k)]
    sk = [rnd(N, C1, H, W).requires_grad_(True) if C1 else None for _ in range(k)]
    rs = [rnd(N, Cout, H, W) for _ in range(k)]
    w = (rnd(Cout, C0 + C1, ks, ks) * 0.2).requires_grad_(True)
    b = rnd(Cout).requires_grad_(True) if bias else None
    sum((_conv_ref(x, s, w, b, up, dil, relu) * r).sum() for x, s, r in zip(xs, sk, rs)).backward()
    rms = lambda t: float(t.norm()) / t.numel() ** 0.5                      # noqa: E731
    # presets with the RMS of the gradient, as the float32 values the device holds
    g0w = (rnd(*w.shape) * rms(w.grad)).float().double()
    g0b = (rnd(Cout) * rms(b.grad)).float().double() if bias else None
    ref = dict(xs=xs, sk=sk, rs=rs, w=w, b=b, g0w=g0w, g0b=g0b)
    _ref_cache[key] = ref
    return ref


def _check_layer(route, case, k, preset, defer, monkeypatch):
    """k uses of one layer on the device; returns the number of batched fold launches the backward pass took."""
    ops = _ops()
    N, H, W, C0, C1, up, Cout, ks, dil, bias, relu = case
    L = ops._L()
    if up and not C1:
        assert L.vqw_conv3x3_up2_supported(C0, Cout, N, H // 2, W // 2) and L.vqw_conv3x3_up2_wgrad_supported(C0, Cout, N, H // 2, W // 2)
    ref = _reference(case, k)
    monkeypatch.setattr(ops, "FOLD_DEFER", defer)
    assert not ops.grad_ready_listeners
    old_backend, old_route = ops.set_conv_backend(0), ops.set_wgrad_route("auto")
    with _fold_hygiene(ops):
        try:
            # OHWI memory with the strides ops.nhwc() normalises to.  For C0 > 1 that is .contiguous(memory_format=channels_last); a
            # 1-channel weight laid out that way keeps its default strides, ops.nhwc() re-strides it, and its gradient then goes
            # through autograd (correct, but the accumulating form of the stem's finalize kernel is never reached)
            dw = torch.empty_strided(ref["w"].shape, (ks * ks * (C0 + C1), 1, ks * (C0 + C1), C0 + C1), dtype=torch.float32, device=DEV)
            dw.copy_(ref["w"].detach().float()).requires_grad_(True)
            db = ref["b"].detach().float().to(DEV).requires_grad_(True) if bias else None
            if preset:      # the parameter's own strides: the side lane rejects another layout
                dw.grad = torch.empty_strided(dw.shape, dw.stride(), dtype=torch.float32, device=DEV).copy_(ref["g0w"].float())
                if bias:
                    db.grad = torch.empty_like(db).copy_(ref["g0b"].float())
            dxs = [x.detach().float().to(DEV).requires_grad_(True) for x in ref["xs"]]
            dsk = [s.detach().float().to(DEV).requires_grad_(True) if s is not None else None for s in ref["sk"]]
            f0 = ops.fold_flushes
            loss = sum((ops.conv2d(x, dw, db, dilation=dil, up2x=up, skip=s, relu=relu) * r.float().to(DEV)).sum()
                       for x, s, r in zip(dxs, dsk, ref["rs"]))
            loss.backward()
            flushes = ops.fold_flushes - f0
            assert _lib().vqw_fold_pending() == 0 and not ops._fold_keep, "folds left behind after the backward pass"
            torch.cuda.synchronize()
        finally:
            ops.set_conv_backend(old_backend)
            ops.set_wgrad_route(old_route)
        assert getattr(dw, "_vqw_pending", None) == 0, "the weight gradient did not take the side lane"
        tag = "%s k=%d%s %s" % (route, k, "+preset" if preset else "", "deferred" if defer else "immediate")
        gw, gb = ref["w"].grad, (ref["b"].grad if bias else None)
        _report(tag, "dw", dw.grad, gw + ref["g0w"] if preset else gw, gw)
        if bias:
            _report(tag, "db", db.grad, gb + ref["g0b"] if preset else gb, gb)
        for i in range(k):
            assert_close(dxs[i].grad, ref["xs"][i].grad, TOL, "dx0 of use %d" % i)
            if C1:
                assert_close(dsk[i].grad, ref["sk"][i].grad, TOL, "dx1 of use %d" % i)
        print("ACC %s | dx %.3e" % (tag, max(rel_err(dxs[i].grad, ref["xs"][i].grad) for i in range(k))))
    return flushes


@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("entry", WG_CASES, ids=_id)
def test_two_views_accumulate_onto_a_preset_gradient(entry, defer, monkeypatch):
    """(a) k = 2 with preset: both launches accumulate; deferred, the two folds are one two-segment record with acc = 1."""
    route, case, _, _ = entry
    n = _check_layer(route, case, 2, True, defer, monkeypatch)
    assert n == (1 if defer else 0), n


@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("entry", WG_EACH, ids=_id)
def test_one_accumulating_launch_onto_a_preset_gradient(entry, defer, monkeypatch):
    """(b) k = 1 with preset: a pure accumulate launch (deferred: a one-segment record with acc = 1)."""
    route, case, _, _ = entry
    _check_layer(route, case, 1, True, defer, monkeypatch)


@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("entry", WG_EACH, ids=_id)
def test_two_views_overwrite_then_accumulate(entry, defer, monkeypatch):
    """(c) k = 2 without preset: the first use overwrites (deferred: the only merged record with acc = 0; on the per-tap kernel
    with splits == 1 the first launch writes dW itself and the second one its workspace)."""
    route, case, _, _ = entry
    _check_layer(route, case, 2, False, defer, monkeypatch)


@pytest.mark.parametrize("entry", WG_EACH, ids=_id)
def test_third_use_flushes_the_recorded_folds_and_retries(entry, monkeypatch):
    """(d) k = 3 with preset, deferred: a record holds two segments, so the third fold into one output is refused ("flush
    first") and ops._run_wgrad folds what is recorded and records again."""
    route, case, folds, _ = entry
    n = _check_layer(route, case, 3, True, True, monkeypatch)
    if folds:       # a gradient of the layer folds through reduce_rows: the flush of the retry plus the one at the end of the pass
        assert n == 2, n
    else:           # k_stem_wgrad_finalize / k_head_wgrad_finalize / k_reduce_wgup without a bias add in their own launch:
        assert n <= 1, n        # nothing is ever recorded, only the end-of-pass launch (over an empty table) may count


# --------------------------------------------------------------------------------------------------
# 2. input gradients summed in place by ops.GradGroup
# --------------------------------------------------------------------------------------------------
# (route, x shape (N, C, H, W) - the low-resolution one for up2x -, members [(Cout, ks, dil)], up2x, group_acc_calls expected)
# The input-gradient convolution of a member maps its Cout channels to C.  The first member autograd runs writes the buffer,
# every later one adds to it on the route under test.
GROUP_CASES = [
    # vqw_conv3x3_wino_fwd_acc: 16 -> 64 on the 64-cout kernel (..._masked_supported: Cin % 16 == 0, Cout % 64 == 0), ragged H
    # (22 = 16 + 6); W % 32 == 16 takes the 16-wide regions, there with m = 3: the buffer is accumulated into twice
    ("wino_fwd_acc", (2, 64, 22, 32), [(16, 3, 1), (16, 3, 1)], False, 1),
    ("wino_fwd_acc", (2, 64, 22, 48), [(16, 3, 1), (16, 3, 1), (16, 3, 1)], False, 2),
    # vqw_conv3x3_wino_dil2_fwd(accumulate = 1): H even, W % 64 == 0, 32 -> 32 (not counted in group_acc_calls)
    ("wino_dil2_acc", (2, 32, 16, 64), [(32, 3, 2), (32, 3, 2)], False, 0),
    # vqw_conv2d_fwd_acc, row-chain kernel (conv_dil_fwd_ok: 32 source channels, <= 32 couts, 2 <= dil <= H, W % 32 == 0):
    # dilations 18 and 37 == H (not counted)
    ("fwd_acc-row-chain", (1, 32, 37, 64), [(32, 3, 18), (32, 3, 37)], False, 0),
    # ... with fewer than 32 output channels: x has 24 channels and the members 32 couts, a 32 -> 24 input-gradient convolution.
    # (The other way round - 32-channel x, 24-cout members - is a 24 -> 32 convolution, which the row-chain kernel does not serve:
    # its source must have 32 channels, and that group falls back to buf.add_.)
    ("fwd_acc-row-chain", (2, 24, 24, 128), [(32, 3, 6), (32, 3, 3)], False, 0),
    # vqw_conv2d_fwd_acc, 1x1 on the implicit-GEMM kernel's relu == 2 epilogue (HW = 2560 < 16 384): 32 -> 32 and 48 -> 32
    ("fwd_acc-1x1-gemm", (2, 32, 40, 64), [(32, 1, 1), (48, 1, 1)], False, 1),
    # vqw_conv2d_fwd_acc, 1x1 on conv_pw_stream mode 1: channels in {16, 32, 64}, HW = 16 384 is the smallest it serves
    ("fwd_acc-1x1-stream", (1, 32, 128, 128), [(32, 1, 1), (32, 1, 1)], False, 1),
    # vqw_conv3x3_up2_dgrad_acc (nine-product kernel: Cin % 64 == 0, Cout % 16 == 0, 2 w % 32 == 0): the 128-channel N tile and
    # the 64-channel one
    ("up2_dgrad_acc", (3, 128, 8, 48), [(32, 3, 1), (32, 3, 1)], True, 1),
    ("up2_dgrad_acc", (1, 64, 20, 16), [(16, 3, 1), (16, 3, 1)], True, 1),
    # no accumulating route (W = 10: no Winograd form; dil 1: no row chains): GradGroup.member_done's buf.add_
    ("buf.add_", (3, 48, 12, 10), [(80, 3, 1), (80, 3, 1)], False, 0),
]


@pytest.mark.parametrize("entry", GROUP_CASES, ids=lambda e: "%s-%s-m%d" % (e[0], "x".join(map(str, e[1])), len(e[2])))
def test_gradient_group_accumulates_input_gradients(entry, monkeypatch):
    ops = _ops()
    route, (N, C, H, W), members, up, n_acc = entry
    L = ops._L()
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    for Cout, ks, dil in members:           # the route every member but the first to run takes (conv2d_backward_impl's order)
        wino = ks == 3 and dil == 1 and not up and L.vqw_conv3x3_wino_supported(Cout, C, N, H, W) \
            and L.vqw_conv3x3_wino_masked_supported(Cout, C, N, H, W)
        dil2 = ks == 3 and dil == 2 and not up and L.vqw_conv3x3_wino_dil2_supported(Cout, C, N, H, W)
        facc = not up and L.vqw_conv2d_fwd_acc_supported(Cout, N, H, W, C, ks, dil)
        if route == "wino_fwd_acc":
            assert wino
        elif route == "wino_dil2_acc":
            assert dil2 and not wino
        elif route.startswith("fwd_acc"):
            assert facc and not wino and not dil2
        elif route == "up2_dgrad_acc":
            assert L.vqw_conv3x3_up2_supported(C, Cout, N, H, W) and L.vqw_conv3x3_up2_dgrad_acc_supported(C, Cout, N, H, W)
        else:
            assert not (wino or dil2 or facc)
    g = torch.Generator().manual_seed(hash((N, C, H, W) + tuple(members[-1])) & 0xFFFF)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rnd(N, C, H, W).requires_grad_(True)
    ws = [(rnd(Cout, C, ks, ks) * 0.2).requires_grad_(True) for Cout, ks, _ in members]
    rs = [rnd(N, Cout, Ho, Wo) for Cout, _, _ in members]
    sum((_conv_ref(x, None, w, None, up, dil, False) * r).sum() for w, r, (_, _, dil) in zip(ws, rs, members)).backward()

    monkeypatch.setattr(ops, "GRAD_GROUPS", True)
    old_backend = ops.set_conv_backend(0)
    with _fold_hygiene(ops):
        try:
            dx = x.detach().float().to(DEV).requires_grad_(True)
            dws = [w.detach().float().to(DEV).contiguous(memory_format=CL).requires_grad_(True) for w in ws]
            grp = ops.GradGroup(len(members))
            n0 = ops.group_acc_calls
            ys = [ops.conv2d(dx, w, None, dilation=dil, up2x=up, grad_group=grp) for w, (_, _, dil) in zip(dws, members)]
            assert grp.members == len(members), "a member opted out of the group"
            sum((y * r.float().to(DEV)).sum() for y, r in zip(ys, rs)).backward()
            torch.cuda.synchronize()
            assert ops.group_acc_calls - n0 == n_acc, (route, ops.group_acc_calls - n0)
        finally:
            ops.set_conv_backend(old_backend)
        print("ACC group %s m=%d | dx %.3e" % (route, len(members), rel_err(dx.grad, x.grad)))
        assert_close(dx.grad, x.grad, TOL, "x.grad of %d grouped members (%s)" % (len(members), route))
        for i, (dw, w) in enumerate(zip(dws, ws)):
            assert_close(dw.grad, w.grad, TOL, "weight gradient of member %d" % i)


# --------------------------------------------------------------------------------------------------
# 3. accumulating forms the header promises and ops.py never asks for
# --------------------------------------------------------------------------------------------------
SCONV_ACC = [
    (2, 32, 32, 16, 32, 4, 2, 1, True, 1.0),      # stride 2 on the matrix cores: k_reduce_wg_k4s2's own accumulate, db through bias_grad
    (3, 16, 16, 32, 16, 4, 1, 1, False, 1.0),     # stride 1 on the common grid: the per-tap kernel's slabs through reduce_rows
    (2, 32, 32, 1, 8, 4, 2, 1, True, 0.2),        # 1-channel direct kernel (k_sconv_wgrad_c1), LeakyReLU mask
    (1, 16, 16, 8, 12, 4, 2, 1, True, 1.0),       # low-res width 8: the generic direct kernel
]
assert all(c in SCONV_CASES for c in SCONV_ACC)


@pytest.mark.parametrize("case", SCONV_ACC)
def test_sconv_wgrad_accumulates(case):
    ops = _ops()
    L = ops._L()
    N, H, W, Cin, Cout, ks, stride, pad, bias, slope = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rnd(N, Cin, H, W)
    w = (rnd(Cout, Cin, ks, ks) * 0.2).requires_grad_(True)
    b = rnd(Cout).requires_grad_(True) if bias else None
    y = F.conv2d(x, w, b, stride=stride, padding=pad)
    gy = rnd(*y.shape)
    if slope != 1.0:        # the kernel takes the gradient behind the LeakyReLU mask (ops.sconv2d applies vqw_leaky_relu_bwd first)
        gy = torch.where(y.detach() > 0, gy, gy * slope)
    (y * gy).sum().backward()
    rms = lambda t: float(t.norm()) / t.numel() ** 0.5                      # noqa: E731
    g0w = (rnd(*w.shape) * rms(w.grad)).float().double()
    g0b = (rnd(Cout) * rms(b.grad)).float().double() if bias else None
    with _fold_hygiene(ops):
        dx = ops.nhwc(x.float().to(DEV))
        dgy = ops.nhwc(gy.float().to(DEV))
        gw = g0w.float().to(DEV).contiguous(memory_format=CL)
        gb = g0b.float().to(DEV) if bias else None
        ws = ops._ws(L.vqw_sconv_wgrad_ws_bytes(Cin, Cout, ks, N, H, W, stride, pad), dx)
        L.vqw_sconv_wgrad(dx, dgy, gw, gb, ws, ws.numel(), N, H, W, Cin, Cout, ks, stride, pad, 1)
        torch.cuda.synchronize()
        tag = "sconv %dx%d s%d %d->%d" % (ks, ks, stride, Cin, Cout)
        _report(tag, "dw", gw, g0w + w.grad, w.grad)
        if bias:
            _report(tag, "db", gb, g0b + b.grad, b.grad)


def test_bn_affine_bwd_apply_accumulates():
    """dgamma / dbeta added to preset buffers, C = 6 (no multiple of 4); the bound is the one the discriminator's BatchNorm
    gradients are held to in test_gpu_gan_norms.py (1e-3, _run_block's gradient tolerance), on the gradient part."""
    ops = _ops()
    L = ops._L()
    N, C, H, W, slope, eps = 3, 6, 5, 7, 0.2, 1e-5
    g = torch.Generator().manual_seed(611)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = (rnd(N, C, H, W) * 1.5 + 0.3).requires_grad_(True)
    gamma = (rnd(C) * 0.5 + 1.0).requires_grad_(True)
    beta = (rnd(C) * 0.3).requires_grad_(True)
    r = rnd(N, C, H, W)
    y = F.leaky_relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps), slope)
    (y * r).sum().backward()
    mean = x.detach().mean((0, 2, 3))
    rstd = (x.detach().var((0, 2, 3), unbiased=False) + eps).rsqrt()
    rms = lambda t: float(t.norm()) / t.numel() ** 0.5                      # noqa: E731
    g0g = (rnd(C) * rms(gamma.grad)).float().double()
    g0b = (rnd(C) * rms(beta.grad)).float().double()
    with _fold_hygiene(ops):
        dx = ops.nhwc(x.detach().float().to(DEV))
        dgy = ops.nhwc(r.float().to(DEV))
        mr = torch.stack([mean, rstd], 1).reshape(-1).float().to(DEV)
        dga, dbe = gamma.detach().float().to(DEV), beta.detach().float().to(DEV)
        sums = torch.empty(2 * C, dtype=torch.float64, device=DEV)
        ws = ops._ws(L.vqw_plane_ws_bytes(N, C, H * W), dx)
        L.vqw_bn_affine_bwd_reduce(dx, mr, dga, dbe, dgy, sums, ws, ws.numel(), N, H * W, C, slope)
        gx = torch.empty_like(dx, memory_format=CL)
        dgamma, dbeta = g0g.float().to(DEV), g0b.float().to(DEV)
        L.vqw_bn_affine_bwd_apply(dx, mr, dga, dbe, dgy, sums, float(N * H * W), gx, dgamma, dbeta, N * H * W, C, slope, 1, 1)
        torch.cuda.synchronize()
        _report("bn_affine_bwd_apply", "dgamma", dgamma, g0g + gamma.grad, gamma.grad, tol=1e-3)
        _report("bn_affine_bwd_apply", "dbeta", dbeta, g0b + beta.grad, beta.grad, tol=1e-3)
        print("ACC bn_affine_bwd_apply | dx %.3e" % rel_err(gx, x.grad))
        assert_close(gx, x.grad, 1e-3, "dx")
