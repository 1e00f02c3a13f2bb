"""GPU tests of the VQGAN decoder blocks: the GroupNorm(+swish) and self-attention kernels against the float64 restatement
(tests/vqgan_ref.py) at the smallest shapes that can go wrong, run-to-run bit-identity, and the modules on the reference's
fixtures (tests/golden/vqgan_blocks_*.npz, made by tests/golden/make_golden_vqgan_blocks.py).  Run with `pytest -m gpu` on an
MI355X.

Tolerances.  Kernel cases: the relative L2 distance of the kernel's result from the float64 restatement may be at most twice
the distance of the fp32 restatement (the same formulas in plain torch on the host, same input) from it - the project's factor
2 on the reference's own fp32 error, measured per quantity and case.  Module cases: outputs within twice the fixture's own
fp32-against-fp64 spread, gradients through helpers.grad_gate with the float64 restatement as the truth and three fp32
evaluations of it (eight threads, one thread, channels_last) as the variants."""
import pytest
import torch

from helpers import assert_close, grad_gate, rel_err
from unet_dis_ref import weight_pattern
import vqgan_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

# vqw_groupnorm_splits: a plane of at most this many elements (H W C per image) is reduced and finalised by one workgroup,
# a larger one is split across workgroups with a finalise pass (GN_ONE_WG_ELEMS in csrc/groupnorm.hip)
GN_ONE_WG_ELEMS = 16384
SMALLEST_SPLIT_PLANE = (19, 27)          # 513 pixels x 32 channels = 16416 elements: the smallest C = 32 plane that is split


def _dev4(t):
    return t.detach().float().contiguous(memory_format=CL).to(DEV)


def _gate(got, truth, ref32, what):
    """|got - truth| <= 2 |ref32 - truth| (relative L2), figures printed first."""
    spread, e = rel_err(ref32, truth), rel_err(got, truth)
    print("%-34s %.3e from float64, the fp32 restatement %.3e (ratio %.2f)" % (what, e, spread, e / max(spread, 1e-300)))
    assert_close(got, truth, 2.0 * spread, what)


# ------------------------------------------------------------------------------------------------ group_norm
def _gn_inputs(N, C, H, W, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g) + offset
    gamma = 1 + torch.randn(C, generator=g) / 4
    beta = torch.randn(C, generator=g) / 4
    gy = torch.randn(N, C, H, W, generator=g)
    return x, gamma, beta, gy


def _gn_ref(x, gamma, beta, gy, swish, dtype):
    x, gamma, beta = (t.detach().to(dtype).requires_grad_(True) for t in (x, gamma, beta))
    y = V.group_norm_ref(x, gamma, beta, act=swish)
    (y * gy.to(dtype)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _gn_run(x, gamma, beta, gy, swish):
    from hipops import ops
    xd = _dev4(x).requires_grad_(True)
    gd, bd = (t.float().to(DEV).requires_grad_(True) for t in (gamma, beta))
    y = ops.group_norm(xd, gd, bd, eps=1e-6, swish=swish)
    y.backward(_dev4(gy))
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)


def _gn_check(N, C, H, W, swish, seed, offset=0.0, only=None):
    x, gamma, beta, gy = _gn_inputs(N, C, H, W, seed, offset)
    truth = _gn_ref(x, gamma, beta, gy, swish, torch.float64)
    ref32 = _gn_ref(x, gamma, beta, gy, swish, torch.float32)
    got = _gn_run(x, gamma, beta, gy, swish)
    for k in only or ("y", "dx", "dgamma", "dbeta"):
        _gate(got[k], truth[k], ref32[k], "group_norm C=%d %dx%d swish=%d %s" % (C, H, W, swish, k))


@pytest.mark.parametrize("swish", [False, True])
@pytest.mark.parametrize("plane", [(4, 4), (5, 7), (64, 64)])
@pytest.mark.parametrize("C", [32, 64, 96, 512])         # 1, 2, 3 (a group is no float4 multiple) and 16 channels per group
def test_group_norm(C, plane, swish):
    _gn_check(2, C, plane[0], plane[1], swish, seed=C + plane[0])


def test_group_norm_plane_60_sigma_off_zero():
    """The case the double statistics exist for: var = E[x^2] - mean^2 from fp32 sums would lose 3600 x 6e-8 of the output."""
    _gn_check(2, 64, 16, 16, True, seed=5, offset=60.0, only=("y",))


def test_group_norm_smallest_split_plane():
    from hipops import ops
    L = ops._L()
    H, W = SMALLEST_SPLIT_PLANE
    assert (H * W - 1) * 32 <= GN_ONE_WG_ELEMS < H * W * 32
    assert L.vqw_groupnorm_splits(H * W - 1, 32) == 1 and L.vqw_groupnorm_splits(H * W, 32) == 2
    for swish in (False, True):
        _gn_check(2, 32, H, W, swish, seed=9)


@pytest.mark.parametrize("C,plane", [(96, (5, 7)), (64, (64, 64))])         # one-workgroup tier, split tier
def test_group_norm_is_deterministic(C, plane):
    x, gamma, beta, gy = _gn_inputs(2, C, plane[0], plane[1], 3)
    a, b = _gn_run(x, gamma, beta, gy, True), _gn_run(x, gamma, beta, gy, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_swish_operator():
    from networks import nonlinearity
    g = torch.Generator().manual_seed(1)
    x, gy = torch.randn(2, 8, 5, 7, generator=g) * 3, torch.randn(2, 8, 5, 7, generator=g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).requires_grad_(True)
        y = V.swish(xr)
        (y * gy.to(dtype)).sum().backward()
        res[dtype] = (y.detach(), xr.grad)
    xd = _dev4(x).requires_grad_(True)
    y = nonlinearity(xd)
    y.backward(_dev4(gy))
    torch.cuda.synchronize()
    _gate(y, res[torch.float64][0], res[torch.float32][0], "swish y")
    _gate(xd.grad, res[torch.float64][1], res[torch.float32][1], "swish dx")


# ------------------------------------------------------------------------------------------------ self_attention
# Tiles: a workgroup owns 32 rows and walks the other axis in steps of 64 (AT_BM, AT_BN in csrc/attention.hip).  12 x 12 =
# 144 = 4 x 32 + 16 = 2 x 64 + 16: ragged on both axes, three steps.  40 x 40 = 1600 = 25 x 64 would leave no ragged last key
# tile, so that case runs at 41 x 41 = 1681 = 52 x 32 + 17 = 26 x 64 + 17.  The last two cases reach the unsplit route's two- and
# three-block column windows (C = 256, 384): 5 x 7 = 35 is one ragged key step and a ragged second row tile, 9 x 9 = 81 two key
# steps with both axes ragged.
ATTN_CASES = [(2, 4, 4, 32), (1, 12, 12, 64), (1, 41, 41, 128), (2, 16, 16, 512), (1, 5, 7, 256), (1, 9, 9, 384)]


def _attn_inputs(B, H, W, C, seed, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(B, C, H, W, generator=g) for _ in range(4))
    return q * qscale, k, v, go


def _attn_ref(q, k, v, go, scale, dtype):
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    o, lse = V.attention_ref(q, k, v, scale)
    (o * go.to(dtype)).sum().backward()
    return dict(o=o.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _attn_run(q, k, v, go, scale):
    from hipops import ops
    qd, kd, vd = (_dev4(t).requires_grad_(True) for t in (q, k, v))
    o = ops.self_attention(qd, kd, vd, scale)
    o.backward(_dev4(go))
    with torch.no_grad():
        o2, lse = ops.self_attention_lse(qd, kd, vd, scale)
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), o2)
    return dict(o=o.detach(), lse=lse, dq=qd.grad, dk=kd.grad, dv=vd.grad)


def _attn_check(B, H, W, C, seed, qscale=1.0):
    q, k, v, go = _attn_inputs(B, H, W, C, seed, qscale)
    scale = int(C) ** (-0.5)
    truth = _attn_ref(q, k, v, go, scale, torch.float64)
    ref32 = _attn_ref(q, k, v, go, scale, torch.float32)
    got = _attn_run(q, k, v, go, scale)
    for key in ("o", "lse", "dq", "dk", "dv"):
        assert got[key].shape == truth[key].shape, key
        _gate(got[key], truth[key], ref32[key], "self_attention %dx%dx%d C=%d %s" % (B, H, W, C, key))
    return q, k, scale


@pytest.mark.parametrize("B,H,W,C", ATTN_CASES)
def test_self_attention(B, H, W, C):
    assert (B, H, W, C) != (1, 41, 41, 128) or ((H * W) % 64 != 0 and (H * W) % 32 != 0)
    assert (B, H, W, C) != (1, 12, 12, 64) or ((H * W) % 64 != 0 and (H * W) % 32 != 0 and H * W > 2 * 64)
    _attn_check(B, H, W, C, seed=C + H)


def test_self_attention_large_logits():
    """scale * S spans more than +-100: exp overflows without the running row maximum."""
    q, k, scale = _attn_check(1, 12, 12, 64, seed=4, qscale=40.0)
    s = torch.einsum("bchw,bcxy->bhwxy", q.double(), k.double()) * scale
    assert float(s.max()) > 100 and float(s.min()) < -100


@pytest.mark.parametrize("B,H,W,C", [(1, 12, 12, 64), (2, 16, 16, 512)])
def test_self_attention_is_deterministic(B, H, W, C):
    q, k, v, go = _attn_inputs(B, H, W, C, 6)
    a, b = _attn_run(q, k, v, go, C ** -0.5), _attn_run(q, k, v, go, C ** -0.5)
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ modules on the fixtures
_cache = {}


def _case(golden, name):
    """The fixture, its state and input, the float64 truth and the three fp32 evaluations of the restatement: computed once."""
    if name not in _cache:
        g = golden("vqgan_blocks_%s.npz" % name)
        state = {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}
        x = g.t(name + "/in")
        out64, truth = V.grads_ref(name, state, x, torch.float64)
        variants = [V.grads_ref(name, state, x, torch.float32)[1]]
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            variants.append(V.grads_ref(name, state, x, torch.float32)[1])
        finally:
            torch.set_num_threads(n)
        variants.append(V.grads_ref(name, state, x, torch.float32, CL)[1])
        _cache[name] = (g, state, x, out64, truth, variants)
    return _cache[name]


def _module(name, state):
    import networks
    cls, kw, _, _ = V.CASES[name]
    m = getattr(networks, cls)(**kw)
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_module_fixture(golden, name):
    g, state, x, out64, truth, variants = _case(golden, name)
    m = _module(name, state).train()
    xin = _dev4(x).requires_grad_(True)
    out = m(xin)
    (out * weight_pattern(out.shape, torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == out64.shape
    sp = float(g[name + "/spread.out"])
    print("%s output: %.3e from float64 (fixture spread %.1e)" % (name, rel_err(out, out64), sp))
    test = {k: p.grad for k, p in m.named_parameters()}
    test["input"] = xin.grad
    assert set(test) == set(truth)
    ok_out = rel_err(out, out64) <= 2.0 * sp
    grad_gate(truth, variants, test, what=name)
    assert ok_out, "%s output %.3e from float64 > 2 x %.1e" % (name, rel_err(out, out64), sp)


def test_decoder_eval_forward(golden):
    g, state, x, out64, _, _ = _case(golden, "decoder")
    m = _module("decoder", state).eval()
    with torch.no_grad():
        out = m(_dev4(x))
    torch.cuda.synchronize()
    sp = float(g["decoder/spread.eval_out"])
    print("decoder eval output: %.3e from float64 (fixture spread %.1e)" % (rel_err(out, out64), sp))
    assert_close(out, out64, 2.0 * sp, "decoder eval output")
