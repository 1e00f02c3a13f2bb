"""GPU tests of the rest of the VQGAN: the 3x3 stride-2 convolution behind a bottom / right pad (ops.conv2d_down2), self-attention
above 512 channels, and Downsample / Encoder / VQGAN on the reference's fixtures (tests/golden/vqgan_model_*.npz, made by
tests/golden/make_golden_vqgan_model.py).  Run with `pytest -m gpu` on an MI355X.

Tolerances, the project's rule: a kernel quantity may be at most twice as far (relative L2) from the float64 CPU result
as the fp32 CPU evaluation of the same formula on the same input is; module outputs within twice the fixture's own
fp32-against-fp64 spread, gradients through helpers.grad_gate with the float64 restatement as the truth and three fp32 evaluations
of it (eight threads, one thread, channels_last) as the variants.  The ratios are printed."""
import pytest
import torch

from helpers import assert_close, assert_ids_equal_where_clear, grad_gate, rel_err
from unet_dis_ref import weight_pattern
import vqgan_ref as V
import vqgan_model_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


def _dev4(t):
    return t.detach().float().contiguous(memory_format=CL).to(DEV)


def _gate(got, truth, ref32, what):
    """|got - truth| <= 2 |ref32 - truth| (relative L2), figures printed first."""
    spread, e = rel_err(ref32, truth), rel_err(got, truth)
    print("%-44s %.3e from float64, the fp32 restatement %.3e (ratio %.2f)" % (what, e, spread, e / max(spread, 1e-300)))
    assert_close(got, truth, 2.0 * spread, what)


# ------------------------------------------------------------------------------------------------ conv2d_down2
# (N, Cin, Cout, H, W).  The forward and the input gradient tile 128 pixels (of y, of gy) per workgroup; the weight gradient takes
# the nine-matrix row kernel when W / 2 is a multiple of 16 and the per-tap kernel otherwise, in splits of at least 256 pixels.
DOWN_CASES = [
    (1, 32, 32, 4, 4),          # every output touches the padding
    (2, 32, 64, 6, 10),         # non-square, odd output height, Cin != Cout
    (2, 64, 64, 18, 34),        # 153 output pixels per image: ragged pixel tile, and a tile that crosses the image boundary
    (1, 96, 96, 8, 8),          # three 32-channel chunks
    (1, 512, 512, 8, 8),        # the widest layer with the fewest pixels
    (2, 32, 32, 64, 64),        # several weight-gradient splits, the row kernel
]
_down_cache = {}


def _down_inputs(case):
    N, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(Cin + Cout + H)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    gy = torch.randn(N, Cout, H // 2, W // 2, generator=g)
    return x, w, b, gy


def _down_ref(case, dtype):
    """y, gx, gw, gb of the restatement on the host: computed once per case and dtype, shared by the tests below."""
    if (case, dtype) not in _down_cache:
        x, w, b, gy = (t.to(dtype).requires_grad_(True) for t in _down_inputs(case))
        y = M.down2_ref(x, w, b)
        (y * gy.detach()).sum().backward()
        _down_cache[(case, dtype)] = dict(y=y.detach(), gx=x.grad, gw=w.grad, gb=b.grad)
    return _down_cache[(case, dtype)]


def _down_run(case, op=None):
    from hipops import ops
    x, w, b, gy = _down_inputs(case)
    xd, wd = _dev4(x).requires_grad_(True), _dev4(w).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    y = ops.conv2d_down2(xd, wd, bd) if op is None else op(xd, wd, bd)
    y.backward(_dev4(gy))
    torch.cuda.synchronize()
    return dict(y=y.detach(), gx=xd.grad, gw=wd.grad, gb=bd.grad)


@pytest.mark.parametrize("case", DOWN_CASES, ids=lambda c: "%dx%dto%d_%dx%d" % c)
def test_conv2d_down2(case):
    truth, ref32, got = _down_ref(case, torch.float64), _down_ref(case, torch.float32), _down_run(case)
    assert got["y"].shape == truth["y"].shape and got["y"].is_contiguous(memory_format=CL) and got["gw"].is_contiguous(memory_format=CL)
    for k in ("y", "gx", "gw", "gb"):
        _gate(got[k], truth[k], ref32[k], "conv2d_down2 %dx%d->%d %dx%d %s" % (case + (k,)))


@pytest.mark.parametrize("case", [DOWN_CASES[2], DOWN_CASES[5]], ids=["per_tap", "rows"])
def test_conv2d_down2_wgrad_accumulates(case):
    """accumulate = 1 adds the weight and bias gradients into what the buffers hold."""
    from hipops import ops
    N, Cin, Cout, H, W = case
    x, w, b, gy = _down_inputs(case)
    g = torch.Generator().manual_seed(11)
    gw0, gb0 = torch.randn(Cout, Cin, 3, 3, generator=g), torch.randn(Cout, generator=g)
    truth, ref32 = _down_ref(case, torch.float64), _down_ref(case, torch.float32)
    L = ops._L()
    gw, gb = _dev4(gw0), gb0.to(DEV)
    ws = torch.empty(L.vqw_conv3s2_wgrad_ws_bytes(N, H, W, Cin, Cout), dtype=torch.uint8, device=DEV)
    L.vqw_conv3s2_wgrad(_dev4(x), _dev4(gy), gw, gb, ws, ws.numel(), N, H, W, Cin, Cout, 1)
    torch.cuda.synchronize()
    _gate(gw, gw0.double() + truth["gw"], gw0 + ref32["gw"], "conv2d_down2 accumulate gw")
    _gate(gb, gb0.double() + truth["gb"], gb0 + ref32["gb"], "conv2d_down2 accumulate gb")


@pytest.mark.parametrize("case", [DOWN_CASES[2], DOWN_CASES[5]], ids=["per_tap", "rows"])
def test_conv2d_down2_is_deterministic(case):
    a, b = _down_run(case), _down_run(case)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_conv2d_down2_agrees_with_the_embedded_4x4_route():
    """ops.sconv2d on the 3x3 kernel embedded in a zero 4x4 one (stride 2, padding 1) computes the same layer: both routes sit inside
    the float64 gate (different summation orders, so no bit equality is asked)."""
    from hipops import ops
    case = DOWN_CASES[2]
    truth, ref32 = _down_ref(case, torch.float64), _down_ref(case, torch.float32)
    w4 = {}

    def embedded(x, w, b):
        w4["w"] = _dev4(M.embed4(w.detach())).requires_grad_(True)
        return ops.sconv2d(x, w4["w"], b, stride=2, padding=1)
    got, emb = _down_run(case), _down_run(case, embedded)
    emb["gw"] = w4["w"].grad[:, :, 1:, 1:]
    for k in ("y", "gx", "gw", "gb"):
        _gate(got[k], truth[k], ref32[k], "conv2d_down2 %s" % k)
        _gate(emb[k], truth[k], ref32[k], "embedded 4x4 %s" % k)


# ------------------------------------------------------------------------------------------------ self_attention above 512 channels
# C > 512 runs every pass as two halves of the value / output columns.  576 = 2 x 288: three 128-channel blocks per half, the last
# one ragged (32 channels); 5 x 7 = 35 positions: a ragged row tile and a ragged key step.
def _attn_ref(q, k, v, go, scale, dtype):
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    o, lse = V.attention_ref(q, k, v, scale)
    (o * go.to(dtype)).sum().backward()
    return dict(o=o.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _attn_inputs(B, H, W, C, seed, qscale):
    g = torch.Generator().manual_seed(seed)
    q, k, v, go = (torch.randn(B, C, H, W, generator=g) for _ in range(4))
    return q * qscale, k, v, go


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


@pytest.mark.parametrize("B,H,W,C", [(1, 4, 4, 1024), (2, 5, 7, 576), (1, 16, 16, 1024)])
def test_self_attention_wide(B, H, W, C):
    """o, lse and the three gradients, q scaled so that scale S spans beyond +-100; two runs give the same bits."""
    q, k, v, go = _attn_inputs(B, H, W, C, seed=C + H, qscale=40.0)
    scale = int(C) ** (-0.5)
    s = torch.einsum("bchw,bcxy->bhwxy", q.double(), k.double()) * scale
    print("scale S spans %.1f ... %.1f" % (float(s.min()), float(s.max())))
    assert float(s.max()) > 100 and float(s.min()) < -100
    truth, ref32 = _attn_ref(q, k, v, go, scale, torch.float64), _attn_ref(q, k, v, go, scale, torch.float32)
    got, again = _attn_run(q, k, v, go, scale), _attn_run(q, k, v, go, scale)
    for key in ("o", "lse", "dq", "dk", "dv"):
        assert got[key].shape == truth[key].shape, key
        assert torch.equal(got[key], again[key]), key
        _gate(got[key], truth[key], ref32[key], "self_attention %dx%dx%d C=%d %s" % (B, H, W, C, key))


def test_self_attention_512_is_unsplit_and_repeatable():
    """(2, 16x16, 512), the widest unsplit shape: one column window, the same bits on two runs, and inside the gate as before."""
    q, k, v, go = _attn_inputs(2, 16, 16, 512, seed=6, qscale=1.0)
    scale = 512 ** -0.5
    a, b = _attn_run(q, k, v, go, scale), _attn_run(q, k, v, go, scale)
    truth, ref32 = _attn_ref(q, k, v, go, scale, torch.float64), _attn_ref(q, k, v, go, scale, torch.float32)
    for key in a:
        assert torch.equal(a[key], b[key]), key
        _gate(a[key], truth[key], ref32[key], "self_attention 2x16x16 C=512 %s" % key)


# ------------------------------------------------------------------------------------------------ modules on the fixtures
_cache = {}


def _case(golden, name):
    """The fixture, its state and input, the float64 truth and the three fp32 evaluations of the restatement: computed once."""
    if name not in _cache:
        g = golden("vqgan_model_%s.npz" % name)
        state = {str(k): g.t("%s/P.%s" % (name, k)) for k in g["%s/keys" % name]}
        x = g.t(name + "/in")
        res64, truth = M.grads_ref(name, state, x, torch.float64)
        variants = [M.grads_ref(name, state, x, torch.float32)[1]]
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            variants.append(M.grads_ref(name, state, x, torch.float32)[1])
        finally:
            torch.set_num_threads(n)
        variants.append(M.grads_ref(name, state, x, torch.float32, CL)[1])
        _cache[name] = (g, state, x, res64, truth, variants)
    return _cache[name]


def _module(name, state):
    import networks
    cls, args, _ = M.CASES[name]
    m = getattr(networks, cls)(*args)
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


def _within(got, truth, sp, what):
    print("%-24s %.3e from float64 (fixture spread %.1e)" % (what, rel_err(got, truth), sp))
    assert_close(got, truth, 2.0 * sp, what)


@pytest.mark.parametrize("name", ["down64", "encoder"])
def test_module_fixture(golden, name):
    g, state, x, res64, truth, variants = _case(golden, name)
    m = _module(name, state).train()
    xin = _dev4(x).requires_grad_(True)
    out = m(xin)
    (out * weight_pattern(out.shape, torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == res64["out"].shape
    test = {k: p.grad for k, p in m.named_parameters()}
    test["input"] = xin.grad
    assert set(test) == set(truth)
    grad_gate(truth, variants, test, what=name)
    _within(out, res64["out"], float(g[name + "/spread.out"]), name + " output")


def test_vqgan_fixture(golden):
    name = "vqgan"
    g, state, x, res64, truth, variants = _case(golden, name)
    m = _module(name, state).train()
    xin = _dev4(x).requires_grad_(True)
    recon, commit, ids, emb = m(xin)
    ((recon * weight_pattern(recon.shape, torch.float32).to(DEV)).sum() + commit).backward()
    torch.cuda.synchronize()
    assert recon.shape == res64["recon"].shape and ids.shape == res64["ids"].shape and emb.shape == res64["emb"].shape
    clear = assert_ids_equal_where_clear(ids, g[name + "/ids"], g[name + "/gap"], what="vqgan ids")
    assert clear == 1.0 and torch.equal(ids.cpu(), res64["ids"])          # the fixture's margins: equal everywhere
    test = {k: p.grad for k, p in m.named_parameters()}
    test["input"] = xin.grad
    assert set(test) == set(truth)
    grad_gate(truth, variants, test, what=name)
    _within(recon, res64["recon"], float(g[name + "/spread.out"]), "vqgan recon")
    _within(commit, res64["commit"], float(g[name + "/spread.commit"]), "vqgan commit_loss")
    _within(emb, res64["emb"], float(g[name + "/spread.emb"]), "vqgan emb")


def test_vqgan_fixture_vq_buffers_after_the_step(golden):
    """embed, cluster_size and embed_avg after one training forward, within twice the fixture's spreads.  The VQGAN's quantiser
    weighs the new statistics with the double 1 - momentum rounded once, as torch does (VQ.torch_ema_weight): with 1.f - momentum
    formed in float32, 9.5e-7 away at 0.99, cluster_size alone sat 9.5e-7 from float64 against a bound of 1.3e-7."""
    name = "vqgan"
    g, state, x, res64, _, _ = _case(golden, name)
    m = _module(name, state).train()
    with torch.no_grad():
        m(_dev4(x))
    torch.cuda.synchronize()
    figures = {k: (rel_err(getattr(m.vq, k), res64["buffers"][k]), float(g["%s/spread.buf.%s" % (name, k)])) for k in ("embed", "cluster_size", "embed_avg")}
    for k, (e, sp) in figures.items():
        print("vqgan vq.%-14s %.3e from float64 (fixture spread %.1e)" % (k, e, sp))
    for k, (e, sp) in figures.items():
        assert e <= 2.0 * sp, "vq.%s: %.3e from float64 > 2 x %.1e" % (k, e, sp)


def test_vqgan_generate_and_forward_composition(golden):
    name = "vqgan"
    g, state, x, res64, _, _ = _case(golden, name)
    m = _module(name, state).eval()
    with torch.no_grad():
        gen = m.generate_image_from_ids(g.t(name + "/ids").to(DEV))
        gen64 = M.generate_ref(g.t(name + "/ids"), {k: v.double() for k, v in state.items()})
        recon, commit, ids, emb = m(_dev4(x))
        z = m.encoder(_dev4(x))
        e2, c2, i2 = m.vq(z)
        r2 = m.decoder(e2)
    torch.cuda.synchronize()
    _within(gen, gen64, float(g[name + "/spread.gen_out"]), "vqgan generate_image_from_ids")
    assert torch.equal(recon, r2) and torch.equal(commit, c2) and torch.equal(ids, i2) and torch.equal(emb, e2)
