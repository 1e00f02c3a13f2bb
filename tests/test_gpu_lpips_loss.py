"""LPIPS perceptual loss on the MI355X: the HIP path (hipops.ops.lpips_loss / functions.LPIPSLoss) against the fp64
restatement of lpips.LPIPS(net='alex') in lpips_ref.py, and the loss inside both trainers.

Pool routing.  Two overlapping 3x3 / 2 max-pools sit behind ReLUs, and any fp32 evaluation routes a near-tie of a window
differently from fp64.  A window reaches far (19 x 19 input pixels for the first pool, 67 x 67 for the second), so the
gradient comparison leaves out the input pixels reached by a window whose fp64 top-2 gap is positive and at most
1e-5 (1 + |top|) - fp32 accumulation error is of the order 1e-6 relative, so that covers every window an fp32 evaluation
can flip - and asserts that at least 0.9 of the pixels are kept.  Exact ties (gap 0) are never left out: the kernels keep
equal neighbourhoods bit-equal and must route them as fp64 does.
"""
import pytest
import torch

from helpers import assert_close
from lpips_ref import he_weights, lpips_loss_ref, module_ref, unclear_pixels, unpool3, maxpool3

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEEP_MIN = 0.9


def _lp(seed=0, **kw):
    from functions import LPIPSLoss
    return LPIPSLoss(weights=he_weights(seed, **kw)).to(DEV)


def _pair(shape, seed, plateau=False):
    g = torch.Generator().manual_seed(seed)
    sr = torch.rand(shape, generator=g) * 2 - 1
    hr = torch.rand(shape, generator=g) * 2 - 1
    if plateau:                    # a tanh-saturated recon: exact -1 over the left half and a band
        sr[..., :, : shape[-1] // 2] = -1.0
        sr[..., shape[-2] // 3: shape[-2] // 2, :] = -1.0
    return sr, hr


def _ref32(sr, hr, sd, window=None):
    """the reference's own form in fp32 (the F.conv2d / F.max_pool2d stack under autograd on the GPU): its spread around
    fp64 sets the tolerance"""
    x = sr.to(DEV).float().requires_grad_(True)
    loss = module_ref(sd, dtype=torch.float32, device=DEV)(x, hr.to(DEV).float(), window)
    loss.backward()
    return loss.detach().double(), x.grad.double()


def _window():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW
    return ops.window_map((2000, 0, 2.0), LUNG_WINDOW)


def _run(lp, sr, hr, **kw):
    x = sr.to(DEV).contiguous().requires_grad_(True)
    t = hr.to(DEV).contiguous().requires_grad_(True)
    loss = lp(x, t, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, t


@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (4, 1, 96, 80), (1, 1, 31, 31), (1, 1, 67, 93), (2, 3, 64, 64),
                                   (32, 1, 256, 256), (2, 1, 512, 512)])
def test_loss_and_gradient_match_fp64(shape):
    lp = _lp(1)
    sd = lp.state_dict()
    sr, hr = _pair(shape, 3)        # seeds for which the restatement alone keeps >= 0.92 of the pixels at every shape
    loss, g, t = _run(lp, sr, hr)
    rl, rg, info = lpips_loss_ref(sr, hr, sd, device=DEV)          # asserts: no all-zero feature pixel
    unclear, nwin = unclear_pixels(info, shape[2], shape[3])
    keep = (~unclear).double()
    kept = float(keep.mean())
    # the reference's fp32 spread around fp64, from two fp32 renderings of it: the F.conv2d module stack and the
    # restatement's own operations in fp32
    variants = [_ref32(sr, hr, sd), lpips_loss_ref(sr, hr, sd, device=DEV, dtype=torch.float32)[:2]]
    gmax = float(rg.abs().max())
    spread_l = max(max(abs(float(l32) - float(rl)) / float(rl) for l32, _ in variants), 1e-7)
    spread_g = max(max(float(((g32.double() - rg).abs() * keep).max()) / gmax for _, g32 in variants), 1e-7)
    err_l = abs(float(loss) - float(rl)) / float(rl)
    err_g = float(((g.double() - rg).abs() * keep).max()) / gmax
    print("lpips %s: loss err %.2e (fp32 reference %.2e, ratio %.2f), grad err %.2e of max (fp32 reference %.2e, ratio %.2f), "
          "%d unclear pool windows, %.4f of the pixels kept"
          % (shape, err_l, spread_l, err_l / spread_l, err_g, spread_g, err_g / spread_g, nwin, kept))
    assert kept >= KEEP_MIN
    assert bool(torch.isfinite(g).all())
    assert err_l <= 2 * spread_l and err_g <= 2 * spread_g
    assert t.grad is None


@pytest.mark.parametrize("windowed", [False, True])
def test_plateau_ties_route_like_fp64(windowed):
    """exact plateaus make exact max-pool ties; the gradient must match fp64 wherever every pool window that reaches the
    pixel is an exact tie or has a clear top-2 gap.  The bound: fp32 accumulation error through five layers stays far
    below 1e-4 of the largest gradient, a tie routed to another pixel moves a whole contribution."""
    lp = _lp(2)
    shape = (4, 1, 128, 128)
    sr, hr = _pair(shape, 9, plateau=True)       # a seed for which the restatement keeps >= 0.92 of the pixels in both cases
    kw = dict(window=_window()) if windowed else {}
    _, g, _ = _run(lp, sr, hr, **kw)
    rl, rg, info = lpips_loss_ref(sr, hr, lp.state_dict(), device=DEV, **kw)
    ties = sum(int(((info["gap%d" % i] == 0) & (info["top%d" % i] > 0)).sum()) for i in (0, 1))
    unclear, nwin = unclear_pixels(info, shape[2], shape[3])
    keep = (~unclear).double()
    gmax = float(rg.abs().max())
    err = float(((g.double() - rg).abs() * keep).max()) / gmax
    print("plateau windowed=%s: %d exact-tie windows with a positive maximum, %d unclear, %.4f of the pixels kept, grad err "
          "%.2e of max" % (windowed, ties, nwin, float(keep.mean()), err))
    assert ties > 1000 and float(keep.mean()) >= KEEP_MIN
    assert err <= 1e-4


def test_pool_kernels_route_ties_to_the_first_maximum():
    """the gather backward against ATen's max_pool2d backward on heavily tied (integer) inputs: exact"""
    from hipops import ops
    L = ops._L()
    g = torch.Generator().manual_seed(7)
    for (N, C, H, W) in ((3, 64, 15, 15), (2, 192, 31, 30), (1, 64, 7, 3)):
        x = torch.randint(0, 3, (N, C, H, W), generator=g).float().to(DEV).contiguous(memory_format=torch.channels_last)
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        gy = torch.randn(N, C, Ho, Wo, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        y = torch.empty_like(gy)
        gx = torch.empty_like(x)
        L.vqw_lpips_pool_fwd(x, y, N, H, W, C)
        L.vqw_lpips_pool_bwd(x, gy, gx, N, H, W, C)
        xr = x.clone().requires_grad_(True)
        yr = torch.nn.functional.max_pool2d(xr, 3, 2)
        yr.backward(gy)
        m, idx, _ = maxpool3(x.double())
        want = unpool3(gy.double(), idx, H, W) * (x > 0)
        assert torch.equal(y, yr.detach()) and torch.equal(y.double(), m)
        # single visits are exact; a pixel that wins several windows sums them in the kernel's own fixed order
        assert float((gx.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
        assert float((gx - xr.grad * (x > 0)).abs().max()) <= 1e-6 * float(want.abs().max())
        assert bool(((gx != 0) == (want != 0)).all())


def test_zero_norm_pixels_give_a_finite_gradient():
    """A strongly negative first-layer bias and, over the left half of the recon, an input that the scaling layer maps to
    exactly 0: every first-tap pixel whose 11 x 11 patch lies in that half has all 64 features zero.

    The case is built to be well conditioned.  A feature that survives the bias as a small remainder of a large sum carries
    that sum's fp32 rounding (~1e-6 here), and the normalisation divides it by the pixel's norm r, so some pixel with
    r ~ 0.01 - which random inputs under such a bias always have - puts ~1e-4 of the largest gradient out of reach of any
    fp32 evaluation.  Here the first layer's weights are He-normal x 10 against a bias of -4: where the input is random,
    many channels clear the bias by a wide margin, and where it is the scaling layer's zero none does.  The restatement
    confirms it (smallest non-zero norm of any pixel > 1, asserted), so the 1e-5 bound tests the kernels."""
    from lpips_ref import SHIFT
    lp = _lp(3, bias0=-4.0, gain0=10.0)
    shape = (2, 3, 64, 64)
    sr, hr = _pair(shape, 4)
    sr[:, :, :, :32] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    loss, g, _ = _run(lp, sr, hr)
    rl, rg, info = lpips_loss_ref(sr, hr, lp.state_dict(), device=DEV, allow_zero_norm=True)
    unclear, nwin = unclear_pixels(info, shape[2], shape[3])
    err = float((g.double() - rg).abs().max()) / float(rg.abs().max())
    print("zero-norm: %d all-zero feature pixels, smallest non-zero norm %.3f, %d unclear pool windows, grad err %.2e of max"
          % (info["zero_norm"], info["rmin"], nwin, err))
    assert info["zero_norm"] > 50 and info["rmin"] > 1 and nwin == 0
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss))
    assert float(rg.abs().max()) > 0
    assert abs(float(loss) - float(rl)) <= 1e-5 * float(rl)
    assert err <= 1e-5


def test_multi_window_batch_matches_fp64_and_single_calls():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW, MEDIASTINAL_WINDOW
    lp = _lp(3)
    sd = lp.state_dict()
    dw = (2000, 0, 2.0)
    wins = (None, ops.window_map(dw, LUNG_WINDOW), ops.window_map(dw, MEDIASTINAL_WINDOW))
    sr, hr = _pair((2, 1, 64, 64), 4)
    x = sr.to(DEV).requires_grad_(True)
    losses = lp(x, hr.to(DEV), windows=wins)
    assert len(losses) == 3
    torch.autograd.backward(list(losses), [torch.tensor(c, device=DEV) for c in (1.0, 0.5, 2.0)])
    torch.cuda.synchronize()
    g_single = torch.zeros_like(x)
    for l, wv, c in zip(losses, wins, (1.0, 0.5, 2.0)):
        rl, rg, _ = lpips_loss_ref(sr, hr, sd, window=wv, device=DEV, allow_zero_norm=True)
        assert abs(float(l) - float(rl)) <= 1e-5 * float(rl)
        one, g, _ = _run(lp, sr, hr, window=wv)
        assert abs(float(one) - float(l)) <= 1e-6 * float(l)
        g_single += c * g
    assert_close(x.grad, g_single, 1e-5, "multi-window gradient vs three single-window calls")


def test_no_parameter_grads_and_new_weights_change_the_loss():
    lp = _lp(4)
    sr, hr = _pair((2, 1, 64, 64), 5)
    l0, _, t = _run(lp, sr, hr)
    assert t.grad is None
    assert all(p.grad is None for p in lp.parameters()) and not any(p.requires_grad for p in lp.parameters())
    lp.load_state_dict(he_weights(5), strict=False)
    l1, _, _ = _run(lp, sr, hr)
    rl, _, _ = lpips_loss_ref(sr, hr, lp.state_dict(), device=DEV)
    assert float(l1) != float(l0) and abs(float(l1) - float(rl)) <= 1e-5 * float(rl)


def test_bit_deterministic():
    lp = _lp(6)
    sr, hr = _pair((8, 1, 128, 128), 6)
    a = _run(lp, sr, hr)
    b = _run(lp, sr, hr)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_errors():
    from hipops import ops
    lp = _lp(0)
    with pytest.raises(ValueError):
        lp(torch.zeros(2, 2, 64, 64, device=DEV), torch.zeros(2, 2, 64, 64, device=DEV))
    p = lp.params()
    with pytest.raises(RuntimeError, match="not served"):
        ops.lpips_loss(torch.zeros(2, 2, 64, 64, device=DEV), torch.zeros(2, 2, 64, 64, device=DEV), p)
    with pytest.raises(RuntimeError, match="not served"):
        ops.lpips_loss(torch.zeros(2, 1, 30, 64, device=DEV), torch.zeros(2, 1, 30, 64, device=DEV), p)
    with pytest.raises(RuntimeError, match="not served"):
        ops.lpips_loss(torch.zeros(2, 1, 64, 30, device=DEV), torch.zeros(2, 1, 64, 30, device=DEV), p)
    with pytest.raises(RuntimeError, match="mismatch"):
        ops.lpips_loss(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 1, 64, 60, device=DEV), p)
    with pytest.raises(RuntimeError):
        ops.lpips_loss(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 1, 64, 64, device=DEV), p[:-1])
    with pytest.raises(RuntimeError):
        ops.lpips_loss(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 1, 64, 64, device=DEV), p, window=_window(),
                       windows=(None,))


def _first_step_trainer(percep=True, **kw):
    from trainers import FirstStepTrainer, FlipViews, LossWeights
    torch.manual_seed(0)
    w = LossWeights(commit=0.0, cross=0.0, dist=0.0, reg=0.0, recon=0.0, freq=0.0, perceptual=1.0)
    return FirstStepTrainer(views=FlipViews(border=2), device=DEV, loss_weight=w,
                            perceptual_loss=_lp(7) if percep else None, **kw)


def _batch(B=2, S=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, S, S, generator=g) * 2 - 1).to(DEV), (0.05 * torch.randn(B, 1, S, S, generator=g)).to(DEV)


@pytest.mark.parametrize("two_streams", [True, False])
def test_first_step_decoder_gradients_match_fp64_restatement(two_streams):
    from hipops import ops
    tr = _first_step_trainer(concurrent_views=two_streams)
    sd = tr.perceptual_loss.state_dict()
    state = {k: v.detach().clone() for k, v in tr.decoder.state_dict().items()}
    image, noise = _batch()
    out = tr.training_step({"image": image}, noise=noise)
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in tr.decoder.named_parameters()}
    clear = (image, torch.flip(image, dims=[3]))
    for v in (1, 2):
        rl = lpips_loss_ref(out["recon_%d" % v], clear[v - 1], sd, device=DEV, allow_zero_norm=True)[0]
        assert abs(float(out["perceptual_%d" % v]) - float(rl)) <= 1e-5 * float(rl)
    assert "perceptual" in tr.scalars(out)
    # replay: same decoder state, same embeddings, the restatement's gradient seeded into recon.backward - in fp64 (the
    # yardstick) and in fp32 (its spread: the max-pools route near-ties of the recon differently in any fp32 evaluation)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        tr.decoder.load_state_dict(state)
        for p in tr.decoder.parameters():
            p.grad = None
        ops.begin_step()
        recs = [tr.decoder(out["embed_%d" % v].detach()) for v in (1, 2)]
        seeds = [lpips_loss_ref(r, c, sd, device=DEV, dtype=dtype, allow_zero_norm=True)[1].float()
                 .contiguous(memory_format=torch.channels_last) for r, c in zip(recs, clear)]
        torch.autograd.backward(recs, seeds)
        ops.join_streams()
        torch.cuda.synchronize()
        ref[dtype] = {k: p.grad.detach().double().clone() for k, p in tr.decoder.named_parameters()}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    gmax = max(float(v.norm()) for v in r64.values())
    assert gmax > 0
    worst = 0.0
    for k in r64:
        if float(r64[k].norm()) < 1e-5 * gmax:
            continue
        scale = float(r64[k].abs().max())
        err = float((got[k].double() - r64[k]).abs().max())
        bound = max(2 * float((r32[k] - r64[k]).abs().max()), 1e-3 * scale)
        worst = max(worst, err / bound)
        assert err <= bound, "decoder grad %s: %.3e from fp64, bound %.3e (fp32 spread x 2, floor 1e-3 of max)" % (k, err, bound)
    print("first step (two streams %s): worst decoder-gradient error / bound %.2f" % (two_streams, worst))


def test_first_step_without_perceptual_loss_returns_what_it_did():
    tr = _first_step_trainer(percep=False)
    image, noise = _batch(seed=9)
    out = tr.training_step({"image": image}, noise=noise)
    torch.cuda.synchronize()
    assert set(out) == {"total", "commit_1", "commit_2", "cross", "dist", "reg", "recon_l1", "recon_l2", "ids_1", "ids_2",
                        "recon_1", "recon_2", "embed_1", "embed_2"}
    assert "perceptual" not in tr.scalars(out)


def test_multi_window_first_step_terms():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW, MEDIASTINAL_WINDOW
    dw = (2000, 0, 2.0)
    tr = _first_step_trainer(multi_window=dict(dataset_window=dw, recon_weights=(1.0, 1.0, 1.0)), percep_weights=(1.0, 0.5, 2.0))
    image, noise = _batch(seed=7)
    with torch.no_grad():
        recon = tr.decoder(tr.encoder(image)[0])
    terms = tr._percep_terms(recon, image)
    assert [c for _, c in terms] == [1.0 / 3, 0.5 / 3, 2.0 / 3]
    for (t, _), win in zip(terms, (None, LUNG_WINDOW, MEDIASTINAL_WINDOW)):
        ref = lpips_loss_ref(recon, image, tr.perceptual_loss.state_dict(), window=None if win is None else ops.window_map(dw, win),
                             device=DEV, allow_zero_norm=True)[0]
        assert abs(float(t) - float(ref)) <= 1e-5 * float(ref)
    out = tr.training_step({"image": image}, noise=noise)
    torch.cuda.synchronize()
    assert tr.scalars(out)["perceptual"] > 0


def test_second_step_adds_the_perceptual_term():
    from networks import UNetEncoder, UNetDecoder, NLayerDiscriminator
    from trainers import SecondStepTrainer, GanLossWeights
    torch.manual_seed(3)
    ef, df, K = [8, 8, 16, 16, 16], [8, 16, 16, 16, 32], 6
    enc = UNetEncoder(1, ef, K, 0.99, 'torch', False, 1, True)
    dec = UNetDecoder(ef[0], 1, df, use_dropblock=False, dropped_skip_layers=[], use_styled_up_block=True, use_pixel_shuffle=False)
    dis = NLayerDiscriminator(1, 1, n_filters=8, n_layers=3)
    image = _batch(S=64, seed=8)[0]
    lp = _lp(8)
    tr = SecondStepTrainer(enc, dec, dis, loss_weight=GanLossWeights(recon=1.0, gen=0.1, dis=0.8, perceptual=0.5), device=DEV,
                           perceptual_loss=lp)
    out = tr.training_step(image)
    torch.cuda.synchronize()
    ref = lpips_loss_ref(out["recon_image"], image, lp.state_dict(), device=DEV, allow_zero_norm=True)[0]
    assert abs(float(out["perceptual"]) - float(ref)) <= 1e-5 * float(ref)
    expect = float(out["recon"]) + 0.1 * float(out["gen"]) + 0.5 * float(out["perceptual"])
    assert abs(float(out["gen_total"]) - expect) <= 1e-5 * abs(float(out["gen_total"]))
