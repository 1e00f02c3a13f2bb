"""VGG perceptual loss on the MI355X: the HIP path (hipops.ops.perceptual_loss / functions.VGGLoss) against the fp64
restatement of the reference's VGGLoss in vgg_ref.py, and the loss inside both trainers."""
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close
from vgg_ref import he_weights, vgg_loss_ref, sequential_ref, _sd64

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _vgg(seed=0):
    from functions import VGGLoss
    return VGGLoss(weights=he_weights(seed)).to(DEV)


def _pair(shape, seed, plateau=False):
    g = torch.Generator().manual_seed(seed)
    sr = torch.rand(shape, generator=g) * 2 - 1
    hr = torch.rand(shape, generator=g) * 2 - 1
    if plateau:                    # a tanh-saturated recon: exact -1 over the left half and a band
        sr[..., :, : shape[-1] // 2] = -1.0
        sr[..., shape[-2] // 3: shape[-2] // 2, :] = -1.0
    return sr, hr


def _ref32(sr, hr, sd):
    """the reference's own form in fp32 (F.conv2d module stack on the GPU): its spread around fp64 sets the tolerance"""
    seq = sequential_ref(_sd64(sd, "cpu")).float().to(DEV)
    x = sr.to(DEV).float().requires_grad_(True)
    B, _, H, W = x.shape
    with torch.no_grad():
        yh = seq(hr.to(DEV).float().expand(B, 3, H, W))
    loss = F.mse_loss(seq(x.expand(B, 3, H, W)), yh)
    loss.backward()
    return loss.detach().double(), x.grad.double()


def _window():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW
    return ops.window_map((2000, 0, 2.0), LUNG_WINDOW)


def _run(vgg, sr, hr, **kw):
    x = sr.to(DEV).contiguous().requires_grad_(True)
    t = hr.to(DEV).contiguous().requires_grad_(True)
    loss = vgg(x, t, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, t


@pytest.mark.parametrize("shape", [(2, 1, 32, 32), (4, 1, 64, 48), (1, 1, 33, 47), (2, 3, 32, 32), (32, 1, 256, 256),
                                   (2, 1, 512, 512)])
def test_loss_and_gradient_match_fp64(shape):
    vgg = _vgg(1)
    sd = vgg.state_dict()
    sr, hr = _pair(shape, 2)
    loss, g, t = _run(vgg, sr, hr)
    rl, rg, _ = vgg_loss_ref(sr, hr, sd, device=DEV)
    # the reference's fp32 spread around fp64, from two fp32 renderings of it: the F.conv2d module stack and the
    # restatement's own operations in fp32
    variants = [_ref32(sr, hr, sd), vgg_loss_ref(sr, hr, sd, device=DEV, dtype=torch.float32)[:2]]
    gmax = float(rg.abs().max())
    spread_l = max(max(abs(float(l32) - float(rl)) / float(rl) for l32, _ in variants), 1e-7)
    spread_g = max(max(float((g32.double() - rg).abs().max()) / gmax for _, g32 in variants), 1e-7)
    err_l = abs(float(loss) - float(rl)) / float(rl)
    err_g = float((g.double() - rg).abs().max()) / gmax
    print("perceptual %s: loss err %.2e (fp32 reference %.2e, ratio %.2f), grad err %.2e of max (fp32 reference %.2e, ratio %.2f)"
          % (shape, err_l, spread_l, err_l / spread_l, err_g, spread_g, err_g / spread_g))
    assert err_l <= 2 * spread_l and err_g <= 2 * spread_g
    assert t.grad is None


@pytest.mark.parametrize("windowed", [False, True])
def test_plateau_ties_route_like_fp64(windowed):
    """exact plateaus make exact max-pool ties; the gradient must match fp64 wherever every pool window that reaches the
    pixel is an exact tie or has a clear top-2 gap"""
    vgg = _vgg(2)
    sr, hr = _pair((4, 1, 64, 64), 3, plateau=True)
    kw = dict(window=_window()) if windowed else {}
    _, g, _ = _run(vgg, sr, hr, **kw)
    rl, rg, gap = vgg_loss_ref(sr, hr, vgg.state_dict(), device=DEV, **kw)
    ties = int((gap == 0).sum())
    unclear = ((gap > 0) & (gap <= 1e-4 * (1 + gap.abs()))).any(dim=1, keepdim=True).double()
    near = F.max_pool2d(F.interpolate(unclear, scale_factor=2), 5, 1, 2) > 0      # input pixels those windows reach
    keep = ~near
    gmax = float(rg.abs().max())
    err = float(((g.double() - rg).abs() * keep).max()) / gmax
    print("plateau windowed=%s: %d exact-tie windows, %.4f of the pixels kept, grad err %.2e of max" % (
        windowed, ties, float(keep.double().mean()), err))
    assert ties > 1000 and float(keep.double().mean()) > 0.5
    assert err <= 1e-4


def test_multi_window_batch_matches_fp64_and_single_calls():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW, MEDIASTINAL_WINDOW
    vgg = _vgg(3)
    sd = vgg.state_dict()
    dw = (2000, 0, 2.0)
    wins = (None, ops.window_map(dw, LUNG_WINDOW), ops.window_map(dw, MEDIASTINAL_WINDOW))
    sr, hr = _pair((2, 1, 64, 64), 4)
    x = sr.to(DEV).requires_grad_(True)
    losses = vgg(x, hr.to(DEV), windows=wins)
    assert len(losses) == 3
    torch.autograd.backward(list(losses), [torch.tensor(c, device=DEV) for c in (1.0, 0.5, 2.0)])
    torch.cuda.synchronize()
    g_single = torch.zeros_like(x)
    for l, wv, c in zip(losses, wins, (1.0, 0.5, 2.0)):
        rl, rg, _ = vgg_loss_ref(sr, hr, sd, window=wv, device=DEV)
        assert abs(float(l) - float(rl)) <= 1e-5 * float(rl)
        one, g, _ = _run(vgg, sr, hr, window=wv)
        assert abs(float(one) - float(l)) <= 1e-6 * float(l)
        g_single += c * g
    assert_close(x.grad, g_single, 1e-5, "multi-window gradient vs three single-window calls")


def test_no_parameter_grads_and_new_weights_change_the_loss():
    vgg = _vgg(4)
    sr, hr = _pair((2, 1, 32, 32), 5)
    l0, _, _ = _run(vgg, sr, hr)
    assert all(p.grad is None for p in vgg.parameters())
    vgg.load_state_dict({k.replace("features.", "vgg."): v for k, v in he_weights(5).items()})
    l1, _, _ = _run(vgg, sr, hr)
    rl, _, _ = vgg_loss_ref(sr, hr, vgg.state_dict(), device=DEV)
    assert float(l1) != float(l0) and abs(float(l1) - float(rl)) <= 1e-5 * float(rl)


def test_bit_deterministic():
    vgg = _vgg(6)
    sr, hr = _pair((8, 1, 128, 128), 6)
    a = _run(vgg, sr, hr)
    b = _run(vgg, sr, hr)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_errors():
    vgg = _vgg(0)
    with pytest.raises(ValueError):
        vgg(torch.zeros(2, 2, 8, 8, device=DEV), torch.zeros(2, 2, 8, 8, device=DEV))
    from hipops import ops
    w = [p for p in vgg.parameters()]
    with pytest.raises(RuntimeError):
        ops.perceptual_loss(torch.zeros(2, 1, 8, 8, device=DEV), torch.zeros(2, 1, 8, 6, device=DEV), *w)


def _first_step_trainer(percep=True, **kw):
    from trainers import FirstStepTrainer, FlipViews, LossWeights
    torch.manual_seed(0)
    w = LossWeights(commit=0.0, cross=0.0, dist=0.0, reg=0.0, recon=0.0, freq=0.0, perceptual=1.0)
    return FirstStepTrainer(views=FlipViews(border=2), device=DEV, loss_weight=w,
                            perceptual_loss=_vgg(7) if percep else None, **kw)


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
        rl = vgg_loss_ref(out["recon_%d" % v], clear[v - 1], sd, device=DEV)[0]
        assert abs(float(out["perceptual_%d" % v]) - float(rl)) <= 1e-5 * float(rl)
    assert "perceptual" in tr.scalars(out)
    # replay: same decoder state, same embeddings, the restatement's gradient seeded into recon.backward - in fp64 (the
    # yardstick) and in fp32 (its spread: the max-pool routes near-ties of the recon differently in any fp32 evaluation)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        tr.decoder.load_state_dict(state)
        for p in tr.decoder.parameters():
            p.grad = None
        ops.begin_step()
        recs = [tr.decoder(out["embed_%d" % v].detach()) for v in (1, 2)]
        seeds = [vgg_loss_ref(r, c, sd, device=DEV, dtype=dtype)[1].float().contiguous(memory_format=torch.channels_last)
                 for r, c in zip(recs, clear)]
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
        ref = vgg_loss_ref(recon, image, tr.perceptual_loss.state_dict(), window=None if win is None else ops.window_map(dw, win),
                           device=DEV)[0]
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
    vgg = _vgg(8)
    tr = SecondStepTrainer(enc, dec, dis, loss_weight=GanLossWeights(recon=1.0, gen=0.1, dis=0.8, perceptual=0.5), device=DEV,
                           perceptual_loss=vgg)
    out = tr.training_step(image)
    torch.cuda.synchronize()
    ref = vgg_loss_ref(out["recon_image"], image, vgg.state_dict(), device=DEV)[0]
    assert abs(float(out["perceptual"]) - float(ref)) <= 1e-5 * float(ref)
    expect = float(out["recon"]) + 0.1 * float(out["gen"]) + 0.5 * float(out["perceptual"])
    assert abs(float(out["gen_total"]) - expect) <= 1e-5 * abs(float(out["gen_total"]))
