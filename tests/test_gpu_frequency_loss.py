"""Focal frequency loss on the MI355X: the HIP kernels (hipops.ops.frequency_loss / functions.FocalFrequencyLoss) against
the fp64 restatement of focal-frequency-loss 0.3.0 in test_frequency_loss_host.py, and the loss inside both trainers."""
import pytest
import torch

from helpers import assert_close
from test_frequency_loss_host import ffl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_RTOL = 1e-6
GRAD_TOL = 2e-6          # x max |g_64|


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g) * 2 - 1
    t = torch.rand(shape, generator=g) * 2 - 1
    return p, t


def _check(shape, seed=0, **kw):
    from hipops import ops
    p, t = _pair(shape, seed)
    pd = p.to(DEV).requires_grad_(True)
    td = t.to(DEV).requires_grad_(True)
    loss = ops.frequency_loss(pd, td, **kw)
    loss.backward()
    torch.cuda.synchronize()
    rl, rgp, rgt = ffl_ref(p, t, **kw)
    rel = abs(float(loss) - float(rl)) / abs(float(rl))
    gerr = float((pd.grad.double().cpu() - rgp).abs().max()) / float(rgp.abs().max())
    print("frequency_loss %s %s: loss rel err %.2e, grad max err / max |g| %.2e" % (shape, kw, rel, gerr))
    assert rel <= LOSS_RTOL, "%s %s: loss rel err %.3e" % (shape, kw, rel)
    gmax = float(rgp.abs().max())
    err = float((pd.grad.double().cpu() - rgp).abs().max())
    assert err <= GRAD_TOL * gmax, "%s %s: grad max err %.3e of max |g| %.3e" % (shape, kw, err, gmax)
    errt = float((td.grad.double().cpu() - rgt).abs().max())
    assert errt <= GRAD_TOL * float(rgt.abs().max()), "%s %s: target grad" % (shape, kw)
    if kw.get("window") is None:
        assert torch.equal(td.grad, -pd.grad)
    return rel, err / gmax


@pytest.mark.parametrize("shape,pf", [((4, 1, 32, 32), 1), ((4, 1, 80, 80), 1), ((64, 1, 256, 256), 1),
                                      ((4, 1, 512, 512), 1), ((3, 1, 48, 80), 1), ((2, 1, 30, 45), 3),
                                      ((2, 3, 64, 48), 1), ((2, 3, 64, 48), 2)])
def test_shapes_match_fp64(shape, pf):
    _check(shape, patch_factor=pf)


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(alpha=0.5), dict(alpha=1.0), dict(alpha=2.0),
                                dict(patch_factor=2), dict(patch_factor=4), dict(log_matrix=True),
                                dict(batch_matrix=True), dict(batch_matrix=True, patch_factor=2, alpha=2.0),
                                dict(loss_weight=2.5), "lung"])
def test_options_match_fp64(kw):
    if kw == "lung":
        from hipops import ops
        from trainers.first_step import LUNG_WINDOW
        kw = dict(window=ops.window_map((2000, 0, 2.0), LUNG_WINDOW))
    _check((4, 1, 64, 64), seed=1, **kw)


def test_alpha0_is_mse():
    from hipops import ops
    p, t = _pair((8, 1, 96, 96), 2)
    a = p.to(DEV).requires_grad_(True)
    b = p.to(DEV).requires_grad_(True)
    lf = ops.frequency_loss(a, t.to(DEV), alpha=0.0)
    lm = ops.mse_loss(b, t.to(DEV))
    lf.backward()
    lm.backward()
    torch.cuda.synchronize()
    assert abs(float(lf) - float(lm)) <= 1e-6 * float(lm)
    assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())


def test_equal_images_give_exact_zero():
    from hipops import ops
    p, _ = _pair((4, 1, 64, 64), 3)
    for kw in (dict(), dict(alpha=2.0, log_matrix=True), dict(batch_matrix=True, patch_factor=2)):
        x = p.to(DEV).requires_grad_(True)
        loss = ops.frequency_loss(x, p.to(DEV), **kw)
        loss.backward()
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0 and not torch.isnan(x.grad).any(), kw


def test_bit_deterministic():
    from functions import FocalFrequencyLoss
    p, t = _pair((16, 1, 128, 128), 4)
    ffl = FocalFrequencyLoss()
    res = []
    for _ in range(2):
        x = p.to(DEV).requires_grad_(True)
        loss = ffl(x, t.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_argument_errors():
    from hipops import ops
    x = torch.zeros(2, 1, 30, 30, device=DEV)
    with pytest.raises(RuntimeError):
        ops.frequency_loss(x, torch.zeros(2, 1, 30, 32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.frequency_loss(x, x, patch_factor=4)
    with pytest.raises(RuntimeError):
        ops.frequency_loss(x, x, alpha=-1.0)


def _first_step_trainer(freq=True, **kw):
    from functions import FocalFrequencyLoss
    from trainers import FirstStepTrainer, FlipViews, LossWeights
    torch.manual_seed(0)
    w = LossWeights(commit=0.0, cross=0.0, dist=0.0, reg=0.0, recon=0.0, freq=1.0, perceptual=0.0)
    return FirstStepTrainer(views=FlipViews(border=2), device=DEV, loss_weight=w,
                            frequency_loss=FocalFrequencyLoss() if freq else None, **kw)


def _batch(B=2, S=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, S, S, generator=g) * 2 - 1).to(DEV), (0.05 * torch.randn(B, 1, S, S, generator=g)).to(DEV)


def test_first_step_decoder_gradients_match_fp64_restatement():
    """Every loss weight 0 but freq: the decoder's parameter gradients of one step equal the ones of back-propagating the
    restatement's dL/drecon of both views through the same decoder state."""
    from hipops import ops
    tr = _first_step_trainer()
    state = {k: v.detach().clone() for k, v in tr.decoder.state_dict().items()}
    image, noise = _batch()
    out = tr.training_step({"image": image}, noise=noise)
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in tr.decoder.named_parameters()}
    sc = tr.scalars(out)
    clear = (image, torch.flip(image, dims=[3]))                     # FlipViews: the clear views
    l1, _, _ = ffl_ref(out["recon_1"], clear[0])
    l2, _, _ = ffl_ref(out["recon_2"], clear[1])
    assert abs(sc["freq"] - float(l1 + l2)) <= 1e-5 * float(l1 + l2)
    # replay: same decoder state, same embeddings, the restatement's gradient seeded into recon.backward
    tr.decoder.load_state_dict(state)
    for p in tr.decoder.parameters():
        p.grad = None
    ops.begin_step()
    recs = [tr.decoder(out["embed_%d" % v].detach()) for v in (1, 2)]
    seeds = [ffl_ref(r, c)[1].float().to(DEV).contiguous(memory_format=torch.channels_last) for r, c in zip(recs, clear)]
    for r, v in zip(recs, (1, 2)):
        assert_close(r, out["recon_%d" % v], 1e-6, "replayed recon_%d" % v)
    torch.autograd.backward(recs, seeds)
    ops.join_streams()
    torch.cuda.synchronize()
    ref = {k: p.grad.detach().clone() for k, p in tr.decoder.named_parameters()}
    gmax = max(float(v.norm()) for v in ref.values())
    assert gmax > 0
    for k in ref:
        if float(ref[k].norm()) < 1e-5 * gmax:       # analytically zero (biases in front of a norm): rounding noise only
            continue
        assert_close(got[k], ref[k], 1e-3, "decoder grad " + k)


def test_first_step_without_frequency_loss_returns_what_it_did():
    """frequency_loss=None: the step's result dict has no frequency entries (same outputs as before the loss was built);
    scalars() reports freq = 0.0."""
    tr = _first_step_trainer(freq=False)
    image, noise = _batch(seed=9)
    out = tr.training_step({"image": image}, noise=noise)
    torch.cuda.synchronize()
    assert set(out) == {"total", "commit_1", "commit_2", "cross", "dist", "reg", "recon_l1", "recon_l2", "ids_1", "ids_2",
                        "recon_1", "recon_2", "embed_1", "embed_2"}
    assert tr.scalars(out)["freq"] == 0.0


def test_first_step_with_frequency_loss_is_bit_deterministic():
    res = []
    for _ in range(2):
        tr = _first_step_trainer()
        tr.w = tr.w._replace(commit=1.0, cross=1.0, dist=1.0, reg=1.0, recon=1.0)
        image, noise = _batch(seed=6)
        out = tr.training_step({"image": image}, noise=noise)
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in list(tr.encoder.named_parameters()) + list(tr.decoder.named_parameters())
                 if p.grad is not None}
        res.append((tr.scalars(out), grads))
    (s0, g0), (s1, g1) = res
    assert s0 == s1 and s0["freq"] > 0
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_multi_window_first_step_reports_the_three_window_terms():
    from hipops import ops
    from trainers.first_step import LUNG_WINDOW, MEDIASTINAL_WINDOW
    dw = (2000, 0, 2.0)
    tr = _first_step_trainer(multi_window=dict(dataset_window=dw, recon_weights=(1.0, 1.0, 1.0)), freq_weights=(1.0, 0.5, 2.0))
    image, noise = _batch(seed=7)
    with torch.no_grad():
        recon = tr.decoder(tr.encoder(image)[0])
    terms = tr._freq_terms(recon, image)
    assert [c for _, c in terms] == [1.0 / 3, 0.5 / 3, 2.0 / 3]
    for (t, _), win in zip(terms, (None, LUNG_WINDOW, MEDIASTINAL_WINDOW)):
        ref = ffl_ref(recon, image, window=None if win is None else ops.window_map(dw, win))[0]
        assert abs(float(t) - float(ref)) <= 1e-6 * float(ref)


def test_second_step_reports_frequency_loss():
    from functions import FocalFrequencyLoss
    from networks import UNetEncoder, UNetDecoder, NLayerDiscriminator
    from trainers import SecondStepTrainer, GanLossWeights
    torch.manual_seed(3)
    ef, df, K = [8, 8, 16, 16, 16], [8, 16, 16, 16, 32], 6
    enc = UNetEncoder(1, ef, K, 0.99, 'torch', False, 1, True)
    dec = UNetDecoder(ef[0], 1, df, use_dropblock=False, dropped_skip_layers=[], use_styled_up_block=True, use_pixel_shuffle=False)
    dis = NLayerDiscriminator(1, 1, n_filters=8, n_layers=3)
    image = _batch(S=64, seed=8)[0]
    tr = SecondStepTrainer(enc, dec, dis, loss_weight=GanLossWeights(recon=1.0, gen=0.1, dis=0.8, freq=1.0), device=DEV,
                           frequency_loss=FocalFrequencyLoss())
    out = tr.training_step(image)
    torch.cuda.synchronize()
    ref = ffl_ref(out["recon_image"], image)[0]
    assert abs(float(out["freq"]) - float(ref)) <= 1e-6 * float(ref)
    assert abs(float(out["gen_total"]) - (float(out["recon"]) + 0.1 * float(out["gen"]) + float(out["freq"]))) <= 1e-5 * abs(float(out["gen_total"]))
