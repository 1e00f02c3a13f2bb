"""CPU-side checks of the GPT code prior's training (no GPU): the C ABI additions and their refusals, hipops.AdamW's constructor and
state_dict contract, minGPT's parameter groups, the learning-rate schedule, the config checks and the launcher's refusals of -p,
the committed config, the float64 restatement of the three-step recipe (tests/prior_ref.py) against the reference's fixtures
(tests/golden/prior_step_*.npz, made by tests/golden/make_golden_prior_step.py), the raster-order bookkeeping of
VQGAN.encode_to_ids / decode_from_ids on a CPU stand-in, and PriorTrainer's construction."""
import argparse
import copy
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import checksum, sample_idx
from run_helpers import ROOT, write_config
import gpt_ref as G
import prior_ref as P

NEW_SYMBOLS = ("vqw_grad_norm_ws_bytes", "vqw_grad_norm_multi", "vqw_adamw_multi", "vqw_adamw_step", "vqw_prior_tokens")
CASES = sorted(P.CASES)


def _gpt(name="p64", **kw):
    from networks import GPT
    args = P.gpt_kwargs(name)
    args.update(kw)
    return GPT(**args)


def _tiny_vqgan(**kw):
    from networks import VQGAN
    args = dict(P.TINY_VQGAN)
    args.update(kw)
    return VQGAN(**args)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
    ops = library.register()
    for s in NEW_SYMBOLS:
        assert (s in ops) == (not s.endswith("_ws_bytes")), s
    sch = str(torch.ops.vqw.grad_norm_multi.default._schema)
    assert "Tensor? chunks_dev" in sch and "float max_norm" in sch and "Tensor(a!)? ws" in sch and "Tensor(b!)? norm_out" in sch
    sch = str(torch.ops.vqw.adamw_multi.default._schema)          # the table is read; p, m, v are reached through it
    assert "Tensor? chunks_dev" in sch and "Tensor? clip" in sch and "!" not in sch and "float weight_decay" in sch
    sch = str(torch.ops.vqw.adamw_step.default._schema)
    assert "Tensor(a!)? p" in sch and "Tensor? g" in sch and "Tensor(b!)? m" in sch and "Tensor(c!)? v" in sch and "Tensor? clip" in sch
    sch = str(torch.ops.vqw.prior_tokens.default._schema)
    assert "Tensor? ids" in sch and "Tensor? u_keep" in sch and "Tensor? u_rand" in sch and "Tensor(a!)? inp" in sch
    assert "int sos" in sch and "float pkeep" in sch
    # the argument order follows vqw_adam_multi / vqw_adam_step, with `clip` in front of the stream
    names = lambda f: [n for _, n, _ in _lib.parse_header()[f][1]]  # noqa: E731
    assert names("vqw_adamw_multi") == names("vqw_adam_multi")[:-1] + ["clip", "stream"]
    assert names("vqw_adamw_step") == names("vqw_adam_step")[:-1] + ["clip", "stream"]
    L = _lib.load()
    assert L.vqw_grad_norm_ws_bytes(1) == 8 and L.vqw_grad_norm_ws_bytes(1025) == 8200 and L.vqw_grad_norm_ws_bytes(0) == 0
    assert L.vqw_grad_norm_ws_bytes(-3) == 0


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """Every refusal is a non-zero status with a message; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    P_ = 4096          # an aligned non-null stand-in for every pointer
    err = L.vqw_last_error

    def gn(chunks=P_, n=3, max_norm=1.0, ws=P_, wsb=24, out=P_):
        return L.vqw_grad_norm_multi(chunks, n, max_norm, ws, wsb, out, None)

    for name in ("chunks", "ws", "out"):
        assert gn(**{name: None}) != 0 and b"null pointer" in err(), name
    assert gn(n=0) != 0 and b"n_chunks=0" in err()
    assert gn(wsb=16) != 0 and b"workspace of 16 bytes, 24 needed" in err()
    assert gn(ws=P_ + 4) != 0 and b"8-byte aligned" in err()
    assert gn(max_norm=float("nan")) != 0 and b"max_norm" in err()

    def multi(chunks=P_, n=3, lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, bc1=0.1, bc2=0.05, clip=None):
        return L.vqw_adamw_multi(chunks, n, lr, b1, b2, eps, wd, bc1, bc2, clip, None)

    def single(p=P_, g=P_, m=P_, v=P_, n=3, lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, bc1=0.1, bc2=0.05, clip=None):
        return L.vqw_adamw_step(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2, clip, None)

    assert multi(chunks=None) != 0 and b"vqw_adamw_multi: bad arguments" in err()
    assert multi(n=0) != 0 and b"bad arguments" in err()
    for name in "pgmv":
        assert single(**{name: None}) != 0 and b"vqw_adamw_step: bad arguments" in err(), name
    assert single(n=0) != 0 and b"bad arguments" in err()
    for call in (multi, single):
        assert call(bc1=0.0) != 0 and b"bias corrections must be positive" in err()
        assert call(bc2=-1.0) != 0 and b"bias corrections must be positive" in err()
        assert call(lr=-1.0) != 0 and b"must not be negative" in err()
        assert call(wd=-0.1) != 0 and b"must not be negative" in err()
        assert call(b1=1.0) != 0 and b"betas" in err()
        assert call(b2=-0.5) != 0 and b"betas" in err()

    def tok(ids=P_, uk=P_, ur=P_, inp=P_, B=2, T=16, V=64, sos=0, pkeep=0.5):
        return L.vqw_prior_tokens(ids, uk, ur, inp, B, T, V, sos, pkeep, None)

    assert tok(ids=None) != 0 and b"null pointer" in err()
    assert tok(inp=None) != 0 and b"null pointer" in err()
    assert tok(uk=None) != 0 and b"needs u_keep and u_rand" in err()
    assert tok(ur=None, pkeep=0.0) != 0 and b"needs u_keep and u_rand" in err()
    assert tok(B=0) != 0 and b"B=0" in err()
    assert tok(T=0) != 0 and b"T=0" in err()
    assert tok(V=0) != 0 and b"V=0" in err()
    assert tok(pkeep=float("nan")) != 0 and b"pkeep" in err()


def test_prior_tokens_has_no_cpu_fallback_and_traces():
    from hipops import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    ids = torch.zeros(2, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prior_tokens(ids, 0, 1.0, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prior_tokens(ids, 0, 0.5, 64, torch.rand(2, 16), torch.rand(2, 16))
    with FakeTensorMode():
        ids = torch.empty(2, 16, dtype=torch.long, device="cuda")
        u = torch.empty(2, 16, device="cuda")
        out = ops.prior_tokens(ids, 0, 0.5, 64, u, u)
        assert out.shape == (2, 16) and out.dtype == torch.long
        with pytest.raises(RuntimeError, match="needs u_keep and u_rand"):
            ops.prior_tokens(ids, 0, 0.5, 64)
        with pytest.raises(RuntimeError, match="torch.long"):
            ops.prior_tokens(ids.int(), 0, 1.0, 64)


# ------------------------------------------------------------------------------------------------ hipops.AdamW
def test_adamw_constructor_validation():
    from hipops import AdamW, Adam
    from hipops.optim import _FusedOptimizer
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.01),
                dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError, match="AdamW"):
            AdamW(p, **bad)
    o = AdamW(p)
    assert o.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)          # torch.optim.AdamW's
    assert o.max_grad_norm is None and o.last_grad_norm is None
    assert AdamW(p, max_grad_norm=0.0).max_grad_norm is None and AdamW(p, max_grad_norm=2).max_grad_norm == 2.0
    # one copy of the pointer-table ring and the layout rules
    assert issubclass(AdamW, _FusedOptimizer) and issubclass(Adam, _FusedOptimizer)
    assert "_upload_table" not in vars(AdamW) and "_upload_table" not in vars(Adam) and "load_state_dict" not in vars(AdamW)
    p[0].grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        o.step()


def test_adamw_state_dict_round_trip_with_stock_adamw():
    from hipops import AdamW
    torch.manual_seed(0)
    ref = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    groups = lambda ps: [{"params": [ps[0]], "weight_decay": 0.01}, {"params": [ps[1]], "weight_decay": 0.0}]  # noqa: E731
    kw = dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8)
    stock = torch.optim.AdamW(groups(ref), **kw)
    for _ in range(2):
        for q in ref:
            q.grad = torch.randn(q.shape)
        stock.step()
    mine_p = [torch.nn.Parameter(q.detach().clone()) for q in ref]
    mine = AdamW(groups(mine_p), max_grad_norm=1.0, **kw)
    mine.load_state_dict(copy.deepcopy(stock.state_dict()))          # (a loaded state shares its tensors with its source)
    for q, r in zip(mine_p, ref):
        st = mine.state[q]
        assert st["step"] == 2 and isinstance(st["step"], int)
        assert torch.equal(st["exp_avg"], stock.state[r]["exp_avg"]) and torch.equal(st["exp_avg_sq"], stock.state[r]["exp_avg_sq"])
    assert [g["weight_decay"] for g in mine.param_groups] == [0.01, 0.0] and mine.param_groups[0]["betas"] == (0.9, 0.95)
    sd = copy.deepcopy(mine.state_dict())
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # and back: a stock AdamW continues from this optimiser's state exactly as from its own
    back_p = [torch.nn.Parameter(q.detach().clone()) for q in ref]
    back = torch.optim.AdamW(groups(back_p), **kw)
    back.load_state_dict(sd)
    g = [torch.randn(q.shape) for q in ref]
    for q, r, gr in zip(back_p, ref, g):
        q.grad, r.grad = gr.clone(), gr.clone()
    back.step()
    stock.step()
    for q, r in zip(back_p, ref):
        assert torch.equal(q, r)


def test_parameter_groups_follow_mingpts_rule_by_name():
    from trainers import parameter_groups
    gpt = _gpt("p96")
    groups, (decay, no_decay) = parameter_groups(gpt, 0.01)
    names = [k for k, _ in gpt.named_parameters()]
    assert sorted(decay + no_decay) == sorted(names) and not set(decay) & set(no_decay)
    assert sorted(decay) == sorted(k for k in names if P.decays(k))
    assert "tok_embed.weight" in no_decay and "pos_embed" in no_decay and "ln_f.weight" in no_decay and "head.weight" in decay
    assert "blocks.0.ln1.weight" in no_decay and "blocks.1.mlp.2.weight" in decay and "blocks.1.mlp.2.bias" in no_decay
    params = dict(gpt.named_parameters())
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    assert [id(p) for p in groups[0]["params"]] == [id(params[k]) for k in decay]
    assert [id(p) for p in groups[1]["params"]] == [id(params[k]) for k in no_decay]
    gpt.stray = torch.nn.Parameter(torch.zeros(2))
    with pytest.raises(ValueError, match="stray falls in neither"):
        parameter_groups(gpt, 0.01)
    del gpt.stray
    gpt.conv = torch.nn.Conv1d(2, 2, 1)
    with pytest.raises(ValueError, match="conv.weight falls in neither"):
        parameter_groups(gpt, 0.01)


def test_learning_rate_schedule_at_known_steps():
    from trainers import learning_rate
    lr = 4.5e-4
    assert learning_rate(0, lr) == lr and learning_rate(10 ** 6, lr) == lr                    # no warm-up, no decay
    assert learning_rate(0, lr, 10) == pytest.approx(lr / 10) and learning_rate(4, lr, 10) == pytest.approx(lr / 2)
    assert learning_rate(9, lr, 10) == pytest.approx(lr) and learning_rate(10, lr, 10) == lr and learning_rate(999, lr, 10) == lr
    assert learning_rate(10, lr, 10, 110) == pytest.approx(lr)                                  # the cosine starts at lr
    assert learning_rate(60, lr, 10, 110) == pytest.approx(0.55 * lr)                           # half way: (1 + 0.1) / 2
    assert learning_rate(110, lr, 10, 110) == pytest.approx(0.1 * lr) and learning_rate(5000, lr, 10, 110) == pytest.approx(0.1 * lr)
    assert learning_rate(35, lr, 10, 110) == pytest.approx(lr * (0.1 + 0.9 * 0.5 * (1 + np.cos(np.pi * 0.25))))
    for step in (0, 3, 10, 11, 50, 109, 110, 200):
        for w, d in ((0, 0), (10, 0), (10, 110), (0, 100)):
            assert learning_rate(step, lr, w, d) == pytest.approx(P.learning_rate_ref(step, lr, w, d), rel=1e-12)
    rates = [learning_rate(s, lr, 10, 110) for s in range(200)]
    assert all(a <= b for a, b in zip(rates[:10], rates[1:10])) and all(a >= b for a, b in zip(rates[10:], rates[11:]))


# ------------------------------------------------------------------------------------------------ config and launcher
def _launcher():
    import importlib
    return importlib.import_module("run_vqwnet")


def _args(**kw):
    a = dict(config="x.json", mode="train", multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)
    a.update(kw)
    return argparse.Namespace(**a)


def test_check_prior_config_names_missing_keys(tmp_path):
    from utils import load_json
    from trainers import check_prior_config
    raw = P.prior_run_config(tmp_path / "out")
    check_prior_config(load_json(write_config(tmp_path / "ok.json", raw)))
    for section, key in (("prior", "pkeep"), ("prior", "n_layer"), ("prior", "sos_token")):
        bad = json.loads(json.dumps(raw))
        del bad["model"][section][key]
        with pytest.raises(NotImplementedError, match=r"model\.prior.*missing: %s" % key):
            check_prior_config(load_json(write_config(tmp_path / "bad.json", bad)))
    for key in ("grad_norm_clip", "warmup_steps", "b2"):
        bad = json.loads(json.dumps(raw))
        del bad["prior_optim"][key]
        with pytest.raises(NotImplementedError, match=r"prior_optim.*missing: %s" % key):
            check_prior_config(load_json(write_config(tmp_path / "bad.json", bad)))
    bad = json.loads(json.dumps(raw))
    del bad["prior_optim"]
    with pytest.raises(NotImplementedError, match="prior_optim.*missing: lr, b1, b2"):
        check_prior_config(load_json(write_config(tmp_path / "bad.json", bad)))
    bad = json.loads(json.dumps(raw))
    del bad["model"]["vqgan"]["emb_dim"]
    with pytest.raises(NotImplementedError, match="missing: emb_dim"):
        check_prior_config(load_json(write_config(tmp_path / "bad.json", bad)))


def test_launcher_refuses_what_the_prior_trainer_cannot_do(tmp_path):
    from utils import load_json
    rv = _launcher()
    a = rv.build_parser().parse_args(["-c", "x.json", "-p"])
    assert a.prior and not a.vqgan and rv.build_parser().parse_args(["-c", "x.json", "--prior"]).prior
    assert not rv.build_parser().parse_args(["-c", "x.json"]).prior
    cfg = lambda **run: load_json(write_config(tmp_path / "c.json", P.prior_run_config(tmp_path / "out", **run)))  # noqa: E731
    assert rv.check_arguments(cfg(), _args()) == ("second_step", 1)
    with pytest.raises(ValueError, match="-p with -v"):
        rv.check_arguments(cfg(), _args(vqgan=True))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step"):
        rv.check_arguments(cfg(), _args(mode="test"))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step and no inference export"):
        rv.check_arguments(cfg(training_mode="inference"), _args(mode="test"))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step and no inference export"):
        rv.check_arguments(cfg(training_mode="inference"), _args())
    with pytest.raises(ValueError, match="data-parallel training of the prior is not built"):
        rv.check_arguments(cfg(num_gpus=2), _args())
    raw = P.prior_run_config(tmp_path / "out")
    del raw["model"]["prior"]
    with pytest.raises(NotImplementedError, match="model.prior"):
        rv.check_arguments(load_json(write_config(tmp_path / "c.json", raw)), _args())
    assert "-p" in rv.__doc__ and "[-v | -p]" in rv.__doc__
    # the workers of a multi-process launch would be handed the flag
    assert "-p" in open(rv.__file__).read().split("def launch")[1].split("def seed_everything")[0]


def test_committed_config_parses_and_builds_on_the_cpu():
    from utils import load_json
    from trainers import check_prior_config, configure_prior
    from trainers.config import latent_size
    rv = _launcher()
    path = os.path.join(ROOT, "configs", "prior_vqgan_512.json")
    config = load_json(path)
    assert rv.check_arguments(config, _args(config=path)) == ("second_step", 1)
    check_prior_config(config)
    raw, ref = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "vqgan_unet_512.json")))
    assert raw["model"]["vqgan"] == ref["model"]["vqgan"] and raw["model"]["dis"]["normalization"] == "batchnorm"
    assert raw["prior_optim"] == dict(lr=4.5e-4, b1=0.9, b2=0.95, weight_decay=0.01, grad_norm_clip=1.0, warmup_steps=100, decay_steps=0)
    assert latent_size(config) == 16
    gpt = configure_prior(config)
    c = gpt.config
    assert (c.vocab_size, c.block_size, c.n_layer, c.n_head, c.n_embed, c.n_unmasked) == (64, 256, 12, 8, 256, 0)
    assert (gpt.drop.p, c.att_pdrop, c.res_pdrop) == (0.0, 0.0, 0.0)
    assert "prior_vqgan_512.json" in open(os.path.join(ROOT, "configs", "README.md")).read()


def test_tiny_run_config_builds_a_trainer_on_the_cpu(tmp_path):
    """build_prior_trainer up to the point a device is needed: construction runs no kernel."""
    from utils import load_json
    from utils.checkpoint import save_lightning_style_ckpt
    from trainers import build_prior_trainer, PriorTrainer
    from hipops import AdamW
    from networks import VQGAN
    raw = P.prior_run_config(tmp_path / "out")
    torch.manual_seed(5)
    first = VQGAN(**{k: (tuple(v) if k.endswith("multiplier") else v) for k, v in raw["model"]["vqgan"].items()})
    ck = str(tmp_path / "first.ckpt")
    save_lightning_style_ckpt(ck, decoder=first)
    tr = build_prior_trainer(load_json(write_config(tmp_path / "c.json", P.prior_run_config(tmp_path / "out", first_stage_ckpt_path=ck))),
                             device="cpu")
    assert isinstance(tr, PriorTrainer) and list(tr.modules()) == ["decoder", "transformer"] and list(tr.optimizers()) == ["prior_optim"]
    assert isinstance(tr.optim, AdamW) and tr.optim.max_grad_norm == 1.0
    assert (tr.h, tr.w, tr.dict_size, tr.pkeep, tr.sos_token, tr.warmup_steps, tr.decay_steps) == (16, 16, 8, 0.5, 0, 2, 0)
    assert tr.gpt.block_size == 256 and tr.gpt.training
    assert not tr.vqgan.training and not any(p.requires_grad for p in tr.vqgan.parameters())
    for k, v in first.state_dict().items():          # the -v checkpoint's decoder.* keys reached the frozen first stage
        assert torch.equal(tr.vqgan.state_dict()[k], v), k
    assert [g["weight_decay"] for g in tr.optim.param_groups] == [0.01, 0.0] and tr.current_lr() == pytest.approx(0.5e-3)
    st = tr.state_dict()
    assert set(st["modules"]) == {"decoder", "transformer"} and set(st["optimizers"]) == {"prior_optim"}
    assert st["extra"]["prior_step"] == 0 and st["extra"]["prior_generator"].dtype == torch.uint8


def test_prior_trainer_refusals_before_any_kernel():
    from trainers import PriorTrainer
    vq = _tiny_vqgan()
    for kw, what in ((dict(emb_pdrop=0.1), "emb_pdrop"), (dict(res_pdrop=0.1), "res_pdrop"), (dict(att_pdrop=0.1), "att_pdrop")):
        with pytest.raises(NotImplementedError, match="dropout with p = 0.1 in training mode has no kernel.*%s = 0.0" % what):
            PriorTrainer(vq, _gpt(**kw), device="cpu")
    with pytest.raises(ValueError, match="vocab_size=32 must equal the VQGAN's dict_size=64"):
        PriorTrainer(vq, _gpt(vocab_size=32), device="cpu")
    with pytest.raises(ValueError, match="block_size=15 must be at least the latent's h w = 16"):
        PriorTrainer(vq, _gpt(block_size=15), device="cpu")
    with pytest.raises(ValueError, match="sos_token=64"):
        PriorTrainer(vq, _gpt(), sos_token=64, device="cpu")
    with pytest.raises(ValueError, match="pkeep"):
        PriorTrainer(vq, _gpt(), pkeep=1.5, device="cpu")
    with pytest.raises(TypeError):
        PriorTrainer(_gpt(), _gpt(), device="cpu")
    tr = PriorTrainer(vq, _gpt(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the step itself has no CPU route
        tr.training_step({"ids": torch.zeros(2, 16, dtype=torch.long)})


# ------------------------------------------------------------------------------------------------ the fixture and the restatement
def _initial_state(g, name, model):
    """gpt_ref.init_gpt_'s state of a model built under the fixture's seed, checked against the fixture's checksums."""
    G.init_gpt_(model, int(g[name + "/seed"]))
    for k, v in model.named_parameters():
        c, s = g["%s/init.%s" % (name, k)], checksum(v)
        assert s[2] == c[2] and abs(s[0] - c[0]) <= 1e-9 * max(1.0, abs(c[0])) and abs(s[1] - c[1]) <= 1e-9 * max(1.0, c[1]), k
    return model


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture_in_fp64(golden, name):
    g = golden("prior_step_%s.npz" % name)
    seed, clip = int(g[name + "/seed"]), float(g[name + "/clip"])
    assert seed == P.SEEDS[name] and clip == P.GRAD_NORM_CLIP[name]
    torch.manual_seed(seed)
    model = _initial_state(g, name, _gpt(name))
    ids = P.case_ids(name, seed)
    assert torch.equal(ids, g.t(name + "/ids"))
    keys = [str(k) for k in g[name + "/keys"]]
    assert keys == [k for k, _ in model.named_parameters()] and int(g[name + "/nparams"]) == sum(p.numel() for p in model.parameters())
    # some steps clip and some do not
    norms, coefs = g[name + "/norm64"], g[name + "/coef64"]
    assert norms.shape == (P.STEPS,) and norms.min() < clip < norms.max()
    assert [bool(c < 1) for c in coefs] == [bool(n > clip) for n in norms] and (coefs < 1).any() and (coefs == 1).any()
    r = P.steps_ref(name, model.state_dict(), ids, torch.float64, clip)
    for q in ("loss", "norm", "coef"):
        want = g["%s/%s64" % (name, q)]
        assert np.abs(np.array(r[q]) - want).max() <= 1e-12 * np.abs(want).max(), q
        assert g["%s/%s32" % (name, q)].shape == (3, P.STEPS)
    live = [str(k) for k in g[name + "/live"]]
    nl = P.CASES[name][2]
    assert sorted(set(keys) - set(live)) == ["blocks.%d.att.k.bias" % i for i in range(nl)]
    for k in keys:
        idx = sample_idx(r["P"][k].numel(), 256, seed=1)
        got, want = r["P"][k].reshape(-1)[idx], g.t("%s/p64.%s" % (name, k))
        # (an analytically zero gradient moves its parameter by Adam's quotient of rounding noise: 1e-17 / 1e-8)
        assert float((got - want).abs().max()) <= (1e-11 if k in live else 1e-8) * float(want.abs().max()), k
        assert g["%s/p32.%s" % (name, k)].shape == (3,) + tuple(want.shape)
        if k in live:
            got, want = r["g0"][k].reshape(-1)[idx], g.t("%s/g64.%s" % (name, k))
            assert float((got - want).abs().max()) <= 1e-10 * float(g["%s/gnorm64.%s" % (name, k)]), k
            assert abs(float(r["g0"][k].norm()) - float(g["%s/gnorm64.%s" % (name, k)])) <= 1e-9 * float(r["g0"][k].norm()), k


def test_tokens_restatement():
    ids = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    assert P.tokens_ref(ids, 9, 1.0, 10).tolist() == [[9, 5, 6, 7], [9, 1, 2, 3]]
    u_keep = torch.tensor([[0.1, 0.9, 0.4999, 0.5], [0.0, 0.7, 0.2, 0.0]])
    u_rand = torch.tensor([[0.0, 0.25, 0.0, 1 - 2.0 ** -24], [0.0, 0.999, 0.0, 0.0]])
    assert P.tokens_ref(ids, 9, 0.5, 10, u_keep, u_rand).tolist() == [[9, 5, 2, 7], [9, 1, 9, 3]]
    assert P.tokens_ref(ids, 9, 0.0, 10, u_keep, u_rand).tolist() == [[9, 0, 2, 0], [9, 0, 9, 0]]
    # the clamp: a product that rounds up to V in fp32 stays a code
    assert P.tokens_ref(ids[:, :2], 0, 0.0, 3, torch.ones(2, 2), torch.full((2, 2), 1 - 2.0 ** -24)).tolist() == [[0, 2], [0, 2]]


# ------------------------------------------------------------------------------------------------ the VQGAN's code side
def test_raster_order_bookkeeping_on_a_cpu_stand_in():
    """VQ.forward hands out ids[b, i, j] = the code of latent pixel (h = j, w = i); encode_to_ids must return the code of pixel
    (r, c) at r * w + c, and decode_from_ids must hand generate_image_from_ids the transposed view back."""
    from networks import VQGAN
    B, h, w = 2, 3, 3
    code = torch.arange(B * h * w).reshape(B, h, w) * 7 % 11          # code[b, r, c] of latent pixel (r, c)

    class StandIn(torch.nn.Module):          # the quantiser's output layout on the CPU
        def forward(self, x):
            return x, torch.zeros(()), code.transpose(1, 2)

    vq = _tiny_vqgan()
    vq.encoder, vq.vq = torch.nn.Identity(), StandIn()
    with pytest.raises(RuntimeError, match="encode_to_ids: eval mode only"):
        vq.encode_to_ids(torch.zeros(B, 1, 4, 4))
    with pytest.raises(RuntimeError, match="encode_to_ids: eval mode only"):
        vq.decode_from_ids(torch.zeros(B, h * w, dtype=torch.long), h, w)
    vq.eval()
    seq = vq.encode_to_ids(torch.zeros(B, 1, 4, 4))
    assert seq.shape == (B, h * w) and seq.dtype == torch.long and seq.is_contiguous()
    for b in range(B):
        for r in range(h):
            for c in range(w):
                assert int(seq[b, r * w + c]) == int(code[b, r, c])
    seen = {}
    vq.generate_image_from_ids = lambda ids: seen.setdefault("ids", ids)
    vq.decode_from_ids(seq, h, w)
    assert torch.equal(seen["ids"], code.transpose(1, 2))          # what VQ.forward handed out
    assert torch.equal(VQGAN.raster_from_vq_ids(VQGAN.vq_ids_from_raster(seq, h, w)), seq)
    with pytest.raises(ValueError, match="decode_from_ids"):
        vq.decode_from_ids(seq[:, :-1], h, w)
    x = torch.zeros(B, 1, 4, 4, requires_grad=True)
    assert not vq.encode_to_ids(x).requires_grad
