"""Host tests of the GPT prior's dropout: the C ABI's new symbols, the refusal without a seed and what a seed changes, the site
numbering, the configuration keys, the trainer's state, and the statistics of the restated mask (tests/dropout_ref.py, the
formulas of csrc/dropout.h).

The statistical conditions are derived from the binomial, 5 sigma each: of n independent draws kept with probability 1 - p,
|kept - n (1 - p)| <= 5 sqrt(n p (1 - p)); two independent masks agree on an element with probability a = p^2 + (1 - p)^2, so
their agreement count lies within 5 sqrt(n a (1 - a)) of n a.  The threshold round(p 2^32) moves 1 - p by less than 2^-32."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref as D
import prior_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vqw_dropout", "vqw_add_dropout", "vqw_dropout_mask", "vqw_attention_dropout_mask", "vqw_causal_attention_drop_fwd",
               "vqw_causal_attention_drop_bwd"]


def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.SIGNATURES and s in ops_, s
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES["vqw_dropout"] == (i, [p, p, l, f, l, l, i, p])
    assert _lib.SIGNATURES["vqw_add_dropout"] == (i, [p, p, p, l, f, l, l, i, p])
    assert _lib.SIGNATURES["vqw_attention_dropout_mask"][1] == [p, i, i, i, i, f, l, l, i, p]
    base, drop = _lib.SIGNATURES["vqw_causal_attention_fwd"][1], _lib.SIGNATURES["vqw_causal_attention_drop_fwd"][1]
    assert drop == base[:-1] + [f, l, l, i, p]          # vqw_causal_attention_fwd's list, then p, seed, call, site
    base, drop = _lib.SIGNATURES["vqw_causal_attention_bwd"][1], _lib.SIGNATURES["vqw_causal_attention_drop_bwd"][1]
    assert drop == base[:-1] + [f, l, l, i, p]
    sch = str(torch.ops.vqw.add_dropout.default._schema)
    assert "Tensor? a" in sch and "Tensor? b" in sch and "Tensor(a!)? y" in sch and "float p" in sch and "int seed" in sch and "int site" in sch
    sch = str(torch.ops.vqw.dropout_mask.default._schema)
    assert "Tensor(a!)? out" in sch
    sch = str(torch.ops.vqw.causal_attention_drop_bwd.default._schema)
    assert "Tensor? lse" in sch and "Tensor(b!)? gq" in sch and "float p" in sch and "int call" in sch
    for name in ("dropout", "add_dropout", "dropout_keep_mask", "attention_keep_mask"):
        from hipops import ops
        assert callable(getattr(ops, name)), name


def _small(**kw):
    from networks import GPT
    args = dict(vocab_size=16, block_size=8, n_layer=2, n_head=2, n_embed=64)
    args.update(kw)
    return GPT(**args)


def test_unseeded_refusal_is_unchanged_and_a_seed_reaches_the_kernels():
    from networks import Block, CausalSelfAttention, GPTConfig
    idx, x = torch.zeros(1, 8, dtype=torch.long), torch.randn(1, 8, 64)
    for what in ("emb_pdrop", "res_pdrop", "att_pdrop"):
        m = _small(**{what: 0.1}).train()
        with pytest.raises(NotImplementedError, match="dropout with p = 0.1 in training mode has no kernel.*%s = 0.0.*seed_dropout" % what):
            m(idx)                                                  # before any kernel: these are CPU tensors
        m.seed_dropout(3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # the forward now runs - and has no CPU route
            m(idx)
        assert m.dropout_call == 0          # a forward that did not happen takes no call
    for cls in (Block, CausalSelfAttention):
        m = cls(GPTConfig(16, 8, n_embed=64, n_head=2)).train()          # the class defaults: every p = 0.1
        with pytest.raises(NotImplementedError, match="has no kernel"):
            m(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.seed_dropout(0)(x)
    from hipops import ops
    for call in (lambda: ops.dropout(x, 0.1, (0, 0, 0)), lambda: ops.add_dropout(x, x, 0.1, (0, 0, 0)),
                 lambda: ops.causal_attention(x, x, x, 2, dropout_p=0.1, dropout_key=(0, 0, 0)),
                 lambda: ops.dropout_keep_mask(4, 0.1, (0, 0, 0), device="cpu"), lambda: ops.attention_keep_mask(1, 1, 4, 4, 0.1, (0, 0, 0), device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.dropout(x, 1.0, (0, 0, 0))


def test_site_numbering_and_the_call_counter():
    m = _small(emb_pdrop=0.1, res_pdrop=0.1, att_pdrop=0.1)
    assert m.dropout_seed is None and all(b.dropout_seed is None and b.att.dropout_seed is None for b in m.blocks)
    keys = list(m.state_dict())
    assert m.seed_dropout(9, call=4) is m
    assert list(m.state_dict()) == keys          # nothing of it is a parameter or a buffer
    # site 0 is `drop`, then per block att_drop, att.res_drop, mlp[3]
    assert m.dropout_site == 0
    assert [(b.att.dropout_site, b.att.dropout_site + 1, b.dropout_site) for b in m.blocks] == [(1, 2, 3), (4, 5, 6)]
    mods = [m] + [x for b in m.blocks for x in (b, b.att)]
    assert all(x.dropout_seed == 9 and x.dropout_call == 4 for x in mods)
    m.set_dropout_call(17)
    assert all(x.dropout_call == 17 for x in mods)
    assert m._dropout_call() == 17 and m.eval()._dropout_call() is None
    from networks import Block, GPTConfig
    b = Block(GPTConfig(16, 8, n_embed=64, n_head=2)).seed_dropout(1)
    assert (b.att.dropout_site, b.dropout_site, b.dropout_call, b.att.dropout_call) == (0, 2, 0, 0)


def _config(tmp_path, raw):
    from utils import load_json
    path = tmp_path / "config.json"
    path.write_text(json.dumps(raw))
    return load_json(str(path))


def test_configuration_keys_and_the_dropout_config(tmp_path):
    from utils import load_json
    from trainers import check_prior_config, configure_prior
    raw = P.prior_run_config(tmp_path / "out")
    m = configure_prior(_config(tmp_path, raw))
    assert (m.drop.p, m.blocks[0].att.att_drop.p, m.blocks[0].att.res_drop.p, m.blocks[0].mlp[3].p) == (0.0, 0.0, 0.0, 0.0)
    raw["model"]["prior"].update(emb_pdrop=0.3, res_pdrop=0.2, att_pdrop=False)
    m = configure_prior(_config(tmp_path, raw))
    assert (m.drop.p, m.blocks[1].att.att_drop.p, m.blocks[1].att.res_drop.p, m.blocks[1].mlp[3].p) == (0.3, 0.0, 0.2, 0.2)
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_dropout.json")
    new, old = json.load(open(path)), json.load(open(os.path.join(ROOT, "configs", "prior_vqgan_512.json")))
    assert new["save"]["study_name"] == "prior_vqgan_512_dropout" != old["save"]["study_name"]
    assert {k: new["model"]["prior"][k] for k in ("emb_pdrop", "res_pdrop", "att_pdrop")} == dict(emb_pdrop=0.1, res_pdrop=0.1, att_pdrop=0.1)
    for d in (new, old):
        d.pop("comment"), d["save"].pop("study_name")
        for k in ("emb_pdrop", "res_pdrop", "att_pdrop"):
            d["model"]["prior"].pop(k, None)
    assert new == old          # a copy otherwise
    check_prior_config(load_json(path))
    m = configure_prior(load_json(path))
    assert (m.drop.p, m.blocks[11].att.att_drop.p, m.blocks[11].mlp[3].p) == (0.1, 0.1, 0.1)
    assert "prior_vqgan_512_dropout.json" in open(os.path.join(ROOT, "configs", "README.md")).read()


def test_prior_trainer_state_carries_the_seed():
    from networks import GPT, VQGAN
    from trainers import PriorTrainer
    vq = VQGAN(**P.TINY_VQGAN)
    gpt = GPT(emb_pdrop=0.1, res_pdrop=0.1, att_pdrop=0.1, **P.gpt_kwargs("p64"))
    with pytest.raises(NotImplementedError, match="dropout with p = 0.1 in training mode has no kernel"):
        PriorTrainer(vq, gpt, device="cpu")
    tr = PriorTrainer(vq, gpt, device="cpu", dropout_seed=21)
    assert gpt.dropout_seed == 21 and tr.state_dict()["extra"]["prior_dropout_seed"] == 21
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # not the dropout refusal: the step itself has no CPU route
        tr.training_step({"ids": torch.zeros(2, 16, dtype=torch.long)})
    state = tr.state_dict()
    state["extra"]["prior_dropout_seed"] = 22
    with pytest.raises(ValueError, match="dropout_seed=22"):
        tr.load_state_dict(state)
    plain = PriorTrainer(vq, GPT(**P.gpt_kwargs("p64")), device="cpu")
    assert plain.state_dict()["extra"]["prior_dropout_seed"] is None


# ------------------------------------------------------------------------------------------------ the mask's statistics
N = 1 << 20
_masks = {}


def _mask(p, seed, call=3, site=5, start=0):
    key = (p, seed, call, site, start)
    if key not in _masks:
        _masks[key] = D.keep_mask(N, p, seed, call, site, start=start)
    return _masks[key]


def _agree(a, b, p, what):
    n, q = a.size, p * p + (1 - p) ** 2
    z = (int((a == b).sum()) - n * q) / math.sqrt(n * q * (1 - q))
    print("%-40s agreement z = %+.2f" % (what, z))
    assert abs(z) <= 5, what


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mask_statistics(p, seed):
    m = _mask(p, seed)
    z = (int(m.sum()) - N * (1 - p)) / math.sqrt(N * p * (1 - p))
    print("p=%g seed=%d kept z = %+.2f" % (p, seed, z))
    assert abs(z) <= 5
    _agree(m, _mask(p, seed, site=6), p, "p=%g seed=%d site s, s + 1" % (p, seed))
    _agree(m, _mask(p, seed, call=4), p, "p=%g seed=%d call c, c + 1" % (p, seed))
    _agree(m, _mask(p, seed + 1), p, "p=%g seed=%d seed, seed + 1" % (p, seed))
    _agree(m[:-1], m[1:], p, "p=%g seed=%d element e, e + 1" % (p, seed))
    am = D.attention_keep_mask(1, 2, 512, 512, p, seed, 3, 5)
    _agree(am[0, 0], am[0, 1], p, "p=%g seed=%d attention h, h + 1" % (p, seed))
    _agree(am[0, :, :-1], am[0, :, 1:], p, "p=%g seed=%d attention i, i + 1" % (p, seed))
    _agree(am[0, :, :, :-1], am[0, :, :, 1:], p, "p=%g seed=%d attention j, j + 1" % (p, seed))


def test_restatement_details():
    assert D.threshold(0.5) == 1 << 31 and D.threshold(0.0) == 0 and D.threshold(0.1) == int(round(float(np.float32(0.1)) * 2.0 ** 32))
    assert D.scale(0.5) == np.float32(2.0) and D.scale(0.0) == np.float32(1.0)
    assert D.key_words(0, 0, 0) != D.key_words(0, 0, 1) != D.key_words(0, 1, 0) != D.key_words(1, 0, 0)
    assert D.key_words(-1, 0, 0) == D.key_words((1 << 64) - 1, 0, 0)          # two's complement on 64 bits
    # the index is 64 bits: an element behind 2^32 is not the element 2^32 before it
    a, b = D.keep_mask(4096, 0.5, 1, 2, 3), D.keep_mask(4096, 0.5, 1, 2, 3, start=1 << 32)
    assert 0.4 < float((a == b).mean()) < 0.6
    # an attention mask's row is the element-wise site's row hi = (b n_head + h) Tq + i
    am = D.attention_keep_mask(2, 3, 5, 7, 0.5, 1, 2, 3)
    assert np.array_equal(am[1, 2, 4], D.keep_mask(7, 0.5, 1, 2, 3, start=((1 * 3 + 2) * 5 + 4) << 32))
