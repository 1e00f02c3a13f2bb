"""CPU-side checks of the label-conditioned masked prior (no GPU): the C ABI and operator plumbing of vqw_embed_cond_fwd and its
refusals before any device work, model.prior.masked.cond through the config checks, the trainer builder and the launcher's
argument check, the refusals of MaskedGPT.generate_parallel and of ConditionalMaskedPriorTrainer that need no device, the shared
mixin, the committed configs, and self-checks of the restatement (tests/masked_cond_ref.py): its drop decision against the integer
formula of tests/dropout_ref.py, its embedding against the two-operator composition in float64, its summation bound."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
from trainers.label_cond import LabelConditionMixin          # the feature's own module: without the feature nothing here runs
import dropout_ref as DR
import gpt_ref as G
import masked_cond_ref as MC
import prior_ref as P

COND = dict(source="label", n_labels=2, labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})
MASKED = dict(n_steps=4, choice_temperature=4.5, mask_seed=3)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbol_in_header_signature_and_schema():
    from hipops import _lib, library, ops
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # a function added only
    assert "vqw_embed_cond_fwd(" in hdr and "vqw_embed_cond_fwd" in _lib.SIGNATURES and "vqw_embed_cond_fwd" in library.register()
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES["vqw_embed_cond_fwd"] == (i, [p, p, p, p, p, p, p, i, i, i, i, i, i, l, f, l, l, p])
    sch = str(torch.ops.vqw.embed_cond_fwd.default._schema)
    for read in ("idx", "tok", "pos", "cidx", "ctab"):
        assert "Tensor? %s" % read in sch, read
    assert "Tensor(a!)? x" in sch and "Tensor(b!)? eff" in sch and "int null_index" in sch and "float p" in sch
    assert ops.COND_DROP_SITE == MC.COND_DROP_SITE == -1 and callable(ops.embedding_cond)


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    """A non-zero status with a message that names the constraint; the pointers are never dereferenced and no HIP call is made."""
    from hipops import _lib
    L = _lib.load()
    A = 4096          # an aligned non-null stand-in for every pointer

    def refused(pattern, **kw):
        a = dict(idx=A, tok=A, pos=A, cidx=A, ctab=A, x=A, eff=None, B=2, T=5, E=8, V=7, L=3, block_size=5, null_index=2, p=0.5, seed=1, call=0)
        a.update(kw)
        rc = L.vqw_embed_cond_fwd(a["idx"], a["tok"], a["pos"], a["cidx"], a["ctab"], a["x"], a["eff"], a["B"], a["T"], a["E"], a["V"], a["L"],
                                  a["block_size"], a["null_index"], ctypes.c_float(a["p"]), a["seed"], a["call"], None)
        assert rc != 0, pattern
        msg = (L.vqw_last_error() or b"").decode()
        assert msg.startswith("vqw_embed_cond_fwd") and pattern in msg, (pattern, msg)

    for E in (0, 6, 4100):
        refused("E=%d must be a multiple of 4 with 4 <= E <= 4096" % E, E=E)
    refused("V=0 must be at least 1", V=0)
    refused("L=0 must be at least 1", L=0)
    refused("B=0, T=5 must be at least 1", B=0)
    refused("B=2, T=0 must be at least 1", T=0)
    refused("T = 5 exceeds block_size=4", block_size=4)
    refused("rows are too many", B=1 << 20, T=1 << 12, block_size=1 << 12)
    refused("p=1 must lie in [0, 1)", p=1.0)
    refused("p=-0.25 must lie in [0, 1)", p=-0.25)
    refused("null_index=3 must be a row of the table, [0, L = 3), when p > 0", null_index=3)
    refused("null_index=-1 must be a row of the table", null_index=-1)
    for name in ("idx", "tok", "pos", "cidx", "ctab", "x"):
        refused("null pointer", **{name: None})
    for name in ("tok", "pos", "ctab", "x"):
        refused("16-byte aligned", **{name: A + 4})


def test_operator_refuses_before_any_kernel():
    from hipops import ops
    idx, tok, pos, cidx, ctab = torch.zeros(2, 5, dtype=torch.long), torch.zeros(7, 8), torch.zeros(1, 5, 8), torch.zeros(2, 5, dtype=torch.long), torch.zeros(3, 8)
    with pytest.raises(ValueError, match=r"null_index=None must be a row of the table \(L = 3\) when p > 0"):
        ops.embedding_cond(idx, tok, pos, cidx, ctab, drop=(0.5, 1, 0))
    with pytest.raises(ValueError, match="null_index=3 must be a row of the table"):
        ops.embedding_cond(idx, tok, pos, cidx, ctab, null_index=3, drop=(0.5, 1, 0))
    with pytest.raises(ValueError, match=r"p=1.0 must lie in \[0, 1\)"):
        ops.embedding_cond(idx, tok, pos, cidx, ctab, null_index=2, drop=(1.0, 1, 0))
    with pytest.raises(RuntimeError, match="ROCm device"):          # a CPU tensor reaches no kernel: there is no fallback
        ops.embedding_cond(idx, tok, pos, cidx, ctab)


# ------------------------------------------------------------------------------------------------ the config
def _raw(tmp_path, cond=COND, masked=MASKED, **sections):
    raw = P.prior_run_config(tmp_path / "out", resume_checkpoint="prior.ckpt")
    raw["model"]["prior"]["masked"] = dict(masked)
    if cond is not None:
        raw["model"]["prior"]["masked"]["cond"] = cond
    raw.update(sections)
    return raw


SYNTH = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, discs=[[16, 16, 5, 1]])
EDIT = dict(n_slices=2, n_candidates=3, temperature=1.0, top_k=4, top_p=0.9, seed=5, box=[8, 16, 8, 24])


def test_config_checks_and_the_trainer_class(tmp_path):
    from utils import load_json
    from networks import MaskedGPT
    from trainers import (ConditionalMaskedPriorTrainer, MaskedPriorTrainer, build_prior_trainer, check_edit_config, check_prior_config,
                          check_synth_config, configure_prior, guidance, prior_cond_drop, prior_condition, prior_masked, synth_n_steps)
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    c = cfg(_raw(tmp_path, synth=SYNTH, edit=EDIT))
    check_prior_config(c)
    check_synth_config(c)
    check_edit_config(c)
    assert prior_masked(c) == MASKED
    assert prior_condition(c) == {"n_labels": 2, "label_modality": None, "lesions": dict(n=2, radius=5, contrast=0.8)}
    assert prior_cond_drop(c) == {"null_token": False, "p_uncond": 0.0, "drop_seed": None} and synth_n_steps(c) is None
    gpt = configure_prior(c)
    assert isinstance(gpt, MaskedGPT) and gpt.block_size == 256          # the sequence stays h w long: the condition is added
    tr = build_prior_trainer(c, device="cpu")
    assert type(tr) is ConditionalMaskedPriorTrainer and isinstance(tr, MaskedPriorTrainer) and sorted(tr.modules()) == ["cond", "decoder", "transformer"]
    assert tr.cond.null_index is None and tuple(tr.cond.embed.weight.shape) == (2, 64) and (tr.n_steps, tr.mask_seed, tr.Tc) == (4, 3, 256)
    assert any(p is tr.cond.embed.weight for p in tr.optim.param_groups[1]["params"])          # the undecayed group
    assert sum(len(g["params"]) for g in tr.optim.param_groups) == len(list(tr.gpt.parameters())) + 1
    assert "cond_drop_seed" not in tr.state_dict()["extra"]
    # absent or `false`: the unconditional masked prior, as it was
    for absent in (None, False):
        c = cfg(_raw(tmp_path, cond=absent))
        assert prior_condition(c) is None and type(build_prior_trainer(c, device="cpu")) is MaskedPriorTrainer
    # classifier-free guidance keys
    cfg_keys = dict(COND, null_token=True, p_uncond=0.25, drop_seed=11)
    c = cfg(_raw(tmp_path, cond=cfg_keys, synth=dict(SYNTH, guidance_scale=3.0, rank="gain", n_steps=6), edit=dict(EDIT, guidance_scale=2.0)))
    check_synth_config(c)
    check_edit_config(c)
    assert prior_cond_drop(c) == {"null_token": True, "p_uncond": 0.25, "drop_seed": 11}
    assert guidance(c, "synth") == (3.0, "gain") and guidance(c, "edit") == (2.0, "cond") and synth_n_steps(c) == 6
    tr = build_prior_trainer(c, device="cpu")
    assert (tr.p_uncond, tr.cond_drop_seed, tr.cond.null_index) == (0.25, 11, 2) and tr.state_dict()["extra"]["cond_drop_seed"] == 11
    state = tr.state_dict()
    state["extra"]["cond_drop_seed"] = 12
    with pytest.raises(ValueError, match="ConditionalMaskedPriorTrainer: the checkpoint was trained with cond_drop_seed=12"):
        tr.load_state_dict(state)
    # missing keys are named
    for key in ("source", "n_labels", "labels"):
        bad = dict(COND)
        del bad[key]
        with pytest.raises(NotImplementedError, match=r"model\.prior\.masked\.cond\.\{source, n_labels, labels\}; missing: %s$" % key):
            check_prior_config(cfg(_raw(tmp_path, cond=bad)))
    with pytest.raises(ValueError, match=r"model\.prior\.masked\.cond\.p_uncond=0\.25 .* needs model\.prior\.masked\.cond\.null_token: true"):
        prior_cond_drop(cfg(_raw(tmp_path, cond=dict(COND, p_uncond=0.25, drop_seed=1))))
    with pytest.raises(ValueError, match=r"model\.prior\.masked\.cond\.p_uncond=0\.25 needs model\.prior\.masked\.cond\.drop_seed"):
        prior_cond_drop(cfg(_raw(tmp_path, cond=dict(COND, p_uncond=0.25, null_token=True))))
    with pytest.raises(ValueError, match=r"synth\.guidance_scale=3 needs .* model\.prior\.masked\.cond\.null_token: true"):
        check_synth_config(cfg(_raw(tmp_path, synth=dict(SYNTH, guidance_scale=3.0))))
    with pytest.raises(NotImplementedError, match=r"needs a conditional prior; missing: model\.prior\.masked\.cond"):
        check_synth_config(cfg(_raw(tmp_path, cond=None, synth=SYNTH)))
    with pytest.raises(ValueError, match=r"synth\.n_steps=0 must be an integer >= 1"):
        check_synth_config(cfg(_raw(tmp_path, synth=dict(SYNTH, n_steps=0))))
    with pytest.raises(NotImplementedError, match=r"edit\.nll_threshold"):
        check_edit_config(cfg(_raw(tmp_path, edit=dict({k: v for k, v in EDIT.items() if k != "box"}, nll_threshold=2.0))))
    # model.prior.cond beside model.prior.masked stays refused, and now names the new key
    raw = _raw(tmp_path)
    raw["model"]["prior"]["cond"] = COND
    with pytest.raises(NotImplementedError, match=r"model\.prior\.cond beside model\.prior\.masked .* model\.prior\.masked\.cond"):
        check_prior_config(cfg(raw))
    # synth.n_steps means nothing to the autoregressive conditional prior
    raw = P.prior_run_config(tmp_path / "out", resume_checkpoint="prior.ckpt")
    raw["model"]["prior"]["cond"] = COND
    raw["synth"] = dict(SYNTH, n_steps=4)
    with pytest.raises(ValueError, match=r"synth\.n_steps=4 .* needs model\.prior\.masked"):
        check_synth_config(cfg(raw))


def test_prior_condition_names_what_is_missing(tmp_path):
    from utils import load_json
    from trainers import check_prior_config, prior_condition
    with pytest.raises(ValueError, match=r"model\.prior\.masked\.cond\.p_uncond=0\.25 .* needs model\.prior\.masked\.cond\.null_token"):
        check_prior_config(load_json(write_config(tmp_path / "c.json", _raw(tmp_path, cond=dict(COND, p_uncond=0.25, drop_seed=1)))))
    bad = {k: v for k, v in COND.items() if k != "labels"}
    with pytest.raises(NotImplementedError, match=r"model\.prior\.masked\.cond\.\{source, n_labels, labels\}; missing: labels$"):
        prior_condition(load_json(write_config(tmp_path / "c.json", _raw(tmp_path, cond=bad))))
    with pytest.raises(NotImplementedError, match=r"model\.prior\.masked\.cond\.source is 'label'"):
        prior_condition(load_json(write_config(tmp_path / "c.json", _raw(tmp_path, cond=dict(COND, source="text")))))


def test_launcher_argument_check(tmp_path):
    import argparse
    import importlib.util
    from utils import load_json
    spec = importlib.util.spec_from_file_location("run_vqwnet_masked_cond", os.path.join(ROOT, "medical-image-editing_amd", "run_vqwnet.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    args = lambda mode: argparse.Namespace(config="x.json", mode=mode, multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)  # noqa: E731
    raw = _raw(tmp_path, synth=SYNTH, edit=EDIT)
    raw["detect"] = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0,
                         against="image", weight="mask", labels=False)
    raw["score"] = dict(n_slices=4, n_samples=4, batch_size=2, k=1, temperature=1.0, top_k=4, top_p=0.9, against="image", seed=5,
                        guidance_scale=False, n_steps=False)
    config = load_json(write_config(tmp_path / "c.json", raw))
    for mode in ("train", "edit", "synth", "score"):
        assert rv.check_arguments(config, args(mode)) == ("second_step", 1), mode
    with pytest.raises(NotImplementedError, match="-m detect with model.prior"):
        rv.check_arguments(config, args("detect"))
    assert "model.prior.masked.cond" in rv.__doc__


def test_committed_configs_parse():
    from utils import load_json
    from trainers import check_prior_config, check_synth_config, guidance, prior_cond_drop, prior_condition, prior_masked
    names = ("prior_vqgan_512_masked_cond", "prior_vqgan_512_masked_cond_synth")
    for name in names:
        config = load_json(os.path.join(ROOT, "configs", name + ".json"))
        check_prior_config(config)
        assert prior_masked(config) == {"n_steps": 8, "choice_temperature": 4.5, "mask_seed": 0}
        assert prior_condition(config)["n_labels"] == 2 and prior_cond_drop(config) == {"null_token": True, "p_uncond": 0.1, "drop_seed": 0}
    synth = load_json(os.path.join(ROOT, "configs", names[1] + ".json"))
    check_synth_config(synth)
    assert guidance(synth, "synth") == (3.0, "cond")
    a, b = (json.load(open(os.path.join(ROOT, "configs", n + ".json"))) for n in (names[0], "prior_vqgan_512_masked"))
    a["model"]["prior"]["masked"].pop("cond")
    assert a["model"] == b["model"] and a["prior_optim"] == b["prior_optim"] and a["save"]["study_name"] == names[0]
    readme = open(os.path.join(ROOT, "configs", "README.md")).read()
    assert all(n + ".json" in readme for n in names)


# ------------------------------------------------------------------------------------------------ the model and the trainer on the CPU
def test_refusals_on_the_cpu():
    from networks import LabelCondition, MaskedGPT, VQGAN
    from trainers import ConditionalMaskedPriorTrainer, ConditionalPriorTrainer
    kw = dict(vocab_size=64, block_size=16, n_layer=2, n_head=2, n_embed=64)
    m = MaskedGPT(**kw)
    ids, masked = torch.zeros(2, 4, dtype=torch.long), torch.ones(2, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="guidance_scale=3.0 needs cond"):
        m.generate_parallel(ids, masked, 2, guidance_scale=3.0)
    with pytest.raises(ValueError, match="guidance_scale=3.0 needs cond"):
        m.generate_parallel(ids, masked, 2, cond=(ids, torch.zeros(3, 64), None), guidance_scale=3.0)
    with pytest.raises(ValueError, match="guidance_scale=-1.0 must be finite and not negative"):
        m.generate_parallel(ids, masked, 2, cond=(ids, torch.zeros(3, 64), 2), guidance_scale=-1.0)
    with pytest.raises(ValueError, match=r"cond tokens \(B, T\) = \(2, 4\)"):
        m.generate_parallel(ids, masked, 2, cond=(ids[:, :3], torch.zeros(3, 64), 2))
    vqgan = VQGAN(**P.TINY_VQGAN)
    with pytest.raises(TypeError, match="ConditionalMaskedPriorTrainer conditions on a networks.LabelCondition"):
        ConditionalMaskedPriorTrainer(vqgan, m, None, device="cpu")
    with pytest.raises(ValueError, match=r"p_uncond=0.2 needs a condition with the null embedding.*model\.prior\.masked\.cond\.null_token"):
        ConditionalMaskedPriorTrainer(vqgan, m, LabelCondition(2, 64, 4, 4), p_uncond=0.2, cond_drop_seed=1, device="cpu")
    with pytest.raises(ValueError, match=r"p_uncond=0.2 needs cond_drop_seed \(model\.prior\.masked\.cond\.drop_seed\)"):
        ConditionalMaskedPriorTrainer(vqgan, m, LabelCondition(2, 64, 4, 4, null_token=True), p_uncond=0.2, device="cpu")
    with pytest.raises(ValueError, match="the condition's n_embed=32 must equal the GPT's n_embed=64"):
        ConditionalMaskedPriorTrainer(vqgan, m, LabelCondition(2, 32, 4, 4), device="cpu")
    with pytest.raises(TypeError, match="MaskedPriorTrainer trains a networks.MaskedGPT"):
        from networks import GPT
        ConditionalMaskedPriorTrainer(vqgan, GPT(**kw), LabelCondition(2, 64, 4, 4), device="cpu")
    tr = ConditionalMaskedPriorTrainer(vqgan, m, LabelCondition(2, 64, 4, 4), n_steps=4, mask_seed=5, device="cpu")
    assert isinstance(tr, LabelConditionMixin) and issubclass(ConditionalPriorTrainer, LabelConditionMixin)
    for name in ("cond_tokens", "_label", "_guidance", "_rank", "cell_mask"):          # one copy, used by both classes
        assert getattr(ConditionalMaskedPriorTrainer, name) is getattr(ConditionalPriorTrainer, name), name
    batch = {"ids": torch.zeros(2, 16, dtype=torch.long), "cond": torch.zeros(2, 16, dtype=torch.long)}
    for call in (lambda: tr.token_nll(batch), lambda: tr.detect(batch, nll_threshold=1.0), lambda: tr.edit(batch, nll_threshold=1.0)):
        with pytest.raises(NotImplementedError, match="raster-order likelihood is not defined"):
            call()
    with pytest.raises(NotImplementedError, match="ConditionalMaskedPriorTrainer: sampling needs a condition"):
        tr.sample_ids(2)
    with pytest.raises(ValueError, match="rank='gain' compares the conditional and the unconditional score"):
        tr.synthesize(cond=batch["cond"], rank="gain")
    with pytest.raises(ValueError, match=r"guidance_scale=3.0 needs a prior trained with the null embedding \(model\.prior\.masked\.cond\.null_token\)"):
        tr.edit(batch, box=(0, 4, 0, 4), guidance_scale=3.0)
    with pytest.raises(ValueError, match="exactly one of mask, box and new_label"):
        tr.edit(batch)
    with pytest.raises(ValueError, match="exactly one of label and cond"):
        tr.synthesize()
    with pytest.raises(ValueError, match="the batch has no 'cond'"):
        tr.cond_tokens({"ids": batch["ids"]})
    with pytest.raises(ValueError, match="one sample is drawn per held-out slice: n_samples=3"):
        list(tr._score_draws([batch["cond"]], 3, 2, 1.0, None, None, None))


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_drop_is_dropout_refs_formula():
    for seed, call in MC.EMBED_KEYS + [(0, 0), (-5, 2 ** 62), (21, 3)]:
        for p in (0.0, 0.1, 0.5, 0.999):
            assert np.array_equal(MC.dropped(70, p, seed, call), ~DR.keep_mask(70, p, seed, call, MC.COND_DROP_SITE)), (seed, call, p)
        assert [MC.draw(b, seed, call) for b in range(5)] == DR.draws(np.zeros(5, dtype=np.uint32), np.arange(5, dtype=np.uint32), seed, call, -1).tolist()
        assert not MC.dropped(70, 0.0, seed, call).any()
    assert MC.threshold(0.5) == 2 ** 31 == DR.threshold(0.5) and MC.threshold(0.0) == 0
    assert 0.4 < MC.dropped(4000, 0.5, 9, 9).mean() < 0.6


def test_embed_keys_drop_one_sample_and_keep_one_in_every_case():
    """What the GPU test asserts from eff: over the three (seed, call) pairs at p = 0.5 every case has a dropped and a kept sample -
    within one pair wherever B >= 2 allows it."""
    for B in sorted({c[0] for c in MC.EMBED_CASES}):
        gone = np.stack([MC.dropped(B, 0.5, s, c) for s, c in MC.EMBED_KEYS])
        assert gone.any() and not gone.all(), B
        if B >= 2:
            assert any(g.any() and not g.all() for g in gone), B


def test_reference_embedding_is_the_two_operator_composition():
    for case in MC.EMBED_CASES:
        B, T, E, V, L, bs = case
        idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*case)
        assert pos.shape[1] == (T if bs is None else bs) and ctab.shape[0] == L + 1
        for drop in (None, (0.5,) + MC.EMBED_KEYS[0]):
            x32, e = MC.embedding_cond_ref(idx, tok, pos, cidx, ctab, L, drop)
            x64, _ = MC.embedding_cond_ref(idx, tok.double(), pos.double(), cidx, ctab.double(), L, drop)
            mag = tok[idx].abs().double() + pos[0, :T].abs().double() + ctab[e].abs().double()
            assert bool(((x32.double() - x64).abs() <= 2 * MC.U * (1 + MC.U) * mag).all()), case          # two roundings of partial sums
            assert torch.equal(x32, G.embedding_ref(idx, tok, pos) + ctab[e])
            gone = MC.dropped(B, *drop) if drop else np.zeros(B, dtype=bool)
            assert bool((e[torch.from_numpy(gone)] == L).all()) and torch.equal(e[torch.from_numpy(~gone)], cidx[torch.from_numpy(~gone)])
    # the inputs round: on every case but the one-row one, each other order or rounding of the three summands gives other bits
    # somewhere, so a bit comparison on these inputs pins the order (tok + pos) + ctab
    for case in MC.EMBED_CASES:
        idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*case)
        x = MC.embedding_cond_ref(idx, tok, pos, cidx, ctab)[0]
        differ = [not torch.equal(x, o) for o in MC.other_orders(idx, tok, pos, cidx, ctab)]
        assert all(differ) or case[0] * case[1] * case[2] <= 4, (case, differ)
    idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*MC.EMBED_CASES[1])
    idx[0, 2], cidx[1, 4] = 7, -1
    x, e = MC.embedding_cond_ref(idx, tok, pos, cidx, ctab)
    bad = torch.zeros(3, 15, dtype=torch.bool)
    bad[0, 2] = bad[1, 4] = True
    assert bool(torch.isnan(x[bad]).all()) and bool(torch.isfinite(x[~bad]).all())


def test_reference_gradients_and_sum_bound():
    case = MC.EMBED_CASES[1]
    B, T, E, V, L, _ = case
    idx, tok, pos, cidx, ctab, gx = MC.embed_inputs(*case)
    t, p, c = (v.double().requires_grad_(True) for v in (tok, pos, ctab))
    x, e = MC.embedding_cond_ref(idx, t, p, cidx, c)
    (x * gx.double()).sum().backward()
    (gtok, mt, nt), (gpos, mp, npos), (gctab, mcb, nc) = MC.embedding_cond_grads(idx, e, gx, V, L + 1, T)
    assert torch.allclose(gtok, t.grad, rtol=0, atol=1e-12) and torch.allclose(gpos, p.grad[0], rtol=0, atol=1e-12)
    assert torch.allclose(gctab, c.grad, rtol=0, atol=1e-12) and int(nc[L]) == 0 and not bool(gctab[L].any())          # the null row is unused
    assert int(nt.sum()) == B * T == int(nc.sum()) and npos.tolist() == [B] * T
    # a one-by-one fp32 sum stays inside the bound, and the bound of a single term is 0
    acc = torch.zeros(T, E)
    for b in range(B):
        acc = acc + gx[b]
    assert bool(((acc.double() - gpos).abs() <= MC.sum_bound(mp, npos)).all())
    assert float(MC.sum_bound(torch.ones(1, 1, dtype=torch.float64), torch.tensor([1])).max()) == 0.0


def test_learn_batch_codes_are_their_label_tokens():
    ids, tokens = MC.learn_batch()
    assert torch.equal(ids, tokens) and int(tokens.max()) < MC.N_LABELS <= MC.TINY["vocab_size"] and 0 < MC.LEARN_STEPS <= 200
