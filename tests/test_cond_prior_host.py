"""CPU-side checks of the conditional code prior (no GPU): the restatement (tests/cond_prior_ref.py) on hand-made label maps, the C
ABI and operator plumbing of vqw_cell_labels, vqw_cells_changed and vqw_embed_lookup with their refusals before any device work,
networks.LabelCondition, the construction refusals of trainers.ConditionalPriorTrainer, model.prior.cond and the `synth` section,
and the launcher's `-m synth` beside the argument paths it had."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import cond_prior_ref as C
import prior_ref as P

NEW_SYMBOLS = ("vqw_cell_labels", "vqw_cells_changed", "vqw_embed_lookup")


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_cell_labels_ref_on_hand_made_maps():
    lab = np.array([[[0, 0, 1, 2, 9, 9],
                     [0, 1, 2, 1, 9, -1]]])          # three cells of 2 x 2: a majority, a tie between 1 and 2, no valid pixel
    tokens, purity = C.cell_labels_ref(lab, 1, 3, 3)
    assert tokens.tolist() == [[[0, 1, -1]]] and tokens.dtype == np.int64
    assert purity.dtype == np.float32 and purity.tolist() == [[[0.75, 0.5, 0.0]]]
    lab = np.array([[[3, 0], [3, 3]]])               # out-of-range pixels count for nothing: the one valid pixel wins
    tokens, purity = C.cell_labels_ref(lab, 1, 1, 3)
    assert tokens.tolist() == [[[0]]] and purity.tolist() == [[[0.25]]]
    assert C.cell_labels_ref(lab, 1, 1, 4)[0].tolist() == [[[3]]]
    assert C.cell_labels_ref(lab[:, None], 2, 2, 4)[0].tolist() == [[[3, 0], [3, 3]]]          # (B, 1, H, W), one-pixel cells
    a = np.zeros((2, 4, 6), dtype=np.uint8)
    b = a.copy()
    b[1, 3, 5] = 1
    assert C.cells_changed_ref(a, a, 2, 3).sum() == 0
    want = np.zeros((2, 2, 3), dtype=np.uint8)
    want[1, 1, 2] = 1
    assert np.array_equal(C.cells_changed_ref(a, b, 2, 3), want)


@pytest.mark.parametrize("dtype", C.LABEL_DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_label_inputs_hold_what_the_cases_promise(dtype):
    for case in C.LABEL_CASES:
        B, H, W, h, w, L = case
        lab = C.label_inputs(case, dtype).numpy().astype(np.int64)
        tokens, purity = C.cell_labels_ref(lab, h, w, L)
        fy, fx = H // h, W // w
        has_invalid, has_tie, has_empty = C.label_features(case, dtype)
        assert bool(((lab < 0) | (lab >= L)).any()) == has_invalid and bool((tokens == -1).any()) == has_empty, case
        if has_tie:
            cells = lab.reshape(B, h, fy, w, fx).transpose(0, 1, 3, 2, 4).reshape(B, h, w, -1)
            counts = np.stack([(cells == v).sum(-1) for v in range(L)], -1)
            top2 = np.sort(counts, -1)[..., -2:]
            assert ((top2[..., 0] == top2[..., 1]) & (top2[..., 1] * 2 >= fy * fx - 2 * (fy * fx // 16)) & (top2[..., 1] > 0)).any(), "an exact tie at the top in %s" % (case,)
    assert any(C.label_features(c, dtype) == (True, True, True) for c in C.LABEL_CASES) or dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and s in ops_, s
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES["vqw_cell_labels"] == (ctypes.c_int, [p, p, p, i, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_cells_changed"] == (ctypes.c_int, [p, p, p, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["vqw_embed_lookup"] == (ctypes.c_int, [p, p, p, l, i, i, p])
    sch = str(torch.ops.vqw.cell_labels.default._schema)
    assert "Tensor? label" in sch and "Tensor(a!)? tokens" in sch and "Tensor(b!)? purity" in sch and "int n_labels" in sch
    sch = str(torch.ops.vqw.cells_changed.default._schema)
    assert "Tensor? a" in sch and "Tensor? b" in sch and "Tensor(a!)? out" in sch
    sch = str(torch.ops.vqw.embed_lookup.default._schema)
    assert "Tensor? idx" in sch and "Tensor? table" in sch and "Tensor(a!)? out" in sch


def test_the_c_entry_points_refuse_before_any_launch():
    from hipops import _lib
    L = _lib.load()
    P8 = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused by its argument check

    def err():
        return L.vqw_last_error().decode()
    assert L.vqw_cell_labels(P8, P8, None, 1, 24, 40, 5, 5, 3, 1, None) != 0 and "multiples of the cell grid" in err()
    assert L.vqw_cell_labels(P8, P8, None, 1, 24, 40, 3, 5, 0, 1, None) != 0 and "n_labels=0" in err()
    assert L.vqw_cell_labels(P8, P8, None, 1, 24, 40, 3, 5, 257, 1, None) != 0 and "n_labels=257" in err()
    assert L.vqw_cell_labels(P8, P8, None, 1, 24, 40, 3, 5, 3, 2, None) != 0 and "elem_bytes=2" in err()
    assert L.vqw_cell_labels(None, P8, None, 1, 24, 40, 3, 5, 3, 1, None) != 0 and "null pointer" in err()
    assert L.vqw_cell_labels(ctypes.c_void_p(4100), P8, None, 1, 24, 40, 3, 5, 3, 8, None) != 0 and "element size" in err()
    assert L.vqw_cell_labels(P8, P8, None, 0, 24, 40, 3, 5, 3, 1, None) != 0 and "must be positive" in err()
    assert L.vqw_cell_labels(P8, P8, None, 70000, 24, 40, 3, 5, 3, 1, None) != 0 and "65535" in err()
    assert L.vqw_cells_changed(P8, P8, P8, 1, 24, 40, 5, 5, 1, None) != 0 and "multiples of the cell grid" in err()
    assert L.vqw_cells_changed(P8, None, P8, 1, 24, 40, 3, 5, 1, None) != 0 and "null pointer" in err()
    assert L.vqw_cells_changed(P8, P8, P8, 1, 24, 40, 3, 5, 3, None) != 0 and "elem_bytes=3" in err()
    assert L.vqw_embed_lookup(P8, P8, P8, 0, 32, 3, None) != 0 and "rows=0" in err()
    assert L.vqw_embed_lookup(P8, P8, P8, 4, 30, 3, None) != 0 and "E=30" in err()
    assert L.vqw_embed_lookup(P8, P8, P8, 4, 32, 0, None) != 0 and "L=0" in err()
    assert L.vqw_embed_lookup(P8, ctypes.c_void_p(4100), P8, 4, 32, 3, None) != 0 and "16-byte aligned" in err()


def test_the_ops_refuse_cpu_tensors_and_bad_arguments():
    from hipops import ops
    lab = torch.zeros(1, 24, 40, dtype=torch.uint8)
    for call in (lambda: ops.cell_labels(lab, 3, 5, 2), lambda: ops.cells_changed(lab, lab, 3, 5),
                 lambda: ops.embedding_lookup(torch.zeros(1, 3, dtype=torch.long), torch.zeros(2, 32))):
        with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):
            call()

    class OnDevice(torch.Tensor):          # claims to live on the device: the checks behind _dev run, no kernel is reached
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)  # noqa: E731
    with pytest.raises(RuntimeError, match="torch.uint8, torch.int32 or torch.long"):
        ops.cell_labels(dev(lab.float()), 3, 5, 2)
    with pytest.raises(RuntimeError, match=r"\(B, H, W\) or \(B, 1, H, W\)"):
        ops.cell_labels(dev(lab[0]), 3, 5, 2)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.cell_labels(dev(lab.transpose(1, 2)), 5, 3, 2)
    with pytest.raises(RuntimeError, match="multiples of the cell grid"):
        ops.cell_labels(dev(lab), 5, 5, 2)
    with pytest.raises(RuntimeError, match=r"n_labels=257 must lie in \[1, 256\]"):
        ops.cell_labels(dev(lab), 3, 5, 257)
    with pytest.raises(RuntimeError, match="one dtype and shape"):
        ops.cells_changed(dev(lab), dev(lab.long()), 3, 5)
    with pytest.raises(RuntimeError, match="one dtype and shape"):
        ops.cells_changed(dev(lab), dev(lab[:, :12]), 3, 5)
    with pytest.raises(RuntimeError, match="must be torch.long"):
        ops.embedding_lookup(dev(torch.zeros(1, 3, dtype=torch.int32)), dev(torch.zeros(2, 32)))
    with pytest.raises(RuntimeError, match=r"idx \(B, T\) and table \(L, E\)"):
        ops.embedding_lookup(dev(torch.zeros(3, dtype=torch.long)), dev(torch.zeros(2, 32)))


# ------------------------------------------------------------------------------------------------ the modules
def test_label_condition_keys_and_refusals():
    from networks import GPT, LabelCondition
    torch.manual_seed(0)
    cond = LabelCondition(3, 64, 3, 5)
    assert list(cond.state_dict()) == ["embed.weight"] and cond.embed.weight.shape == (3, 64)
    assert [n for n, _ in cond.named_parameters()] == ["embed.weight"]
    big = LabelCondition(256, 512, 16, 16).embed.weight
    assert abs(float(big.detach().std()) - 0.02) < 1e-3 and abs(float(big.detach().mean())) < 1e-3          # N(0, 0.02), as the GPT's embeddings
    gpt = GPT(vocab_size=16, block_size=30, n_layer=1, n_head=2, n_embed=64, n_unmasked=15)
    assert not any("cond" in k for k in gpt.state_dict())          # the table lives outside the GPT
    for bad, msg in (((0, 64, 3, 5), "n_labels=0"), ((257, 64, 3, 5), "n_labels=257"), ((3, 30, 3, 5), "n_embed=30"), ((3, 64, 0, 5), "h=0")):
        with pytest.raises(ValueError, match=msg):
            LabelCondition(*bad)
    with pytest.raises(ValueError, match=r"tokens \(B, h w\) = \(B, 15\)"):
        cond(torch.zeros(2, 16, dtype=torch.long))
    with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):
        cond(torch.zeros(2, 15, dtype=torch.long))
    with pytest.raises(ValueError, match="n_tail=4"):
        gpt.forward_tail(torch.zeros(1, 3, dtype=torch.long), n_tail=4)


def test_conditional_trainer_refuses_at_construction():
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer, PriorTrainer
    vqgan = lambda: VQGAN(**dict(P.TINY_VQGAN, dict_size=16))  # noqa: E731
    gpt = lambda **kw: GPT(**dict(C.GPT_KW, **kw))  # noqa: E731
    cond = lambda *a: LabelCondition(*(a or (C.L, C.E, C.LAT_H, C.LAT_W)))  # noqa: E731
    assert issubclass(ConditionalPriorTrainer, PriorTrainer)
    with pytest.raises(TypeError, match="networks.LabelCondition"):
        ConditionalPriorTrainer(vqgan(), gpt(), torch.nn.Embedding(3, 64), device="cpu")
    with pytest.raises(ValueError, match="n_embed=32 must equal the GPT's n_embed=64"):
        ConditionalPriorTrainer(vqgan(), gpt(), cond(3, 32, 3, 5), device="cpu")
    with pytest.raises(ValueError, match=r"block_size=29 must be at least Tc \+ T = 2 h w = 30"):
        ConditionalPriorTrainer(vqgan(), gpt(block_size=29), cond(), device="cpu")
    with pytest.raises(ValueError, match="n_unmasked=0 must be Tc = h w = 15"):
        ConditionalPriorTrainer(vqgan(), gpt(n_unmasked=0), cond(), device="cpu")
    with pytest.raises(ValueError, match="n_unmasked=14 must be Tc = h w = 15"):
        ConditionalPriorTrainer(vqgan(), gpt(n_unmasked=14), cond(), device="cpu")
    with pytest.raises(ValueError, match="vocab_size=16 must equal the VQGAN's dict_size=64"):          # the parent's checks stand
        ConditionalPriorTrainer(VQGAN(**P.TINY_VQGAN), gpt(), cond(), device="cpu")
    with pytest.raises(ValueError, match="pkeep"):
        ConditionalPriorTrainer(vqgan(), gpt(), cond(), pkeep=1.5, device="cpu")


# ------------------------------------------------------------------------------------------------ the config and the launcher
COND = dict(source="label", n_labels=2, labels={"synthetic": dict(n=2, radius=5, contrast=0.8)})
SYNTH = dict(n_slices=2, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, discs=[[16, 16, 5, 1]])


def _raw(tmp_path, cond=COND, synth=SYNTH, **run):
    raw = P.prior_run_config(tmp_path / "out", **dict(dict(resume_checkpoint="prior.ckpt"), **run))
    if cond is not None:
        raw["model"]["prior"]["cond"] = cond if cond is False else dict(cond)
    if synth is not None:
        raw["synth"] = dict(synth)
    return raw


def _args(**kw):
    a = dict(config="x.json", mode="synth", multiwindow=False, vqgan=False, prior=True, rank=None, seed=None)
    a.update(kw)
    return argparse.Namespace(**a)


def test_prior_condition_and_configure_prior(tmp_path):
    from utils import load_json
    from trainers import configure_prior, prior_condition
    from trainers.config import PRIOR_KEYS
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    assert PRIOR_KEYS == ("n_layer", "n_head", "n_embed", "n_unmasked", "pkeep", "sos_token")
    assert prior_condition(cfg(_raw(tmp_path, cond=None))) is None and prior_condition(cfg(_raw(tmp_path, cond=False))) is None
    assert prior_condition(cfg(_raw(tmp_path))) == dict(n_labels=2, label_modality=None, lesions=dict(n=2, radius=5, contrast=0.8))
    assert prior_condition(cfg(_raw(tmp_path, cond=dict(COND, labels="seg")))) == dict(n_labels=2, label_modality="seg", lesions=None)
    with pytest.raises(NotImplementedError, match=r"model\.prior\.cond\.\{source, n_labels, labels\}; missing: n_labels$"):
        prior_condition(cfg(_raw(tmp_path, cond={k: v for k, v in COND.items() if k != "n_labels"})))
    with pytest.raises(NotImplementedError, match="source is 'label'"):
        prior_condition(cfg(_raw(tmp_path, cond=dict(COND, source="class"))))
    with pytest.raises(ValueError, match="n_labels=300"):
        prior_condition(cfg(_raw(tmp_path, cond=dict(COND, n_labels=300))))
    with pytest.raises(NotImplementedError, match="missing: model.prior.cond.labels.synthetic.radius"):
        prior_condition(cfg(_raw(tmp_path, cond=dict(COND, labels={"synthetic": dict(n=2, contrast=0.8)}))))
    with pytest.raises(NotImplementedError, match="missing: model.prior.cond.labels$"):
        prior_condition(cfg(_raw(tmp_path, cond=dict(COND, labels=False))))
    plain = configure_prior(cfg(_raw(tmp_path, cond=None)))          # as it was: the latent's 16 x 16 positions, the causal mask
    assert plain.block_size == 256 and plain.config.n_unmasked == 0
    gpt = configure_prior(cfg(_raw(tmp_path)))
    assert gpt.block_size == 512 and gpt.config.n_unmasked == 256
    raw = _raw(tmp_path)
    raw["model"]["prior"]["n_unmasked"] = 256
    assert configure_prior(cfg(raw)).config.n_unmasked == 256
    raw["model"]["prior"]["n_unmasked"] = 5
    with pytest.raises(ValueError, match="n_unmasked=5 with model.prior.cond"):
        configure_prior(cfg(raw))


def test_check_synth_config_names_what_is_missing(tmp_path):
    from utils import load_json
    from trainers import check_synth_config
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    check_synth_config(cfg(_raw(tmp_path)))
    check_synth_config(cfg(_raw(tmp_path, synth=dict(SYNTH, discs=False))))
    for key in SYNTH:
        with pytest.raises(NotImplementedError, match=r"synth\.\{.*\}; missing: synth\.%s$" % key):
            check_synth_config(cfg(_raw(tmp_path, synth={k: v for k, v in SYNTH.items() if k != key})))
    with pytest.raises(NotImplementedError, match="missing: synth.n_slices, synth.n_candidates"):
        check_synth_config(cfg(_raw(tmp_path, synth=None)))
    with pytest.raises(NotImplementedError, match="missing: model.prior.cond$"):
        check_synth_config(cfg(_raw(tmp_path, cond=None)))
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        check_synth_config(cfg(_raw(tmp_path, resume_checkpoint=False)))
    with pytest.raises(ValueError, match=r"synth\.discs is false or a list of \[cy, cx, radius, value\]"):
        check_synth_config(cfg(_raw(tmp_path, synth=dict(SYNTH, discs=[[1, 2, 3]]))))
    raw = _raw(tmp_path)
    del raw["model"]["prior"]["pkeep"]
    with pytest.raises(NotImplementedError, match=r"model\.prior.*missing: pkeep"):          # check_prior_config's keys come first
        check_synth_config(cfg(raw))


def test_launcher_accepts_synth_and_keeps_its_other_paths(tmp_path):
    import importlib
    from utils import load_json
    rv = importlib.import_module("run_vqwnet")
    cfg = lambda raw: load_json(write_config(tmp_path / "c.json", raw))  # noqa: E731
    assert rv.build_parser().parse_args(["-c", "x.json", "-p", "-m", "synth"]).mode == "synth"
    assert rv.check_arguments(cfg(_raw(tmp_path)), _args()) == ("second_step", 1)
    with pytest.raises(ValueError, match="-m synth: .* needs -p"):
        rv.check_arguments(cfg(_raw(tmp_path)), _args(prior=False))
    with pytest.raises(NotImplementedError, match="missing: model.prior.cond$"):
        rv.check_arguments(cfg(_raw(tmp_path, cond=None)), _args())
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        rv.check_arguments(cfg(_raw(tmp_path, resume_checkpoint=False)), _args())
    with pytest.raises(NotImplementedError, match=r"missing: synth\.discs$"):
        rv.check_arguments(cfg(_raw(tmp_path, synth={k: v for k, v in SYNTH.items() if k != "discs"})), _args())
    # the unknown-mode message keeps its pinned wording and names the new mode
    with pytest.raises(ValueError, match="'train' or 'test'") as e:
        rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="fit"))
    assert "'synth'" in str(e.value) and "'edit'" in str(e.value) and "'detect'" in str(e.value)
    # the argument paths there were give what they gave
    plain = _raw(tmp_path, cond=None, synth=None)
    assert rv.check_arguments(cfg(plain), _args(mode="train")) == ("second_step", 1)
    assert rv.check_arguments(cfg(_raw(tmp_path)), _args(mode="train")) == ("second_step", 1)          # -p with a condition trains
    edit = dict(plain, edit=dict(n_slices=1, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=1, box=[0, 8, 0, 8]))
    assert rv.check_arguments(cfg(edit), _args(mode="edit")) == ("second_step", 1)
    detect = dict(n_slices=0, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=5, nll_threshold=2.0, sigma=1.0, against="image",
                  weight="mask", labels=False)
    assert rv.check_arguments(cfg(dict(plain, detect=detect)), _args(mode="detect")) == ("second_step", 1)
    with pytest.raises(NotImplementedError, match="-m detect with model.prior.cond"):
        rv.check_arguments(cfg(dict(_raw(tmp_path), detect=detect)), _args(mode="detect"))
    with pytest.raises(ValueError, match="-m edit: .* needs -p"):
        rv.check_arguments(cfg(edit), _args(mode="edit", prior=False))
    with pytest.raises(ValueError, match="-p: the prior trainer has no test step"):
        rv.check_arguments(cfg(plain), _args(mode="test"))
    with pytest.raises(ValueError, match="data-parallel training of the prior is not built"):
        rv.check_arguments(cfg(_raw(tmp_path, num_gpus=2)), _args())
    assert "-m synth" in rv.__doc__


def test_committed_cond_configs_parse():
    from utils import load_json
    from trainers import check_prior_config, check_synth_config, prior_condition
    from trainers.config import latent_size
    train, synth = (os.path.join(ROOT, "configs", n) for n in ("prior_vqgan_512_cond.json", "prior_vqgan_512_cond_synth.json"))
    for path in (train, synth):
        c = load_json(path)
        check_prior_config(c)
        cond = prior_condition(c)
        assert cond["n_labels"] == 2 and cond["label_modality"] is None and set(cond["lesions"]) == {"n", "radius", "contrast"}
        assert c.dataset.dataset_name == "synthetic" and latent_size(c) == 16
        assert os.path.basename(path) in open(os.path.join(ROOT, "configs", "README.md")).read()
    raw = json.load(open(train))
    assert raw["run"]["resume_checkpoint"] is False and "synth" not in raw          # trains from scratch as committed
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        check_synth_config(load_json(train))
    check_synth_config(load_json(synth))
    assert set(json.load(open(synth))["synth"]) == set(SYNTH)
