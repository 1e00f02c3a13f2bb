"""CPU-side checks of classifier-free guidance for the conditional code prior (no GPU): the restatement
(tests/cond_guidance_ref.py) - the mix and its double-rounding flag on every seeded input the GPU tests use, the tie case's exactness,
the per-sample drop against tests/dropout_ref.py's integer functions - the C ABI of vqw_sample_guided and vqw_embed_lookup_drop with
their refusals before any launch, networks.LabelCondition's null embedding, the refusals of GPT.generate_masked, of
trainers.ConditionalPriorTrainer and of the config keys, and that absent keys build what they built before."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from run_helpers import ROOT, write_config
import cond_guidance_ref as CG
import cond_prior_ref as C
import dropout_ref as DR
import prior_ref as P
from test_cond_prior_host import COND, SYNTH, _raw

NEW_SYMBOLS = ("vqw_sample_guided", "vqw_embed_lookup_drop")


# ------------------------------------------------------------------------------------------------ the mix
def test_mix_ref_by_hand_and_its_flag():
    z, flag = CG.mix_ref(np.float32([1.0, 2.0, -3.0]), np.float32([0.5, 2.0, 1.0]), 3.0)
    assert z.dtype == np.float32 and z.tolist() == [2.0, 2.0, -11.0] and not flag.any()
    z0, _ = CG.mix_ref(np.float32([1.25]), np.float32([-7.5]), 0.0)
    assert z0.tolist() == [-7.5]          # scale 0: the unconditional row
    # a sum that lies exactly on a float32 tie but is exact in double is not flagged: both roundings are the same round-half-even
    z, flag = CG.mix_ref(np.float32([1.0 + 2.0 ** -24 * 0 + 2.0 ** -1]), np.float32([2.0 ** 24]), 1.0)
    assert not flag.any()


def test_no_seeded_input_of_the_gpu_tests_is_flagged():
    """A condition on the inputs: where the double sum of the restatement is inexact AND on a float32 tie, float32(double sum) could
    differ from the kernel's fused multiply-add.  No element of any seeded input may be such an element."""
    n = 0
    for V in CG.GUIDED_V:
        for B in CG.GUIDED_B:
            zc, zu, _ = CG.guided_inputs(V, B)
            for scale in CG.GUIDED_SCALES:
                z, flag = CG.mix_ref(zc.numpy(), zu.numpy(), scale)
                assert not flag.any(), (V, B, scale, int(flag.sum()))
                assert np.isfinite(z).all()
                n += z.size
    zc, zu, mixed = CG.tie_inputs()
    z, flag = CG.mix_ref(zc.numpy(), zu.numpy(), CG.TIE_SCALE)
    assert not flag.any() and np.array_equal(z.astype(np.float64), mixed), "the tie case is exact: the mixed values are the built ones"
    assert n > 30000


def test_the_tie_case_holds_what_it_promises():
    zc, zu, mixed = CG.tie_inputs()
    grid = lambda t: np.array_equal(np.round(t.numpy().astype(np.float64) * 1024), t.numpy().astype(np.float64) * 1024)  # noqa: E731
    assert grid(zc) and grid(zu) and float(zc.abs().max()) <= 16 and float(zu.abs().max()) <= 16
    assert CG.TIE_SCALE == 2.0          # dyadic
    for r in range(2):
        for value, count in ((3.0, 3), (1.0, 2)):
            cols = np.flatnonzero(mixed[r] == value)
            assert len(cols) == count
            pairs = {(float(zc[r, c]), float(zu[r, c])) for c in cols}
            assert len(pairs) == count, "different (zc, zu) pairs behind one mixed value"
    # the thresholds the GPU test uses fall where the docstring says: strictly-greater masses relative to the total
    p = np.exp(mixed[0] - mixed[0].max())
    g3, g1 = p[mixed[0] > 3].sum() / p.sum(), p[mixed[0] > 1].sum() / p.sum()
    assert 0.3 < g3 < 0.9 < g1 < 0.98


# ------------------------------------------------------------------------------------------------ the drop
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropped_share_is_binomial(p):
    B = 4096
    for seed, call in ((0, 0), (CG.DROP_SEED, 3), (-5, 2 ** 40)):
        drop = CG.dropped_ref(B, p, seed, call)
        assert drop.dtype == np.bool_ and drop.shape == (B,)
        if p == 0:
            assert not drop.any(), "p = 0 drops nobody"
        else:
            assert abs(int(drop.sum()) - p * B) <= 4 * (B * p * (1 - p)) ** 0.5, (p, seed, call, int(drop.sum()))
    a, b = CG.dropped_ref(B, 0.5, 1, 0), CG.dropped_ref(B, 0.5, 1, 1)
    assert (a != b).any() and np.array_equal(a, CG.dropped_ref(B, 0.5, 1, 0)), "a function of (seed, call) alone"


def test_the_drop_site_is_outside_the_gpts_sites():
    from hipops import ops
    from networks import GPT
    assert CG.COND_DROP_SITE == ops.COND_DROP_SITE == -1
    src = open(os.path.join(ROOT, "medical-image-editing_amd", "csrc", "cond.hip")).read()
    assert "#define COND_DROP_SITE (-1)" in src
    gpt = GPT(**dict(C.GPT_KW, emb_pdrop=0.1, res_pdrop=0.1, att_pdrop=0.1))
    assert gpt._seed_sites(1, 0) == 1 + 3 * C.N_LAYER and gpt.dropout_site == 0, "GPT.seed_dropout numbers its sites from 0 upwards"
    # the restated sample draw is element b of an element-wise site: dropout_ref.keep_mask under site -1
    assert np.array_equal(CG.dropped_ref(64, 0.5, 9, 4), ~DR.keep_mask(64, 0.5, 9, 4, -1))


def test_lookup_drop_ref_by_hand():
    idx = torch.tensor([[0, 1], [2, 0], [1, 1]])
    table = torch.arange(16.0).reshape(4, 4)
    out, eff = CG.lookup_drop_ref(idx, table, 3, 0.0, 1, 0)
    assert torch.equal(eff, idx) and torch.equal(out, table[idx])
    seen = set()
    for call in range(16):
        out, eff = CG.lookup_drop_ref(idx, table, 3, 0.5, 1, call)
        drop = CG.dropped_ref(3, 0.5, 1, call)
        for b in range(3):
            assert torch.equal(eff[b], torch.full((2,), 3) if drop[b] else idx[b]), "every row of a dropped sample reads the null row"
        assert torch.equal(out, table[eff])
        seen.add(tuple(drop.tolist()))
    assert len(seen) > 2


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_signatures_and_schemas():
    from hipops import _lib, library
    hdr = open(os.path.join(ROOT, "include", "vqwnet_hip.h")).read()
    assert _lib.ABI_VERSION == 9          # functions added only
    ops_ = library.register()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr and s in _lib.SIGNATURES and s in ops_, s
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES["vqw_sample_guided"] == (ctypes.c_int, [p, p, p, p, p, p, i, i, f, f, i, f, p])
    assert _lib.SIGNATURES["vqw_embed_lookup_drop"] == (ctypes.c_int, [p, p, p, p, l, i, i, i, l, f, l, l, p])
    sch = str(torch.ops.vqw.sample_guided.default._schema)
    assert "Tensor? logits" in sch and "Tensor(a!)? out" in sch and "Tensor(b!)? logp" in sch and "Tensor(c!)? logp_u" in sch and "float scale" in sch
    sch = str(torch.ops.vqw.embed_lookup_drop.default._schema)
    assert "Tensor? idx" in sch and "Tensor(a!)? out" in sch and "Tensor(b!)? eff" in sch and "int null_index" in sch and "float p" in sch


def test_the_c_entry_points_refuse_before_any_launch():
    from hipops import _lib
    L = _lib.load()
    P8 = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused by its argument check
    f = ctypes.c_float

    def err():
        return L.vqw_last_error().decode()

    def guided(logits=P8, u=P8, out=P8, B=2, V=16, scale=3.0, temperature=1.0, top_k=0, top_p=1.0):
        return L.vqw_sample_guided(logits, u, None, out, None, None, B, V, f(scale), f(temperature), top_k, f(top_p), None)
    assert guided(V=0) != 0 and "V=0" in err()
    assert guided(V=65537) != 0 and "V=65537" in err()
    assert guided(B=0) != 0 and "B=0" in err()
    assert guided(temperature=0.0) != 0 and "temperature=0" in err()
    assert guided(top_k=-1) != 0 and "top_k=-1" in err()
    assert guided(top_p=0.0) != 0 and "top_p=0" in err()
    assert guided(scale=-0.5) != 0 and "scale=-0.5" in err()
    assert guided(scale=float("inf")) != 0 and "scale=inf" in err()
    assert guided(scale=float("nan")) != 0 and "scale=nan" in err().lower()
    for null in ("logits", "u", "out"):
        assert guided(**{null: None}) != 0 and "null pointer" in err(), null

    def drop(idx=P8, table=P8, out=P8, eff=P8, rows=12, rps=6, E=32, Lr=4, null=3, p=0.5):
        return L.vqw_embed_lookup_drop(idx, table, out, eff, rows, rps, E, Lr, null, f(p), 1, 0, None)
    assert drop(rows=0) != 0 and "rows=0" in err()
    assert drop(rps=5) != 0 and "rows_per_sample=5" in err()
    assert drop(rps=0) != 0 and "rows_per_sample=0" in err()
    assert drop(E=30) != 0 and "E=30" in err()
    assert drop(Lr=0) != 0 and "L=0" in err()
    assert drop(null=4) != 0 and "null_index=4" in err()
    assert drop(null=-1) != 0 and "null_index=-1" in err()
    assert drop(p=1.0) != 0 and "p=1" in err()
    assert drop(p=-0.1) != 0 and "p=-0.1" in err()
    assert drop(eff=None) != 0 and "null pointer" in err()
    assert drop(table=ctypes.c_void_p(4100)) != 0 and "16-byte aligned" in err()


def test_the_ops_refuse_cpu_tensors_and_bad_arguments():
    from hipops import ops
    z, u = torch.zeros(4, 16), torch.zeros(2)
    with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):
        ops.sample_guided(z, u, 3.0)
    with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):
        ops.embedding_lookup_drop(torch.zeros(2, 3, dtype=torch.long), torch.zeros(4, 32), 3, 0.5, 1, 0)

    class OnDevice(torch.Tensor):          # claims to live on the device: the checks behind _dev run, no kernel is reached
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)  # noqa: E731
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="guidance_scale"):
            ops.sample_guided(dev(z), dev(u), bad)
    with pytest.raises(RuntimeError, match=r"logits \(2B, V\) and u \(B,\)"):
        ops.sample_guided(dev(z), dev(torch.zeros(4)), 3.0)
    with pytest.raises(RuntimeError, match=r"forced \(B,\) = \(2,\)"):
        ops.sample_guided(dev(z), dev(u), 3.0, forced=dev(torch.zeros(4, dtype=torch.long)))
    with pytest.raises(ValueError, match="null_index=4"):
        ops.embedding_lookup_drop(dev(torch.zeros(2, 3, dtype=torch.long)), dev(torch.zeros(4, 32)), 4, 0.5, 1, 0)
    with pytest.raises(ValueError, match=r"p=1.0 must lie in \[0, 1\)"):
        ops.embedding_lookup_drop(dev(torch.zeros(2, 3, dtype=torch.long)), dev(torch.zeros(4, 32)), 3, 1.0, 1, 0)


# ------------------------------------------------------------------------------------------------ the modules
def test_label_condition_null_token_and_the_module_without_it():
    from networks import LabelCondition
    torch.manual_seed(11)
    plain = LabelCondition(3, 64, 3, 5)
    torch.manual_seed(11)
    off = LabelCondition(3, 64, 3, 5, null_token=False)
    assert off.embed.weight.shape == (3, 64) and torch.equal(off.embed.weight, plain.embed.weight), "off: the same shape, the same draws"
    assert off.null_index is None and list(off.state_dict()) == ["embed.weight"]
    # the same bits as the module drew before it knew a null token: nn.Embedding's own draw, then N(0, 0.02)
    torch.manual_seed(11)
    want = torch.nn.Embedding(3, 64)
    torch.nn.init.normal_(want.weight, mean=0.0, std=0.02)
    assert torch.equal(plain.embed.weight, want.weight)
    on = LabelCondition(3, 64, 3, 5, null_token=True)
    assert on.embed.weight.shape == (4, 64) and on.null_index == 3 and on.n_labels == 3 and list(on.state_dict()) == ["embed.weight"]
    with pytest.raises(ValueError, match="null_token"):
        plain.null_prefix(2)
    with pytest.raises(ValueError, match="null_token"):
        plain(torch.zeros(2, 15, dtype=torch.long), drop=(0.5, 1, 0))
    with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):          # past the checks, at the kernel's door
        on.null_prefix(2)
    with pytest.raises(RuntimeError, match="need tensors on a ROCm device"):
        on(torch.zeros(2, 15, dtype=torch.long), drop=(0.5, 1, 0))
    with pytest.raises(ValueError, match=r"tokens \(B, h w\) = \(B, 15\)"):
        on(torch.zeros(2, 16, dtype=torch.long), drop=(0.5, 1, 0))


def test_generate_masked_refuses_bad_guidance_before_any_kernel():
    from networks import GPT
    gpt = GPT(**C.GPT_KW).eval()
    idx, known = torch.zeros(2, 1, dtype=torch.long), torch.zeros(2, C.T, dtype=torch.long)
    mask = np.ones(C.T, dtype=bool)
    emb = torch.zeros(2, C.TC, C.E)
    with pytest.raises(ValueError, match="needs embeddings and uncond_embeddings"):
        gpt.generate_masked(idx, known, mask, embeddings=emb, guidance_scale=3.0)
    with pytest.raises(ValueError, match="needs embeddings and uncond_embeddings"):
        gpt.generate_masked(idx, known, mask, uncond_embeddings=emb, guidance_scale=3.0)
    with pytest.raises(ValueError, match="uncond_embeddings of shape"):
        gpt.generate_masked(idx, known, mask, embeddings=emb, uncond_embeddings=emb[:1], guidance_scale=3.0)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="guidance_scale"):
            gpt.generate_masked(idx, known, mask, embeddings=emb, uncond_embeddings=emb, guidance_scale=bad)
    with pytest.raises(ValueError, match="top_p"):          # what it refused before, it refuses under guidance
        gpt.generate_masked(idx, known, mask, embeddings=emb, uncond_embeddings=emb, guidance_scale=3.0, top_p=1.5)
    with pytest.raises(RuntimeError, match="training mode"):
        gpt.train().generate_masked(idx, known, mask, embeddings=emb, uncond_embeddings=emb, guidance_scale=3.0)


def test_conditional_trainer_refuses_bad_guidance_settings():
    from networks import GPT, VQGAN, LabelCondition
    from trainers import ConditionalPriorTrainer
    vqgan = lambda: VQGAN(**dict(P.TINY_VQGAN, dict_size=16))  # noqa: E731
    gpt = lambda: GPT(**C.GPT_KW)  # noqa: E731
    cond = lambda null: LabelCondition(C.L, C.E, C.LAT_H, C.LAT_W, null_token=null)  # noqa: E731
    with pytest.raises(ValueError, match="p_uncond=0.1 needs a condition with the null embedding.*null_token"):
        ConditionalPriorTrainer(vqgan(), gpt(), cond(False), p_uncond=0.1, cond_drop_seed=1, device="cpu")
    with pytest.raises(ValueError, match="p_uncond=0.1 needs cond_drop_seed"):
        ConditionalPriorTrainer(vqgan(), gpt(), cond(True), p_uncond=0.1, device="cpu")
    with pytest.raises(ValueError, match=r"p_uncond=1.0 must lie in \[0, 1\)"):
        ConditionalPriorTrainer(vqgan(), gpt(), cond(True), p_uncond=1.0, cond_drop_seed=1, device="cpu")
    off = ConditionalPriorTrainer(vqgan(), gpt(), cond(False), device="cpu")
    assert off.p_uncond == 0.0 and off.cond_drop_seed is None and "cond_drop_seed" not in off.state_dict()["extra"]
    cells = torch.zeros(1, C.TC, dtype=torch.long)
    with pytest.raises(ValueError, match="guidance_scale=3.0 needs a prior trained with the null embedding.*null_token"):
        off.synthesize(cond=cells, guidance_scale=3.0)
    with pytest.raises(ValueError, match="guidance_scale=3.0 needs a prior trained with the null embedding.*null_token"):
        off.edit({"ids": torch.zeros(1, C.T, dtype=torch.long), "cond": cells}, mask=np.ones((C.LAT_H, C.LAT_W), bool), guidance_scale=3.0)
    on = ConditionalPriorTrainer(vqgan(), gpt(), cond(True), p_uncond=0.25, cond_drop_seed=7, device="cpu")
    state = on.state_dict()
    assert state["extra"]["cond_drop_seed"] == 7
    for bad in (-2.0, float("nan")):
        with pytest.raises(ValueError, match="guidance_scale"):
            on.synthesize(cond=cells, guidance_scale=bad)
    with pytest.raises(ValueError, match="rank='best'"):
        on.synthesize(cond=cells, guidance_scale=3.0, rank="best")
    with pytest.raises(ValueError, match="rank='gain'.*needs\\s+guidance"):
        on.synthesize(cond=cells, rank="gain")
    other = ConditionalPriorTrainer(vqgan(), gpt(), cond(True), p_uncond=0.25, cond_drop_seed=8, device="cpu")
    with pytest.raises(ValueError, match="cond_drop_seed=7, this trainer has 8"):
        other.load_state_dict(state)


# ------------------------------------------------------------------------------------------------ the config
CFG_COND = dict(COND, null_token=True, p_uncond=0.1, drop_seed=11)


def _cfg(tmp_path, raw):
    from utils import load_json
    return load_json(write_config(tmp_path / "c.json", raw))


def test_the_new_keys_parse_and_absent_keys_mean_off(tmp_path):
    from trainers import check_synth_config, guidance, prior_cond_drop, prior_condition
    from trainers.config import EDIT_KEYS, SYNTH_KEYS, check_edit_config
    assert SYNTH_KEYS == ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed", "discs")          # the required keys stay
    assert EDIT_KEYS == ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed")
    off = _cfg(tmp_path, _raw(tmp_path))
    assert prior_cond_drop(off) == dict(null_token=False, p_uncond=0.0, drop_seed=None) and guidance(off, "synth") == (1.0, "cond")
    assert prior_cond_drop(_cfg(tmp_path, _raw(tmp_path, cond=None))) == dict(null_token=False, p_uncond=0.0, drop_seed=None)
    on = _cfg(tmp_path, _raw(tmp_path, cond=CFG_COND, synth=dict(SYNTH, guidance_scale=3, rank="gain")))
    assert prior_cond_drop(on) == dict(null_token=True, p_uncond=0.1, drop_seed=11) and guidance(on, "synth") == (3.0, "gain")
    assert prior_condition(on) == prior_condition(off), "the condition itself is what it was"
    check_synth_config(on)
    false = _cfg(tmp_path, _raw(tmp_path, cond=dict(COND, null_token=False, p_uncond=False, drop_seed=False),
                                synth=dict(SYNTH, guidance_scale=False, rank=False)))
    assert prior_cond_drop(false) == prior_cond_drop(off) and guidance(false, "synth") == (1.0, "cond")
    for cond, msg in ((dict(COND, p_uncond=0.1, drop_seed=1), r"model\.prior\.cond\.p_uncond=0\.1 .* needs model\.prior\.cond\.null_token"),
                      (dict(COND, null_token=True, p_uncond=0.1), r"model\.prior\.cond\.p_uncond=0\.1 needs model\.prior\.cond\.drop_seed"),
                      (dict(COND, null_token=True, p_uncond=1.0, drop_seed=1), r"model\.prior\.cond\.p_uncond=1\.0"),
                      (dict(COND, null_token=True, p_uncond="x", drop_seed=1), r"model\.prior\.cond\.p_uncond='x'"),
                      (dict(COND, null_token=True, p_uncond=0.1, drop_seed=1.5), r"model\.prior\.cond\.drop_seed=1\.5")):
        with pytest.raises(ValueError, match=msg):
            prior_cond_drop(_cfg(tmp_path, _raw(tmp_path, cond=cond)))
    for synth, msg in ((dict(SYNTH, guidance_scale=-1), r"synth\.guidance_scale=-1"), (dict(SYNTH, guidance_scale="3"), r"synth\.guidance_scale='3'"),
                       (dict(SYNTH, guidance_scale=3, rank="best"), r"synth\.rank='best'"), (dict(SYNTH, rank="gain"), r"synth\.rank='gain'")):
        with pytest.raises(ValueError, match=msg):
            check_synth_config(_cfg(tmp_path, _raw(tmp_path, cond=CFG_COND, synth=synth)))
    with pytest.raises(ValueError, match=r"synth\.guidance_scale=3 needs .*model\.prior\.cond\.null_token"):
        check_synth_config(_cfg(tmp_path, _raw(tmp_path, synth=dict(SYNTH, guidance_scale=3))))
    edit = dict(n_slices=1, n_candidates=2, temperature=1.0, top_k=4, top_p=0.9, seed=1, box=[0, 8, 0, 8])
    raw = dict(_raw(tmp_path, cond=CFG_COND, synth=None), edit=dict(edit, guidance_scale=2.0))
    check_edit_config(_cfg(tmp_path, raw))
    assert guidance(_cfg(tmp_path, raw), "edit") == (2.0, "cond")
    with pytest.raises(ValueError, match=r"edit\.guidance_scale=2 needs .*model\.prior\.cond\.null_token"):
        check_edit_config(_cfg(tmp_path, dict(_raw(tmp_path, cond=None, synth=None), edit=dict(edit, guidance_scale=2.0))))


def test_absent_keys_build_the_trainer_that_was_built(tmp_path):
    from trainers import build_prior_trainer
    raw = _raw(tmp_path, resume_checkpoint=False)
    torch.manual_seed(3)
    tr = build_prior_trainer(_cfg(tmp_path, raw), device="cpu")
    assert tr.cond.embed.weight.shape == (2, 64) and tr.cond.null_index is None and tr.p_uncond == 0.0
    torch.manual_seed(3)
    again = build_prior_trainer(_cfg(tmp_path, _raw(tmp_path, resume_checkpoint=False, cond=dict(COND, null_token=False, p_uncond=0))), device="cpu")
    assert torch.equal(tr.cond.embed.weight, again.cond.embed.weight) and torch.equal(tr.gpt.head.weight, again.gpt.head.weight)
    assert sorted(tr.state_dict()["extra"]) == sorted(again.state_dict()["extra"]) and "cond_drop_seed" not in tr.state_dict()["extra"]
    on = build_prior_trainer(_cfg(tmp_path, _raw(tmp_path, resume_checkpoint=False, cond=CFG_COND)), device="cpu")
    assert on.cond.embed.weight.shape == (3, 64) and on.cond.null_index == 2 and on.p_uncond == 0.1 and on.cond_drop_seed == 11


def test_committed_cfg_config_parses():
    from utils import load_json
    from trainers import check_prior_config, check_synth_config, guidance, prior_cond_drop, prior_condition
    path = os.path.join(ROOT, "configs", "prior_vqgan_512_cond_cfg.json")
    c = load_json(path)
    check_prior_config(c)
    assert prior_condition(c)["n_labels"] == 2
    drop = prior_cond_drop(c)
    assert drop["null_token"] and drop["p_uncond"] == 0.1 and isinstance(drop["drop_seed"], int)
    assert guidance(c, "synth") == (3.0, "cond") or guidance(c, "synth")[0] == 3.0
    raw = json.load(open(path))
    assert set(SYNTH) <= set(raw["synth"]) and raw["synth"]["guidance_scale"] == 3
    assert raw["run"]["resume_checkpoint"] is False          # trains from scratch as committed: -m synth asks for the checkpoint
    with pytest.raises(NotImplementedError, match="missing: run.resume_checkpoint"):
        check_synth_config(c)
    assert os.path.basename(path) in open(os.path.join(ROOT, "configs", "README.md")).read()
