"""Config-driven construction: the reference's config namedtuple (utils.load_json: JSON `false` -> None) to modules,
optimisers, loss and the first-step trainer - TrainerBase.configure_models / configure_optimizers / configure_losses /
set_transform (trainers/base.py:189-237, 164-183, 261-282) with the reference's key names.

    config.run.{num_gpus, training_mode, seed}
    config.model.vqmodel.{in_channels, enc_filters, dec_filters, dict_size, momentum, knn_backend, enc_use_styled_up_block,
                          dec_use_styled_up_block, use_init_embed, use_dropblock, block_size, start_value, stop_value,
                          nr_steps, dropped_skip_layers, use_pixel_shuffle}
    config.loss.{loss_weight.{commit, cross, dist, reg, recon, freq, perceptual}, embed_loss.{margin, use_distance_loss,
                 use_regularization_loss}, use_recon_loss, use_frequency_loss, use_perceptual_loss}
    config.{enc_optim, dec_optim, dis_optim}.{lr, b1, b2, weight_decay}
    config.model.dis.{model_name, n_filters, n_layers, normalization, apply_spectral_norm}, config.loss.{loss_weight.{gen, dis},
                 n_inner_loops, dis_loss_type}, config.run.{first_stage_ckpt_path, discriminator_ckpt_path}   (second_step)
    config.model.dis.{D_ch, D_wide, D_attn, resolution}, config.loss.{loss_weight.{unet_perceptual, cutmix, consistency},
                 use_unet_perceptual_loss, use_l1_loss}                  (second_step with model_name 'UNetDiscriminator')
    config.augmentation.{modules, ...}            (optional: absent -> the exact-integer flip views of the benchmark)
    config.dataset.{window_width, window_center, window_scale}, config.loss.{recon_weights, freq_weights, percep_weights}
                 (multi-window runs, -w); config.loss.clamp_windows (second_step, a key of this project: absent -> true, see
                 trainers/second_step_unet_mw.py)
    config.loss.{perceptual_loss_type, conv_index, perceptual_weights, lpips_weights}   (with use_perceptual_loss)
    config.model.prior.{n_layer, n_head, n_embed, n_unmasked, pkeep, sos_token}, config.prior_optim.{lr, b1, b2, weight_decay,
                 grad_norm_clip, warmup_steps, decay_steps}    (the GPT code prior, -p: keys of this project, the reference has
                 no trainer for its GPT; trainers/prior.py)
    config.model.prior.cond.{source, n_labels, labels} (optional: the prior conditioned on label maps, trainers/cond_prior.py; its
                 optional {null_token, p_uncond, drop_seed} and synth.{guidance_scale, rank} / edit.{guidance_scale, rank}:
                 classifier-free guidance, absent meaning off) and
                 config.synth.{n_slices, n_candidates, temperature, top_k, top_p, seed, discs}, config.run.resume_checkpoint
                 (synthesis from label maps, -p -m synth: keys of this project; Fit.synth)
    config.model.prior.masked.{n_steps, choice_temperature, mask_seed} (optional: the bidirectional masked prior decoded in n_steps
                 parallel passes, trainers/masked_prior.py; absent or `false`: the autoregressive prior.  pkeep and sos_token are
                 ignored with it, model.prior.cond beside it is refused; edit.n_steps overrides n_steps for -p -m edit)
    config.model.prior.masked.cond.{source, n_labels, labels} and its optional {null_token, p_uncond, drop_seed} (optional: the
                 masked prior conditioned on label maps, trainers/masked_cond_prior.py - model.prior.cond's keys, read by
                 prior_condition / prior_cond_drop in its place; synth.n_steps overrides n_steps for -p -m synth)
    config.edit.{n_slices, n_candidates, temperature, top_k, top_p, seed} and one of edit.{box, mask_path, nll_threshold},
                 config.run.resume_checkpoint    (editing with the prior, -p -m edit: keys of this project; Fit.edit)
    config.detect.{n_slices, n_candidates, temperature, top_k, top_p, seed, nll_threshold, sigma, against, weight, labels},
                 config.run.resume_checkpoint    (anomaly detection with the prior, -p -m detect: keys of this project; Fit.detect)
    config.detect.pseudo.{threshold, stride} (optional, with model.prior.masked and detect.nll_threshold false: detection by the
                 masked prior's pseudo-likelihood map, MaskedPriorTrainer.detect_pseudo) and config.edit.pnll_threshold with the
                 optional edit.stride (with model.prior.masked: one more selector of -p -m edit, the same map)
    config.detect.lesionwise.{thresholds, min_size, connectivity} (optional, with detect.labels: lesion-wise scores of the maps,
                 functions.LesionScores; detect_lesionwise)

The focal frequency loss (use_frequency_loss) is functions.FocalFrequencyLoss, built on HIP kernels in place of the
third-party focal-frequency-loss package.  The perceptual loss (use_perceptual_loss with perceptual_loss_type 'vgg', the
reference's VGGLoss()) is functions.VGGLoss on HIP kernels.  The reference downloads its VGG19 weights; this build never
downloads anything, so `config.loss.perceptual_weights` - a key of this project, not of the reference - names a local
file: torchvision's vgg19 state dict (vgg19-dcbb9e9d.pth), a VGGLoss state dict or a reference checkpoint of a run with the
loss on.  Without it a config that switches the loss on raises, as does conv_index '54', which is not built: nothing
silently trains something else.  perceptual_loss_type 'lpips' (the reference's LPIPSLoss(): the lpips package with AlexNet
weights) is functions.LPIPSLoss on HIP kernels, with its weights named by `config.loss.lpips_weights` - again a key of this
project: a path to an LPIPS state dict / reference checkpoint, or a two-element list [alexnet-owt-7be5be79.pth, alex.pth]
(torchvision's AlexNet and the package's weights/v0.1/alex.pth).  Without that key 'lpips' raises in the same way;
`perceptual_weights` stays the VGG19 file's key.
"""
from functions import EmbeddingLoss, FocalFrequencyLoss, LPIPSLoss, VGGLoss
from hipops import Adam
from networks import UNetEncoder, UNetDecoder, RandomTransform, NLayerDiscriminator, UNetDiscriminator
from utils import apply_spectral_norm
from utils.checkpoint import load_first_stage_from_ckpt, load_discriminator_from_ckpt, load_vqgan_from_ckpt

from .first_step import FirstStepTrainer, FlipViews, RandomTransformViews, LossWeights
from .second_step import SecondStepTrainer, GanLossWeights
from .second_step_unet import UNetSecondStepTrainer, UNetGanLossWeights
from .second_step_unet_mw import UNetMultiWindowSecondStepTrainer
from .vqgan_unet_dis import VQGANUNetDisTrainer, VQGANLossWeights
from .evaluation import Evaluator


def _get(cfg, name, default=None):
    return getattr(cfg, name) if hasattr(cfg, name) else default


def configure_models(config):
    """-> (UNetEncoder, UNetDecoder) exactly as base.py:189-237 calls the constructors (`init_embed = not use_init_embed`)."""
    g = config.model.vqmodel
    if _get(g, "model_name") == "VQGAN":
        raise NotImplementedError("model_name 'VQGAN': configure_models builds the U-Net encoder / decoder pair; the VQGAN and "
                                  "its trainer are built by trainers.build_vqgan_trainer (run_vqwnet.py -v)")
    encoder = UNetEncoder(
        in_channels=g.in_channels,
        filters=list(g.enc_filters),
        dict_size=g.dict_size,
        momentum=g.momentum,
        knn_backend=g.knn_backend,
        use_styled_up_block=bool(g.enc_use_styled_up_block),
        num_gpus=config.run.num_gpus,
        init_embed=not g.use_init_embed,
    )
    decoder = UNetDecoder(
        in_channels=g.enc_filters[0],
        out_channels=g.in_channels,
        filters=list(g.dec_filters),
        use_dropblock=bool(g.use_dropblock),
        block_size=g.block_size,
        start_value=g.start_value,
        stop_value=g.stop_value,
        nr_steps=g.nr_steps,
        dropped_skip_layers=list(g.dropped_skip_layers or []),
        use_styled_up_block=bool(g.dec_use_styled_up_block),
        use_pixel_shuffle=bool(g.use_pixel_shuffle),
    )
    return encoder, decoder


_UNET_DIS_KEYS = ("D_ch", "D_wide", "D_attn", "resolution")
VQGAN_KEYS = ("in_channels", "mid_channels", "out_channels", "emb_dim", "dict_size", "enc_ch_multiplier", "dec_ch_multiplier",
              "num_res_blocks", "enc_attn_resolutions", "dec_attn_resolutions", "resolution", "p_dropout", "resamp_with_conv",
              "knn_backend")


def check_vqgan_config(config):
    """NotImplementedError unless the config describes the VQGAN trainer's model: model.vqmodel.model_name 'VQGAN' and the
    fourteen keys of model.vqgan (no device work: the launcher calls it before anything else)."""
    name = _get(_get(config.model, "vqmodel"), "model_name")
    section = _get(config.model, "vqgan")
    missing = [k for k in VQGAN_KEYS if section is None or not hasattr(section, k)]
    if name != "VQGAN" or missing:
        raise NotImplementedError("the VQGAN trainer (run_vqwnet.py -v, trainers.build_vqgan_trainer) needs model.vqmodel.model_name "
                                  "'VQGAN' (got %r) and model.vqgan.{%s}, as the reference's constructor call does (base.py:204-222); "
                                  "missing: %s" % (name, ", ".join(VQGAN_KEYS), ", ".join(missing) or "none"))


def configure_vqgan(config):
    """The VQGAN autoencoder of config.model.vqgan (reference: trainers/base.py:204-222, the same fourteen keys)."""
    from networks import VQGAN
    c = config.model.vqgan
    return VQGAN(in_channels=c.in_channels, mid_channels=c.mid_channels, out_channels=c.out_channels, emb_dim=c.emb_dim,
                 dict_size=c.dict_size, enc_ch_multiplier=c.enc_ch_multiplier, dec_ch_multiplier=c.dec_ch_multiplier,
                 num_res_blocks=c.num_res_blocks, enc_attn_resolutions=c.enc_attn_resolutions,
                 dec_attn_resolutions=c.dec_attn_resolutions, resolution=c.resolution, p_dropout=c.p_dropout,
                 resamp_with_conv=c.resamp_with_conv, knn_backend=c.knn_backend)


PRIOR_KEYS = ("n_layer", "n_head", "n_embed", "n_unmasked", "pkeep", "sos_token")
PRIOR_OPTIM_KEYS = ("lr", "b1", "b2", "weight_decay", "grad_norm_clip", "warmup_steps", "decay_steps")


def check_prior_config(config):
    """NotImplementedError unless the config describes the prior trainer's models and optimiser: check_vqgan_config's keys (the
    first stage whose codes are modelled), the six keys of model.prior and the seven of prior_optim (no device work: the launcher
    calls it before anything else)."""
    check_vqgan_config(config)
    for where, section, keys in (("model.prior", _get(config.model, "prior"), PRIOR_KEYS),
                                 ("prior_optim", _get(config, "prior_optim"), PRIOR_OPTIM_KEYS)):
        missing = [k for k in keys if section is None or not hasattr(section, k)]
        if missing:
            raise NotImplementedError("the prior trainer (run_vqwnet.py -p, trainers.build_prior_trainer) needs %s.{%s}; missing: %s"
                                      % (where, ", ".join(keys), ", ".join(missing)))
    if prior_masked(config) is not None:          # the optional model.prior.masked: its keys and what it excludes
        prior_condition(config)                   # and its optional condition, model.prior.masked.cond: missing keys are named here
        prior_cond_drop(config)


MASKED_KEYS = ("n_steps", "choice_temperature", "mask_seed")


def prior_masked(config):
    """The optional model.prior.masked = {"n_steps", "choice_temperature", "mask_seed"} -> None (absent or `false`: the
    autoregressive prior, exactly as without the key) or {n_steps, choice_temperature, mask_seed}: the bidirectional masked prior
    (trainers/masked_prior.py).  model.prior.{pkeep, sos_token} are ignored with it; model.prior.cond beside it raises: its
    condition is the optional model.prior.masked.cond (prior_condition)."""
    masked = _get(_get(config.model, "prior"), "masked")
    if masked is None or masked is False:
        return None
    what = "the masked prior (run_vqwnet.py -p with model.prior.masked)"
    missing = [k for k in MASKED_KEYS if not hasattr(masked, k)]
    if missing:
        raise NotImplementedError("%s needs model.prior.masked.{%s}; missing: %s" % (what, ", ".join(MASKED_KEYS), ", ".join(missing)))
    cond = _get(config.model.prior, "cond")
    if cond is not None and cond is not False:
        raise NotImplementedError("%s: model.prior.cond beside model.prior.masked - model.prior.cond is the autoregressive prior's "
                                  "conditioning prefix; the masked prior is conditioned on label maps by model.prior.masked.cond" % what)
    n_steps, tau, seed = masked.n_steps, masked.choice_temperature, masked.mask_seed
    if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
        raise ValueError("%s: model.prior.masked.n_steps=%r must be an integer >= 1" % (what, n_steps))
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 <= float(tau) < float("inf"):
        raise ValueError("%s: model.prior.masked.choice_temperature=%r must be a finite number >= 0" % (what, tau))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError("%s: model.prior.masked.mask_seed=%r must be an integer" % (what, seed))
    return {"n_steps": n_steps, "choice_temperature": float(tau), "mask_seed": seed}


EDIT_KEYS = ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed")
EDIT_SELECTORS = ("box", "mask_path", "nll_threshold")


def check_edit_config(config):
    """NotImplementedError unless the config describes an editing run (run_vqwnet.py -p -m edit): check_prior_config's keys,
    run.resume_checkpoint (the -p checkpoint whose prior edits), the six keys of the `edit` section and exactly one selector
    among edit.{box, mask_path, nll_threshold} (a JSON `false` is no selector).  No device work."""
    check_prior_config(config)
    if not _get(config.run, "resume_checkpoint"):
        raise NotImplementedError("editing with the prior (run_vqwnet.py -p -m edit) needs run.resume_checkpoint, the -p checkpoint "
                                  "of the prior; missing: run.resume_checkpoint")
    section = _get(config, "edit")
    missing = [k for k in EDIT_KEYS if section is None or not hasattr(section, k)]
    if missing:
        raise NotImplementedError("editing with the prior (run_vqwnet.py -p -m edit) needs edit.{%s}; missing: %s"
                                  % (", ".join(EDIT_KEYS), ", ".join(missing)))
    given = [k for k in EDIT_SELECTORS if _get(section, k) is not None]
    selectors = EDIT_SELECTORS
    if prior_masked(config) is not None:          # the masked prior's own selector, edit.pnll_threshold, counts among them
        selectors = EDIT_SELECTORS + ("pnll_threshold",)
        given += ["pnll_threshold"] if edit_pnll(config) is not None else []
    else:
        edit_pnll(config)                         # refused without model.prior.masked
    if len(given) != 1:
        raise NotImplementedError("editing with the prior (run_vqwnet.py -p -m edit) needs exactly one of edit.{%s}; given: %s"
                                  % (", ".join(selectors), ", ".join(given) or "none"))
    guidance(config, "edit")          # the optional edit.{guidance_scale, rank}
    edit_n_steps(config)              # the optional edit.n_steps of the masked prior
    blend(config, "edit")             # the optional edit.{blend, blend_levels, blend_source}


BLEND_MODES, BLEND_SOURCES, BLEND_MAX_LEVELS, BLEND_DEFAULT_LEVELS = ("paste", "pyramid"), ("edit", "delta"), 12, 3


def default_blend_levels(fy, fx):
    """The pyramid depth of a blended composite when none is given: min(3, the largest L with 2^L dividing both sides fy = H / h and
    fx = W / w of a latent cell in pixels) - the mixing zone of the lowest band stays within a cell or so.  0 (a cell of odd size
    has no pyramid) raises ValueError."""
    fy, fx = int(fy), int(fx)
    if fy < 1 or fx < 1:
        raise ValueError("blend: a latent cell of %d x %d pixels" % (fy, fx))
    levels = 0
    while levels < BLEND_DEFAULT_LEVELS and fy % (2 << levels) == 0 and fx % (2 << levels) == 0:
        levels += 1
    if levels == 0:
        raise ValueError("blend='pyramid': a latent cell of %d x %d pixels has an odd side and no pyramid; there is no default "
                         "blend_levels for it" % (fy, fx))
    return levels


def check_blend(blend, blend_levels, blend_source, where=""):
    """The three blending values of an edit -> (blend, blend_levels, blend_source) normalised, ValueError otherwise.  blend: None
    (or `false`) and 'paste' - the hard per-cell paste, ops.paste_cells - or 'pyramid', ops.blend_cells; blend_levels: None (or
    `false`: default_blend_levels) or an integer in [1, 12]; blend_source: 'edit' (d = edit - image) or 'delta' (d = edit - recon,
    the difference of two decodes).  `where`: the prefix of the names in the messages.  No device work."""
    names = tuple(where + k for k in ("blend", "blend_levels", "blend_source"))
    blend = None if blend is None or blend is False else blend
    if blend is not None and (not isinstance(blend, str) or blend not in BLEND_MODES):
        raise ValueError("%s=%r is None, 'paste' or 'pyramid'" % (names[0], blend))
    levels = None if blend_levels is None or blend_levels is False else blend_levels
    if levels is not None and (isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= BLEND_MAX_LEVELS):
        raise ValueError("%s=%r must be an integer in [1, %d]" % (names[1], blend_levels, BLEND_MAX_LEVELS))
    source = "edit" if blend_source is None or blend_source is False else blend_source
    if not isinstance(source, str) or source not in BLEND_SOURCES:
        raise ValueError("%s=%r is 'edit' or 'delta'" % (names[2], blend_source))
    return blend, levels, source


def blend(config, name):
    """The three optional blending keys of the `edit` or `synth` section `name` -> {blend, blend_levels, blend_source}, the keywords
    of the trainers' edit(); absent (or `false`) means off: the hard paste, default levels, source 'edit'.  No device work."""
    section = _get(config, name)
    mode, levels, source = check_blend(_get(section, "blend"), _get(section, "blend_levels"), _get(section, "blend_source"), where=name + ".")
    return {"blend": mode, "blend_levels": levels, "blend_source": source}


def _stride(stride, where):
    """A lattice stride [sy, sx] of a config -> (sy, sx): two integers >= 1 (the latent grid bounds them from above: the trainer)."""
    ok = isinstance(stride, (list, tuple)) and len(stride) == 2 and all(
        isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in stride)
    if not ok:
        raise ValueError("%s=%r must be [sy, sx], two integers >= 1" % (where, stride))
    return int(stride[0]), int(stride[1])


def _threshold(value, where):
    """A pseudo-likelihood threshold of a config -> float: a number, not a boolean."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value:
        raise ValueError("%s=%r must be a number" % (where, value))
    return float(value)


def edit_pnll(config):
    """The optional edit.pnll_threshold with the optional edit.stride -> None (absent or `false`) or (threshold, (sy, sx) or None:
    the trainer's default (2, 2)): the masked prior picks the region itself, the codes whose pseudo-likelihood map
    (MaskedPriorTrainer.pseudo_nll) exceeds the threshold.  Both keys need model.prior.masked; edit.stride needs
    edit.pnll_threshold."""
    section = _get(config, "edit")
    thr, stride = _get(section, "pnll_threshold"), _get(section, "stride")
    has_thr, has_stride = thr is not None and thr is not False, stride is not None and stride is not False
    if (has_thr or has_stride) and prior_masked(config) is None:
        raise ValueError("edit.%s selects by the pseudo-likelihood map of the masked prior and needs model.prior.masked"
                         % ("pnll_threshold" if has_thr else "stride"))
    if has_stride and not has_thr:
        raise ValueError("edit.stride=%r is the lattice of edit.pnll_threshold and needs it" % (stride,))
    if not has_thr:
        return None
    return _threshold(thr, "edit.pnll_threshold"), (_stride(stride, "edit.stride") if has_stride else None)


def edit_n_steps(config):
    """The optional edit.n_steps -> None (absent or `false`: the trainer's model.prior.masked.n_steps) or the number of parallel
    decoding passes of an edit with the masked prior.  It means nothing to the autoregressive prior, which refuses it; the masked
    prior in turn has no likelihood map: edit.nll_threshold is refused with it."""
    section, masked = _get(config, "edit"), prior_masked(config)
    n_steps = _get(section, "n_steps")
    if n_steps is not None and n_steps is not False:
        if masked is None:
            raise ValueError("edit.n_steps=%r is the number of decoding passes of the masked prior and needs model.prior.masked" % (n_steps,))
        if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
            raise ValueError("edit.n_steps=%r must be an integer >= 1" % (n_steps,))
    else:
        n_steps = None
    if masked is not None and _get(section, "nll_threshold") is not None:
        raise NotImplementedError("editing with the masked prior (run_vqwnet.py -p -m edit with model.prior.masked): edit.nll_threshold "
                                  "selects by a raster-order likelihood, which the masked prior does not define; use edit.box or "
                                  "edit.mask_path")
    return n_steps


DETECT_KEYS = ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed", "nll_threshold", "sigma", "against", "weight",
               "labels")
DETECT_AGAINST, DETECT_WEIGHT = ("image", "reconstruction"), ("mask", "none")
DETECT_LESION_KEYS = ("n", "radius", "contrast")


def _labels(labels, what, where):
    """A `labels` entry -> (label_modality or None, synthetic lesions {n, radius, contrast} or None): `false` (no labels), a
    modality name (MICCAIBraTSDataset's sibling files), or {"synthetic": {n, radius, contrast}}."""
    if labels is None or labels is False:
        return None, None
    if isinstance(labels, str):
        return labels, None
    lesions = _get(labels, "synthetic")
    missing = [k for k in DETECT_LESION_KEYS if lesions is None or not hasattr(lesions, k)]
    if missing:
        raise NotImplementedError("%s: %s is false, a modality name or "
                                  "{\"synthetic\": {%s}}; missing: %s" % (what, where, ", ".join(DETECT_LESION_KEYS), ", ".join("%s.synthetic.%s" % (where, k) for k in missing)))
    return None, {k: getattr(lesions, k) for k in DETECT_LESION_KEYS}


def detect_labels(config):
    """config.detect.labels -> (label_modality or None, synthetic lesions {n, radius, contrast} or None): `false` (no labels), a
    modality name (MICCAIBraTSDataset's sibling files), or {"synthetic": {n, radius, contrast}}."""
    return _labels(_get(config.detect, "labels"), "detecting with the prior (run_vqwnet.py -p -m detect)", "detect.labels")


COND_KEYS = ("source", "n_labels", "labels")


def _cond_section(config):
    """(the condition's section, its key): model.prior.masked.cond when model.prior.masked is set (the masked prior's condition,
    trainers/masked_cond_prior.py), else model.prior.cond."""
    prior = _get(config.model, "prior")
    masked = _get(prior, "masked")
    if masked is not None and masked is not False:
        return _get(masked, "cond"), "model.prior.masked.cond"
    return _get(prior, "cond"), "model.prior.cond"


def prior_condition(config):
    """The optional model.prior.cond = {"source": "label", "n_labels": N, "labels": ...} -> None (absent or `false`: the
    unconditional prior) or {n_labels, label_modality, lesions}: the label maps the loaders deliver beside the slices (`labels` in
    detect.labels' two forms) become one conditioning token per latent cell (trainers/cond_prior.py).  With model.prior.masked the
    section is model.prior.masked.cond, the same keys (trainers/masked_cond_prior.py)."""
    cond, key = _cond_section(config)
    if cond is None or cond is False:
        return None
    what = "the conditional prior (run_vqwnet.py -p with %s)" % key
    missing = [k for k in COND_KEYS if not hasattr(cond, k)]
    if missing:
        raise NotImplementedError("%s needs %s.{%s}; missing: %s" % (what, key, ", ".join(COND_KEYS), ", ".join(missing)))
    if cond.source != "label":
        raise NotImplementedError("%s: %s.source is 'label', one token per latent cell from a label map (got %r); other "
                                  "conditions are not built" % (what, key, cond.source))
    if isinstance(cond.n_labels, bool) or not isinstance(cond.n_labels, int) or not 1 <= cond.n_labels <= 256:
        raise ValueError("%s: %s.n_labels=%r must be an integer in [1, 256]" % (what, key, cond.n_labels))
    label_modality, lesions = _labels(cond.labels, what, key + ".labels")
    if label_modality is None and lesions is None:
        raise NotImplementedError("%s needs label maps: %s.labels is a modality name or {\"synthetic\": {%s}}; missing: "
                                  "%s.labels" % (what, key, ", ".join(DETECT_LESION_KEYS), key))
    return {"n_labels": int(cond.n_labels), "label_modality": label_modality, "lesions": lesions}


def prior_cond_drop(config):
    """The three optional classifier-free guidance keys of model.prior.cond -> {null_token, p_uncond, drop_seed}; absent (or
    `false`) means off: no null embedding, p_uncond 0, no seed.  p_uncond > 0 needs null_token and drop_seed.  With
    model.prior.masked they are model.prior.masked.cond's."""
    cond, key = _cond_section(config)
    what = "the conditional prior (run_vqwnet.py -p with %s)" % key
    if cond is None or cond is False:
        return {"null_token": False, "p_uncond": 0.0, "drop_seed": None}
    null_token = bool(_get(cond, "null_token") or False)
    p_uncond = _get(cond, "p_uncond")
    p_uncond = 0.0 if p_uncond is None or p_uncond is False else p_uncond
    if isinstance(p_uncond, bool) or not isinstance(p_uncond, (int, float)) or not 0.0 <= p_uncond < 1.0:
        raise ValueError("%s: %s.p_uncond=%r must be a number in [0, 1)" % (what, key, p_uncond))
    drop_seed = _get(cond, "drop_seed")
    drop_seed = None if drop_seed is None or drop_seed is False else drop_seed
    if drop_seed is not None and (isinstance(drop_seed, bool) or not isinstance(drop_seed, int)):
        raise ValueError("%s: %s.drop_seed=%r must be an integer" % (what, key, drop_seed))
    if p_uncond > 0 and not null_token:
        raise ValueError("%s: %s.p_uncond=%g drops the condition onto the null embedding and needs "
                         "%s.null_token: true" % (what, key, p_uncond, key))
    if p_uncond > 0 and drop_seed is None:
        raise ValueError("%s: %s.p_uncond=%g needs %s.drop_seed, the seed of the dropped samples" % (what, key, p_uncond, key))
    return {"null_token": null_token, "p_uncond": float(p_uncond), "drop_seed": drop_seed}


GUIDANCE_RANKS = ("cond", "gain")


def guidance(config, name):
    """The two optional guidance keys of the `synth` or `edit` section `name` -> (guidance_scale, rank); absent (or `false`) means
    1.0 and 'cond': no guidance, the conditional score ranks.  A scale other than 1 needs model.prior.cond.null_token; rank 'gain'
    needs a scale other than 1.  No device work."""
    section = _get(config, name)
    scale, rank = _get(section, "guidance_scale"), _get(section, "rank")
    scale = 1.0 if scale is None or scale is False else scale
    rank = "cond" if rank is None or rank is False else rank
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (scale == scale and 0.0 <= scale < float("inf")):
        raise ValueError("%s.guidance_scale=%r must be a finite number >= 0 (1: no guidance)" % (name, scale))
    if rank not in GUIDANCE_RANKS:
        raise ValueError("%s.rank=%r is one of %s" % (name, rank, ", ".join(repr(r) for r in GUIDANCE_RANKS)))
    if float(scale) != 1.0:
        if prior_condition(config) is None or not prior_cond_drop(config)["null_token"]:
            raise ValueError("%s.guidance_scale=%g needs a prior trained with the null embedding: %s.null_token: true" % (
                name, scale, _cond_section(config)[1]))
    elif rank == "gain":
        raise ValueError("%s.rank='gain' compares the conditional and the unconditional score and needs %s.guidance_scale other than 1" % (name, name))
    return float(scale), rank


SYNTH_KEYS = ("n_slices", "n_candidates", "temperature", "top_k", "top_p", "seed", "discs")


def check_synth_config(config):
    """NotImplementedError unless the config describes a synthesis run (run_vqwnet.py -p -m synth): check_prior_config's keys,
    model.prior.cond, run.resume_checkpoint (the -p checkpoint of the conditional prior) and the seven keys of the `synth` section;
    synth.discs is `false` or a list of [cy, cx, radius, value] drawn into the label map for edit(new_label=...).  No device work."""
    check_prior_config(config)
    if prior_condition(config) is None:
        raise NotImplementedError("synthesising from label maps (run_vqwnet.py -p -m synth) needs a conditional prior; missing: "
                                  "%s" % _cond_section(config)[1])
    if not _get(config.run, "resume_checkpoint"):
        raise NotImplementedError("synthesising from label maps (run_vqwnet.py -p -m synth) needs run.resume_checkpoint, the -p checkpoint "
                                  "of the conditional prior; missing: run.resume_checkpoint")
    section = _get(config, "synth")
    missing = [k for k in SYNTH_KEYS if section is None or not hasattr(section, k)]
    if missing:
        raise NotImplementedError("synthesising from label maps (run_vqwnet.py -p -m synth) needs synth.{%s}; missing: %s"
                                  % (", ".join(SYNTH_KEYS), ", ".join("synth." + k for k in missing)))
    discs = section.discs
    if discs is not None and discs is not False:
        if not isinstance(discs, (list, tuple)) or any(not isinstance(d, (list, tuple)) or len(d) != 4 for d in discs):
            raise ValueError("synth.discs is false or a list of [cy, cx, radius, value] (got %r)" % (discs,))
    guidance(config, "synth")          # the optional synth.{guidance_scale, rank}
    synth_n_steps(config)              # the optional synth.n_steps of the masked prior
    blend(config, "synth")             # the optional synth.{blend, blend_levels, blend_source} of the edit through the label map


def synth_n_steps(config):
    """The optional synth.n_steps -> None (absent or `false`: the trainer's model.prior.masked.n_steps) or the number of parallel
    decoding passes of a synthesis with the conditional masked prior; the autoregressive prior refuses it (edit_n_steps' rule)."""
    n_steps = _get(_get(config, "synth"), "n_steps")
    if n_steps is None or n_steps is False:
        return None
    if prior_masked(config) is None:
        raise ValueError("synth.n_steps=%r is the number of decoding passes of the masked prior and needs model.prior.masked" % (n_steps,))
    if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
        raise ValueError("synth.n_steps=%r must be an integer >= 1" % (n_steps,))
    return n_steps


DETECT_PSEUDO_KEYS = ("threshold", "stride")


def detect_pseudo(config):
    """The optional detect.pseudo = {"threshold": number, "stride": [sy, sx]} -> None (absent or `false`: detection by token_nll, the
    autoregressive prior's) or {"threshold": float, "stride": (sy, sx)}: detection with the masked prior
    (MaskedPriorTrainer.detect_pseudo restores the codes whose pseudo-likelihood map under the lattice `stride` exceeds `threshold`).
    It needs model.prior.masked and refuses model.prior.masked.cond: a prior that is told where the lesion is cannot detect it."""
    pseudo = _get(_get(config, "detect"), "pseudo")
    if pseudo is None or pseudo is False:
        return None
    what = "detecting with the masked prior (run_vqwnet.py -p -m detect with detect.pseudo)"
    if prior_masked(config) is None:
        raise ValueError("%s: detect.pseudo is the masked prior's pseudo-likelihood selector and needs model.prior.masked; the "
                         "autoregressive prior detects by detect.nll_threshold" % what)
    if prior_condition(config) is not None:
        raise NotImplementedError("%s: detect.pseudo with model.prior.masked.cond - a prior conditioned on the lesion labels is told "
                                  "where the lesion is; detection needs the unconditional masked prior" % what)
    missing = [k for k in DETECT_PSEUDO_KEYS if not hasattr(pseudo, k)]
    if missing:
        raise NotImplementedError("%s needs detect.pseudo.{%s}; missing: %s" % (what, ", ".join(DETECT_PSEUDO_KEYS), ", ".join(missing)))
    return {"threshold": _threshold(pseudo.threshold, "detect.pseudo.threshold"), "stride": _stride(pseudo.stride, "detect.pseudo.stride")}


DETECT_LESIONWISE_KEYS = ("thresholds", "min_size", "connectivity")


def detect_lesionwise(config):
    """The optional detect.lesionwise = {"thresholds": [...], "min_size": int, "connectivity": 4 | 8} -> None (absent or `false`: pixel-wise
    scores only) or {"thresholds": [float, ...], "min_size": int, "connectivity": int}: lesion-wise scores of the maps at every
    threshold (functions.LesionScores: connected components of the thresholded map against those of the labels; Fit.detect writes
    detect_lesions.csv).  Thresholds are finite numbers >= 0, at least one; predicted components smaller than min_size >= 1 pixels
    are dropped.  It needs detect.labels: there is nothing to match without a ground truth."""
    section = _get(_get(config, "detect"), "lesionwise")
    if section is None or section is False:
        return None
    what = "lesion-wise detection scores (run_vqwnet.py -p -m detect with detect.lesionwise)"
    missing = [k for k in DETECT_LESIONWISE_KEYS if not hasattr(section, k)]
    if missing:
        raise NotImplementedError("%s needs detect.lesionwise.{%s}; missing: %s" % (what, ", ".join(DETECT_LESIONWISE_KEYS), ", ".join(missing)))
    thresholds = section.thresholds
    ok = isinstance(thresholds, (list, tuple)) and len(thresholds) >= 1 and all(
        isinstance(t, (int, float)) and not isinstance(t, bool) and t == t and 0 <= t < float("inf") for t in thresholds)
    if not ok:
        raise ValueError("detect.lesionwise.thresholds=%r must be a list of at least one finite number >= 0" % (thresholds,))
    if isinstance(section.min_size, bool) or not isinstance(section.min_size, int) or section.min_size < 1:
        raise ValueError("detect.lesionwise.min_size=%r must be an integer >= 1" % (section.min_size,))
    if isinstance(section.connectivity, bool) or section.connectivity not in (4, 8):
        raise ValueError("detect.lesionwise.connectivity=%r must be 4 or 8" % (section.connectivity,))
    if detect_labels(config) == (None, None):
        raise ValueError("%s matches components against the ground truth and needs detect.labels (a modality name or "
                         "{\"synthetic\": {...}}); detect.labels is false" % what)
    return {"thresholds": [float(t) for t in thresholds], "min_size": int(section.min_size), "connectivity": int(section.connectivity)}


def check_detect_config(config):
    """NotImplementedError unless the config describes a detection run (run_vqwnet.py -p -m detect): check_prior_config's keys,
    run.resume_checkpoint (the -p checkpoint whose prior restores), and the eleven keys of the `detect` section - n_slices (0: the
    whole test split), n_candidates, temperature, top_k, top_p, seed, nll_threshold (a number), sigma, against ('image' or
    'reconstruction'), weight ('mask' or 'none'), labels (detect_labels).  With the optional detect.pseudo (detect_pseudo: the masked
    prior's detection) detect.nll_threshold must be `false` instead.  The optional detect.lesionwise is read by detect_lesionwise.
    No device work."""
    check_prior_config(config)
    if not _get(config.run, "resume_checkpoint"):
        raise NotImplementedError("detecting with the prior (run_vqwnet.py -p -m detect) needs run.resume_checkpoint, the -p checkpoint "
                                  "of the prior; missing: run.resume_checkpoint")
    section = _get(config, "detect")
    missing = [k for k in DETECT_KEYS if section is None or not hasattr(section, k)]
    if missing:
        raise NotImplementedError("detecting with the prior (run_vqwnet.py -p -m detect) needs detect.{%s}; missing: %s"
                                  % (", ".join(DETECT_KEYS), ", ".join(missing)))
    pseudo = detect_pseudo(config)            # the masked prior's detection: detect.pseudo in place of detect.nll_threshold
    if pseudo is not None:
        if section.nll_threshold is not None and section.nll_threshold is not False:
            raise ValueError("detect.nll_threshold=%r beside detect.pseudo: the masked prior restores by its pseudo-likelihood map "
                             "(detect.pseudo.threshold) and defines no token_nll; set detect.nll_threshold to false" % (section.nll_threshold,))
    elif section.nll_threshold is None or isinstance(section.nll_threshold, bool):
        raise NotImplementedError("detecting with the prior (run_vqwnet.py -p -m detect) needs a number for detect.nll_threshold, the "
                                  "token_nll above which a code is restored; missing: detect.nll_threshold")
    for key, allowed in (("against", DETECT_AGAINST), ("weight", DETECT_WEIGHT)):
        if getattr(section, key) not in allowed:
            raise NotImplementedError("detecting with the prior (run_vqwnet.py -p -m detect): detect.%s is one of %s (got %r)"
                                      % (key, ", ".join(repr(a) for a in allowed), getattr(section, key)))
    detect_labels(config)
    detect_lesionwise(config)          # the optional lesion-wise scores


SCORE_KEYS = ("n_slices", "n_samples", "batch_size", "k", "temperature", "top_k", "top_p", "against", "seed", "guidance_scale")
SCORE_AGAINST = ("image", "recon")


def check_score_config(config):
    """NotImplementedError unless the config describes a scoring run (run_vqwnet.py -p -m score): check_prior_config's keys,
    run.resume_checkpoint (the -p checkpoint whose samples are scored) and the ten keys of the `score` section - n_slices (the
    held-out test slices), n_samples (the draws; with model.prior.cond one per slice: equal to n_slices), batch_size, k (the
    neighbour of the manifold scores, 1..8), temperature, top_k, top_p, against ('image' or 'recon'), seed, guidance_scale;
    score.n_steps is added with model.prior.masked.  ValueError for a value out of range: n_samples < k + 1, n_slices < 2 (k + 1) -
    the floor splits the slices into two halves.  Returns the keywords of PriorTrainer.score.  No device work."""
    what = "scoring the prior's samples (run_vqwnet.py -p -m score)"
    check_prior_config(config)
    if not _get(config.run, "resume_checkpoint"):
        raise NotImplementedError("%s needs run.resume_checkpoint, the -p checkpoint of the prior; missing: run.resume_checkpoint" % what)
    section, masked, cond = _get(config, "score"), prior_masked(config), prior_condition(config)
    keys = SCORE_KEYS + (("n_steps",) if masked is not None else ())
    missing = [k for k in keys if section is None or not hasattr(section, k)]
    if missing:
        raise NotImplementedError("%s needs score.{%s}; missing: %s" % (what, ", ".join(keys), ", ".join("score." + k for k in missing)))
    for key in ("n_slices", "n_samples", "batch_size", "k"):
        v = getattr(section, key)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("%s: score.%s=%r must be an integer >= 1" % (what, key, v))
    k = section.k
    if k > 8:
        raise ValueError("%s: score.k=%d out of [1, 8]" % (what, k))
    if section.n_samples < k + 1:
        raise ValueError("%s: score.n_samples=%d must be at least k + 1 = %d" % (what, section.n_samples, k + 1))
    if section.n_slices < 2 * (k + 1):
        raise ValueError("%s: score.n_slices=%d must be at least 2 (k + 1) = %d: the floor compares two halves of the real set"
                         % (what, section.n_slices, 2 * (k + 1)))
    if section.against not in SCORE_AGAINST:
        raise ValueError("%s: score.against is one of %s (got %r)" % (what, ", ".join(repr(a) for a in SCORE_AGAINST), section.against))
    kw = dict(n_samples=section.n_samples, batch_size=section.batch_size, k=k, temperature=float(section.temperature or 1.0),
              top_k=section.top_k or None, top_p=section.top_p or None, against=section.against)
    scale = section.guidance_scale
    scale = 1.0 if scale is None or scale is False else scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (scale == scale and 0.0 <= scale < float("inf")):
        raise ValueError("score.guidance_scale=%r must be a finite number >= 0 (1: no guidance)" % (scale,))
    if float(scale) != 1.0:
        if cond is None or not prior_cond_drop(config)["null_token"]:
            raise ValueError("score.guidance_scale=%g needs a prior trained with the null embedding: %s.null_token: true" % (
                scale, _cond_section(config)[1]))
        kw["guidance_scale"] = float(scale)
    if cond is not None and section.n_samples != section.n_slices:
        raise ValueError("%s: with model.prior.cond one sample is drawn per held-out slice: score.n_samples=%d must equal "
                         "score.n_slices=%d" % (what, section.n_samples, section.n_slices))
    if masked is not None:
        n_steps = section.n_steps
        if n_steps is not None and n_steps is not False:
            if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
                raise ValueError("score.n_steps=%r must be an integer >= 1 (false: model.prior.masked.n_steps)" % (n_steps,))
            kw["n_steps"] = n_steps
    return kw


def latent_size(config):
    """Side of the VQGAN's latent map: resolution halved once per encoder level but the first."""
    c = config.model.vqgan
    return int(c.resolution) // 2 ** (len(c.enc_ch_multiplier) - 1)


def configure_prior(config):
    """The GPT of config.model.prior over the codes of config.model.vqgan: vocab_size = the VQGAN's dict_size, block_size = the
    latent's h w (model.prior.block_size, if given, overrides it); the optional model.prior.{emb_pdrop, res_pdrop, att_pdrop} are
    the dropout probabilities, absent or `false` meaning 0 (a JSON `false` / absent n_unmasked, like 0, means the plain causal
    mask).  build_prior_trainer seeds the dropout from run.seed."""
    from networks import GPT
    p = config.model.prior
    side = latent_size(config)
    if prior_masked(config) is not None:          # the bidirectional masked prior: h w positions, every one sees every one
        from networks import MaskedGPT
        return MaskedGPT(vocab_size=config.model.vqgan.dict_size, block_size=side * side, n_layer=p.n_layer, n_head=p.n_head,
                         n_embed=p.n_embed, **{k: float(_get(p, k) or 0.0) for k in ("emb_pdrop", "res_pdrop", "att_pdrop")})
    positions, n_unmasked = side * side, int(p.n_unmasked or 0)
    if prior_condition(config) is not None:          # [h w conditioning tokens | h w codes], the prefix fully visible
        if n_unmasked not in (0, side * side):
            raise ValueError("model.prior.n_unmasked=%d with model.prior.cond: the conditioning prefix is the latent's h w = %d tokens "
                             "(0 or `false` leaves it to the condition)" % (n_unmasked, side * side))
        positions, n_unmasked = 2 * side * side, side * side
    return GPT(vocab_size=config.model.vqgan.dict_size, block_size=int(_get(p, "block_size") or positions), n_layer=p.n_layer,
               n_head=p.n_head, n_embed=p.n_embed, n_unmasked=n_unmasked,
               **{k: float(_get(p, k) or 0.0) for k in ("emb_pdrop", "res_pdrop", "att_pdrop")})


def build_prior_trainer(config, device="cuda", first_stage_ckpt_path=None):
    """config -> PriorTrainer (run_vqwnet.py -p): the GPT of model.prior trained on the codes of the frozen VQGAN of model.vqgan;
    with model.prior.cond (prior_condition) the ConditionalPriorTrainer and its LabelCondition; with model.prior.masked the
    MaskedPriorTrainer, and with model.prior.masked.cond the ConditionalMaskedPriorTrainer.
    first_stage_ckpt_path (argument, else run.first_stage_ckpt_path) loads a -v checkpoint's `decoder.*` keys into the VQGAN, as
    build_vqgan_trainer does.  A JSON `false` for pkeep, sos_token, warmup_steps or decay_steps arrives as None: pkeep then means
    1 (no corruption), the others 0.  run.seed seeds the trainer's generator and the prior's dropout (model.prior.*_pdrop)."""
    from .prior import PriorTrainer
    check_prior_config(config)
    vqgan, gpt = configure_vqgan(config), configure_prior(config)
    first = first_stage_ckpt_path or _get(config.run, "first_stage_ckpt_path")
    if first:
        load_vqgan_from_ckpt(first, vqgan)
    p, o = config.model.prior, config.prior_optim
    cls, extra, cond = PriorTrainer, {}, prior_condition(config)
    masked = prior_masked(config)
    if masked is not None:
        from .masked_prior import MaskedPriorTrainer
        cls, extra = MaskedPriorTrainer, dict(masked)
        if cond is not None:          # model.prior.masked.cond: the condition is added to every position, the GPT stays h w long
            from networks import LabelCondition
            from .masked_cond_prior import ConditionalMaskedPriorTrainer
            side, drop = latent_size(config), prior_cond_drop(config)
            cls = ConditionalMaskedPriorTrainer
            extra["cond"] = LabelCondition(cond["n_labels"], p.n_embed, side, side, null_token=drop["null_token"])
            if drop["p_uncond"] > 0:
                extra.update(p_uncond=drop["p_uncond"], cond_drop_seed=drop["drop_seed"])
    elif cond is not None:
        from networks import LabelCondition
        from .cond_prior import ConditionalPriorTrainer
        side = latent_size(config)
        drop = prior_cond_drop(config)
        cls, extra = ConditionalPriorTrainer, {"cond": LabelCondition(cond["n_labels"], p.n_embed, side, side, null_token=drop["null_token"])}
        if drop["p_uncond"] > 0:
            extra.update(p_uncond=drop["p_uncond"], cond_drop_seed=drop["drop_seed"])
    return cls(vqgan, gpt, pkeep=1.0 if p.pkeep is None else p.pkeep, sos_token=int(p.sos_token or 0), lr=o.lr,
                        betas=(o.b1, o.b2), weight_decay=o.weight_decay or 0.0, grad_norm_clip=o.grad_norm_clip or None,
                        warmup_steps=int(o.warmup_steps or 0), decay_steps=int(o.decay_steps or 0),
                        seed=int(_get(config.run, "seed", 0) or 0), dropout_seed=int(_get(config.run, "seed", 0) or 0), device=device, **extra)


def configure_discriminator(config):
    """-> the discriminator as base.py:239-259 builds it.  PatchGAN: NLayerDiscriminator over config.model.dis, with spectral
    normalisation on its convolutions when dis.apply_spectral_norm is set.  model_name 'UNetDiscriminator': the U-Net
    discriminator over config.model.dis.{D_ch, D_wide, D_attn, resolution} (only the 512 arch, no attention)."""
    d = config.model.dis
    name = _get(d, "model_name", "NLayerDiscriminator")
    if name == "UNetDiscriminator":
        missing = [k for k in _UNET_DIS_KEYS if not hasattr(d, k)]
        if missing:
            raise NotImplementedError("model.dis.model_name 'UNetDiscriminator' needs model.dis.{%s} (missing: %s), as the "
                                      "reference's constructor call does (base.py:239-247)" % (", ".join(_UNET_DIS_KEYS), ", ".join(missing)))
        return UNetDiscriminator(in_channels=config.model.vqmodel.in_channels, D_ch=d.D_ch, D_wide=bool(d.D_wide), D_attn=str(d.D_attn),
                                 resolution=d.resolution, unconditional=True)
    if name != "NLayerDiscriminator":
        raise NotImplementedError("model.dis.model_name %r is unknown" % (name,))
    dis = NLayerDiscriminator(in_channels=config.model.vqmodel.in_channels, out_channels=1, n_filters=d.n_filters,
                              n_layers=d.n_layers, normalization=d.normalization)
    if _get(d, "apply_spectral_norm"):
        apply_spectral_norm(dis)
    return dis


def _weights(kind, config, absent_is_zero=False):
    """-> the namedtuple `kind` from config.loss.loss_weight; an absent key keeps the namedtuple's default or, with
    absent_is_zero, is 0.0 like a key that is `false`."""
    w = config.loss.loss_weight
    return kind(**{k: float(_get(w, k) or 0.0) for k in kind._fields if absent_is_zero or hasattr(w, k)})


def gan_loss_weights(config):
    """-> GanLossWeights from config.loss.loss_weight.{recon, gen, dis, freq, perceptual}; an absent key keeps the
    namedtuple's default."""
    return _weights(GanLossWeights, config)


def unet_gan_loss_weights(config):
    """-> UNetGanLossWeights from config.loss.loss_weight.{recon, gen, dis, freq, perceptual, unet_perceptual, cutmix,
    consistency}; an absent key keeps the namedtuple's default."""
    return _weights(UNetGanLossWeights, config)


def vqgan_loss_weights(config):
    """-> VQGANLossWeights from config.loss.loss_weight.{recon, freq, perceptual, commit, gen, unet_perceptual, dis, cutmix,
    consistency}; an absent key keeps the namedtuple's default."""
    return _weights(VQGANLossWeights, config)


def _adam_kwargs(o):
    return dict(lr=o.lr, betas=(o.b1, o.b2), weight_decay=o.weight_decay or 0.0)


def configure_optimizers(config, encoder, decoder):
    """-> (enc_optim, dec_optim): Adam over each sub-network's trainable parameters (base.py:164-175)."""
    return (Adam([p for p in encoder.parameters() if p.requires_grad], **_adam_kwargs(config.enc_optim)),
            Adam([p for p in decoder.parameters() if p.requires_grad], **_adam_kwargs(config.dec_optim)))


def configure_losses(config):
    """-> EmbeddingLoss (base.py:261-278); None-for-false flags pass through as the reference's do."""
    c = config.loss
    if _get(c, "use_perceptual_loss"):
        _perceptual_settings(c)         # raises for what is not built
    return EmbeddingLoss(dict_size=config.model.vqmodel.dict_size, margin=c.embed_loss.margin,
                         use_distance_loss=c.embed_loss.use_distance_loss,
                         use_regularization_loss=c.embed_loss.use_regularization_loss)


def configure_frequency_loss(config):
    """-> FocalFrequencyLoss(loss_weight=1.0, alpha=1.0) as base.py:277-278 builds it when use_frequency_loss is set,
    else None."""
    if _get(config.loss, "use_frequency_loss"):
        return FocalFrequencyLoss(loss_weight=1.0, alpha=1.0)
    return None


def _perceptual_settings(c):
    """-> ('vgg', conv_index, weights path) or ('lpips', None, weights) of a config with use_perceptual_loss;
    NotImplementedError for what is not built."""
    kind = _get(c, "perceptual_loss_type") or "vgg"
    if kind == "lpips":
        weights = _get(c, "lpips_weights")
        if not weights:
            raise NotImplementedError("use_perceptual_loss with perceptual_loss_type 'lpips' needs the pretrained LPIPS weights, "
                                      "which this build never downloads: set config.loss.lpips_weights to a local LPIPS state "
                                      "dict or reference checkpoint, or to the pair [alexnet-owt-7be5be79.pth, alex.pth] "
                                      "(config.loss.perceptual_weights names the VGG19 file of the 'vgg' perceptual loss only)")
        if not isinstance(weights, str):
            weights = tuple(weights)
            if len(weights) != 2:
                raise ValueError("config.loss.lpips_weights: a path, or the two paths [alexnet, lins]")
        return "lpips", None, weights
    if kind != "vgg":
        raise NotImplementedError("use_perceptual_loss: unknown perceptual_loss_type %r" % (kind,))
    conv_index = str(_get(c, "conv_index") or "22")
    if conv_index != "22":
        raise NotImplementedError("use_perceptual_loss with conv_index %r is not built: only VGGLoss()'s '22' slice "
                                  "(vgg19.features[:8], trainers/base.py:273)" % (conv_index,))
    path = _get(c, "perceptual_weights")
    if not path:
        raise NotImplementedError("use_perceptual_loss needs the pretrained VGG19 weights, which this build never downloads: "
                                  "set config.loss.perceptual_weights to a local vgg19 state dict (vgg19-dcbb9e9d.pth), "
                                  "a VGGLoss state dict or a reference checkpoint of a run with the loss on")
    return "vgg", conv_index, path


def configure_perceptual_loss(config):
    """-> VGGLoss() or LPIPSLoss() as base.py:271-275 builds them when use_perceptual_loss is set (weights from
    config.loss.perceptual_weights / config.loss.lpips_weights), else None."""
    c = config.loss
    if not _get(c, "use_perceptual_loss"):
        return None
    kind, conv_index, weights = _perceptual_settings(c)
    if kind == "lpips":
        return LPIPSLoss(net='alex', weights=weights)
    return VGGLoss(conv_index=conv_index, weights=weights)


def loss_weights(config):
    return _weights(LossWeights, config, absent_is_zero=True)


def set_transform(config, seed=0):
    """The pair of RandomTransform modules (base.py:280-282) behind the trainer's `views` protocol; without an
    `augmentation` section: identity / horizontal flip (the benchmark's exact-integer views)."""
    aug = _get(config, "augmentation")
    if aug is None:
        return FlipViews()
    return RandomTransformViews(RandomTransform(aug, seed=seed), RandomTransform(aug, seed=seed + 1))


def build_evaluator(config, encoder, decoder):
    """-> trainers.evaluation.Evaluator for `-m test` (the metrics of base.py:75-77 and the code entropy of
    single_window_trainer.py:794-797 over config.model.vqmodel.dict_size codes)."""
    return Evaluator(encoder, decoder, config.model.vqmodel.dict_size)


def _multi_window(config, multi_window, frequency_loss, perceptual_loss):
    """-> (multi_window, freq_weights, percep_weights) of a builder's `multi_window` argument: None derives the dict from
    loss.recon_weights and dataset.window_*, False (the launcher without -w) is the single-window step whatever keys the
    config carries; the per-window weights of a loss that is on are required in a multi-window run."""
    if multi_window is None and _get(config.loss, "recon_weights") is not None and _get(_get(config, "dataset"), "window_width") is not None:
        d = config.dataset
        multi_window = dict(dataset_window=(d.window_width, d.window_center, d.window_scale), recon_weights=tuple(config.loss.recon_weights))
    if multi_window is False:
        multi_window = None
    percep_weights = None
    if perceptual_loss is not None and multi_window is not None:
        percep_weights = _get(config.loss, "percep_weights")
        if percep_weights is None:
            raise ValueError("config.loss.percep_weights is required for a multi-window run with use_perceptual_loss "
                             "(multi_window_trainer.py:54, 101-119)")
        percep_weights = tuple(percep_weights)
    freq_weights = None
    if frequency_loss is not None and multi_window is not None:
        freq_weights = _get(config.loss, "freq_weights")
        if freq_weights is None:
            raise ValueError("config.loss.freq_weights is required for a multi-window run with use_frequency_loss "
                             "(multi_window_trainer.py:100-126)")
        freq_weights = tuple(freq_weights)
    return multi_window, freq_weights, percep_weights


def build_first_step_trainer(config, device="cuda", data_parallel=None, views=None, multi_window=None):
    """config -> FirstStepTrainer (the `first_step` training mode of run_vqwnet.py).  data_parallel defaults to
    torch.distributed being initialised with more than one rank."""
    import torch.distributed as dist
    mode = _get(config.run, "training_mode", "first_step")
    if mode != "first_step":
        raise NotImplementedError("training_mode %r: use trainers.build_second_step_trainer (or trainers.SecondStepTrainer) "
                                  "for the GAN step" % mode)
    frequency_loss = configure_frequency_loss(config)
    perceptual_loss = configure_perceptual_loss(config)
    multi_window, freq_weights, percep_weights = _multi_window(config, multi_window, frequency_loss, perceptual_loss)
    encoder, decoder = configure_models(config)
    if data_parallel is None:
        data_parallel = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    g = config.model.vqmodel
    return FirstStepTrainer(
        in_channels=g.in_channels, enc_filters=tuple(g.enc_filters), dec_filters=tuple(g.dec_filters), dict_size=g.dict_size,
        momentum=g.momentum, margin=config.loss.embed_loss.margin, loss_weight=loss_weights(config),
        views=views if views is not None else set_transform(config, seed=_get(config.run, "seed", 0) or 0), device=device,
        encoder=encoder, decoder=decoder, data_parallel=data_parallel, multi_window=multi_window,
        embed_loss=configure_losses(config), enc_optim=_adam_kwargs(config.enc_optim), dec_optim=_adam_kwargs(config.dec_optim),
        use_recon_loss=bool(_get(config.loss, "use_recon_loss", True)), frequency_loss=frequency_loss, freq_weights=freq_weights,
        perceptual_loss=perceptual_loss, percep_weights=percep_weights)


def build_second_step_trainer(config, device="cuda", data_parallel=None, first_stage_ckpt_path=None,
                              discriminator_ckpt_path=None, multi_window=None):
    """config -> SecondStepTrainer (the `second_step` training mode of run_vqwnet.py with the PatchGAN discriminator,
    single_window_trainer.py:434-488) or, when model.dis names the U-Net discriminator, UNetSecondStepTrainer
    (:264-432) or, multi-window, UNetMultiWindowSecondStepTrainer (multi_window_trainer.py:208-321).  multi_window: as in
    build_first_step_trainer - None derives it from loss.recon_weights and dataset.window_*, False builds the single-window
    step whatever keys the config carries.  The multi-window step trains the U-Net discriminator only (the reference unpacks
    three outputs of self.dis): with the PatchGAN it raises.  The first-stage weights (encoder strictly, decoder
    non-strictly) and, optionally, the discriminator's come from the path arguments, else from
    config.run.first_stage_ckpt_path / discriminator_ckpt_path, as TrainerBase.__init__ loads them (base.py:79-83)."""
    import torch.distributed as dist
    mode = _get(config.run, "training_mode", "second_step")
    if mode != "second_step":
        raise NotImplementedError("training_mode %r: build_second_step_trainer builds 'second_step' only" % (mode,))
    c = config.loss
    loss_type = _get(c, "dis_loss_type") or "hinge_d_loss"
    if loss_type != "hinge_d_loss":
        raise NotImplementedError("loss.dis_loss_type %r: only 'hinge_d_loss' is built (single_window_trainer.py:478)" % (loss_type,))
    frequency_loss, perceptual_loss = configure_frequency_loss(config), configure_perceptual_loss(config)
    multi_window, freq_weights, percep_weights = _multi_window(config, multi_window, frequency_loss, perceptual_loss)
    encoder, decoder = configure_models(config)
    dis = configure_discriminator(config)
    if multi_window is not None and not isinstance(dis, UNetDiscriminator):
        raise NotImplementedError("a multi-window second step trains the U-Net discriminator (model.dis.model_name "
                                  "'UNetDiscriminator'): the reference's step unpacks three outputs of its discriminator "
                                  "(multi_window_trainer.py:245); with the PatchGAN it is not built")
    first = first_stage_ckpt_path or _get(config.run, "first_stage_ckpt_path")
    if first:
        load_first_stage_from_ckpt(first, encoder, decoder)
    dck = discriminator_ckpt_path or _get(config.run, "discriminator_ckpt_path")
    if dck:
        load_discriminator_from_ckpt(dck, dis)
    if data_parallel is None:
        data_parallel = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    kw = dict(dis=dis, n_inner_loops=int(_get(c, "n_inner_loops") or 1), device=device, data_parallel=data_parallel,
              frequency_loss=frequency_loss, perceptual_loss=perceptual_loss,
              dec_optim=_adam_kwargs(config.dec_optim), dis_optim=_adam_kwargs(config.dis_optim),
              use_recon_loss=bool(_get(c, "use_recon_loss", True)))
    if isinstance(dis, UNetDiscriminator):          # single_window_trainer.py:264-432
        kw.update(loss_weight=unet_gan_loss_weights(config), use_unet_perceptual_loss=bool(_get(c, "use_unet_perceptual_loss")),
                  use_l1_loss=bool(_get(c, "use_l1_loss")))
        if multi_window is not None:
            # (a JSON `false` arrives as None: only an absent key means true)
            clamp = bool(c.clamp_windows) if hasattr(c, "clamp_windows") else True
            return UNetMultiWindowSecondStepTrainer(encoder, decoder, multi_window=multi_window, freq_weights=freq_weights,
                                                    percep_weights=percep_weights, clamp_windows=clamp, **kw)
        return UNetSecondStepTrainer(encoder, decoder, **kw)
    return SecondStepTrainer(encoder, decoder, loss_weight=gan_loss_weights(config), **kw)


def build_vqgan_trainer(config, device="cuda", data_parallel=None, first_stage_ckpt_path=None, discriminator_ckpt_path=None):
    """config -> VQGANUNetDisTrainer (run_vqwnet.py -v; reference trainers/vqgan_unet_dis.py): the VQGAN of model.vqgan trained
    against the U-Net discriminator of model.dis, whatever run.training_mode says (the reference's step has no mode dispatch).
    first_stage_ckpt_path (argument, else run.first_stage_ckpt_path) loads a checkpoint's `decoder.*` keys into the VQGAN
    non-strictly, discriminator_ckpt_path its `dis.*` keys into the discriminator, as TrainerBase.__init__ does (base.py:79-83)."""
    import torch.distributed as dist
    check_vqgan_config(config)
    c = config.loss
    loss_type = _get(c, "dis_loss_type") or "hinge_d_loss"
    if loss_type != "hinge_d_loss":
        raise NotImplementedError("loss.dis_loss_type %r: only 'hinge_d_loss' is built (vqgan_unet_dis.py:85)" % (loss_type,))
    frequency_loss, perceptual_loss = configure_frequency_loss(config), configure_perceptual_loss(config)
    vqgan = configure_vqgan(config)
    dis = configure_discriminator(config)
    if not isinstance(dis, UNetDiscriminator):
        raise NotImplementedError("the VQGAN trainer trains against the U-Net discriminator (model.dis.model_name "
                                  "'UNetDiscriminator'): its step unpacks three outputs of its discriminator "
                                  "(vqgan_unet_dis.py:59); with the PatchGAN it is not built")
    first = first_stage_ckpt_path or _get(config.run, "first_stage_ckpt_path")
    if first:
        load_vqgan_from_ckpt(first, vqgan)
    dck = discriminator_ckpt_path or _get(config.run, "discriminator_ckpt_path")
    if dck:
        load_discriminator_from_ckpt(dck, dis)
    if data_parallel is None:
        data_parallel = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    return VQGANUNetDisTrainer(vqgan, dis, loss_weight=vqgan_loss_weights(config), n_inner_loops=int(_get(c, "n_inner_loops") or 1),
                               device=device, data_parallel=data_parallel, frequency_loss=frequency_loss,
                               perceptual_loss=perceptual_loss, dec_optim=_adam_kwargs(config.dec_optim),
                               dis_optim=_adam_kwargs(config.dis_optim), use_recon_loss=bool(_get(c, "use_recon_loss", True)),
                               use_unet_perceptual_loss=bool(_get(c, "use_unet_perceptual_loss")))
