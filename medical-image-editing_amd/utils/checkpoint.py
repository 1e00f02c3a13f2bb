"""Checkpoint wire format of the reference (PyTorch-Lightning `.ckpt` = torch.save'd dict whose 'state_dict' holds the
LightningModule's parameters under the attribute prefixes `encoder.`, `decoder.`, `dis.`): trainers/base.py:85-114,
run_recon.py:98-112.  The modules of this build keep the reference's state_dict keys, so these are plain filters."""
import torch


def _state_dict(path):
    return torch.load(path, map_location='cpu')['state_dict']


def load_first_stage_from_ckpt(path, encoder, decoder=None, load_only_enc=False):
    """base.py:85-102: encoder strictly, decoder with strict=False."""
    sd = _state_dict(path)
    enc = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder')}
    dec = {k[len('decoder.'):]: v for k, v in sd.items() if k.startswith('decoder')}
    encoder.load_state_dict(enc, strict=True)
    if not load_only_enc and decoder is not None:
        decoder.load_state_dict(dec, strict=False)
    return encoder, decoder


def load_vqgan_from_ckpt(path, vqgan):
    """The VQGAN trainer's first-stage load (base.py:85-102 with the VQGAN as `decoder`): the `decoder.*` keys, strict=False."""
    sd = _state_dict(path)
    vqgan.load_state_dict({k[len('decoder.'):]: v for k, v in sd.items() if k.startswith('decoder.')}, strict=False)
    return vqgan


def load_discriminator_from_ckpt(path, dis):
    """base.py:104-113"""
    sd = _state_dict(path)
    dis.load_state_dict({k[len('dis.'):]: v for k, v in sd.items() if k.startswith('dis')}, strict=True)
    return dis


def perceptual_state_from_ckpt(path):
    """The VGG slice a reference run with use_perceptual_loss saved (`perceptual_loss.vgg.N.*`, base.py:271-275) as a
    functions.VGGLoss state dict (`vgg.N.*`)."""
    sd = _state_dict(path)
    pre = 'perceptual_loss.'
    out = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre + 'vgg.')}
    if not out:
        raise KeyError("%s holds no perceptual_loss.vgg.* entries" % (path,))
    return out


def init_from_ckpt(path, model, key_name, delete_string='model.'):
    """run_recon.py:98-112: keep the keys that start with `key_name`, strip `delete_string` from those that carry it."""
    sd = _state_dict(path)
    new = {}
    for k, v in sd.items():
        if k.startswith(delete_string):
            new[k[len(delete_string):]] = v
        elif k.startswith(key_name):
            new[k] = v
    model.load_state_dict(new, strict=True)
    return model


def save_lightning_style_ckpt(path, encoder=None, decoder=None, dis=None, extra=None):
    """Write a checkpoint the reference's loaders accept (plain contiguous tensors, attribute prefixes)."""
    sd = {}
    for pre, m in (("encoder.", encoder), ("decoder.", decoder), ("dis.", dis)):
        if m is not None:
            for k, v in m.state_dict().items():
                sd[pre + k] = v.detach().cpu().contiguous().clone()
    d = {"state_dict": sd}
    d.update(extra or {})
    torch.save(d, path)


# ----------------------------------------------------------------------------------------------------
# checkpoints of this build's own runs (trainers/fit.py): the reference's wire format plus one project-own key
# ----------------------------------------------------------------------------------------------------
# configure_optimizers' list, trainers/base.py:164-183; behind it what the reference does not have: the GPT prior's optimiser
# and module (trainers/prior.py) - a checkpoint of the other trainers is unchanged by the longer lists
OPTIMIZER_ORDER = ("enc", "dec", "dis", "prior_optim")
MODULE_ORDER = ("encoder", "decoder", "dis", "transformer", "cond")          # cond: the conditional prior's label table (trainers/cond_prior.py)
RUN_STATE_KEY = "vqw_run_state"                  # not a key of the reference: everything a bit-exact continuation needs


def _to_cpu(obj):
    """Tensors of a nested state moved to the host, values, dtypes and strides as they are."""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def save_run_checkpoint(path, trainer_state, epoch, global_step, run_state=None):
    """Write `trainer_state` (a trainer's state_dict(): {'modules', 'optimizers', 'extra'}) as a Lightning-style checkpoint:
    'state_dict' with the attribute prefixes `encoder.` / `decoder.` / `dis.` (plain contiguous tensors, read unchanged by
    load_first_stage_from_ckpt, load_discriminator_from_ckpt and init_from_ckpt), 'epoch', 'global_step',
    'optimizer_states' (the reference's list enc, dec, dis without the optimisers the training mode does not own;
    'optimizer_indices' records which positions of that order are present), and RUN_STATE_KEY = {'trainer': the trainer's
    `extra`, **run_state}."""
    sd = {}
    for name in MODULE_ORDER:
        for k, v in (trainer_state["modules"].get(name) or {}).items():
            sd[name + "." + k] = v.detach().cpu().contiguous().clone()
    present = [i for i, k in enumerate(OPTIMIZER_ORDER) if k in trainer_state["optimizers"]]
    ckpt = {"state_dict": sd, "epoch": int(epoch), "global_step": int(global_step),
            "optimizer_states": [_to_cpu(trainer_state["optimizers"][OPTIMIZER_ORDER[i]]) for i in present],
            "optimizer_indices": present,
            RUN_STATE_KEY: dict(_to_cpu(run_state or {}), trainer=_to_cpu(trainer_state.get("extra") or {}))}
    tmp = str(path) + ".tmp"
    torch.save(ckpt, tmp)
    import os
    os.replace(tmp, path)           # a run killed while writing leaves the previous checkpoint, never half a file
    return ckpt


def load_run_checkpoint(path):
    """-> (trainer_state for a trainer's load_state_dict(), epoch, global_step, run_state) of a file save_run_checkpoint
    wrote.  A reference checkpoint (no RUN_STATE_KEY, three optimiser states) loads too, with an empty run state."""
    ckpt = torch.load(path, map_location="cpu")      # tensors and plain containers only: loads with torch's safe unpickler
    sd = ckpt["state_dict"]
    modules = {}
    for name in MODULE_ORDER:
        sub = {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}
        if sub:
            modules[name] = sub
    states = ckpt.get("optimizer_states") or []
    indices = ckpt.get("optimizer_indices", list(range(len(states))))
    optimizers = {OPTIMIZER_ORDER[i]: s for i, s in zip(indices, states)}
    run_state = dict(ckpt.get(RUN_STATE_KEY) or {})
    extra = run_state.pop("trainer", {})
    return ({"modules": modules, "optimizers": optimizers, "extra": extra}, int(ckpt.get("epoch", 0)),
            int(ckpt.get("global_step", 0)), run_state)
