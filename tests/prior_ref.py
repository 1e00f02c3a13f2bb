"""Plain-torch restatement of the training recipe of the GPT code prior (trainers/prior.py), written from the formulas on top of
tests/gpt_ref.py and evaluated in any dtype: the check of tests/golden/prior_step_*.npz in tests/test_prior_host.py, the case table
of tests/test_gpu_prior.py and of tests/golden/make_golden_prior_step.py, and the plain-torch yardstick of tools/prior_step_bench.py.

    input       inp[b, 0] = sos; inp[b, t] = corrupted[b, t - 1]; corrupted = ids where u_keep < pkeep else min(V - 1, floor(u_rand V))
    loss        mean over (b, t) of the cross-entropy of gpt(inp)[b, t] against ids[b, t]
    clip        norm = sqrt(sum over ALL parameters of |g|^2); coef = min(1, max_norm / (norm + 1e-6))       (clip_grad_norm_)
    AdamW       g' = coef g; p *= 1 - lr wd; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2;
                p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)        wd: the group's (minGPT's rule, decays())
    rate        linear warm-up lr (step + 1) / warmup_steps, then a cosine from lr to 0.1 lr at decay_steps (0: constant)
"""
import math

import torch

import gpt_ref as G

SOS = 0
# the fixture cases: name -> (V, block_size, n_layer, n_head, E, n_unmasked, B, T), gpt_ref.CASES' order without Te
CASES = {
    "p64": (64, 16, 2, 2, 64, 0, 2, 16),
    "p96": (64, 16, 2, 3, 96, 3, 2, 16),
}
SEEDS = {"p64": 131, "p96": 132}
STEPS = 3
OPTIM = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
# between the smallest and the largest of the three recorded pre-clip norms of the case, so that some steps clip and some do not
# (asserted when the fixture is made and in tests/test_prior_host.py)
GRAD_NORM_CLIP = {"p64": 4.5, "p96": 5.0}
VARIANTS = G.VARIANTS


# the smallest VQGAN whose codes the fixture's GPTs can model: 64 codes, an 8 x 8 picture, a 4 x 4 latent = 16 tokens
TINY_VQGAN = dict(in_channels=1, mid_channels=32, out_channels=1, emb_dim=32, dict_size=64, enc_ch_multiplier=(1, 2),
                  dec_ch_multiplier=(1, 2), num_res_blocks=1, enc_attn_resolutions=[], dec_attn_resolutions=[], resolution=8,
                  p_dropout=0.0, resamp_with_conv=True, knn_backend="torch")
PRIOR_MONITORED = ["epoch", "iteration", "loss", "grad_norm", "lr", "val_loss", "ppl"]


def prior_run_config(save_dir, **run):
    """A tiny -p run: the VQGAN of vqgan_model_ref.CASES['vqgan'] with 1 output channel (32 x 32 synthetic slices, a 16 x 16
    latent of 8 codes), a 2-layer GPT over its 256-token sequences, one epoch of two steps of batch 4, one validation batch."""
    raw = {
        "run": dict(seed=3, seed_list=[11], training_mode="second_step", num_gpus=1, n_epochs=1, resume_checkpoint=False,
                    first_stage_ckpt_path=False, monitoring_metrics=list(PRIOR_MONITORED), log_every_n_steps=1,
                    use_validation_sanity_check=False),
        "dataset": dict(dataset_name="synthetic", root_dir_path=False, batch_size=4, num_workers=0, modality="mr",
                        augmentations=False, image_size=32, n_samples_train=8, n_samples_val=4, n_samples_test=4),
        "model": {
            "vqmodel": dict(model_name="VQGAN", in_channels=1, dict_size=8),
            "dis": dict(model_name="UNetDiscriminator", normalization="batchnorm"),
            "vqgan": dict(in_channels=1, mid_channels=32, out_channels=1, emb_dim=32, dict_size=8, enc_ch_multiplier=[1, 2],
                          dec_ch_multiplier=[1, 2], num_res_blocks=1, enc_attn_resolutions=[16], dec_attn_resolutions=[16],
                          resolution=32, p_dropout=0.0, resamp_with_conv=True, knn_backend="torch"),
            "prior": dict(n_layer=2, n_head=2, n_embed=64, n_unmasked=0, pkeep=0.5, sos_token=0, top_k=4),
        },
        "prior_optim": dict(lr=1e-3, b1=0.9, b2=0.95, weight_decay=0.01, grad_norm_clip=1.0, warmup_steps=2, decay_steps=0),
        "save": dict(save_dir=str(save_dir), study_name="study", n_save_images=2),
    }
    raw["run"].update(run)
    return raw


def gpt_kwargs(name):
    V, bs, nl, nh, E, nu, B, T = CASES[name]
    return dict(vocab_size=V, block_size=bs, n_layer=nl, n_head=nh, n_embed=E, n_unmasked=nu)


def case_ids(name, seed):
    V, bs, nl, nh, E, nu, B, T = CASES[name]
    return torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed + 2000))


def decays(key):
    """minGPT's rule by parameter name on GPT's state_dict keys: nn.Linear weights decay (the q, k, v, proj and mlp layers and the
    head); biases, LayerNorm weights (ln1, ln2, ln_f), tok_embed.weight and pos_embed do not."""
    if key.endswith(".bias") or key == "pos_embed" or key == "tok_embed.weight":
        return False
    leaf = key.split(".")[-2]
    if leaf.startswith("ln"):
        return False
    if key.endswith(".weight"):
        return True
    raise ValueError("decays: %s falls in neither group" % key)


def tokens_ref(ids, sos, pkeep, V, u_keep=None, u_rand=None):
    """The transformer's input; the uniforms are fp32 and the arithmetic on them is fp32, as in the kernel."""
    cor = ids
    if pkeep < 1:
        rnd = torch.clamp(torch.floor(u_rand.float() * V).long(), max=V - 1)
        cor = torch.where(u_keep.float() < pkeep, ids, rnd)
    return torch.cat((torch.full_like(ids[:, :1], sos), cor[:, :-1]), dim=1)


def learning_rate_ref(step, lr, warmup_steps=0, decay_steps=0):
    if step < warmup_steps:
        return lr * (step + 1) / warmup_steps
    if decay_steps <= 0:
        return lr
    if step >= decay_steps:
        return 0.1 * lr
    x = (step - warmup_steps) / max(1, decay_steps - warmup_steps)
    return lr * (0.1 + 0.9 * 0.5 * (1 + math.cos(math.pi * x)))


def clip_ref(grads, max_norm):
    """(norm, coef) over a list of gradients, in their dtype"""
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    coef = torch.ones_like(norm) if max_norm is None or max_norm <= 0 else torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, coef


def adamw_ref_(p, g, m, v, t, lr, betas, eps, wd):
    b1, b2 = betas
    p.mul_(1 - lr * wd)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).add_(g * g, alpha=1 - b2)
    p.sub_((lr / (1 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))


def loss_and_grads(name, st, ids, sos=SOS):
    """st {key: tensor; the parameters require a gradient} -> (loss, {key: gradient})"""
    V, bs, nl, nh, E, nu, B, T = CASES[name]
    params = {k: v for k, v in st.items() if not k.endswith("mask")}
    for p in params.values():
        p.grad = None
    logits, _ = G.gpt_ref(tokens_ref(ids, sos, 1.0, V), st, nl, nh)
    loss = G.xent_ref(logits, ids)[0].mean()
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in params.items()}


def steps_ref(name, state, ids, dtype, max_norm, steps=STEPS, variant="threads8", optim=OPTIM):
    """`steps` steps of the recipe (pkeep = 1, constant rate) from `state` ->
    dict(loss [steps], norm [steps], coef [steps], g0 {key: the unclipped gradient of step 0}, P {key: the parameter after the
    last step}).  The variants are mathematically identical evaluations: eight threads, one thread, the batch in reversed order."""
    st = {}
    for k, v in state.items():
        v = v.detach().clone()
        st[k] = v if k.endswith("mask") else v.to(dtype).requires_grad_(True)
    if variant == "batch_reversed":
        ids = ids.flip(0)
    keys = [k for k in st if not k.endswith("mask")]
    mom = {k: (torch.zeros_like(st[k]), torch.zeros_like(st[k])) for k in keys}
    out = dict(loss=[], norm=[], coef=[])
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        for t in range(1, steps + 1):
            loss, grads = loss_and_grads(name, st, ids)
            norm, coef = clip_ref([grads[k] for k in keys], max_norm)
            if t == 1:
                out["g0"] = {k: grads[k].detach().clone() for k in keys}
            with torch.no_grad():
                for k in keys:
                    adamw_ref_(st[k], grads[k] * coef, mom[k][0], mom[k][1], t, optim["lr"], optim["betas"], optim["eps"],
                               optim["weight_decay"] if decays(k) else 0.0)
            for key, val in (("loss", loss), ("norm", norm), ("coef", coef)):
                out[key].append(float(val))
    finally:
        torch.set_num_threads(n)
    out["P"] = {k: st[k].detach().clone() for k in keys}
    return out
