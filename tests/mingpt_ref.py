"""Plain-torch restatement of the minGPT blocks (LayerNorm over the last axis, the exact GELU, multi-head attention with a causal
mask and an unmasked prefix, CausalSelfAttention, Block), written from the formulas and evaluated from a state dict in any dtype:
the float64 truth of tests/test_gpu_mingpt_blocks.py and the check of tests/golden/mingpt_blocks_*.npz in
tests/test_mingpt_blocks_host.py.

    LayerNorm   y = gamma (x - mean_r) / sqrt(var_r + eps) + beta over the last axis, biased variance
    GELU        0.5 x (1 + erf(x / sqrt 2))
    attention   per head h (columns [h hs, (h + 1) hs) of the (B, T, E) tensors): o_i = sum_j softmax_j(<q_i, k_j> / sqrt(hs)) v_j
                over the keys query i sees; causal: j <= (i < n_unmasked ? n_unmasked - 1 : i); lse_i = log sum_j exp(.)
"""
import math

import torch

EPS = 1e-5


def layer_norm_ref(x, gamma, beta, eps=EPS):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def gelu_ref(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def visible(Tq, Tk, n_unmasked=0, causal=True):
    """(Tq, Tk) bool: query i sees key j"""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    return j <= torch.where(i < n_unmasked, torch.full_like(i, n_unmasked - 1), i)


def causal_attention_ref(q, k, v, n_head, n_unmasked=0, causal=True, mask=None):
    """q (B, Tq, E), k, v (B, Tk, E) -> (o (B, Tq, E), lse (B, n_head, Tq)); mask: a (Tq, Tk) bool instead of the rule"""
    B, Tq, E = q.shape
    Tk, hs = k.shape[1], E // n_head
    qh, kh, vh = (t.reshape(B, -1, n_head, hs).transpose(1, 2) for t in (q, k, v))          # (B, nh, T, hs)
    s = torch.matmul(qh, kh.transpose(-2, -1)) * (1.0 / math.sqrt(hs))
    see = visible(Tq, Tk, n_unmasked, causal) if mask is None else mask
    s = s.masked_fill(~see[None, None], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    o = torch.matmul(torch.exp(s - lse[..., None]), vh)
    return o.transpose(1, 2).reshape(B, Tq, E), lse


def linear_ref(x, st, pre):
    y = torch.matmul(x, st[pre + "weight"].t())
    return y + st[pre + "bias"] if pre + "bias" in st else y


def attention_module_ref(x, st, pre, n_head, layer_past=None):
    """CausalSelfAttention.forward from its state dict (the stored mask buffer is the mask) -> (y, present)"""
    B, T, C = x.shape
    k, q, v = (linear_ref(x, st, pre + n + ".") for n in "kqv")
    hs = C // n_head
    present = torch.stack((k.reshape(B, T, n_head, hs).transpose(1, 2), v.reshape(B, T, n_head, hs).transpose(1, 2)))
    if layer_past is not None:
        past_k, past_v = layer_past
        k = torch.cat((past_k.to(x.dtype).transpose(1, 2).reshape(B, -1, C), k), dim=1)
        v = torch.cat((past_v.to(x.dtype).transpose(1, 2).reshape(B, -1, C), v), dim=1)
        o, _ = causal_attention_ref(q, k, v, n_head, causal=False)
    else:
        o, _ = causal_attention_ref(q, k, v, n_head, mask=st[pre + "mask"][0, 0, :T, :T] != 0)
    return linear_ref(o, st, pre + "proj."), present


def block_ref(x, st, pre, n_head, layer_past=None):
    """Block.forward from its state dict -> (x, present)"""
    h = layer_norm_ref(x, st[pre + "ln1.weight"], st[pre + "ln1.bias"])
    att, present = attention_module_ref(h, st, pre + "att.", n_head, layer_past)
    x = x + att
    h = layer_norm_ref(x, st[pre + "ln2.weight"], st[pre + "ln2.bias"])
    h = linear_ref(gelu_ref(linear_ref(h, st, pre + "mlp.0.")), st, pre + "mlp.2.")
    return x + h, present


# the fixture cases of tests/golden/make_golden_mingpt_blocks.py: name -> (class name, (E, n_head, T, n_unmasked, B), restatement)
CASES = {
    "att64": ("CausalSelfAttention", (64, 2, 40, 5, 2), attention_module_ref),
    "block64": ("Block", (64, 2, 40, 5, 2), block_ref),
    "block96": ("Block", (96, 3, 70, 0, 2), block_ref),
    "block128": ("Block", (128, 4, 129, 40, 1), block_ref),
}
SEEDS = {"att64": 81, "block64": 82, "block96": 83, "block128": 84}
PAST_CASES = ("att64", "block64")       # these also record an eval-mode forward of PAST_NEW new tokens behind PAST_LEN past ones
PAST_LEN, PAST_NEW = 37, 3


def config_kwargs(name):
    """GPTConfig(**kwargs) of a case: block_size = T, all dropout probabilities 0"""
    E, nh, T, nu, _ = CASES[name][1]
    return dict(vocab_size=16, block_size=T, n_embed=E, n_head=nh, n_unmasked=nu, att_pdrop=0.0, res_pdrop=0.0, emb_pdrop=0.0)


def round64(t):
    return torch.round(t * 64) / 64


def init_case_(module, seed):
    """The fixture's initial state of a freshly constructed module (reference or this project's): nn.Linear weights and biases
    rounded to multiples of 1/64, LayerNorm weight = 1 + N(0, 1) / 4 and bias = N(0, 1) / 4 from a generator seeded with
    seed + 1000, rounded likewise, so that dgamma, dbeta and the gamma factor of dx are exercised.  The module must have been built
    under torch.manual_seed(seed)."""
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(round64(m.weight))
                m.bias.copy_(round64(m.bias))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(round64(1 + torch.randn(m.weight.shape, generator=g) / 4))
                m.bias.copy_(round64(torch.randn(m.bias.shape, generator=g) / 4))
    return module


def case_input(name, seed):
    E, nh, T, nu, B = CASES[name][1]
    g = torch.Generator().manual_seed(seed + 2000)
    return round64(torch.randn(B, T, E, generator=g))


def case_past(name, seed):
    """(layer_past (2, B, n_head, PAST_LEN, hs), the PAST_NEW new tokens (B, PAST_NEW, E)) of a PAST_CASES case"""
    E, nh, T, nu, B = CASES[name][1]
    g = torch.Generator().manual_seed(seed + 3000)
    return round64(torch.randn(2, B, nh, PAST_LEN, E // nh, generator=g)), round64(torch.randn(B, PAST_NEW, E, generator=g))


def cotangent(shape, dtype):
    """unet_dis_ref.weight_pattern for a (B, T, E) tensor: the pattern of its (B, E, T, 1) channels-last view"""
    from unet_dis_ref import weight_pattern
    B, T, E = shape
    return weight_pattern((B, E, T, 1), dtype)[..., 0].transpose(1, 2)


def case_ref(name, x, st, layer_past=None):
    """(output, present) of a case through the restatement"""
    return CASES[name][2](x, st, "", CASES[name][1][1], layer_past)


VARIANTS = ("threads8", "threads1", "batch_reversed")


def grads_ref(name, state, x, dtype, variant="threads8"):
    """(output, present, {parameter name / "input": gradient}) of sum <output, cotangent> through the restatement.  The variants are
    mathematically identical fp32 evaluations: eight threads, one thread, the batch in reversed order."""
    st = {}
    for k, v in state.items():
        v = v.detach().clone()
        st[k] = v if k.endswith("mask") else v.to(dtype).requires_grad_(True)
    rev = variant == "batch_reversed"
    xin = (x.flip(0) if rev else x).detach().clone().to(dtype).requires_grad_(True)
    n = torch.get_num_threads()
    torch.set_num_threads(1 if variant == "threads1" else n)
    try:
        out, present = case_ref(name, xin, st)
        cot = cotangent(out.shape, dtype)
        (out * (cot.flip(0) if rev else cot)).sum().backward()
    finally:
        torch.set_num_threads(n)
    grads = {k: v.grad for k, v in st.items() if not k.endswith("mask")}
    grads["input"] = xin.grad.flip(0) if rev else xin.grad
    out, present = out.detach(), present.detach()
    return (out.flip(0), present.flip(1), grads) if rev else (out, present, grads)
