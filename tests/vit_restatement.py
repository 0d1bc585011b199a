"""Own-words torch restatement of the Point-BERT transformer encoder (PointDA/model_utils.py:201-289: Mlp, Attention, Block,
TransformerEncoder), parameterised by dtype: the float64 yardstick of tests/test_gpu_vit.py and, in fp32 on the CPU, the stand-in for the
reference's own rounding where no golden exists.  Plain torch ops only; runs anywhere.

A block's parameters are a dict keyed like its state_dict (BLOCK_KEYS, `attn.qkv.bias` only with qkv_bias); an encoder's are keyed
`blocks.<i>.<block key>`.  `scales`: optional DropPath scales, one [B] tensor (mask / keep_prob) per DropPath call in call order -- two
per block, after the attention and after the MLP; None stands for the identity."""
import math

import torch

BLOCK_KEYS = ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
              "mlp.fc2.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias")
FETCH = (3, 7, 11)
EPS = 1e-5


def block_keys(qkv_bias):
    return [k for k in BLOCK_KEYS if qkv_bias or k != "attn.qkv.bias"]


def _norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    return c / torch.sqrt((c * c).mean(-1, keepdim=True) + EPS) * w + b


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def attention_logits(p, y, heads, scale=None):
    """y [B,L,C] (the normalised input) -> (scaled logits [B,H,L,L], v [B,H,L,dh])"""
    B, L, C = y.shape
    dh = C // heads
    qkv = y @ p["attn.qkv.weight"].t()
    if "attn.qkv.bias" in p:
        qkv = qkv + p["attn.qkv.bias"]
    q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(B, L, heads, dh).transpose(1, 2) for i in range(3))
    return (q @ k.transpose(-1, -2)) * (scale or dh ** -0.5), v


def block_forward(params, x, heads, dtype=torch.float64, scale=None, scales=None, return_logits=False):
    """x [B,L,C] -> [B,L,C].  Tensors that require grad keep doing so (cast with .to(dtype))."""
    p = {k: v.to(dtype) for k, v in params.items()}
    x = x.to(dtype)
    B, L, C = x.shape
    s1, s2 = (None, None) if scales is None else scales

    def path(t, s):
        return t if s is None else t * s.to(dtype).view(B, 1, 1)
    logits, v = attention_logits(p, _norm(x, p["norm1.weight"], p["norm1.bias"]), heads, scale)
    if return_logits:
        return logits
    o = (torch.softmax(logits, dim=-1) @ v).transpose(1, 2).reshape(B, L, C)
    x = x + path(o @ p["attn.proj.weight"].t() + p["attn.proj.bias"], s1)
    h = _gelu(_norm(x, p["norm2.weight"], p["norm2.bias"]) @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"])
    return x + path(h @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"], s2)


def encoder_forward(params, x, pos, heads, depth, dtype=torch.float64, scale=None, scales=None):
    """-> (x, feature_list): every block runs on x + pos; the outputs of blocks 3, 7, 11 are collected"""
    x, pos = x.to(dtype), pos.to(dtype)
    feats = []
    for i in range(depth):
        pre = "blocks.%d." % i
        bp = {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
        x = block_forward(bp, x + pos, heads, dtype, scale, None if scales is None else scales[2 * i:2 * i + 2])
        if i in FETCH:
            feats.append(x)
    return x, feats


def block_grads(params, x, R, heads, dtype=torch.float64, scale=None, scales=None):
    """-> (out, {"x": d, <param key>: d, ...}) of the scalar (out * R).sum()"""
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xl = x.detach().to(dtype).requires_grad_(True)
    out = block_forward(leaves, xl, heads, dtype, scale, scales)
    (out * R.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["x"] = xl.grad
    return out.detach(), grads


def encoder_grads(params, x, pos, R, R2, heads, depth, dtype=torch.float64, scale=None, scales=None):
    """-> (out, feature_list, {"x", "pos", <param key>}) of (out * R).sum() + sum_f (feature_list[f] * R2[f]).sum(); R2: a list"""
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xl, pl = (t.detach().to(dtype).requires_grad_(True) for t in (x, pos))
    out, feats = encoder_forward(leaves, xl, pl, heads, depth, dtype, scale, scales)
    loss = (out * R.to(dtype)).sum()
    for f, r in zip(feats, R2):
        loss = loss + (f * r.to(dtype)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["x"], grads["pos"] = xl.grad, pl.grad
    return out.detach(), [f.detach() for f in feats], grads


def random_block_params(dim, hidden, seed, qkv_bias=False, scale=1.0, prefix=""):
    """nn.Linear's default initialisation ranges and LayerNorm weights / biases off their (1, 0) defaults, from a seeded generator (fp32)"""
    g = torch.Generator().manual_seed(seed)

    def u(shape, fan_in):
        return (torch.rand(shape, generator=g) * 2 - 1) * (scale / math.sqrt(fan_in))
    p = {"norm1.weight": 1 + 0.2 * torch.randn(dim, generator=g), "norm1.bias": 0.1 * torch.randn(dim, generator=g),
         "norm2.weight": 1 + 0.2 * torch.randn(dim, generator=g), "norm2.bias": 0.1 * torch.randn(dim, generator=g),
         "mlp.fc1.weight": u((hidden, dim), dim), "mlp.fc1.bias": u((hidden,), dim),
         "mlp.fc2.weight": u((dim, hidden), hidden), "mlp.fc2.bias": u((dim,), hidden),
         "attn.qkv.weight": u((3 * dim, dim), dim), "attn.qkv.bias": u((3 * dim,), dim),
         "attn.proj.weight": u((dim, dim), dim), "attn.proj.bias": u((dim,), dim)}
    return {prefix + k: p[k] for k in block_keys(qkv_bias)}


def dist(a, b):
    """max|a - b| / max|b|"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
