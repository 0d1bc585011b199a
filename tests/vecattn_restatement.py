"""Own-words torch restatement of the vector-attention block (PointDA/hengshuang_transformer/transformer.py:28-44), parameterised by
dtype and neighbour index: the float64 yardstick of tests/test_gpu_transformer.py and, in fp32 on the CPU, the stand-in for the
reference's own rounding where no golden exists.  Plain torch ops only; runs anywhere."""
import math

import torch

PARAM_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc_delta.0.weight", "fc_delta.0.bias", "fc_delta.2.weight",
              "fc_delta.2.bias", "fc_gamma.0.weight", "fc_gamma.0.bias", "fc_gamma.2.weight", "fc_gamma.2.bias", "w_qs.weight",
              "w_ks.weight", "w_vs.weight")


def knn_index(xyz, k):
    """the reference's neighbour choice: |a|^2 + |b|^2 - 2 a.b, argsort, first min(k, N) columns"""
    d = -2 * xyz @ xyz.transpose(1, 2)
    d = d + (xyz ** 2).sum(-1)[:, :, None]
    d = d + (xyz ** 2).sum(-1)[:, None, :]
    return d.argsort()[:, :, :k]


def _rows(t, idx):
    """t [B,N,C], idx [B,N,K] -> [B,N,K,C]"""
    B, N, K = idx.shape
    flat = idx.reshape(B, N * K, 1).expand(-1, -1, t.shape[-1])
    return torch.gather(t, 1, flat).reshape(B, N, K, t.shape[-1])


def block_forward(params, xyz, features, idx, dtype=torch.float64, return_logits=False):
    """params: name -> tensor (PARAM_KEYS); xyz [B,N,3], features [B,N,d_points], idx int64 [B,N,K] -> (out, attn).  Tensors that
    require grad keep doing so (they are cast with .to(dtype)).  return_logits: -> the softmax's argument [B,N,K,d] instead."""
    p = {k: v.to(dtype) for k, v in params.items()}
    xyz, features = xyz.to(dtype), features.to(dtype)
    lin = torch.nn.functional.linear
    x = lin(features, p["fc1.weight"], p["fc1.bias"])
    q = lin(x, p["w_qs.weight"])
    kk = _rows(lin(x, p["w_ks.weight"]), idx)
    v = _rows(lin(x, p["w_vs.weight"]), idx)
    rel = xyz[:, :, None, :] - _rows(xyz, idx)
    pos = lin(torch.relu(lin(rel, p["fc_delta.0.weight"], p["fc_delta.0.bias"])), p["fc_delta.2.weight"], p["fc_delta.2.bias"])
    a = lin(torch.relu(lin(q[:, :, None, :] - kk + pos, p["fc_gamma.0.weight"], p["fc_gamma.0.bias"])),
            p["fc_gamma.2.weight"], p["fc_gamma.2.bias"])
    if return_logits:
        return a / math.sqrt(kk.shape[-1])
    attn = torch.softmax(a / math.sqrt(kk.shape[-1]), dim=2)
    res = (attn * (v + pos)).sum(2)
    return lin(res, p["fc2.weight"], p["fc2.bias"]) + features, attn


def block_grads(params, xyz, features, idx, R, dtype=torch.float64):
    """-> (out, attn, {"features": d, <param key>: d, ...}) of the scalar (out * R).sum()"""
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    f = features.detach().to(dtype).requires_grad_(True)
    out, attn = block_forward(leaves, xyz.detach(), f, idx, dtype)
    (out * R.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["features"] = f.grad
    return out.detach(), attn.detach(), grads


def random_params(d_points, d_model, seed, scale=1.0):
    """nn.Linear's default initialisation ranges, drawn from a seeded generator (fp32)"""
    g = torch.Generator().manual_seed(seed)

    def u(shape, fan_in):
        b = scale / math.sqrt(fan_in)
        return (torch.rand(shape, generator=g) * 2 - 1) * b
    d = d_model
    return {"fc1.weight": u((d, d_points), d_points), "fc1.bias": u((d,), d_points),
            "fc2.weight": u((d_points, d), d), "fc2.bias": u((d_points,), d),
            "fc_delta.0.weight": u((d, 3), 3), "fc_delta.0.bias": u((d,), 3),
            "fc_delta.2.weight": u((d, d), d), "fc_delta.2.bias": u((d,), d),
            "fc_gamma.0.weight": u((d, d), d), "fc_gamma.0.bias": u((d,), d),
            "fc_gamma.2.weight": u((d, d), d), "fc_gamma.2.bias": u((d,), d),
            "w_qs.weight": u((d, d), d), "w_ks.weight": u((d, d), d), "w_vs.weight": u((d, d), d)}


def dist(a, b):
    """max|a - b| / max|b|"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
