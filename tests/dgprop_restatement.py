"""Own-words torch restatement of DGCNN_Propagation (PointDA/Models.py:289-363) in the UNFOLDED form of the reference -- gather the
neighbours, concatenate [f_j - f_i ; f_i], 1x1 conv, group_norm, leaky_relu, max over the neighbours -- parameterised by dtype: the
float64 yardstick of tests/test_gpu_dgprop.py and, in fp32, the stand-in for the reference's own rounding.  Plain torch ops only; runs
anywhere.  Also the pieces the fixtures and the tests share: the kNN, farthest point sampling from index 0, and the integer-hash fill of
the reference-width conv weights (tools/make_golden_propagation.py imports it from here).

Parameters are a dict keyed like the state_dict (KEYS).  Every function takes the stage graph(s) as given index tensors; `argk`
(optional, [B, N, C] slot numbers) replaces the max over the neighbours by a gather of those slots, which routes a gradient the way a
kernel's recorded selection does."""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("layer1.0.weight", "layer1.1.weight", "layer1.1.bias", "layer2.0.weight", "layer2.1.weight", "layer2.1.bias")
GROUPS, EPS, SLOPE = 4, 1e-5, 0.2


def hash_fill(shape, seed, scale):
    """float32 array of `shape` whose entry at flat index n is a pure integer-hash function of (n, seed): uniform in [-scale, scale),
    no structure (a sin(a n + b) matrix has rank 2).  Exact 32-bit integer arithmetic: the same on every machine."""
    n = np.arange(int(np.prod(shape)), dtype=np.uint64)
    M = np.uint64(0xFFFFFFFF)
    x = (n * np.uint64(0x9E3779B1) + np.uint64(seed) * np.uint64(0x85EBCA6B) + np.uint64(0x165667B1)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    v = (x >> np.uint64(8)).astype(np.float64) / float(1 << 23) - 1.0          # 24 bits -> [-1, 1), exact in float32 after the scale's rounding
    return (v * scale).astype(np.float32).reshape(shape)


def knn(k, ref, qry):
    """ref [B,Nr,3], qry [B,Nq,3] -> (idx [B,Nq,k] int64, d2 [B,Nq,Nr]): squared distances, stable ascending sort, the first k"""
    d2 = ((qry.unsqueeze(2) - ref.unsqueeze(1)) ** 2).sum(-1)
    return d2.sort(dim=-1, stable=True)[1][:, :, :k], d2


def fps_from_zero(xyz, npoint):
    """xyz [B,N,3] -> [B,npoint] int64: farthest point sampling starting at index 0, ties -> the lower index"""
    B, N, _ = xyz.shape
    dist = torch.full((B, N), float("inf"), dtype=xyz.dtype, device=xyz.device)
    far = torch.zeros((B,), dtype=torch.long, device=xyz.device)
    out = []
    for _ in range(npoint):
        out.append(far)
        c = xyz[torch.arange(B, device=xyz.device), far].unsqueeze(1)
        d = ((xyz - c) ** 2).sum(-1)
        dist = torch.minimum(dist, d)
        far = dist.argmax(dim=1)
    return torch.stack(out, dim=1)


def edge_values(fk, fq, idx, W):
    """fk [B,Nk,Cin], fq [B,Nq,Cin], idx [B,Nq,k], W [Cout, 2 Cin] -> the conv over the edge tensor, [B,Cout,Nq,k]"""
    B, Nq, k = idx.shape
    Cin = fk.shape[2]
    nb = fk.gather(1, idx.reshape(B, Nq * k, 1).expand(-1, -1, Cin)).view(B, Nq, k, Cin)
    ctr = fq.unsqueeze(2).expand(-1, -1, k, -1)
    edge = torch.cat([nb - ctr, ctr], dim=-1).permute(0, 3, 1, 2)                       # [B, 2 Cin, Nq, k]
    return F.conv2d(edge, W.view(W.shape[0], W.shape[1], 1, 1))


def norm_act_max(y, gamma, beta, groups=GROUPS, eps=EPS, slope=SLOPE, argk=None, return_edges=False):
    """y [B,C,Nq,k] -> [B,Nq,C]: group_norm, leaky_relu, max over k (or the slots `argk` [B,Nq,C])"""
    z = F.leaky_relu(F.group_norm(y, groups, gamma, beta, eps), slope)
    if return_edges:
        return z
    if argk is None:
        return z.max(dim=-1)[0].permute(0, 2, 1)
    return z.gather(3, argk.long().permute(0, 2, 1).unsqueeze(-1)).squeeze(-1).permute(0, 2, 1)


def gn_edge_max(u, w, idx, gamma, beta, groups=GROUPS, eps=EPS, slope=SLOPE, dtype=torch.float64, argk=None, return_edges=False):
    """the op of functional.gn_edge_max on given u [B,Nk,C], w [B,Nq,C]: y = u[idx] + w built edge by edge -> [B,Nq,C]"""
    u, w, gamma, beta = (t.to(dtype) for t in (u, w, gamma, beta))
    B, Nq, k = idx.shape
    C = u.shape[2]
    y = u.gather(1, idx.long().reshape(B, Nq * k, 1).expand(-1, -1, C)).view(B, Nq, k, C) + w.unsqueeze(2)
    return norm_act_max(y.permute(0, 3, 1, 2), gamma, beta, groups, eps, slope, argk, return_edges)


def forward(params, coor, f, coor_q, f_q, idx1, idx2, dtype=torch.float64, argk=None, return_edges=False):
    """coor [B,3,G], f [B,C,G], coor_q [B,3,N], f_q [B,C,N] -> [B,C,N].  idx1 [B,N,k]: the neighbours of the query points among the
    G points; idx2 [B,N,k]: among themselves.  argk: None or the two stages' slot tensors.  return_edges: the two stages' activated
    edge tensors [B,C,N,k] instead."""
    p = {k: v.to(dtype) for k, v in params.items()}
    a1, a2 = (None, None) if argk is None else argk
    fk, fq = f.to(dtype).transpose(1, 2), f_q.to(dtype).transpose(1, 2)
    y1 = edge_values(fk, fq, idx1.long(), p["layer1.0.weight"].flatten(1))
    if return_edges:
        e1 = norm_act_max(y1, p["layer1.1.weight"], p["layer1.1.bias"], return_edges=True)
    h = norm_act_max(y1, p["layer1.1.weight"], p["layer1.1.bias"], argk=a1)
    y2 = edge_values(h, h, idx2.long(), p["layer2.0.weight"].flatten(1))
    if return_edges:
        return e1, norm_act_max(y2, p["layer2.1.weight"], p["layer2.1.bias"], return_edges=True)
    return norm_act_max(y2, p["layer2.1.weight"], p["layer2.1.bias"], argk=a2).permute(0, 2, 1)


def fps_downsample(coor, x, num_group):
    """coor [B,3,N], x [B,C,N] -> (idx [B,num_group], coor', x')"""
    idx = fps_from_zero(coor.transpose(1, 2), num_group)
    take = lambda t: t.gather(2, idx.unsqueeze(1).expand(-1, t.shape[1], -1))
    return idx, take(coor), take(x)
