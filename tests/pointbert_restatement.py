"""Own-words torch restatement of the Point-BERT PointTransformer (PointDA/Models.py:365-531) with its Group and Encoder
(PointDA/model_utils.py:170-198, 292-336) and of the two ops of csrc/token.hip, parameterised by dtype: the float64 yardstick of
tests/test_gpu_pointbert.py and, in fp32, the stand-in for the reference's own rounding (tests/test_pointbert_cpu.py pins it to the
reference's fixtures).  Plain torch ops only; runs anywhere.  The transformer stack is vit_restatement's, DGCNN_Propagation
dgprop_restatement's.

Parameters and buffers are one dict keyed like the state_dict.  Every discrete choice is an input (`graph`, a dict):
    fps_g [B,G], fps_512 [B,512], fps_256 [B,256]           farthest-point indices (the last two on the DefRec path only)
    knn_group [B,G,M]                                        each centre's neighbours among the cloud's points
    nn3_2, nn3_1, nn3_0 = (idx [B,n,3], d2 [B,n,3])          the 3-NN of level 2 and level 1 among the centres, of the points among level 1,
                                                             with their squared distances (the interpolation weights are built from these)
    pro2 = (idx1, idx2), pro1 = (idx1, idx2)                 the two stage graphs of each DGCNN_Propagation
and `sel` (optional list) the arg-max selections in call order: the Encoder's three maxima over M ([B*G, C] slots), the token pooling
([B, d] rows), then for dgcnn_pro_2 and dgcnn_pro_1 their two stage selections ([B*n, C] slots).  With `sel` every maximum is a gather of
the given entry, which routes a gradient the way a kernel's recorded selection does."""
import math

import torch

import dgprop_restatement as DG
import vit_restatement as VR
from dgprop_restatement import hash_fill  # noqa: F401  (the fixtures' weight fill)

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 3
BN_EPS, BN_MOMENTUM, LN_EPS = 1e-5, 0.1, 1e-5


def _act(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_GELU:
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    return z


def batch_norm(y, gamma, beta, run_mean, run_var, training, eps=BN_EPS, momentum=BN_MOMENTUM):
    """y [rows, C] -> (normalised, mean, invstd, new running mean, new running var): biased variance to normalise, unbiased for the buffer"""
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        n = y.shape[0]
        new_rm = None if run_mean is None else (1 - momentum) * run_mean + momentum * mean.detach()
        new_rv = None if run_var is None else (1 - momentum) * run_var + momentum * var.detach() * (n / (n - 1.0))
    else:
        mean, var, new_rm, new_rv = run_mean, run_var, run_mean, run_var
    invstd = 1.0 / torch.sqrt(var + eps)
    return (y - mean) * invstd * gamma + beta, mean, invstd, new_rm, new_rv


def thin_in(X, W, bias, gamma=None, beta=None, run_mean=None, run_var=None, training=True, act=ACT_RELU, dtype=torch.float64,
            eps=BN_EPS, momentum=BN_MOMENTUM):
    """the op of functional.thin_in the plain way -> dict(H, mean, invstd, run_mean, run_var) (the last four None without BatchNorm)"""
    c = lambda t: None if t is None else t.to(dtype)                        # noqa: E731
    X, W, bias, gamma, beta, run_mean, run_var = (c(t) for t in (X, W, bias, gamma, beta, run_mean, run_var))
    y = X @ W.t()
    if bias is not None:
        y = y + bias
    if gamma is None:
        return {"H": _act(y, act), "mean": None, "invstd": None, "run_mean": None, "run_var": None}
    z, mean, invstd, rm, rv = batch_norm(y, gamma, beta, run_mean, run_var, training, eps, momentum)
    return {"H": _act(z, act), "mean": mean, "invstd": invstd, "run_mean": rm, "run_var": rv}


def token_pool(y, arg=None):
    """y [B,L,d] -> [B, 2 d] = y[:, 0] | max over the rows 1 .. L-1 (or the rows `arg` [B,d], local to the cloud)"""
    if arg is None:
        return torch.cat([y[:, 0], y[:, 1:].max(1)[0]], dim=-1)
    return torch.cat([y[:, 0], y.gather(1, arg.long().unsqueeze(1)).squeeze(1)], dim=-1)


def index_points(points, idx):
    raw = idx.shape
    flat = idx.reshape(raw[0], -1).long()
    return points.gather(1, flat.unsqueeze(-1).expand(-1, -1, points.shape[-1])).reshape(*raw, -1)


def group(xyz, fps_idx, knn_idx):
    """xyz [B,N,3] -> (neighborhood [B,G,M,3], center [B,G,3])"""
    center = index_points(xyz, fps_idx)
    return index_points(xyz, knn_idx) - center.unsqueeze(2), center


def _seg_max(feat, M, sel):
    """feat [R, C] -> [R // M, C]: max over every M consecutive rows, or the slots `sel` [R // M, C]"""
    f = feat.view(-1, M, feat.shape[1])
    if sel is None:
        return f.max(1)[0]
    return f.gather(1, sel.long().unsqueeze(1)).squeeze(1)


class _Run:
    """the walk's state: parameters in the working dtype, the mode, the selections still to consume, the buffers BatchNorm leaves"""

    def __init__(self, params, training, dtype, sel):
        self.p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
        self.training, self.dtype = training, dtype
        self.sel = None if sel is None else list(sel)
        self.buffers = {}

    def take(self):
        return None if self.sel is None else self.sel.pop(0)

    def conv_bn_relu(self, x, conv, bn):
        p = self.p
        y = x @ p[conv + ".weight"].flatten(1).t() + p[conv + ".bias"]
        z, _, _, rm, rv = batch_norm(y, p[bn + ".weight"], p[bn + ".bias"], p[bn + ".running_mean"], p[bn + ".running_var"], self.training)
        self.buffers[bn + ".running_mean"], self.buffers[bn + ".running_var"] = rm, rv
        return torch.relu(z)

    def conv(self, x, conv):
        return x @ self.p[conv + ".weight"].flatten(1).t() + self.p[conv + ".bias"]


def _encoder(run, pre, neighborhood):
    """neighborhood [B,G,M,3] -> [B*G, C] (model_utils.py:316-336, point-major)"""
    B, G, M, _ = neighborhood.shape
    x = neighborhood.reshape(B * G * M, 3)
    feat = run.conv(run.conv_bn_relu(x, pre + "first_conv.0", pre + "first_conv.1"), pre + "first_conv.3")
    for seq in ("add_conv1", "second_conv"):
        glob = _seg_max(feat, M, run.take())
        cat = torch.cat([glob.unsqueeze(1).expand(-1, M, -1).reshape(B * G * M, -1), feat], dim=1)
        feat = run.conv(run.conv_bn_relu(cat, pre + seq + ".0", pre + seq + ".1"), pre + seq + ".3")
    return _seg_max(feat, M, run.take())


def encoder(params, neighborhood, training=True, dtype=torch.float64, sel=None, prefix=""):
    """-> (tokens [B,G,C], buffers)"""
    run = _Run(params, training, dtype, sel)
    B, G = neighborhood.shape[:2]
    return _encoder(run, prefix, neighborhood.to(dtype)).view(B, G, -1), run.buffers


def _layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    return c / torch.sqrt((c * c).mean(-1, keepdim=True) + LN_EPS) * w + b


def _propagation(run, pre, pts1, nn3, feat2):
    """PointNetFeaturePropagation, point-major: pts1 [B,n,3] (coordinates, also the skip features), nn3 = (idx, d2) of its points among the
    sampled ones, feat2 [B,S,C] -> [B,n,C']"""
    idx, d2 = nn3
    w = 1.0 / (d2.to(run.dtype) + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    interp = (index_points(feat2, idx) * w.unsqueeze(-1)).sum(2)
    B, n, _ = pts1.shape
    x = torch.cat([pts1, interp], dim=-1).reshape(B * n, -1)
    i = 0
    while pre + "mlp_convs.%d.weight" % i in run.p:
        x = run.conv_bn_relu(x, pre + "mlp_convs.%d" % i, pre + "mlp_bns.%d" % i)
        i += 1
    return x.view(B, n, -1)


def _edge_conv(fk, fq, idx, W):
    """dgprop_restatement.edge_values as a plain product: fk [B,Nk,Cin], fq [B,Nq,Cin], idx [B,Nq,k], W [Cout, 2 Cin] -> [B,Cout,Nq,k].
    (Its F.conv2d on the permuted, strided edge tensor loses fp32 digits in the backward at these shapes on the CPU -- 4e-2 of a weight
    gradient against both float64 and the reference, measured while pinning this file; the product below agrees with both to 3e-6.)"""
    B, Nq, k = idx.shape
    Cin = fk.shape[2]
    nb = fk.gather(1, idx.reshape(B, Nq * k, 1).expand(-1, -1, Cin)).view(B, Nq, k, Cin)
    ctr = fq.unsqueeze(2).expand(-1, -1, k, -1)
    return (torch.cat([nb - ctr, ctr], dim=-1) @ W.t()).permute(0, 3, 1, 2)


def _dgcnn_pro(run, pre, coor, f, coor_q, f_q, graphs):
    """point-major in and out: f [B,G,C], f_q [B,n,C] -> [B,n,C]; the normalisation, activation and maximum are dgprop_restatement's"""
    p = {k: run.p[pre + k] for k in DG.KEYS}
    a1, a2 = run.take(), run.take()
    B, n = f_q.shape[:2]
    if a1 is not None:
        a1, a2 = a1.view(B, n, -1), a2.view(B, n, -1)
    y1 = _edge_conv(f, f_q, graphs[0].long(), p["layer1.0.weight"].flatten(1))
    h = DG.norm_act_max(y1, p["layer1.1.weight"], p["layer1.1.bias"], argk=a1)
    y2 = _edge_conv(h, h, graphs[1].long(), p["layer2.0.weight"].flatten(1))
    return DG.norm_act_max(y2, p["layer2.1.weight"], p["layer2.1.bias"], argk=a2)


def forward(params, cfg, pts, graph, activate_DefRec=False, training=True, dtype=torch.float64, sel=None):
    """cfg: an object with trans_dim, depth, num_heads, num_group, group_size.  pts [B,N,3] -> (logits [B,cls_dim] | DefRec output [B,N,3],
    buffers: the running statistics after the forward).  The head's dropout is the identity (rate 0 or eval mode)."""
    run = _Run(params, training, dtype, sel)
    p = run.p
    pts = pts.to(dtype)
    B, N, _ = pts.shape
    d, G = cfg.trans_dim, cfg.num_group
    neighborhood, center = group(pts, graph["fps_g"], graph["knn_group"])
    tokens = _encoder(run, "encoder.", neighborhood).view(B, G, -1)
    tokens = tokens @ p["reduce_dim.weight"].t() + p["reduce_dim.bias"]
    pos = _act(center @ p["pos_embed.0.weight"].t() + p["pos_embed.0.bias"], ACT_GELU) @ p["pos_embed.2.weight"].t() + p["pos_embed.2.bias"]
    x = torch.cat([p["cls_token"].expand(B, -1, -1), tokens], dim=1)
    pos = torch.cat([p["cls_pos"].expand(B, -1, -1), pos], dim=1)
    bp = {k[len("blocks."):]: v for k, v in p.items() if k.startswith("blocks.")}
    x, feats = VR.encoder_forward(bp, x, pos, cfg.num_heads, cfg.depth, dtype)
    x = _layer_norm(x, p["norm.weight"], p["norm.bias"])
    concat_f = token_pool(x, run.take())
    if not activate_DefRec:
        h = torch.relu(concat_f @ p["cls_head_finetune.0.weight"].t() + p["cls_head_finetune.0.bias"])
        return h @ p["cls_head_finetune.3.weight"].t() + p["cls_head_finetune.3.bias"], run.buffers
    feats = [_layer_norm(t, p["norm.weight"], p["norm.bias"])[:, 1:] for t in feats]
    level_1, level_2 = index_points(pts, graph["fps_512"]), index_points(pts, graph["fps_256"])
    f3 = feats[2]
    f2 = _propagation(run, "propagation_2.", level_2, graph["nn3_2"], feats[1])
    f1 = _propagation(run, "propagation_1.", level_1, graph["nn3_1"], feats[0])
    f2 = _dgcnn_pro(run, "dgcnn_pro_2.", center, f3, level_2, f2, graph["pro2"])
    f1 = _dgcnn_pro(run, "dgcnn_pro_1.", level_2, f2, level_1, f1, graph["pro1"])
    f0 = _propagation(run, "propagation_0.", pts, graph["nn3_0"], f1)
    h = torch.cat([f0, concat_f.unsqueeze(1).expand(-1, N, -1)], dim=-1).reshape(B * N, -1)
    for i in (1, 2, 3):
        y = h @ p["DefRec.conv%d.weight" % i].flatten(1).t()
        bn = "DefRec.bn%d" % i
        z, _, _, rm, rv = batch_norm(y, p[bn + ".weight"], p[bn + ".bias"], p[bn + ".running_mean"], p[bn + ".running_var"], training)
        run.buffers[bn + ".running_mean"], run.buffers[bn + ".running_var"] = rm, rv
        h = torch.relu(z)
    return (h @ p["DefRec.conv4.weight"].flatten(1).t()).view(B, N, 3), run.buffers


def grads(params, cfg, pts, graph, Rw, activate_DefRec=False, training=True, dtype=torch.float64, sel=None):
    """-> (out, {param key: gradient of (out * Rw).sum()}, buffers); a parameter the path does not reach has no entry"""
    leaves = {k: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.detach())
              for k, v in params.items()}
    out, buffers = forward(leaves, cfg, pts, graph, activate_DefRec, training, dtype, sel)
    (out * Rw.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items() if v.requires_grad and v.grad is not None}, buffers


def three_nn(ref, qry):
    """ref [B,S,3], qry [B,n,3] -> (idx [B,n,3], d2 [B,n,3]): the reference's square_distance(...).sort()[:, :, :3]"""
    d2 = torch.sum((qry[:, :, None] - ref[:, None]) ** 2, dim=-1)
    d, idx = d2.sort(dim=-1)
    return idx[:, :, :3], d[:, :, :3]


def dist(a, b):
    return VR.dist(a, b)


def load_fixture(path):
    """a tests/golden/ptrans_*.npz of tools/make_golden_pointbert.py -> (z, cfg, params, graph): params keyed like the state_dict (stored
    tensors, hash-filled large ones, fresh BatchNorm buffers), graph as forward() takes it (int64 indices)"""
    import types
    import numpy as np
    z = np.load(path)
    d, depth, heads, M, G, enc, cls_dim = (int(v) for v in z["cfg"])
    cfg = types.SimpleNamespace(trans_dim=d, depth=depth, drop_path_rate=0.0, cls_dim=cls_dim, num_heads=heads, group_size=M, num_group=G,
                                encoder_dims=enc, encoder_type="Encoder", dropout=0.0, model="PointTransformer")
    params = {}
    for k, shape in zip(z["keys"], z["shapes"]):
        k, shape = str(k), tuple(int(s) for s in shape if s > 0)
        if "p." + k in z.files:
            params[k] = torch.from_numpy(z["p." + k])
        elif "wseed." + k in z.files:
            params[k] = torch.from_numpy(hash_fill(shape, int(z["wseed." + k]), float(z["wscale." + k])))
        elif k.endswith("running_mean"):
            params[k] = torch.zeros(shape)
        elif k.endswith("running_var"):
            params[k] = torch.ones(shape)
        else:
            assert k.endswith("num_batches_tracked"), k
            params[k] = torch.zeros((), dtype=torch.long)
        assert tuple(params[k].shape) == shape, (k, params[k].shape, shape)
    lng = lambda name: torch.from_numpy(z[name]).long()                     # noqa: E731
    graph = {"fps_g": lng("fps_g"), "knn_group": lng("knn_group")}
    if "fps_512" in z.files:
        graph.update({"fps_512": lng("fps_512"), "fps_256": lng("fps_256"), "pro2": (lng("pro2.idx1"), lng("pro2.idx2")),
                      "pro1": (lng("pro1.idx1"), lng("pro1.idx2"))})
        for key in ("nn3_2", "nn3_1", "nn3_0"):
            graph[key] = (lng(key + ".idx"), torch.from_numpy(z[key + ".d2"]))
    return z, cfg, params, graph


def stored_selections(path, z, tag):
    """the reference's own arg-max selections of path `tag`, in call order (a companion file ..._sel.npz holds them where the fixture does not)"""
    import os
    import numpy as np
    src = z if tag + ".sel0" in z.files else np.load(os.path.splitext(path)[0] + "_sel.npz")
    out, i = [], 0
    while "%s.sel%d" % (tag, i) in src.files:
        out.append(torch.from_numpy(src["%s.sel%d" % (tag, i)]))
        i += 1
    return out


def stored_grad(z, tag, key, g):
    """(what the fixture stores for parameter `key` on path `tag`, the matching part of the gradient `g`), or None when it stores none"""
    if "%s.g.%s" % (tag, key) in z.files:
        return torch.from_numpy(z["%s.g.%s" % (tag, key)]), g
    if "%s.g16.%s" % (tag, key) in z.files:
        return torch.from_numpy(z["%s.g16.%s" % (tag, key)]), g[::16]
    return None


def residue_bias(key):
    """True for a conv bias whose gradient is exactly 0 in exact arithmetic in training mode: a per-channel constant that only reaches a
    batch-statistics BatchNorm (the Encoder's biases before its last conv -- first_conv.3 / add_conv1.3 shift the per-point feature and its
    group maximum alike -- and the feature-propagation convs).  What fp32 or fp64 report there is rounding residue of sums that cancel; the
    tests measure it against the same layer's weight gradient, whose entries sum the same terms."""
    if not key.endswith(".bias"):
        return False
    if key.startswith("encoder."):
        return ".1." not in key and not key.startswith("encoder.second_conv.3")
    return key.startswith("propagation_") and ".mlp_convs." in key
