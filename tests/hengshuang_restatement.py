"""Own-words torch restatement of the Point Transformer models (PointDA/hengshuang_transformer/hengshuang_model.py: TransitionDown,
TransitionUp, Backbone, PointTransformerCls / Seg / Def) and of the two ops of csrc/pyramid.hip, parameterised by dtype: the float64
yardstick of tests/test_gpu_hengshuang.py and, in fp32, the stand-in for the reference's own rounding (tests/test_hengshuang_cpu.py pins
it to the reference's fixtures).  Plain torch ops only; runs anywhere.  The vector-attention block is vecattn_restatement's, the walk's
state (_Run), index_points and the DefRec head's BatchNorm are pointbert_restatement's; the BatchNorm layers of TransitionDown /
TransitionUp use torch's batch_norm (see _down).

Parameters and buffers are one dict keyed like the state_dict.  Every discrete choice is an input.  `graph`, a dict of lists (L = nblocks
+ 1 levels, level 0 the input cloud):
    fps_idx[i]   [B, N_{i+1}]             the centres TransitionDown i samples from level i
    down_knn[i]  [B, N_{i+1}, nneighbor]  their neighbourhoods in level i
    block_knn[l] [B, N_l, min(k, N_l)]    the TransformerBlock neighbours of level l (both blocks of a level use them)
    up_knn[i]    [B, N_l, 3], l = nblocks - 1 - i: the three nearest points of level l + 1 (None where that level has one point)
and `sel` (optional list) the neighbourhood-max selections of the TransitionDowns in order ([B N_{i+1}, C] slots): with it every maximum
is a gather of the given entry, which routes a gradient the way a kernel's recorded selection does."""
import torch

import vecattn_restatement as VA
from dgprop_restatement import hash_fill
from pointbert_restatement import _Run, batch_norm, index_points


def interp3_add(feat, add, idx=None, d2=None, dtype=torch.float64):
    """feat [B,S,C], add [B,N,C], idx [B,N,3], d2 [B,N,3] squared distances -> add + sum_j w_j feat[idx_j], w = 1 / (d2 + 1e-8) normalised.
    One source point: add + that row."""
    feat, add = feat.to(dtype), add.to(dtype)
    if feat.shape[1] == 1:
        return add + feat
    w = 1.0 / (d2.to(dtype) + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    return add + (index_points(feat, idx) * w.unsqueeze(-1)).sum(2)


def cloud_mean(x, dtype=torch.float64):
    """x [B,N,C] -> [B,C]"""
    return x.to(dtype).sum(1) / x.shape[1]


def sq_dist_to(xyz_q, xyz_src, idx):
    """squared distances of every query point to its listed source points: [B,N,3] coordinates, idx [B,N,K] -> [B,N,K]"""
    return ((xyz_q.unsqueeze(2) - index_points(xyz_src, idx)) ** 2).sum(-1)


def _linear_bn_relu(run, x, lin, bn):
    """relu(BatchNorm(x W^T + b)) on rows [R, Cin] with torch's own batch_norm (batch statistics in training mode, the running buffers
    otherwise); the buffers it would leave are recorded in run.buffers, the dict's own entries stay as they were"""
    p = run.p
    y = x @ p[lin + ".weight"].flatten(1).t() + p[lin + ".bias"]
    rm, rv = p[bn + ".running_mean"].clone(), p[bn + ".running_var"].clone()
    z = torch.nn.functional.batch_norm(y, rm, rv, p[bn + ".weight"], p[bn + ".bias"], run.training, 0.1, 1e-5)
    run.buffers[bn + ".running_mean"], run.buffers[bn + ".running_var"] = rm, rv
    return torch.relu(z)


def _stack(run, pre, x, slots):
    """Linear + ReLU at every slot but the last, a plain Linear there"""
    for n, s in enumerate(slots):
        x = x @ run.p["%s%d.weight" % (pre, s)].t() + run.p["%s%d.bias" % (pre, s)]
        if n < len(slots) - 1:
            x = torch.relu(x)
    return x


def _block(run, pre, xyz, feats, idx):
    p = {k: run.p[pre + k] for k in VA.PARAM_KEYS}
    return VA.block_forward(p, xyz, feats, idx, run.dtype)[0]


def _down(run, pre, xyz, points, fps_idx, knn_idx):
    """-> (new_xyz [B,S,3], new_points [B,S,C]).  The edge tensor is walked channel-major, [B, C, nsample, S], with torch's conv2d and
    batch_norm: the layout the reference's layers see, so that the fp32 run rounds its BatchNorm sums the way the reference's does."""
    F = torch.nn.functional
    B, S, ns = knn_idx.shape
    new_xyz = index_points(xyz, fps_idx)
    h = torch.cat([index_points(xyz, knn_idx) - new_xyz.unsqueeze(2), index_points(points, knn_idx)], dim=-1).permute(0, 3, 2, 1)
    i = 0
    while "%ssa.mlp_convs.%d.weight" % (pre, i) in run.p:
        conv, bn = "%ssa.mlp_convs.%d" % (pre, i), "%ssa.mlp_bns.%d" % (pre, i)
        rm, rv = run.p[bn + ".running_mean"].clone(), run.p[bn + ".running_var"].clone()
        h = F.conv2d(h, run.p[conv + ".weight"], run.p[conv + ".bias"])
        h = torch.relu(F.batch_norm(h, rm, rv, run.p[bn + ".weight"], run.p[bn + ".bias"], run.training, 0.1, 1e-5))
        run.buffers[bn + ".running_mean"], run.buffers[bn + ".running_var"] = rm, rv
        i += 1
    sel = run.take()
    if sel is None:
        out, arg = h.max(2)
        sel = arg.permute(0, 2, 1).reshape(B * S, -1)
    else:
        out = h.gather(2, sel.long().view(B, S, -1).permute(0, 2, 1).unsqueeze(2)).squeeze(2)
    run.buffers.setdefault("selections", []).append(sel)
    return new_xyz, out.transpose(1, 2)


def _up(run, pre, xyz1, points1, xyz2, points2, idx):
    """xyz1 / points1: the coarse level, xyz2 / points2: the fine one -> [B,N,C]"""
    def branch(name, x):
        B, n, _ = x.shape
        return _linear_bn_relu(run, x.reshape(B * n, -1), pre + name + ".0", pre + name + ".2").view(B, n, -1)
    f1, f2 = branch("fc1", points1), branch("fc2", points2)
    d2 = None if xyz1.shape[1] == 1 else sq_dist_to(xyz2, xyz1, idx)
    return interp3_add(f1, f2, idx, d2, run.dtype)


def transition_down(params, xyz, points, fps_idx, knn_idx, training=True, dtype=torch.float64, sel=None):
    """-> (new_xyz, new_points, buffers)"""
    run = _Run(params, training, dtype, sel)
    a, b = _down(run, "", xyz.to(dtype), points.to(dtype), fps_idx, knn_idx)
    return a, b, run.buffers


def transition_up(params, xyz1, points1, xyz2, points2, idx, training=True, dtype=torch.float64):
    """-> (out, buffers)"""
    run = _Run(params, training, dtype, None)
    return _up(run, "", xyz1.to(dtype), points1.to(dtype), xyz2.to(dtype), points2.to(dtype), idx), run.buffers


def _backbone(run, nblocks, x, graph):
    xyz = x[..., :3]
    points = _block(run, "backbone.transformer1.", xyz, _stack(run, "backbone.fc1.", x, (0, 2)), graph["block_knn"][0])
    levels = [(xyz, points)]
    for i in range(nblocks):
        xyz, points = _down(run, "backbone.transition_downs.%d." % i, xyz, points, graph["fps_idx"][i], graph["down_knn"][i])
        points = _block(run, "backbone.transformers.%d." % i, xyz, points, graph["block_knn"][i + 1])
        levels.append((xyz, points))
    return points, levels


def _decode(run, nblocks, points, levels, graph):
    xyz = levels[-1][0]
    points = _block(run, "transformer2.", xyz, _stack(run, "fc2.", points, (0, 2, 4)), graph["block_knn"][nblocks])
    for i in range(nblocks):
        fine_xyz, fine_points = levels[-i - 2]
        points = _up(run, "transition_ups.%d." % i, xyz, points, fine_xyz, fine_points, graph["up_knn"][i])
        xyz = fine_xyz
        points = _block(run, "transformers.%d." % i, xyz, points, graph["block_knn"][nblocks - 1 - i])
    return points


def forward(kind, params, nblocks, x, graph, activate_DefRec=False, training=True, dtype=torch.float64, sel=None):
    """kind "cls" | "seg" | "def"; x [B,N,d_points] -> (what the model returns, buffers: the running statistics after the forward, and
    under "selections" the list of neighbourhood-max selections used)"""
    run = _Run(params, training, dtype, sel)
    p = run.p
    x = x.to(dtype)
    B, N, _ = x.shape
    points, levels = _backbone(run, nblocks, x, graph)
    if kind == "cls":
        return _stack(run, "fc2.", cloud_mean(points, dtype), (0, 2, 4)), run.buffers
    if kind == "def" and not activate_DefRec:
        return _stack(run, "cls_head_finetune.", cloud_mean(points, dtype), (0, 2, 4)), run.buffers
    glob = cloud_mean(points, dtype)
    points = _decode(run, nblocks, points, levels, graph)
    if kind == "seg":
        return _stack(run, "fc3.", points, (0, 2, 4)), run.buffers
    h = torch.cat([points, glob.unsqueeze(1).expand(-1, N, -1)], dim=-1).reshape(B * N, -1)
    for i in (1, 2, 3):
        y = h @ p["DefRec.conv%d.weight" % i].flatten(1).t()
        bn = "DefRec.bn%d" % i
        z, _, _, rm, rv = batch_norm(y, p[bn + ".weight"], p[bn + ".bias"], p[bn + ".running_mean"], p[bn + ".running_var"], training)
        run.buffers[bn + ".running_mean"], run.buffers[bn + ".running_var"] = rm, rv
        h = torch.relu(z)
    return (h @ p["DefRec.conv4.weight"].flatten(1).t()).view(B, N, 3), run.buffers


def selections(kind, params, nblocks, x, graph, activate_DefRec=False, training=True, dtype=torch.float64):
    """the neighbourhood-max selections a free forward makes, in the layout of `sel`"""
    with torch.no_grad():
        return forward(kind, params, nblocks, x, graph, activate_DefRec, training, dtype)[1]["selections"]


def grads(kind, params, nblocks, x, graph, Rw, activate_DefRec=False, training=True, dtype=torch.float64, sel=None):
    """-> (out, {param key: gradient of (out * Rw).sum()}, buffers); a parameter the path does not reach has no entry"""
    leaves = {k: (v.detach().to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.detach())
              for k, v in params.items()}
    out, buffers = forward(kind, leaves, nblocks, x, graph, activate_DefRec, training, dtype, sel)
    (out * Rw.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in leaves.items() if v.requires_grad and v.grad is not None}, buffers


def levels(params, nblocks, x, graph, training=True, dtype=torch.float64, sel=None):
    """the backbone's [(xyz, points)] per level, detached: the inputs TransitionDown / TransitionUp see inside a model"""
    run = _Run(params, training, dtype, sel)
    with torch.no_grad():
        return [(a.detach(), b.detach()) for a, b in _backbone(run, nblocks, x.to(dtype), graph)[1]]


def fps(xyz, npoint, start):
    """farthest point sampling from the given first samples: xyz [B,N,3], start [B] -> [B,npoint] (the lowest index wins ties)"""
    B, N, _ = xyz.shape
    out = torch.zeros(B, npoint, dtype=torch.long)
    far = start.long().clone()
    best = torch.full((B, N), 1e10, dtype=xyz.dtype)
    for i in range(npoint):
        out[:, i] = far
        c = xyz[torch.arange(B), far].unsqueeze(1)
        best = torch.minimum(best, ((xyz - c) ** 2).sum(-1))
        far = best.argmax(-1)
    return out


def search_graph(x, nblocks, nneighbor, fps_idx):
    """the neighbour lists a model computes for given centres, the plain way (squared distances, argsort): x [B,N,>=3] -> graph"""
    xyz = x[..., :3]
    g = {"fps_idx": list(fps_idx), "down_knn": [], "block_knn": [VA.knn_index(xyz, nneighbor)], "up_knn": []}
    levels = [xyz]
    for i in range(nblocks):
        new_xyz = index_points(xyz, fps_idx[i])
        d = ((new_xyz[:, :, None] - xyz[:, None]) ** 2).sum(-1)
        g["down_knn"].append(d.argsort()[:, :, :nneighbor])
        xyz = new_xyz
        g["block_knn"].append(VA.knn_index(xyz, nneighbor))
        levels.append(xyz)
    for i in range(nblocks):
        coarse, fine = levels[nblocks - i], levels[nblocks - 1 - i]
        if coarse.shape[1] == 1:
            g["up_knn"].append(None)
        else:
            d = ((fine[:, :, None] - coarse[:, None]) ** 2).sum(-1)
            g["up_knn"].append(d.sort(dim=-1)[1][:, :, :3])
    return g


def residue_bias(key, training=True, kind="cls", nblocks=0):
    """True for a bias whose gradient is exactly 0 in exact arithmetic: the last bias of every block's fc_gamma (the same constant on
    all of a point's neighbours, which the softmax over them cancels) and, in training mode, a per-channel constant that only reaches
    batch-statistics BatchNorms -- the TransitionDown convs, the TransitionUp Linears, and the output bias fc2 of every block whose
    consumers all start with such a layer (every block but the backbone's last, which feeds the mean, and the Seg decoder's last, which
    feeds fc3).  What fp32 or fp64 report there is rounding residue of sums that cancel; the tests measure it against the same layer's
    weight gradient, whose entries sum the same terms."""
    if not key.endswith(".bias"):
        return False
    if key.endswith("fc_gamma.2.bias"):
        return True
    if not training:
        return False
    if ".sa.mlp_convs." in key or ("transition_ups." in key and key.endswith(("fc1.0.bias", "fc2.0.bias"))):
        return True
    if key in ("backbone.transformer1.fc2.bias", "transformer2.fc2.bias"):
        return nblocks >= 1
    for pre, last_is_free in (("backbone.transformers.", True), ("transformers.", kind == "seg")):
        if key.startswith(pre) and key.endswith(".fc2.bias"):
            i = int(key[len(pre):].split(".")[0])
            return i < nblocks - 1 or not last_is_free
    return False


def grad_dist(key, g, want, wants, training=True, kind="cls", nblocks=0):
    """max|g - want| / max|want|, an exactly-zero gradient (residue_bias) against the same layer's weight gradient in `wants`"""
    den = wants[key[:-len("bias")] + "weight"] if residue_bias(key, training, kind, nblocks) else want
    return float((g.double() - want.double()).abs().max() / den.double().abs().max().clamp_min(1e-300))


def dist(a, b):
    return VA.dist(a, b)


def load_fixture(path):
    """a tests/golden/hsg_*.npz of tools/make_golden_hengshuang.py -> (z, params, graph): params keyed like the state_dict (stored
    parameters, hash-filled large ones, fresh BatchNorm buffers), graph as forward() takes it (int64 indices)"""
    import numpy as np
    z = np.load(path)
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
    nblocks = int(z["cfg"][1])
    lng = lambda name: torch.from_numpy(z[name]).long() if name in z.files else None      # noqa: E731
    graph = {"fps_idx": [lng("fps_idx.%d" % i) for i in range(nblocks)], "down_knn": [lng("down_knn.%d" % i) for i in range(nblocks)],
             "block_knn": [lng("block_knn.%d" % i) for i in range(nblocks + 1)], "up_knn": [lng("up_knn.%d" % i) for i in range(nblocks)]}
    return z, params, graph
