"""Generate tests/golden/ptrans_*.npz: the UNMODIFIED reference's PointTransformer (PointDA/Models.py:365-531), run on the CPU in fp32 with
autograd.  Build-container only (imports the reference through tools/ref_import.py); the fixtures are numeric and string arrays.

    python tools/make_golden_pointbert.py

Stand-ins for what is not installed anywhere, all plain torch: knn_cuda.KNN (make_golden_propagation's: squared distances, a stable
ascending sort, the first k), pointnet2_ops' furthest_point_sample (start at point 0, ties -> the lower index) and gather_operation.  The
stand-ins log what they return, so the fixture holds every graph index the reference used.  drop_path_rate is 0, where the reference
uses nn.Identity (ref_import's DropPath stub cannot be constructed; make_golden_vit.py runs the stack the same way).  The classification
head's Dropout(0.5) has its rate set to 0 after construction.

  ptrans_cls_s0_B2_N40_G5_M7_d24_h2_depth2.npz            classification path
  ptrans_def_s1_B2_N520_G8_M8_d32_h2_depth12_e32.npz      both paths ("cls." and "def." entries); config dropout 0
In both, the reference's two DGCNN_Propagation Sequentials (fixed at 384 / 512 channels) are replaced after construction by the same three
layers at widths (2 d -> 512, 1024 -> d), as dgprop_s0 does.  After construction every BatchNorm / GroupNorm weight is drawn from N(0,1)
(some negative) and their biases moved off 0, the LayerNorm weights and biases are moved off (1, 0) as make_golden_vit.py does; tensors of more than BIG entries are refilled with
tests/dgprop_restatement.hash_fill from their seed ("wseed.<key>", scale "wscale.<key>") and not stored.

Each fixture stores: pts; the graph (fps_g, knn_group; on the DefRec path fps_512, fps_256, nn3_{2,1,0}.idx / .d2, pro{2,1}.idx{1,2});
per path the output "<path>.out", a fixed random "<path>.R" and the gradients of (out * R).sum() -- "<path>.g.<key>", or every 16th row
"<path>.g16.<key>" of a BIG tensor; "p.<key>" for the stored tensors; "keys" / "shapes" (the state_dict); "fresh.keys" / "fresh.sums":
the float64 sum of every tensor of the freshly constructed module under "seed" whose draw does not depend on the DGCNN_Propagation widths
(everything but dgcnn_pro_* and DefRec.*); the reference's arg-max selections "<path>.sel<i>" in call order, in the layouts of
functional.recorded_selections (the def fixture's in a companion file ..._sel.npz, to stay under the size limit); "cfg" = [trans_dim, depth, num_heads, group_size, num_group, encoder_dims, cls_dim].
The module is constructed under "seed"; the perturbation, the input and R come from a generator seeded 1000 + seed + 100 "draw", and the
draw is the first on which the reference's own fp32 gradients are within OWN_ERROR of the same module run in float64 ("<path>.own_error"):
two fp32 evaluations of a graph can only be held to 1e-5 of each other where rounding decides no ReLU mask, selection or neighbour.
(torch's threaded CPU reductions move that figure by about 1e-6 from run to run, so a second run of this tool may stop at another draw.)
The cls fixture also stores the reference's own widths (trans_dim 384, depth 12; "ref.seed"): "ref.keys", "ref.shapes", "ref.sums" of all
its 246 tensors.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402
import pointbert_restatement as PR  # noqa: E402
import dgprop_restatement as DG  # noqa: E402
from make_golden_propagation import KNN  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
BIG = 1000
OWN_ERROR = 5e-6          # a draw is kept when the reference's fp32 gradients are this close to its own float64 run: half of 1e-5
MAX_DRAWS = 200
LOG = {"knn": [], "fps": [], "max": []}


class LoggedKNN(KNN):
    def __call__(self, ref, query):
        d, idx = KNN.__call__(self, ref, query)
        LOG["knn"].append(idx if self.transpose_mode else idx.transpose(1, 2))
        return d, idx

    forward = __call__


def furthest_point_sample(xyz, npoint):
    idx = DG.fps_from_zero(xyz, npoint)
    LOG["fps"].append(idx)
    return idx


def gather_operation(features, idx):
    return features.gather(2, idx.long().unsqueeze(1).expand(-1, features.shape[1], -1))


class logged_max:
    """While active, torch.max(t, dim) / t.max(dim) log the indices they return, in call order: the reference's arg-max selections (the
    Encoder's three maxima over the group, the token pooling, the two stages of each DGCNN_Propagation)."""

    def __enter__(self):
        self.fn, self.meth = torch.max, torch.Tensor.max

        def wrap(orig):
            def logged(*a, **k):
                r = orig(*a, **k)
                if hasattr(r, "indices"):
                    LOG["max"].append(r.indices.detach())
                return r
            return logged
        torch.max, torch.Tensor.max = wrap(self.fn), wrap(self.meth)

    def __exit__(self, *exc):
        torch.max, torch.Tensor.max = self.fn, self.meth
        return False


def npy(t):
    return t.detach().cpu().numpy()


def config(d, depth, heads, M, G, enc, cls_dim=10, dropout=0.0):
    return types.SimpleNamespace(trans_dim=d, depth=depth, drop_path_rate=0.0, cls_dim=cls_dim, num_heads=heads, group_size=M, num_group=G,
                                 encoder_dims=enc, encoder_type="Encoder", dropout=dropout, model="PointTransformer")


def sums_of(m):
    sd = m.state_dict()
    return list(sd.keys()), [tuple(v.shape) for v in sd.values()], [float(v.double().sum()) for v in sd.values()]


def shapes_array(shapes):
    out = np.zeros((len(shapes), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        out[i, :len(s)] = s
    return out


def build(seed, cfg, draw=0):
    from PointDA.Models import PointTransformer
    nn = torch.nn
    torch.manual_seed(seed)
    m = PointTransformer(cfg)
    keys, _, sums = sums_of(m)
    c = {"seed": np.array(seed), "draw": np.array(draw)}
    fresh = [(k, s) for k, s in zip(keys, sums) if not k.startswith(("dgcnn_pro_", "DefRec."))]
    c["fresh.keys"], c["fresh.sums"] = np.array([k for k, _ in fresh]), np.array([s for _, s in fresh], dtype=np.float64)
    d = cfg.trans_dim
    for pro in (m.dgcnn_pro_1, m.dgcnn_pro_2):
        pro.layer1 = nn.Sequential(nn.Conv2d(2 * d, 512, kernel_size=1, bias=False), nn.GroupNorm(4, 512), nn.LeakyReLU(negative_slope=0.2))
        pro.layer2 = nn.Sequential(nn.Conv2d(1024, d, kernel_size=1, bias=False), nn.GroupNorm(4, d), nn.LeakyReLU(negative_slope=0.2))
    m.cls_head_finetune[2].p = 0.0
    g = torch.Generator().manual_seed(1000 + seed + 100 * draw)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.BatchNorm1d, nn.GroupNorm)):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
            elif isinstance(mod, nn.LayerNorm):             # (make_golden_vit's perturbation: twelve blocks stay well conditioned)
                mod.weight.add_(0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.add_(0.1 * torch.randn(mod.bias.shape, generator=g))
        m.cls_token.copy_(0.5 * torch.randn(m.cls_token.shape, generator=g))
        for i, (name, p) in enumerate(m.named_parameters()):
            if p.numel() > BIG:
                fan_in = p[0].numel()
                s, sc = 7919 * seed + 31 * i + 5, float(np.sqrt(3.0 / fan_in))
                p.copy_(torch.from_numpy(PR.hash_fill(tuple(p.shape), s, sc)))
                c["wseed." + name], c["wscale." + name] = np.array(s), np.array(sc, dtype=np.float64)
    keys, shapes, _ = sums_of(m)
    c["keys"], c["shapes"] = np.array(keys), shapes_array(shapes)
    for name, p in m.named_parameters():
        if p.numel() <= BIG:
            c["p." + name] = npy(p)
    c["cfg"] = np.array([cfg.trans_dim, cfg.depth, cfg.num_heads, cfg.group_size, cfg.num_group, cfg.encoder_dims, cfg.cls_dim])
    return m, c, g


def own_error(m, pts, Rw, activate_DefRec):
    """the reference's own fp32 rounding: the worst distance max|a - b| / max|b| of its parameter gradients (m.grad, just computed) from
    the same module run in float64 on the same input (an exactly-zero bias gradient, pointbert_restatement.residue_bias, against its
    layer's weight gradient).  A graph index or a selection that float64 chooses differently shows as a large distance."""
    m64 = copy.deepcopy(m).double()
    m64.zero_grad()
    (m64(pts.double(), activate_DefRec=activate_DefRec) * Rw.double()).sum().backward()
    g32 = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    g64 = {n: p.grad for n, p in m64.named_parameters() if p.grad is not None}
    assert set(g32) == set(g64)
    worst = 0.0
    for n in g32:
        den = g64[n[:-len("bias")] + "weight"].abs().max() if PR.residue_bias(n) else g64[n].abs().max()
        worst = max(worst, float((g32[n].double() - g64[n]).abs().max() / den))
    return worst


def run_path(m, c, sel, g, pts, tag, activate_DefRec):
    LOG["knn"].clear(); LOG["fps"].clear(); LOG["max"].clear()
    m.zero_grad()
    m.train()
    with logged_max():
        out = m(pts, activate_DefRec=activate_DefRec)
    # the selections in the layouts of functional.recorded_selections: [groups, C] slots, [B, d] rows local to the cloud, [B n, C] slots
    mx = list(LOG["max"])
    assert len(mx) == (8 if activate_DefRec else 4), len(mx)
    for i in range(3):
        sel[tag + ".sel%d" % i] = npy(mx[i].reshape(mx[i].shape[0], -1)).astype(np.uint8)
    sel[tag + ".sel3"] = (npy(mx[3]) + 1).astype(np.int32)
    for i in range(4, len(mx)):
        sel[tag + ".sel%d" % i] = npy(mx[i].permute(0, 2, 1).reshape(-1, mx[i].shape[1])).astype(np.uint8)
    Rw = torch.randn(out.shape, generator=g)
    (out * Rw).sum().backward()
    c[tag + ".out"], c[tag + ".R"] = npy(out), npy(Rw)
    for name, p in m.named_parameters():
        if p.grad is None:
            continue
        if p.numel() > BIG:
            c[tag + ".g16." + name] = npy(p.grad)[::16]
        else:
            c[tag + ".g." + name] = npy(p.grad)
    knn, fps = list(LOG["knn"]), list(LOG["fps"])
    c["fps_g"], c["knn_group"] = npy(fps[0]).astype(np.int32), npy(knn[0]).astype(np.int32)
    if activate_DefRec:
        assert len(fps) == 3 and len(knn) == 5, (len(fps), len(knn))
        c["fps_512"], c["fps_256"] = npy(fps[1]).astype(np.int32), npy(fps[2]).astype(np.int32)
        for key, (i1, i2) in (("pro2", (1, 2)), ("pro1", (3, 4))):
            c[key + ".idx1"], c[key + ".idx2"] = npy(knn[i1]).astype(np.int32), npy(knn[i2]).astype(np.int32)
        center = PR.index_points(pts, fps[0])
        l1, l2 = PR.index_points(pts, fps[1]), PR.index_points(pts, fps[2])
        for key, (ref, qry) in (("nn3_2", (center, l2)), ("nn3_1", (center, l1)), ("nn3_0", (l1, pts))):
            idx, d2 = PR.three_nn(ref, qry)           # the reference's own square_distance + sort on the same fp32 inputs
            c[key + ".idx"], c[key + ".d2"] = npy(idx).astype(np.int32), npy(d2)
    else:
        assert len(fps) == 1 and len(knn) == 1, (len(fps), len(knn))
    c[tag + ".own_error"] = np.array(own_error(m, pts, Rw, activate_DefRec))


def main():
    ref_import.install_stubs()
    sys.modules["knn_cuda"].KNN = LoggedKNN
    p2 = sys.modules["pointnet2_ops.pointnet2_utils"]
    p2.furthest_point_sample, p2.gather_operation = furthest_point_sample, gather_operation
    for p in (ref_import.REF_ROOT + "/PointDA", ref_import.REF_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(8)
    out = {}

    def cls_case(draw):
        m, c, g = build(0, config(24, 2, 2, 7, 5, 32), draw)
        pts = torch.randn(2, 40, 3, generator=g)
        c["pts"] = npy(pts)
        run_path(m, c, c, g, pts, "cls", False)
        return float(c["cls.own_error"]), c, None

    def def_case(draw):
        m, c, g = build(1, config(32, 12, 2, 8, 8, 32), draw)
        pts = torch.randn(2, 520, 3, generator=g)
        c["pts"] = npy(pts)
        sel = {}
        run_path(m, c, sel, g, pts, "cls", False)
        run_path(m, c, sel, g, pts, "def", True)
        return max(float(c["cls.own_error"]), float(c["def.own_error"])), c, sel

    def first_good(case, label):
        """the first draw on which the reference's own fp32 error is under OWN_ERROR, half of the 1e-5 the tests hold a second fp32
        evaluation to (two evaluations within half the bound of the exact value are within the bound of each other).  A draw with a ReLU
        mask, a selection or a neighbour that rounding decides is 1e-3 or more and is passed over: at depth 12 on the DefRec path that is
        four draws in five, and the clean ones measure 4e-6 to 9e-6"""
        for draw in range(MAX_DRAWS):
            err, c, sel = case(draw)
            print("%s draw %d: own fp32 error %.2e" % (label, draw, err), flush=True)
            if err < OWN_ERROR:
                return c, sel
        raise SystemExit("no draw of %s under %g" % (label, OWN_ERROR))

    c, _ = first_good(cls_case, "cls")
    from PointDA.Models import PointTransformer
    torch.manual_seed(2)
    full = PointTransformer(config(384, 12, 6, 32, 64, 256, dropout=0.5))
    keys, shapes, sums = sums_of(full)
    assert len(keys) == 246
    c["ref.seed"], c["ref.keys"], c["ref.shapes"], c["ref.sums"] = np.array(2), np.array(keys), shapes_array(shapes), np.array(sums, dtype=np.float64)
    out["ptrans_cls_s0_B2_N40_G5_M7_d24_h2_depth2.npz"] = c

    c, sel = first_good(def_case, "def")
    out["ptrans_def_s1_B2_N520_G8_M8_d32_h2_depth12_e32.npz"] = c
    out["ptrans_def_s1_B2_N520_G8_M8_d32_h2_depth12_e32_sel.npz"] = sel

    for name, c in out.items():
        np.savez_compressed(os.path.join(OUT, name), **c)
        size = os.path.getsize(os.path.join(OUT, name))
        print(name, size, len(c))
        assert size < 1000000, size


if __name__ == "__main__":
    main()
