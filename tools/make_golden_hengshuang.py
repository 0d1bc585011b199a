"""Generate tests/golden/hsg_*.npz: the UNMODIFIED reference's Point Transformer models (PointDA/hengshuang_transformer/hengshuang_model.py),
run on the CPU in fp32 with autograd.  Build-container only (imports the reference through tools/ref_import.py); the fixtures are numeric
and string arrays.

    python tools/make_golden_hengshuang.py

  hsg_def_B2_N48_nb2_k4.npz    PointTransformerDef, levels 48 / 12 / 3 (the last TransformerBlock runs with k_eff = 3 < k), activate_DefRec=False
  hsg_cls_B2_N64_nb2_k4.npz    PointTransformerCls, levels 64 / 16 / 4
  hsg_seg_B2_N64_nb1_k8.npz    PointTransformerSeg, levels 64 / 16
(The reference's DefRec head is built for 32 + 512 input channels, which only nblocks = 4 produces: activate_DefRec=True cannot run in the
reference at nblocks = 2, and an nblocks = 4 parameter set does not fit a fixture.  The tests cover that path against the float64
restatement.)

The reference's farthest_point_sample and square_distance are wrapped by loggers (they call the originals), so the fixture holds every
index the reference used: "fps_idx.<i>", "down_knn.<i>", "block_knn.<l>", "up_knn.<i>" in the layout of tests/hengshuang_restatement.py,
derived from the logged distance matrices with the reference's own argsort / sort.  torch.max is logged the same way for the
neighbourhood-max selections "<tag>.sel.<i>" ([B S, C] slots, the layout of functional.recorded_selections).

After construction under "seed" every BatchNorm weight is drawn from N(0,1) (some negative) and its bias moved off 0; tensors of more than
BIG entries are refilled with tests/dgprop_restatement.hash_fill from their seed ("wseed.<key>", scale "wscale.<key>") and not stored,
the others are "p.<key>".  "keys" / "shapes": the state_dict.  "cfg" = [num_point, nblocks, nneighbor, input_dim, transformer_dim,
num_class, B].  Per mode tag ("train", "eval"; eval runs a copy of the module with fresh running statistics): "<tag>.out", a fixed random
"<tag>.R" and the gradients of (out * R).sum(): "<tag>.g.<key>", or every 16th row "<tag>.g16.<key>" of a BIG tensor.  The perturbation,
the input and R come from a generator seeded 1000 + seed + 100 "draw"; the draw kept is the first on which (a) the reference's own fp32
outputs and gradients are within OWN_ERROR of the same module run in float64 ("<tag>.own_error"; the training-mode bias gradients that
fp32 cannot hold to it on any draw, see own_error(), are stored per key as "<tag>.own.<key>" instead) and (b) the float64 run's FPS indices,
neighbour lists and selections equal the fp32 run's at every level.
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
import hengshuang_restatement as HR  # noqa: E402
from dgprop_restatement import hash_fill  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
BIG = 2048
OWN_ERROR = 5e-6          # half of the 1e-5 the CPU test holds the fp32 restatement to
MAX_DRAWS = 200
FPS_SEED = 4242           # torch's global generator before every forward: the reference draws the FPS starts from it
LOG = {"fps": [], "dist": [], "max": []}


class logged:
    """While active: the reference's farthest_point_sample / square_distance log what they return, and torch.max logs the indices of the
    [B, C, S] maxima (the neighbourhood max of PointNetSetAbstraction), in call order."""

    def __init__(self, pu, tr):
        self.pu, self.tr = pu, tr

    def __enter__(self):
        pu, tr = self.pu, self.tr
        self.saved = (pu.farthest_point_sample, pu.square_distance, tr.square_distance, torch.max)
        fps0, sq0, _, max0 = self.saved
        for v in LOG.values():
            v.clear()

        def fps(xyz, npoint):
            r = fps0(xyz, npoint)
            LOG["fps"].append(r.detach().clone())
            return r

        def sq(src, dst):
            r = sq0(src, dst)
            LOG["dist"].append(r.detach())
            return r

        def tmax(*a, **k):
            r = max0(*a, **k)
            if hasattr(r, "indices") and r.indices.dim() == 3:
                LOG["max"].append(r.indices.detach())
            return r
        pu.farthest_point_sample, pu.square_distance, tr.square_distance, torch.max = fps, sq, sq, tmax
        return self

    def __exit__(self, *exc):
        self.pu.farthest_point_sample, self.pu.square_distance, self.tr.square_distance, torch.max = self.saved
        return False


def npy(t):
    return t.detach().cpu().numpy()


def shapes_array(shapes):
    out = np.zeros((len(shapes), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        out[i, :len(s)] = s
    return out


def graph_from_log(nblocks, k, decode):
    """the reference's lists from its own distance matrices, in the order its forward computes them"""
    d = list(LOG["dist"])
    g = {"fps_idx": list(LOG["fps"]), "down_knn": [], "block_knn": [None] * (nblocks + 1), "up_knn": [None] * nblocks}
    g["block_knn"][0] = d.pop(0).argsort()[:, :, :k]
    for i in range(nblocks):
        g["down_knn"].append(d.pop(0).argsort()[:, :, :k])
        g["block_knn"][i + 1] = d.pop(0).argsort()[:, :, :k]
    if decode:
        assert torch.equal(d.pop(0).argsort()[:, :, :k], g["block_knn"][nblocks])
        for i in range(nblocks):
            if g["block_knn"][nblocks - i].shape[1] > 1:
                g["up_knn"][i] = d.pop(0).sort(dim=-1)[1][:, :, :3]
            assert torch.equal(d.pop(0).argsort()[:, :, :k], g["block_knn"][nblocks - 1 - i])
    assert not d, len(d)
    sel = [m.permute(0, 2, 1).reshape(-1, m.shape[1]) for m in LOG["max"]]
    assert len(sel) == nblocks and len(g["fps_idx"]) == nblocks
    return g, sel


def same_graph(a, b):
    for key in a:
        for x, y in zip(a[key], b[key]):
            if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
                return False
    return True


def run(m, x, pu, tr, nblocks, k, decode):
    m.zero_grad()
    torch.manual_seed(FPS_SEED)
    with logged(pu, tr):
        out = m(x)
    g, sel = graph_from_log(nblocks, k, decode)
    return out, g, sel


def own_error(m32, out32, m64, out64, kind, nblocks):
    """the reference's own fp32 rounding, max|a - b| / max|b| from the same module run in float64: -> (the worst over the output and every
    gradient that the draw is chosen by, {key: distance} of the training-mode bias gradients above OWN_ERROR).  Those biases shift a
    block's features by a per-channel constant, most of whose effect a downstream batch-statistics BatchNorm cancels: their gradient is
    a small remainder of large cancelling sums, fp32 keeps 1e-4 to 3e-3 of it on every draw, and no draw is chosen or refused by them."""
    g32 = {n: p.grad for n, p in m32.named_parameters() if p.grad is not None}
    g64 = {n: p.grad for n, p in m64.named_parameters() if p.grad is not None}
    assert set(g32) == set(g64)
    worst, wide = HR.dist(out32.detach(), out64.detach()), {}
    for n in g32:
        e = HR.grad_dist(n, g32[n], g64[n], g64, m32.training, kind, nblocks)
        if m32.training and n.endswith(".bias") and e > OWN_ERROR:
            wide[n] = e
        else:
            worst = max(worst, e)
    return worst, wide


def case(kind, seed, draw, B, num_point, nblocks, k, tdim, pu, tr, hm):
    cfg = types.SimpleNamespace(num_point=num_point, nblocks=nblocks, nneighbor=k, num_class=10, input_dim=3, transformer_dim=tdim, dropout=0.0)
    cfg.model = cfg
    nn = torch.nn
    torch.manual_seed(seed)
    m = {"cls": hm.PointTransformerCls, "seg": hm.PointTransformerSeg, "def": hm.PointTransformerDef}[kind](cfg)
    c = {"seed": np.array(seed), "draw": np.array(draw), "cfg": np.array([num_point, nblocks, k, 3, tdim, 10, B])}
    g = torch.Generator().manual_seed(1000 + seed + 100 * draw)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
        for i, (name, p) in enumerate(m.named_parameters()):
            if p.numel() > BIG:
                fan_in = p[0].numel()
                s, sc = 7919 * seed + 31 * i + 5, float(np.sqrt(3.0 / fan_in))
                p.copy_(torch.from_numpy(hash_fill(tuple(p.shape), s, sc)))
                c["wseed." + name], c["wscale." + name] = np.array(s), np.array(sc, dtype=np.float64)
    sd = m.state_dict()
    c["keys"], c["shapes"] = np.array(list(sd.keys())), shapes_array([tuple(v.shape) for v in sd.values()])
    for name, p in m.named_parameters():
        if p.numel() <= BIG:
            c["p." + name] = npy(p)
    x = torch.randn(B, num_point, 3, generator=g)
    c["x"] = npy(x)
    decode = kind == "seg"
    worst, graph0 = 0.0, None
    for tag in ("train", "eval"):
        m32 = copy.deepcopy(m).train(tag == "train")
        out, graph, sel = run(m32, x, pu, tr, nblocks, k, decode)
        Rw = torch.randn(out.shape, generator=g)
        (out * Rw).sum().backward()
        m64 = copy.deepcopy(m).double().train(tag == "train")
        out64, graph64, sel64 = run(m64, x.double(), pu, tr, nblocks, k, decode)
        (out64 * Rw.double()).sum().backward()
        same = same_graph(graph, graph64) and all(torch.equal(a, b) for a, b in zip(sel, sel64))
        if graph0 is None:
            graph0 = graph
            for key, lst in graph.items():
                for i, t in enumerate(lst):
                    if t is not None:
                        c["%s.%d" % (key, i)] = npy(t).astype(np.int32)
        else:
            assert same_graph(graph0, graph)
        for i, s in enumerate(sel):
            c["%s.sel.%d" % (tag, i)] = npy(s).astype(np.uint8)
        err, wide = own_error(m32, out, m64, out64, kind, nblocks) if same else (float("inf"), {})
        c[tag + ".own_error"] = np.array(err)
        for n, e in wide.items():
            c[tag + ".own." + n] = np.array(e)
        worst = max(worst, err)
        c[tag + ".out"], c[tag + ".R"] = npy(out), npy(Rw)
        for name, p in m32.named_parameters():
            if p.grad is None:
                continue
            if p.numel() > BIG:
                c[tag + ".g16." + name] = npy(p.grad)[::16]
            else:
                c[tag + ".g." + name] = npy(p.grad)
    return worst, c


def main():
    ref_import.install_stubs()
    for p in (ref_import.REF_ROOT + "/PointDA", ref_import.REF_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import warnings
    warnings.filterwarnings("ignore")
    from PointDA.hengshuang_transformer import pointnet_util as pu, transformer as tr, hengshuang_model as hm
    torch.set_num_threads(8)
    cases = (("hsg_def_B2_N48_nb2_k4.npz", ("def", 0, 2, 48, 2, 4, 32)),
             ("hsg_cls_B2_N64_nb2_k4.npz", ("cls", 1, 2, 64, 2, 4, 32)),
             ("hsg_seg_B2_N64_nb1_k8.npz", ("seg", 2, 2, 64, 1, 8, 32)))
    for name, (kind, seed, B, N, nb, k, tdim) in cases:
        for draw in range(MAX_DRAWS):
            err, c = case(kind, seed, draw, B, N, nb, k, tdim, pu, tr, hm)
            print("%s draw %d: own fp32 error %.2e" % (name, draw, err), flush=True)
            if err < OWN_ERROR:
                break
        else:
            raise SystemExit("no draw of %s under %g" % (name, OWN_ERROR))
        np.savez_compressed(os.path.join(OUT, name), **c)
        size = os.path.getsize(os.path.join(OUT, name))
        print(name, size, len(c))
        assert size < 1000000, size


if __name__ == "__main__":
    main()
