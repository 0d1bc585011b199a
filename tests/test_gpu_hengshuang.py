"""functional.interp3_add / cloud_mean (csrc/pyramid.hip), TransitionDown, TransitionUp and the three Point Transformer models
(mlsp_amd/hengshuang_model.py) against the float64 restatement (tests/hengshuang_restatement.py) fed the same fp32 inputs.

Distance: max|a - b| / max|b|.  Bar per quantity: max(floor, 3 x the distance of the fp32 restatement run on the same device).  The two
ops reach no GEMM: floor 2e-6.  The modules: floor 2e-6 per chained contraction along the longest path --
    TransformerBlock 6 (fc1, q | k | v, fc_gamma 2, the aggregation, fc2: test_gpu_transformer.py's count)
    TransitionDown   2 (two conv + BatchNorm layers; the first one's folded products are one contraction deep)
    TransitionUp     1 (the two Linear branches are parallel; the interpolation is not a contraction)
    backbone         2 (fc1) + 6 + nblocks (2 + 6);   heads 3;   fc2 + transformer2 3 + 6;   decoder nblocks (1 + 6);   DefRec 4
    Cls and Def without DefRec: 11 + 8 nblocks (27 at nblocks = 2);  Seg: 20 + 15 nblocks (35 at nblocks = 1);  Def with DefRec:
    21 + 15 nblocks (81 at nblocks = 4).
The restatement is fed the fixture's graph (or, where there is no fixture, the build's own) and the selections captured with
functional.recorded_selections.  A bias whose gradient is exactly zero (hengshuang_restatement.residue_bias) is measured against the same
layer's weight gradient.  No entry is left out of any comparison."""
import os
import types

import numpy as np
import pytest
import torch

import hengshuang_restatement as HR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"def": "hsg_def_B2_N48_nb2_k4.npz", "cls": "hsg_cls_B2_N64_nb2_k4.npz", "seg": "hsg_seg_B2_N64_nb1_k8.npz"}
FLOOR = 2e-6
MODES = ("fp32", "f16x3")
UNSUPPORTED = -3
DEEP_SEED = 5             # see test_deeper_defrec_model_against_float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def check(name, got, want64, want32, floor, scale=None):
    """assert dist(got, want64) <= max(floor, 3 dist(want32, want64)); the figures are printed first.  scale: the denominator instead of
    max|want64| (an exactly-zero quantity)"""
    den = float(want64.double().abs().max().clamp_min(1e-300)) if scale is None else float(scale)
    d = float((got.double() - want64.double()).abs().max()) / den
    y = float((want32.double() - want64.double()).abs().max()) / den
    bar = max(floor, 3 * y)
    print("  %-52s distance %.2e  fp32 restatement %.2e  bar %.2e" % (name, d, y, bar))
    assert torch.isfinite(got).all() and d <= bar, (name, d, y, bar)
    return bar


# ---------------------------------------------------------------------------------------------------------------------------------
# the two ops alone

def three_nn(src, qry):
    d, idx = ((qry[:, :, None] - src[:, None]) ** 2).sum(-1).sort(dim=-1)
    return idx[:, :, :3].contiguous(), d[:, :, :3].contiguous()


@pytest.mark.parametrize("shape", [(1, 5, 1, 4), (2, 48, 3, 32), (3, 130, 17, 36)], ids=lambda s: "x".join(map(str, s)))
def test_interp3_add_against_float64(dev, shape):
    from mlsp_amd import functional as Fh
    B, N, S, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    feat, add, Rw = (torch.randn(s, generator=g).to(dev) for s in ((B, S, C), (B, N, C), (B, N, C)))
    idx = d2 = None
    if S > 1:
        src, qry = torch.randn(B, S, 3, generator=g), torch.randn(B, N, 3, generator=g)
        qry[:, 0] = src[:, 0]                                # a query on top of a source point: distance 0
        idx, d2 = (t.to(dev) for t in three_nn(src, qry))
    f, a = feat.clone().requires_grad_(True), add.clone().requires_grad_(True)
    out = Fh.interp3_add(f, a, None if idx is None else idx.to(torch.int32), d2)
    loss = (out * Rw).sum()
    g1 = torch.autograd.grad(loss, [f, a], retain_graph=True)
    g2 = torch.autograd.grad(loss, [f, a])
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))    # two backward passes: bit-identical
    assert torch.equal(g1[1], Rw)                            # the gradient of `add` is dout itself

    def restated(dtype):
        ff, aa = feat.to(dtype).requires_grad_(True), add.to(dtype).requires_grad_(True)
        o = HR.interp3_add(ff, aa, idx, d2, dtype)
        return (o.detach(),) + torch.autograd.grad((o * Rw.to(dtype)).sum(), [ff, aa])
    o64, f64, _ = restated(torch.float64)
    o32, f32, _ = restated(torch.float32)
    check("out", out.detach(), o64, o32, FLOOR)
    check("dfeat", g1[0], f64, f32, FLOOR)


@pytest.mark.parametrize("shape", [(1, 1, 4), (3, 130, 36), (2, 1024, 512)], ids=lambda s: "x".join(map(str, s)))
def test_cloud_mean_against_float64(dev, shape):
    from mlsp_amd import functional as Fh
    B, N, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, Rw = (3.0 + torch.randn(B, N, C, generator=g)).to(dev), torch.randn(B, C, generator=g).to(dev)
    xr = x.reshape(B * N, C).clone().requires_grad_(True)
    out = Fh.cloud_mean(xr, B, N)
    dx, = torch.autograd.grad((out * Rw).sum(), [xr])
    assert torch.equal(out, Fh.cloud_mean(xr.detach(), B, N))               # a fixed summation order: bit-identical run to run

    def restated(dtype):
        xx = x.to(dtype).requires_grad_(True)
        o = HR.cloud_mean(xx, dtype)
        return o.detach(), torch.autograd.grad((o * Rw.to(dtype)).sum(), [xx])[0]
    o64, d64 = restated(torch.float64)
    o32, d32 = restated(torch.float32)
    check("out", out.detach(), o64, o32, FLOOR)
    check("dX", dx.view(B, N, C), d64, d32, FLOOR)
    # fp64 accumulation, one rounding: within an fp32 ulp of the exact mean
    assert float((out.double() - o64).abs().max() / o64.abs().max()) <= 2.0 ** -23
    if N == 1:
        assert torch.equal(out, x.view(B, C)) and torch.equal(dx, Rw)


def test_unsupported_shapes_launch_nothing(dev):
    """C % 4 != 0, rows off 16-byte alignment and S == 2 return MLSP_ERR_UNSUPPORTED and leave the sentinel in every output"""
    from mlsp_amd import _lib, functional as Fh
    lib = _lib.load()
    st = _lib.stream()
    B, N, S = 2, 8, 3
    idx = torch.zeros(B, N, 3, dtype=torch.int32, device=dev)
    d2 = torch.ones(B, N, 3, device=dev)
    rev_off = torch.zeros(B * S + 1, dtype=torch.int32, device=dev)
    rev_ent = torch.zeros(B * N * 3, dtype=torch.int32, device=dev)
    big = torch.randn(B * N * 8 + 4, device=dev)

    def sentinel(n):
        return torch.full((n,), 7.0, device=dev)
    for C, off, s in ((6, 0, S), (4, 1, S), (4, 0, 2)):                     # channel count, element offset of the inputs, source points
        feat, add = big[off:off + B * s * C], big[off:off + B * N * C]
        out, dfeat, mean, dx = sentinel(B * N * C), sentinel(B * s * C), sentinel(B * C), sentinel(B * N * C)
        assert lib.mlsp_interp3_add_fwd_f32(feat.data_ptr(), idx.data_ptr(), d2.data_ptr(), add.data_ptr(), B, N, s, C, out.data_ptr(), st) == UNSUPPORTED
        assert lib.mlsp_interp3_add_bwd_f32(add.data_ptr(), d2.data_ptr(), rev_off.data_ptr(), rev_ent.data_ptr(), B, N, s, C, dfeat.data_ptr(),
                                            st) == UNSUPPORTED
        if s != 2:
            assert lib.mlsp_cloud_mean_fwd_f32(add.data_ptr(), B, N, C, mean.data_ptr(), st) == UNSUPPORTED
            assert lib.mlsp_cloud_mean_bwd_f32(feat.data_ptr(), B, N, C, dx.data_ptr(), st) == UNSUPPORTED
        torch.cuda.synchronize()
        for t in (out, dfeat, mean, dx):
            assert bool((t == 7.0).all())
    with pytest.raises(_lib.MlspLibraryError):
        Fh.cloud_mean(torch.zeros(8, 6, device=dev), 2, 4)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.interp3_add(torch.zeros(2, 2, 4, device=dev), torch.zeros(2, 8, 4, device=dev), idx, d2)


# ---------------------------------------------------------------------------------------------------------------------------------
# modules and models

_cache = {}


def fixture(kind):
    if kind not in _cache:
        _cache[kind] = HR.load_fixture(os.path.join(GOLDEN, FIXTURES[kind]))
    return _cache[kind]


def make_cfg(num_point, nblocks, k, tdim, num_class=10):
    cfg = types.SimpleNamespace(num_point=num_point, nblocks=nblocks, nneighbor=k, num_class=num_class, input_dim=3, transformer_dim=tdim,
                                dropout=0.0)
    cfg.model = cfg
    return cfg


def make_model(kind, z, params, dev):
    from mlsp_amd import hengshuang_model as hm
    num_point, nblocks, k, _, tdim, num_class, _ = (int(v) for v in z["cfg"])
    m = {"def": hm.PointTransformerDef, "cls": hm.PointTransformerCls, "seg": hm.PointTransformerSeg}[kind](make_cfg(num_point, nblocks, k, tdim, num_class))
    m.load_state_dict(params, strict=True)
    return m.to(dev)


def to_pyramid(graph, nblocks, dev):
    from mlsp_amd import hengshuang_model as hm
    pg = hm.PyramidGraph(nblocks)
    for key in ("fps_idx", "down_knn", "block_knn", "up_knn"):
        setattr(pg, key, [None if t is None else t.to(dev) for t in graph[key]])
    return pg


def from_pyramid(pg):
    return {key: [None if t is None else t.long() for t in getattr(pg, key)] for key in ("fps_idx", "down_knn", "block_knn", "up_knn")}


def on(dev, graph):
    return {key: [None if t is None else t.to(dev) for t in lst] for key, lst in graph.items()}


def compare_grads(mod, g64, g32, floor, training, kind, nblocks, prefix=""):
    got = {n: p.grad for n, p in mod.named_parameters() if p.grad is not None}
    assert set(got) == set(g64), set(got) ^ set(g64)
    for n in sorted(got):
        scale = g64[n[:-len("bias")] + "weight"].abs().max() if HR.residue_bias(prefix + n, training, kind, nblocks) else None
        check("d " + n, got[n], g64[n], g32[n], floor, scale=scale)


def compare_buffers(mod, b64, b32, floor):
    sd = mod.state_dict()
    names = sorted(n for n in b64 if n != "selections")
    assert names
    for n in names:
        check(n, sd[n], b64[n], b32[n], floor)


def model_compare(kind, dev, mode, model, params, nblocks, x, graph, floor, defrec=False):
    """training-mode forward + backward, then one eval-mode forward on the running statistics the training forward left"""
    from mlsp_amd import functional as Fh
    pg = to_pyramid(graph, nblocks, dev)
    kw = {"activate_DefRec": True} if defrec else {}
    model.train()
    model.zero_grad()
    with Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = model(x, graph=pg, **kw)
        g = torch.Generator().manual_seed(3)
        Rw = torch.randn(out.shape, generator=g).to(dev)
        (out * Rw).sum().backward()
    assert len(rec.sel) == nblocks
    dparams, dgraph = {k: v.to(dev) for k, v in params.items()}, on(dev, graph)
    o64, g64, b64 = HR.grads(kind, dparams, nblocks, x, dgraph, Rw, defrec, True, torch.float64, sel=rec.sel)
    o32, g32, b32 = HR.grads(kind, dparams, nblocks, x, dgraph, Rw, defrec, True, torch.float32, sel=rec.sel)
    bar = check("out", out.detach(), o64, o32, floor)
    free64 = HR.forward(kind, dparams, nblocks, x, dgraph, defrec, True, torch.float64)[0]
    gap = float((free64 - o64).abs().max() / free64.abs().max())
    print("  recorded selections: worst distance from the float64 optimum %.2e" % gap)
    assert gap <= bar, (gap, bar)
    compare_grads(model, g64, g32, floor, True, kind, nblocks)
    compare_buffers(model, b64, b32, floor)
    assert all(int(m.num_batches_tracked) == 1 for m in model.modules()
               if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) and m.weight.grad is not None)
    model.eval()
    with torch.no_grad(), Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = model(x, graph=pg, **kw)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    e64 = HR.forward(kind, sd, nblocks, x, dgraph, defrec, False, torch.float64, sel=rec.sel)[0]
    e32 = HR.forward(kind, sd, nblocks, x, dgraph, defrec, False, torch.float32, sel=rec.sel)[0]
    check("eval out", out, e64, e32, floor)
    return o64


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["cls", "def", "seg"])
def test_models_on_their_fixtures_against_float64(dev, kind, mode):
    z, params, graph = fixture(kind)
    nblocks = int(z["cfg"][1])
    model = make_model(kind, z, params, dev)
    x = torch.from_numpy(z["x"]).to(dev)
    floor = FLOOR * ((20 + 15 * nblocks) if kind == "seg" else (11 + 8 * nblocks))
    o64 = model_compare(kind, dev, mode, model, params, nblocks, x, graph, floor)
    # the float64 restatement on the build's selections is where the reference's fp32 run is, to the reference's own error
    assert HR.dist(z["train.out"], o64.cpu()) <= 1e-5


def test_model_searches_the_fixture_s_graph(dev):
    """no graph given, fps_start set to the fixture's first samples: every FPS index and neighbour list equals the reference's"""
    from mlsp_amd import hengshuang_model as hm
    for kind in ("def", "seg"):
        z, params, graph = fixture(kind)
        nblocks = int(z["cfg"][1])
        model = make_model(kind, z, params, dev).eval()
        for i, td in enumerate(model.backbone.transition_downs):
            td.sa.fps_start = graph["fps_idx"][i][:, 0].to(dev)
        with torch.no_grad(), hm.recorded_graph() as rec:
            model(torch.from_numpy(z["x"]).to(dev))
        got = from_pyramid(rec.graph)
        for key, lst in graph.items():
            for i, want in enumerate(lst):
                if want is None:
                    assert got[key][i] is None, (key, i)
                else:
                    assert got[key][i] is not None and torch.equal(got[key][i].cpu(), want), (kind, key, i)


@pytest.mark.parametrize("mode", MODES)
def test_transition_down_alone_against_float64(dev, mode):
    from mlsp_amd import functional as Fh
    z, params, graph = fixture("def")
    nblocks = int(z["cfg"][1])
    model = make_model("def", z, params, dev).train()
    x = torch.from_numpy(z["x"]).to(dev)
    lv = HR.levels({k: v.to(dev) for k, v in params.items()}, nblocks, x, on(dev, graph), True, torch.float64,
                   sel=[torch.from_numpy(z["train.sel.%d" % i]).to(dev) for i in range(nblocks)])
    for i in range(nblocks):                                                # 48 -> 12 and 12 -> 3
        td, pre = model.backbone.transition_downs[i], "backbone.transition_downs.%d." % i
        xyz, pts = lv[i][0].float(), lv[i][1].float().requires_grad_(True)
        fps_idx, knn = graph["fps_idx"][i].to(dev), graph["down_knn"][i].to(dev)
        model.zero_grad()
        with Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
            new_xyz, out = td(xyz, pts, fps_idx=fps_idx, knn_idx=knn)
            Rw = torch.randn(out.shape, generator=torch.Generator().manual_seed(i)).to(dev)
            (out * Rw).sum().backward()
        assert len(rec.sel) == 1 and tuple(rec.sel[0].shape) == (out.shape[0] * out.shape[1], out.shape[2])
        sub = {k[len(pre):]: v.to(dev) for k, v in params.items() if k.startswith(pre)}

        def restated(dtype):
            leaves = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v) for k, v in sub.items()}
            p = pts.detach().to(dtype).requires_grad_(True)
            nx, o, bufs = HR.transition_down(leaves, xyz, p, fps_idx, knn, True, dtype, sel=rec.sel)
            (o * Rw.to(dtype)).sum().backward()
            return nx, o.detach(), p.grad, {k: v.grad for k, v in leaves.items() if v.requires_grad}, bufs
        nx64, o64, dp64, g64, b64 = restated(torch.float64)
        _, o32, dp32, g32, b32 = restated(torch.float32)
        assert torch.equal(new_xyz, nx64.float())
        check("down %d out" % i, out.detach(), o64, o32, 2 * FLOOR)
        check("down %d dpoints" % i, pts.grad, dp64, dp32, 2 * FLOOR)
        compare_grads(td, g64, g32, 2 * FLOOR, True, "def", nblocks, prefix=pre)
        compare_buffers(td, b64, b32, 2 * FLOOR)


@pytest.mark.parametrize("mode", MODES)
def test_transition_up_alone_against_float64(dev, mode):
    """transition_ups[0] of the Seg fixture on its level tensors (16 -> 64 points), and a seeded TransitionUp from exactly three points on
    the Def fixture's levels (3 -> 12)"""
    from mlsp_amd import functional as Fh, hengshuang_model as hm
    cases = []
    z, params, graph = fixture("seg")
    model = make_model("seg", z, params, dev)
    lv = HR.levels({k: v.to(dev) for k, v in params.items()}, 1, torch.from_numpy(z["x"]).to(dev), on(dev, graph), True, torch.float64,
                   sel=[torch.from_numpy(z["train.sel.0"]).to(dev)])
    pre = "transition_ups.0."
    cases.append((model.transition_ups[0], {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}, lv[1], lv[0], graph["up_knn"][0]))
    z, params, graph = fixture("def")
    lv = HR.levels({k: v.to(dev) for k, v in params.items()}, 2, torch.from_numpy(z["x"]).to(dev), on(dev, graph), True, torch.float64,
                   sel=[torch.from_numpy(z["train.sel.%d" % i]).to(dev) for i in range(2)])
    torch.manual_seed(21)
    up = hm.TransitionUp(128, 64, 64)
    with torch.no_grad():
        for bn in (up.fc1[2], up.fc2[2]):
            bn.weight.copy_(torch.randn(64))
            bn.bias.copy_(0.3 * torch.randn(64))
    nn3 = HR.search_graph(torch.from_numpy(z["x"]), 2, 4, graph["fps_idx"])["up_knn"][0]
    assert lv[2][0].shape[1] == 3 and nn3.shape == (2, 12, 3)
    cases.append((up.to(dev), {k: v.detach().clone() for k, v in up.state_dict().items()}, lv[2], lv[1], nn3))
    for n, (mod, sub, coarse, fine, idx) in enumerate(cases):
        mod.train()
        mod.zero_grad()
        sub = {k: v.to(dev) for k, v in sub.items()}
        idx = idx.to(dev)
        xyz1, xyz2 = coarse[0].float(), fine[0].float()
        p1, p2 = coarse[1].float().requires_grad_(True), fine[1].float().requires_grad_(True)
        with Fh.gemm_precision(mode):
            out = mod(xyz1, p1, xyz2, p2, knn_idx=idx)
            Rw = torch.randn(out.shape, generator=torch.Generator().manual_seed(n)).to(dev)
            (out * Rw).sum().backward()

        def restated(dtype):
            leaves = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v) for k, v in sub.items()}
            a, b = p1.detach().to(dtype).requires_grad_(True), p2.detach().to(dtype).requires_grad_(True)
            o, bufs = HR.transition_up(leaves, xyz1, a, xyz2, b, idx, True, dtype)
            (o * Rw.to(dtype)).sum().backward()
            return o.detach(), a.grad, b.grad, {k: v.grad for k, v in leaves.items() if v.requires_grad}, bufs
        o64, a64, b64_, g64, bufs64 = restated(torch.float64)
        o32, a32, b32_, g32, bufs32 = restated(torch.float32)
        check("up %d out" % n, out.detach(), o64, o32, FLOOR)
        check("up %d dpoints1" % n, p1.grad, a64, a32, FLOOR)
        check("up %d dpoints2" % n, p2.grad, b64_, b32_, FLOOR)
        compare_grads(mod, g64, g32, FLOOR, True, "seg", 1, prefix="transition_ups.0.")
        compare_buffers(mod, bufs64, bufs32, FLOOR)
        # the model's own 3-NN search gives the same lists
        with torch.no_grad():
            chosen = []
            mod(xyz1, p1, xyz2, p2, chosen=chosen)
        assert torch.equal(chosen[0], idx)


def deep_case(seed, dev=None):
    """PointTransformerDef, B = 2, 768 points, nblocks 4 (768 / 192 / 48 / 12 / 3), nneighbor 8, transformer_dim 32: the module built under
    `seed` with its BatchNorm weights and biases redrawn, and its input"""
    from mlsp_amd import hengshuang_model as hm
    torch.manual_seed(seed)
    model = hm.PointTransformerDef(make_cfg(768, 4, 8, 32))
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    x = torch.randn(2, 768, 3, generator=g)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, params, x


@pytest.mark.parametrize("mode", MODES)
def test_deeper_defrec_model_against_float64(dev, mode):
    """No fixture: the graph is the build's own (recorded_graph), handed to the restatement.  DEEP_SEED = 5 is the first seed of 0, 1, 2, ...
    that is clean on the CPU (fp32 against float64 restatement, training mode, selections pinned to the float64 run's): the fp32 and
    float64 graphs agree, the output is within 5.1e-6 and every weight gradient within 1.5e-5 (seeds 0 - 4: 4e-4 to 3e-2, a ReLU mask
    that rounding decides; 7 and 10 are clean too).  No seed brings EVERY gradient within 1e-4: 17 bias gradients (backbone.fc1.2.bias
    6.9e-3 the worst; the blocks' fc1 / fc_delta.2 biases) are small remainders of sums that a downstream batch-statistics BatchNorm
    cancels, and fp32 keeps 1e-4 to 7e-3 of them at every seed -- their bars follow the fp32 restatement's distance like everyone
    else's.  The bars assume that the build decides no ReLU mask differently from float64 either: measured on an MI355X, it decides none
    at seed 5, and at seeds 7 and 10 one or two of the 1e6 masks of DefRec (the whole discrepancy sits in ONE channel of DefRec.bn3.bias,
    1.2e-3 and 5.7e-3, the other 127 within 9e-8; the head alone is within 1e-6 of float64 at this shape)."""
    from mlsp_amd import hengshuang_model as hm
    model, params, x = deep_case(DEEP_SEED)
    model, x = model.to(dev), x.to(dev)
    start = torch.zeros(2, dtype=torch.long, device=dev)
    for td in model.backbone.transition_downs:
        td.sa.fps_start = start
    with torch.no_grad(), hm.recorded_graph() as rec:
        model.eval()
        model(x, activate_DefRec=True)
    graph = {k: [None if t is None else t.cpu() for t in v] for k, v in from_pyramid(rec.graph).items()}
    want = HR.search_graph(x.cpu(), 4, 8, graph["fps_idx"])
    for key in want:
        assert all(torch.equal(a, b) for a, b in zip(want[key], graph[key])), key
    model_compare("def", dev, mode, model, params, 4, x, graph, FLOOR * 81, defrec=True)


def test_def_fixture_runs_are_bit_identical(dev):
    z, params, graph = fixture("def")
    x = torch.from_numpy(z["x"]).to(dev)
    runs = []
    for _ in range(2):
        model = make_model("def", z, params, dev).train()
        out = model(x, graph=to_pyramid(graph, 2, dev))
        (out * out).sum().backward()
        runs.append((out.detach(), {n: p.grad for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0]) and set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 30
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_transformer_dim_must_be_a_multiple_of_four(dev):
    from mlsp_amd import _lib, hengshuang_model as hm
    model = hm.PointTransformerCls(make_cfg(64, 1, 4, 30)).to(dev)
    with pytest.raises(_lib.MlspLibraryError):
        model(torch.randn(2, 64, 3, device=dev))
