"""functional.thin_in / token_pool (csrc/token.hip), Group, Encoder and PointTransformer (mlsp_amd/pointbert.py) against the float64
restatement (tests/pointbert_restatement.py) fed the same fp32 inputs.

Distance: max|a - b| / max|b|.  Bar per quantity: max(floor, 3 x the distance of the fp32 restatement run on the same device) -- the rule of
test_gpu_vit.py and test_gpu_dgprop.py; floor 2e-6 per chained contraction.  The restatement is fed the indices and 3-NN distances that the
build's own farthest_point_sample / knn_point return for the same input (those kernels have their own tests) and the selections captured
with functional.recorded_selections; that the recorded selections attain the float64 optimum within the forward bar is asserted
separately.  A conv bias that only reaches a batch-statistics BatchNorm has an exactly-zero gradient (pointbert_restatement.residue_bias):
what any precision reports there is residue, measured against the same layer's weight gradient.  No entry is left out of any comparison.

thin_in, token_pool and Group reach no GEMM, so they run once; the Encoder and the model run under gemm_precision("fp32") and the default."""
import math
import os
import types

import pytest
import torch

import pointbert_restatement as PR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLS = os.path.join(GOLDEN, "ptrans_cls_s0_B2_N40_G5_M7_d24_h2_depth2.npz")
DEF = os.path.join(GOLDEN, "ptrans_def_s1_B2_N520_G8_M8_d32_h2_depth12_e32.npz")
FLOOR = 2e-6
MODES = ("fp32", "f16x3")


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
    print("  %-40s distance %.2e  fp32 restatement %.2e  bar %.2e" % (name, d, y, bar))
    assert torch.isfinite(got).all() and d <= bar, (name, d, y, bar)
    return bar


# ---------------------------------------------------------------------------------------------------------------------------------
# thin_in

def thin_inputs(seed, M, Cin, C, bn=True, x=None):
    g = torch.Generator().manual_seed(seed)
    t = {"X": torch.randn(M, Cin, generator=g) if x is None else x(g), "W": torch.randn(C, Cin, generator=g) / math.sqrt(Cin),
         "bias": 0.5 * torch.randn(C, generator=g), "R": torch.randn(M, C, generator=g)}
    if bn:
        t.update({"gamma": 1 + 0.3 * torch.randn(C, generator=g), "beta": 0.3 * torch.randn(C, generator=g),
                  "rm": 0.5 * torch.randn(C, generator=g), "rv": 0.5 + torch.rand(C, generator=g)})
    return t


def thin_gpu(t, dev, training, act):
    from mlsp_amd import functional as Fh
    bn = "gamma" in t
    names = ("W", "bias", "gamma", "beta") if bn else ("W", "bias")
    leaf = {n: t[n].to(dev).requires_grad_(True) for n in names}
    rm, rv = (t["rm"].to(dev).clone(), t["rv"].to(dev).clone()) if bn else (None, None)
    H, save = Fh.thin_in(t["X"].to(dev), leaf["W"], leaf["bias"], leaf.get("gamma"), leaf.get("beta"), rm, rv, training=training, act=act,
                         return_stats=True)
    loss = (H * t["R"].to(dev)).sum()
    g1 = dict(zip(leaf, torch.autograd.grad(loss, list(leaf.values()), retain_graph=True)))
    g2 = dict(zip(leaf, torch.autograd.grad(loss, list(leaf.values()))))
    for n in leaf:
        assert torch.equal(g1[n], g2[n]), n                  # two backward passes: bit-identical
    return H.detach(), save, rm, rv, g1


def thin_restated(t, dev, dtype, training, act):
    bn = "gamma" in t
    names = ("W", "bias", "gamma", "beta") if bn else ("W", "bias")
    leaf = {n: t[n].to(dev).to(dtype).requires_grad_(True) for n in names}
    r = PR.thin_in(t["X"].to(dev), leaf["W"], leaf["bias"], leaf.get("gamma"), leaf.get("beta"), t["rm"].to(dev) if bn else None,
                   t["rv"].to(dev) if bn else None, training=training, act=act, dtype=dtype)
    grads = dict(zip(leaf, torch.autograd.grad((r["H"] * t["R"].to(dev).to(dtype)).sum(), list(leaf.values()))))
    return {k: (None if v is None else v.detach()) for k, v in r.items()}, grads


def thin_compare(t, dev, training=True, act=PR.ACT_RELU):
    bn = "gamma" in t
    H, save, rm, rv, grads = thin_gpu(t, dev, training, act)
    r64, g64 = thin_restated(t, dev, torch.float64, training, act)
    r32, g32 = thin_restated(t, dev, torch.float32, training, act)
    check("H", H, r64["H"], r32["H"], FLOOR)
    check("dW", grads["W"], g64["W"], g32["W"], FLOOR)
    if bn:
        check("dgamma", grads["gamma"], g64["gamma"], g32["gamma"], FLOOR)
        check("dbeta", grads["beta"], g64["beta"], g32["beta"], FLOOR)
        check("bn_save mean", save[2], r64["mean"], r32["mean"], FLOOR)
        check("bn_save invstd", save[3], r64["invstd"], r32["invstd"], FLOOR)
        check("running_mean", rm, r64["run_mean"], r32["run_mean"], FLOOR)
        check("running_var", rv, r64["run_var"], r32["run_var"], FLOOR)
    if bn and training:
        print("  db: exactly 0 (float64 reports %.2e)" % float(g64["bias"].abs().max()))
        assert bool((grads["bias"] == 0).all())              # the bias cancels in a batch-statistics BatchNorm
    else:
        check("db", grads["bias"], g64["bias"], g32["bias"], FLOOR)
    return H, save, grads


THIN_BN_CASES = [(2, 3, 4), (33, 3, 128), (4099, 3, 128), (257, 6, 36)]


@pytest.mark.parametrize("shape", THIN_BN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_thin_in_batchnorm_relu_against_float64(dev, shape):
    thin_compare(thin_inputs(sum(shape), *shape), dev)


def test_thin_in_one_column_no_activation(dev):
    thin_compare(thin_inputs(5, 64, 1, 8), dev, act=PR.ACT_NONE)


@pytest.mark.parametrize("shape", [(65, 3, 128), (130, 8, 128)], ids=lambda s: "x".join(map(str, s)))
def test_thin_in_plain_gelu(dev, shape):
    thin_compare(thin_inputs(sum(shape), *shape, bn=False), dev, act=PR.ACT_GELU)


def test_thin_in_eval_mode(dev):
    t = thin_inputs(6, 1024, 3, 128)
    _, save, _ = thin_compare(t, dev, training=False)
    assert torch.equal(save[2].cpu(), t["rm"])               # the running buffers are read, not written (checked bit for bit by the caller too)


def test_thin_in_off_centre_input(dev):
    """x = 50 + 0.01 randn: the centred form keeps the digits the Gram form loses; the yardstick carries the bar"""
    thin_compare(thin_inputs(7, 1024, 3, 128, x=lambda g: 50 + 0.01 * torch.randn(1024, 3, generator=g)), dev)


def test_thin_in_constant_column(dev):
    """a singular covariance: channels that see only the constant column have variance exactly 0, invstd = 1 / sqrt(eps), H = act(beta)"""
    def x(g):
        v = torch.randn(257, 3, generator=g)
        v[:, 1] = 0.7513
        return v
    t = thin_inputs(8, 257, 3, 36, x=x)
    t["W"][:4, 0] = 0.0
    t["W"][:4, 2] = 0.0
    H, save, _ = thin_compare(t, dev)
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
    assert torch.equal(save[3, :4].cpu(), torch.full((4,), 1.0 / math.sqrt(eps32), dtype=torch.float64).float())
    assert torch.equal(H[:, :4].cpu(), torch.relu(t["beta"][:4]).expand(257, 4))


def test_thin_in_negative_and_zero_gamma(dev):
    t = thin_inputs(9, 33, 3, 128)
    t["gamma"][::3] = -t["gamma"][::3].abs()
    t["gamma"][5] = 0.0
    H, _, grads = thin_compare(t, dev)
    assert torch.equal(H[:, 5].cpu(), torch.relu(t["beta"][5]).expand(33))
    assert bool((grads["W"][5] == 0).all())


def test_thin_in_refusals(dev):
    from mlsp_amd import _lib, functional as Fh
    lib = _lib.load()

    def direct(M, Cin, C, bn):
        """the C entry on a sentinel-filled output: -> (return code, output untouched)"""
        X, W = torch.randn(M, Cin, device=dev), torch.randn(C, Cin, device=dev)
        H = torch.full((M, C), 7.0, device=dev)
        gamma, beta = (torch.ones(C, device=dev), torch.zeros(C, device=dev)) if bn else (None, None)
        save, xmom = torch.full((4, C), 7.0, device=dev), torch.full((72,), 7.0, dtype=torch.float64, device=dev)
        ws, wsn = _lib.workspace_of(dev, 1 << 20)
        rc = lib.mlsp_thin_in_fwd_f32(X.data_ptr(), Cin, M, Cin, W.data_ptr(), None, C, _lib.ptr(gamma), _lib.ptr(beta), None, None, 0.1, 1e-5, 1,
                                      1, H.data_ptr(), save.data_ptr(), xmom.data_ptr(), ws, wsn, _lib.stream())
        torch.cuda.synchronize()
        return rc, bool((H == 7.0).all()) and bool((save == 7.0).all()) and bool((xmom == 7.0).all())
    assert direct(8, 9, 8, True) == (-3, True)               # MLSP_ERR_UNSUPPORTED
    assert direct(8, 3, 6, True) == (-3, True)
    assert direct(1, 3, 8, True) == (-1, True)               # MLSP_ERR_ARG: torch refuses one value per channel in training too
    for M, Cin, C in ((8, 9, 8), (8, 3, 6), (1, 3, 8)):
        with pytest.raises(_lib.MlspLibraryError):
            Fh.thin_in(torch.randn(M, Cin, device=dev), torch.randn(C, Cin, device=dev), None, torch.ones(C, device=dev),
                       torch.zeros(C, device=dev))
    with pytest.raises(NotImplementedError):
        Fh.thin_in(torch.randn(8, 3, device=dev, requires_grad=True), torch.randn(8, 3, device=dev), None)


# ---------------------------------------------------------------------------------------------------------------------------------
# token_pool

POOL_CASES = [(1, 2, 4), (3, 6, 24), (2, 65, 384), (2, 257, 32)]


def pool_torch(y, B, L, R):
    y3 = y.detach().clone().requires_grad_(True)
    v = y3.view(B, L, -1)
    out = torch.cat([v[:, 0], v[:, 1:].max(1)[0]], dim=-1)
    (out * R).sum().backward()
    return out.detach(), v[:, 1:].max(1)[1] + 1, y3.grad


@pytest.mark.parametrize("shape", POOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_token_pool_equals_torch_bit_for_bit(dev, shape):
    from mlsp_amd import functional as Fh
    B, L, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    y = torch.randn(B * L, d, generator=g).to(dev).requires_grad_(True)
    R = torch.randn(B, 2 * d, generator=g).to(dev)
    with Fh.recorded_selections() as rec:
        out = Fh.token_pool(y, B, L)
    (out * R).sum().backward()
    want, arg, dy = pool_torch(y, B, L, R)
    assert len(rec.sel) == 1 and rec.sel[0].dtype == torch.int32 and rec.sel[0].shape == (B, d)
    assert torch.equal(out, want) and torch.equal(rec.sel[0].long(), arg) and torch.equal(y.grad, dy)


def test_token_pool_tie_goes_to_the_lower_row(dev):
    from mlsp_amd import functional as Fh
    B, L, d = 2, 9, 8
    g = torch.Generator().manual_seed(3)
    y = torch.randn(B, L, d, generator=g)
    y[:, 6] = y[:, 3] = 5.0                                  # rows 3 and 6 tie at the top of every column (3 and 6 sit in different row lanes)
    y = y.view(B * L, d).to(dev).requires_grad_(True)
    with Fh.recorded_selections() as rec:
        out = Fh.token_pool(y, B, L)
    out[:, d:].sum().backward()
    assert bool((rec.sel[0] == 3).all()) and bool((out[:, d:] == 5.0).all())
    gy = y.grad.view(B, L, d)
    assert bool((gy[:, 3] == 1).all()) and bool((gy[:, 6] == 0).all()) and float(gy.sum()) == B * d


def test_token_pool_nan_contract(dev):
    from mlsp_amd import functional as Fh
    B, L, d = 2, 6, 8
    g = torch.Generator().manual_seed(4)
    y = torch.randn(B, L, d, generator=g)
    y[0, 1, 0] = float("nan")                                # a NaN in the first candidate row
    y[1, 4, 2] = float("nan")                                # a NaN further down
    y[:, 1:, 5] = float("nan")                               # an all-NaN column
    want = torch.where(torch.isnan(y[:, 1:]), torch.full_like(y[:, 1:], -float("inf")), y[:, 1:]).max(1)
    y = y.view(B * L, d).to(dev).requires_grad_(True)
    with Fh.recorded_selections() as rec:                    # the forward alone first
        out = Fh.token_pool(y, B, L)
    arg = rec.sel[0].cpu()
    assert bool(((arg >= 1) & (arg < L)).all())
    assert arg[0, 0] != 1 and arg[1, 2] != 4
    cols = [c for c in range(d) if c != 5]
    assert torch.equal(arg[:, cols].long(), want[1][:, cols] + 1) and torch.equal(out[:, d:].cpu()[:, cols], want[0][:, cols])
    assert bool((arg[:, 5] == 1).all()) and bool(torch.isnan(out[:, d + 5]).all())
    out.backward(torch.ones_like(out))                       # only then the backward: it routes through arg, all in range
    assert float(y.grad.view(B, L, d)[:, :, 5].sum()) == B * 2


# ---------------------------------------------------------------------------------------------------------------------------------
# Group

def build_graph(pts, G, M, defrec):
    """the indices (and 3-NN squared distances) the build's own kernels return for `pts`, as pointbert_restatement.forward takes them"""
    from mlsp_amd import pointbert, pointnet2
    g = {"fps_g": pointbert._fps0(pts, G)}
    center = pointnet2.index_points(pts, g["fps_g"])
    g["knn_group"] = pointnet2.knn_point(M, pts, center)
    if defrec:
        g["fps_512"], g["fps_256"] = pointbert._fps0(pts, 512), pointbert._fps0(pts, 256)
        l1, l2 = pointnet2.index_points(pts, g["fps_512"]), pointnet2.index_points(pts, g["fps_256"])
        for key, (ref, qry) in (("nn3_2", (center, l2)), ("nn3_1", (center, l1)), ("nn3_0", (l1, pts))):
            g[key] = pointnet2.knn_point(3, ref, qry, return_dist=True)
        g["pro2"] = (pointnet2.knn_point(4, center, l2), pointnet2.knn_point(4, l2, l2))
        g["pro1"] = (pointnet2.knn_point(4, l2, l1), pointnet2.knn_point(4, l1, l1))
    return g


@pytest.mark.parametrize("shape", [(2, 40, 5, 7), (2, 520, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_group_is_gather_and_subtract_bit_for_bit(dev, shape):
    from mlsp_amd import model_utils
    B, N, G, M = shape
    pts = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(N)).to(dev)
    nb, center = model_utils.Group(num_group=G, group_size=M)(pts)
    graph = build_graph(pts, G, M, False)
    want_nb, want_c = PR.group(pts, graph["fps_g"], graph["knn_group"])
    assert nb.shape == (B, G, M, 3) and center.shape == (B, G, 3)
    assert bool((graph["fps_g"][:, 0] == 0).all()) and int(graph["knn_group"].max()) < N and int(graph["knn_group"].min()) >= 0
    assert torch.equal(center, want_c) and torch.equal(nb, want_nb)
    nb2, c2 = model_utils.Group(num_group=G, group_size=M)(pts, fps_idx=graph["fps_g"])
    assert torch.equal(nb2, nb) and torch.equal(c2, center)
    with pytest.raises(ValueError):
        model_utils.Group(num_group=N + 1, group_size=M)(pts)


# ---------------------------------------------------------------------------------------------------------------------------------
# Encoder and model

def perturb_norms(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm, torch.nn.GroupNorm)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))       # some negative
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))


def compare_grads(mod, g64, g32, floor, prefix=""):
    """prefix: where `mod` sits in the PointTransformer (residue_bias names the model's keys)"""
    got = {n: p.grad for n, p in mod.named_parameters() if p.grad is not None}
    assert set(got) == set(g64), set(got) ^ set(g64)
    for n in sorted(got):
        scale = g64[n[:-len("bias")] + "weight"].abs().max() if PR.residue_bias(prefix + n) else None
        check("d " + n, got[n], g64[n], g32[n], floor, scale=scale)


def compare_buffers(mod, b64, b32, floor):
    sd = mod.state_dict()
    assert b64
    for n in sorted(b64):
        check(n, sd[n], b64[n], b32[n], floor)


@pytest.mark.parametrize("mode", MODES)
def test_encoder_against_float64(dev, mode):
    from mlsp_amd import functional as Fh, model_utils
    B, G, M, C = 2, 5, 7, 32
    floor = 6 * FLOOR                                        # six chained contractions
    torch.manual_seed(11)
    enc = model_utils.Encoder(encoder_channel=C)
    perturb_norms(enc, 12)
    params = {k: v.clone() for k, v in enc.state_dict().items()}
    enc = enc.to(dev).train()
    g = torch.Generator().manual_seed(13)
    nb = (0.4 * torch.randn(B, G, M, 3, generator=g)).to(dev)
    Rw = torch.randn(B, G, C, generator=g).to(dev)
    with Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = enc(nb)
        (out * Rw).sum().backward()
    assert [tuple(s.shape) for s in rec.sel] == [(B * G, 256), (B * G, 256), (B * G, C)] and all(int(s.max()) < M for s in rec.sel)

    def restated(dtype, sel):
        leaves = {k: (v.to(dev).to(dtype).requires_grad_(True) if "running_" not in k and v.is_floating_point() else v.to(dev)) for k, v in params.items()}
        o, bufs = PR.encoder(leaves, nb, training=True, dtype=dtype, sel=sel)
        (o * Rw.to(dtype)).sum().backward()
        return o.detach(), {k: v.grad for k, v in leaves.items() if v.requires_grad}, bufs
    o64, g64, b64 = restated(torch.float64, rec.sel)
    o32, g32, b32 = restated(torch.float32, rec.sel)
    free64 = PR.encoder({k: v.to(dev) for k, v in params.items()}, nb, training=True, dtype=torch.float64)[0]
    bar = check("out", out, o64, o32, floor)
    gap = float((free64 - o64).abs().max() / free64.abs().max())
    print("  recorded selections: worst distance from the float64 optimum %.2e" % gap)
    assert gap <= bar, (gap, bar)
    compare_grads(enc, g64, g32, floor, prefix="encoder.")
    compare_buffers(enc, b64, b32, floor)
    assert all(int(m.num_batches_tracked) == 1 for m in enc.modules() if isinstance(m, torch.nn.BatchNorm1d))


def load_model(path, dev):
    from mlsp_amd import Models
    z, cfg, params, _ = PR.load_fixture(path)
    model = Models.PointTransformer(cfg)
    model.load_state_dict(params, strict=True)
    model.cls_head_finetune[2].p = 0.0                       # the fixtures run the head's Dropout(0.5) at rate 0
    return z, cfg, params, model.to(dev)


def model_compare(path, tag, dev, mode):
    from mlsp_amd import functional as Fh
    z, cfg, params, model = load_model(path, dev)
    defrec = tag == "def"
    floor = FLOOR * ((21 if defrec else 9) + 6 * cfg.depth)
    pts, Rw = torch.from_numpy(z["pts"]).to(dev), torch.from_numpy(z[tag + ".R"]).to(dev)
    graph = build_graph(pts, cfg.num_group, cfg.group_size, defrec)
    model.train()
    with Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = model(pts, activate_DefRec=defrec)
        (out * Rw).sum().backward()
    assert len(rec.sel) == (8 if defrec else 4), len(rec.sel)
    assert out.shape == ((pts.shape[0], pts.shape[1], 3) if defrec else (pts.shape[0], cfg.cls_dim))
    dparams = {k: v.to(dev) for k, v in params.items()}
    o64, g64, b64 = PR.grads(dparams, cfg, pts, graph, Rw, defrec, True, torch.float64, sel=rec.sel)
    o32, g32, b32 = PR.grads(dparams, cfg, pts, graph, Rw, defrec, True, torch.float32, sel=rec.sel)
    free64 = PR.forward(dparams, cfg, pts, graph, defrec, True, torch.float64)[0]
    bar = check("out", out.detach(), o64, o32, floor)
    gap = float((free64 - o64).abs().max() / free64.abs().max())
    print("  recorded selections: worst distance from the float64 optimum %.2e" % gap)
    assert gap <= bar, (gap, bar)
    compare_grads(model, g64, g32, floor)
    compare_buffers(model, b64, b32, floor)
    return z, cfg, model, pts, graph


@pytest.mark.parametrize("mode", MODES)
def test_model_classification_path_against_float64(dev, mode):
    from mlsp_amd import functional as Fh
    z, cfg, model, pts, graph = model_compare(CLS, "cls", dev, mode)
    # one eval-mode forward against the restatement on the running statistics the training forward left
    model.eval()
    with torch.no_grad(), Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = model(pts)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    o64 = PR.forward(sd, cfg, pts, graph, False, False, torch.float64, sel=rec.sel)[0]
    o32 = PR.forward(sd, cfg, pts, graph, False, False, torch.float32, sel=rec.sel)[0]
    check("eval logits", out, o64, o32, FLOOR * (9 + 6 * cfg.depth))


@pytest.mark.parametrize("mode", MODES)
def test_model_defrec_path_against_float64(dev, mode):
    model_compare(DEF, "def", dev, mode)


def test_nested_fps_is_bit_identical(dev):
    from mlsp_amd import pointbert, pointnet2
    z, cfg, _, model = load_model(DEF, dev)
    pts = torch.from_numpy(z["pts"]).to(dev)
    full = pointbert._fps0(pts, 512)
    for k in (8, 256):
        assert torch.equal(full[:, :k], pointbert._fps0(pts, k))
    assert torch.equal(pointbert.fps(pts, 256), pointnet2.index_points(pts, full[:, :256]))
    model.eval()
    outs = []
    for nest in (True, False):
        pointbert.NEST_FPS = nest
        try:
            with torch.no_grad():
                outs.append(model(pts, activate_DefRec=True))
        finally:
            pointbert.NEST_FPS = True
    assert torch.equal(outs[0], outs[1])


def test_model_refusals(dev):
    from mlsp_amd import Models
    _, cfg, _, model = load_model(DEF, dev)
    with pytest.raises(ValueError):
        model(torch.randn(2, 300, 3, device=dev), activate_DefRec=True)
    for other in ("Pointnet_Encoder", "Dgcnn_Encoder", "Relative_Encoder"):
        bad = types.SimpleNamespace(**{**vars(cfg), "encoder_type": other})
        with pytest.raises(NotImplementedError):
            Models.PointTransformer(bad)


def test_calc_loss_ptrans_equals_calc_loss(dev):
    from mlsp_amd import mlsp
    g = torch.Generator().manual_seed(21)
    B, N = 3, 128
    pred, labels = torch.randn(B, N, 3, generator=g).to(dev), torch.randn(B, 3, N, generator=g).to(dev)
    mask = (torch.rand(B, 1, N, generator=g) < 0.3).float().expand(B, 3, N).contiguous().to(dev)
    args = types.SimpleNamespace(DefRec_weight=0.5)
    a = mlsp.calc_loss_ptrans(args, pred, labels, mask)
    b = mlsp.calc_loss(args, {"DefRec": pred}, labels, mask)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_reference_width_smoke(dev):
    """B=4, N=1024, G=64, M=32, trans_dim 384, depth 12, 6 heads: forward + backward of both paths; shapes, finiteness, gradient coverage"""
    from mlsp_amd import Models
    cfg = types.SimpleNamespace(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=10, num_heads=6, group_size=32, num_group=64,
                                encoder_dims=256, encoder_type="Encoder", dropout=0.5, model="PointTransformer")
    torch.manual_seed(5)
    model = Models.PointTransformer(cfg).to(dev).train()
    pts = torch.randn(4, 1024, 3, generator=torch.Generator().manual_seed(6)).to(dev)
    defrec_only = ("propagation_", "dgcnn_pro_", "DefRec.")
    for defrec in (False, True):
        model.zero_grad(set_to_none=True)
        out = model(pts, activate_DefRec=defrec)
        assert out.shape == ((4, 1024, 3) if defrec else (4, 10)) and bool(torch.isfinite(out).all())
        out.square().mean().backward()
        for n, p in model.named_parameters():
            want = (not n.startswith("cls_head_finetune.")) if defrec else (not n.startswith(defrec_only))
            assert (p.grad is not None) == want, (defrec, n)
            if want:
                assert bool(torch.isfinite(p.grad).all()), n
