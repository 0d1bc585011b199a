"""The set-abstraction kernel family (mlsp_amd/csrc/sa.hip + the compact reverse lists of reverse.hip), one kernel path per test, against
tests/sa_restatement.py: index results (FPS, ball query, query kNN and its distances, the grouping forward) EXACTLY equal to the fp32
restatement on every row -- no mask, no "fraction of rows" -- and float results (grouping backward, 3-NN interpolation, the folded first
layer, whole modules) against the float64 restatement.

Bars of the float results.  Grouping backward: the summation bound (n + 1) * 2^-24 * sum |terms| per element, derived from the float64
data (sa_restatement.group_backward_bounds).  Everything else: distance = max |a - b| / max |b| against float64, bar = max(floor,
3 x yardstick) -- the project's rule -- where the yardstick is the fp32 restatement's own distance from float64 and the floor is the GEMM
family's 2e-6 (test_gemm_split_bf16_accuracy) per chained contraction.  Every check prints distance, yardstick and bar.

tests/test_sa_restatement_cpu.py proves on the CPU what each case is there for (which FPS kernel an N reaches, pads present, a query
without a hit, exact ties, fp32 and float64 indices identical on the lattice inputs, no ReLU argument within rounding of zero), so nothing
here passes vacuously.

Measured on one MI355X (every printed line: profiles/sa_paths_float64_distances.txt): no quantity comes closer to its bar than 0.31 of it
-- interp3 d feat 5.8e-7 against 2e-6 (its own yardstick), folded layer d W0 5.1e-7 against 2e-6, module sa-knn d W0 1.3e-6 against
4e-6, feature-propagation module 4.7e-7 against 6e-6; grouping backward at most 0.39 of its summation bound.  On the kernels before
this file (expanded-form kNN distance, padding = every repeat of slot 0) the +20 kNN, every interpolation case and every `pinned`
case fail: d xyz of the pinned folded layers sits 0.48 .. 1.05 from float64."""
import pytest
import torch

import sa_restatement as sr
from oracle import ref_sa_cpu as sa

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to_dev(t, dev):
    """the same values in the SAME memory layout (a plain .to() would compact a view of pitch 6 or a transposed batch)"""
    out = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev)
    out.copy_(t)
    assert out.stride() == t.stride()
    return out


def check(tag, got, want64, yard, floor):
    """got / want64 / yard: name -> tensor; yard is the fp32 restatement, whose distance from want64 sets the bar"""
    assert sorted(got) == sorted(want64) == sorted(yard), (sorted(got), sorted(want64))
    bad = []
    for name in want64:
        g = got[name].detach().cpu()
        assert torch.isfinite(g).all(), (tag, name)
        assert g.shape == want64[name].shape, (tag, name, g.shape, want64[name].shape)
        dist, ydist = sr.dist(g, want64[name]), sr.dist(yard[name], want64[name])
        bar = max(floor, 3 * ydist)
        print("%s %-12s distance %.3e  yardstick %.3e  bar %.3e" % (tag, name, dist, ydist, bar))
        if not dist <= bar:
            bad.append((name, dist, bar))
    assert not bad, (tag, bad)


# ----------------------------------------------------------------------------- FPS
@pytest.mark.parametrize("name", list(sr.FPS_CASES))
def test_fps_indices_equal_the_oracle(dev, name):
    from mlsp_amd import _lib, pointnet2 as p2
    c = sr.FPS_CASES[name]
    assert _lib.load().mlsp_fps_plan(c.N) == sr.FPS_PLAN[c.N]                 # the kernel this N reaches (1: fps_kernel, 2: fps_kernel2)
    xyz, start = sr.fps_input(c)
    want = sa.fps(xyz, c.S, start)
    got = p2.farthest_point_sample(to_dev(xyz, dev), c.S, start=start)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)


def test_fps_refuses_what_it_cannot_run(dev):
    from mlsp_amd import _lib, pointnet2 as p2
    lib = _lib.load()
    assert lib.mlsp_fps_plan(8193) == 0
    for N, S in ((100, 101), (8193, 4)):
        xyz = torch.zeros(1, N, 3, device=dev)
        with pytest.raises(_lib.MlspLibraryError):
            p2.farthest_point_sample(xyz, S, start=torch.zeros(1, dtype=torch.long))
        out = torch.full((1, S), -7, dtype=torch.int32, device=dev)            # the C entry: an argument error, and nothing is written
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        assert lib.mlsp_fps_f32(xyz.data_ptr(), 3, 1, N, S, st.data_ptr(), out.data_ptr(), _lib.stream()) == -1
        torch.cuda.synchronize()
        assert bool((out == -7).all())


# ----------------------------------------------------------------------------- ball query
def _ball(dev, c):
    from mlsp_amd import pointnet2 as p2
    xyz, new_xyz = sr.ball_input(c)
    want = sa.ball_query(c.radius, c.nsample, xyz, new_xyz)
    got = p2.query_ball_point(c.radius, c.nsample, to_dev(xyz, dev), to_dev(new_xyz, dev)).cpu()
    assert got.shape == (sr.BALL_B, c.S, c.nsample) and int(got.min()) >= 0 and int(got.max()) < c.N
    hits = sr.ball_hits(c, xyz, new_xyz).sum(-1)
    answered = hits > 0                                                         # (a query without a hit has no reference result)
    assert torch.equal(got[answered], want[answered]), c.name
    return got, hits


@pytest.mark.parametrize("name", list(sr.BALL_CASES))
def test_ball_query_indices_equal_the_oracle(dev, name):
    c = sr.BALL_CASES[name]
    got, hits = _ball(dev, c)
    if name == "zero-hit":
        # the reference indexes out of range for a query without a hit; the kernel's documented answer: every slot 0, which is in range
        assert bool((hits[:, 1] == 0).all()) and bool((got[:, 1] == 0).all())
    else:
        assert int(hits.min()) >= 1


@pytest.mark.parametrize("N", sr.BALL_SWEEP_N)
def test_ball_query_sweep(dev, N):
    for ns in sr.BALL_SWEEP_NS:
        _, hits = _ball(dev, sr.ball_sweep_case(N, ns))
        assert int(hits.min()) >= 1


def test_ball_query_refuses_nsample_256(dev):
    from mlsp_amd import _lib, pointnet2 as p2
    xyz = torch.zeros(1, 300, 3, device=dev)
    with pytest.raises(_lib.MlspLibraryError):
        p2.query_ball_point(0.5, 256, xyz, xyz[:, :4].contiguous())
    assert p2.query_ball_point(0.5, 255, xyz, xyz[:, :4].contiguous()).shape == (1, 4, 255)


# ----------------------------------------------------------------------------- query kNN
def _knn(dev, k, ref, q):
    from mlsp_amd import pointnet2 as p2
    idx, dist = p2.knn_point(k, ref.to(dev), q.to(dev), return_dist=True)
    return idx.cpu(), dist.cpu()


@pytest.mark.parametrize("k", sr.KNN_K)
def test_knn_point_lattice_every_row_exact(dev, k):
    """idx and dist of EVERY row equal the direct-form oracle: references on a coarse lattice (duplicates and exact ties: the lower index
    wins), Nr from k itself across the 256-reference tile edge, Nq across the 256-query block edge; a query that is a reference finds a
    coincident reference first, at distance exactly 0."""
    for Nr in sr.knn_nr(k):
        for Nq in sr.KNN_NQ:
            ref, q, n_own = sr.knn_lattice_input(k, Nr, Nq)
            want_idx, want_d = sr.knn_oracle(k, ref, q)
            idx, dist = _knn(dev, k, ref, q)
            assert torch.equal(idx, want_idx), (k, Nr, Nq)
            assert torch.equal(dist, want_d), (k, Nr, Nq)
            assert bool((dist[:, :n_own, 0] == 0).all()) and torch.equal(sr.gather(ref, idx[:, :n_own, 0]), q[:, :n_own])


@pytest.mark.parametrize("k", [3, 16])
def test_knn_point_offset_cloud_every_row_exact(dev, k):
    """a random cloud shifted by +20, the first 100 queries are references: the direct-form distance is the oracle's to the bit on every
    row and exactly 0 at the coincident points (the expanded form -2ab + a^2 + b^2 ranks 1 row in 10 differently here and goes negative)"""
    g = sr.gen(3100)
    ref = sr.cloud(g, (2, 600, 3), 20.0)
    q = torch.cat([ref[:, :100], sr.cloud(g, (2, 157, 3), 20.0)], 1)
    want_idx, want_d = sr.knn_oracle(k, ref, q)
    idx, dist = _knn(dev, k, ref, q)
    assert torch.equal(idx, want_idx) and torch.equal(dist, want_d)
    assert float(dist.min()) == 0.0 and bool((dist[:, :100, 0] == 0).all()) and idx[0, :100, 0].tolist() == list(range(100))


def test_knn_point_six_coordinates_on_the_lattice(dev):
    ref, q, _ = sr.knn_lattice_input(16, 300, 255, C=6)
    want_idx, want_d = sr.knn_oracle(16, ref, q)
    idx, dist = _knn(dev, 16, ref, q)
    assert torch.equal(idx, want_idx) and torch.equal(dist, want_d)


@pytest.mark.parametrize("k", [4, 17, 64])
def test_knn_point_non_finite_rows(dev, k):
    """cloud 0: reference row 5 is NaN -- it ranks last (behind every finite candidate), its distance reads +inf, the other entries are
    the oracle's; cloud 1 all NaN: indices 0 .. k-1 (the first to enter), every distance +inf; indices stay in [0, Nr) throughout"""
    Nr, Nq = 70, 9
    ref, q, _ = sr.knn_lattice_input(k, Nr, Nq)
    ref[0, 5] = float("nan")
    ref[1] = float("nan")
    idx, dist = _knn(dev, k, ref, q)
    assert int(idx.min()) >= 0 and int(idx.max()) < Nr
    d = sr.square_distance(q[:1], ref[:1])
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    want_d, order = torch.sort(d, dim=-1, stable=True)
    assert torch.equal(idx[0], order[0, :, :k]) and torch.equal(dist[0], want_d[0, :, :k])
    assert not bool((idx[0] == 5).any()) if k < Nr else True
    assert torch.equal(idx[1], torch.arange(k).expand(Nq, k)) and bool(torch.isinf(dist[1]).all()) and bool((dist[1] > 0).all())
    clean_ref, clean_q, _ = sr.knn_lattice_input(k, Nr, Nq)                       # finite rows are unaffected by the NaN next door
    keep = [j for j in range(Nr) if j != 5]
    w_idx, w_d = sr.knn_oracle(min(k, Nr - 1), clean_ref[:1, keep], clean_q[:1])
    assert torch.equal(dist[0, :, :w_d.shape[-1]], w_d[0])


def test_knn_point_refuses_k_beyond_its_limits(dev):
    from mlsp_amd import _lib, pointnet2 as p2
    x = torch.zeros(1, 70, 3, device=dev)
    for k, Nr in ((65, 70), (9, 8)):
        with pytest.raises(_lib.MlspLibraryError):
            p2.knn_point(k, x[:, :Nr].contiguous(), x[:, :4].contiguous())


# ----------------------------------------------------------------------------- grouping (_Group)
@pytest.mark.parametrize("D", sr.GROUP_D)
def test_group_forward_exact_backward_within_the_summation_bound(dev, D):
    """forced idx (sa_restatement.group_idx: repeats inside a row, points nobody names, reverse lists of 4 / 5 / 6 / 7 and 70 entries).
    Forward: one subtraction and copies -- exactly the fp32 restatement.  Backward: every element of d feat, d xyz, d new_xyz is a plain
    sum of n entries of the incoming gradient; |got - float64| <= (n + 1) * 2^-24 * sum |terms| (0 for a point nobody names)."""
    from mlsp_amd import pointnet2 as p2
    B, N, S, ns = sr.GROUP_DIMS
    g = sr.gen(4100 + D)
    idx = sr.group_idx()
    xyz, new_xyz = sr.cloud(g, (B, N, 3)), sr.cloud(g, (B, S, 3))
    feat = torch.randn(B, N, D, generator=g) if D else None
    W = torch.randn(B * S * ns, 3 + D, generator=g)
    xg, qg = xyz.to(dev).requires_grad_(True), new_xyz.to(dev).requires_grad_(True)
    fg = feat.to(dev).requires_grad_(True) if D else None
    G = p2._Group.apply(xg, qg, fg, idx.to(dev))
    assert torch.equal(G.detach().cpu(), sr.group(xyz, new_xyz, feat, idx))
    (G * W.to(dev)).sum().backward()
    got = {"dxyz": xg.grad, "dnew_xyz": qg.grad}
    if D:
        got["dfeat"] = fg.grad
    want = sr.group_backward(xyz, new_xyz, feat, idx, W, F64)
    bounds, n = sr.group_backward_bounds(idx, W, N)
    assert sorted(got) == sorted(want)
    for name in want:
        err = (got[name].cpu().double() - want[name]).abs()
        assert err.shape == bounds[name].shape, name
        worst = float((err / bounds[name].clamp_min(1e-300)).max())
        print("group D=%-3d %-9s max |err| %.3e  max err/bound %.3f" % (D, name, float(err.max()), worst))
        assert bool((err <= bounds[name]).all()), (name, worst)
    unnamed = n == 0
    assert int(unnamed.sum()) >= 10 * B and bool((xg.grad.cpu()[unnamed] == 0).all()) and (not D or bool((fg.grad.cpu()[unnamed] == 0).all()))


# ----------------------------------------------------------------------------- 3-NN interpolation and PointNetFeaturePropagation
@pytest.mark.parametrize("offset", sr.INTERP_OFFSETS)
@pytest.mark.parametrize("S", sr.INTERP_S)
def test_interp3_forward_backward_vs_float64(dev, S, offset):
    """knn_point(3) + _Interp3 on sources that are points of the cloud (exact coincidences: d = 0, never negative), two of them identical
    (weights 1/2, 1/2), at cloud offsets 0 / +5 / +20: the three neighbours and their distances are the fp32 restatement's to the bit, out
    and d feat sit within max(2e-6, 3 x yardstick) of float64; sources nobody names get exactly zero gradient rows."""
    from mlsp_amd import pointnet2 as p2
    B, N = sr.INTERP_DIMS
    xyz1, xyz2 = sr.interp_input(S, offset)
    idx, dist = p2.knn_point(3, xyz2.to(dev), xyz1.to(dev), return_dist=True)
    _, want_idx, want_d = sr.interp3(torch.zeros(B, S, 1), xyz1, xyz2)
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(dist.cpu(), want_d) and float(dist.min()) == 0.0
    named = torch.stack([torch.bincount(want_idx[b].reshape(-1), minlength=S) for b in range(B)])
    for D in sr.INTERP_D:
        g = sr.gen(5100 + D)
        feat, wgt = torch.randn(B, S, D, generator=g), torch.randn(B, N, D, generator=g)

        def restated(dtype):
            f = sr.leaf(feat, dtype)
            out, _, _ = sr.interp3(f, xyz1.to(dtype), xyz2.to(dtype))
            (out * wgt.to(dtype)).sum().backward()
            return {"out": out.detach(), "dfeat": f.grad}
        fg = feat.to(dev).requires_grad_(True)
        out = p2._Interp3.apply(fg, idx.to(torch.int32).contiguous(), dist)
        (out * wgt.to(dev)).sum().backward()
        check("interp3 S=%d offset=%+.0f D=%d" % (S, offset, D), {"out": out, "dfeat": fg.grad}, restated(F64), restated(F32), sr.PER_CONTRACTION)
        assert bool((fg.grad.cpu()[named == 0] == 0).all())
    if S == 64:
        assert int((named == 0).sum()) >= 4 * B


def _fp_module(dev, S, offset, D1=4, D2=7, mlp=(16, 12)):
    from mlsp_amd import pointnet2 as p2
    B, N = sr.INTERP_DIMS
    g = sr.gen(5200 + S)
    if S >= 3:
        xyz1, xyz2 = sr.interp_input(S, offset)
    else:
        xyz1 = sr.cloud(g, (B, N, 3), offset)
        xyz2 = xyz1[:, :S].clone()
    layer = p2.PointNetFeaturePropagation(D1 + D2, list(mlp))
    with torch.no_grad():
        for bn in layer.mlp_bns:
            bn.weight.uniform_(0.5, 1.5, generator=g)
            bn.weight[::3] *= -1
            bn.bias.uniform_(-0.3, 0.3, generator=g)
    p1, pts2 = torch.randn(B, D1, N, generator=g), torch.randn(B, D2, S, generator=g)
    wgt = torch.randn(B, mlp[-1], N, generator=g)
    return layer, xyz1.permute(0, 2, 1).contiguous(), xyz2.permute(0, 2, 1).contiguous(), p1, pts2, wgt


@pytest.mark.parametrize("S,offset", [(64, 20.0), (4, 0.0), (1, 5.0)])
def test_feature_propagation_module_vs_float64(dev, S, offset):
    """PointNetFeaturePropagation (the 3-NN search, the interpolation, two Conv1d + BN + ReLU layers; S = 1: the repeat path) against
    oracle.fp_forward in float64: output, both feature gradients, every parameter gradient but the conv biases (in front of batch
    statistics) and the BatchNorm buffers.  Three chained contractions: floor 6e-6."""
    layer, x1, x2, p1, pts2, wgt = _fp_module(dev, S, offset)
    names = [k for k, _ in layer.named_parameters() if not (k.startswith("mlp_convs") and k.endswith("bias"))]

    def restated(dtype):
        pr = {k: sr.leaf(v, dtype) for k, v in layer.named_parameters()}
        bf = {k: v.detach().clone().to(dtype) for k, v in layer.named_buffers() if not k.endswith("num_batches_tracked")}
        a, b = sr.leaf(p1, dtype), sr.leaf(pts2, dtype)
        out, nb = sa.fp_forward(pr, bf, [c.out_channels for c in layer.mlp_convs], x1.to(dtype), x2.to(dtype), a, b)
        (out * wgt.to(dtype)).sum().backward()
        q = {"out": out.detach(), "dpoints1": a.grad, "dpoints2": b.grad}
        q.update({"d " + k: pr[k].grad for k in names})
        q.update({k: v for k, v in nb.items()})
        return q
    want, yard = restated(F64), restated(F32)
    layer = layer.to(dev).train()
    a, b = p1.to(dev).requires_grad_(True), pts2.to(dev).requires_grad_(True)
    out = layer(x1.to(dev), x2.to(dev), a, b)
    (out * wgt.to(dev)).sum().backward()
    got = {"out": out, "dpoints1": a.grad, "dpoints2": b.grad}
    got.update({"d " + k: p.grad for k, p in layer.named_parameters() if k in names})
    got.update({k: v for k, v in layer.named_buffers() if not k.endswith("num_batches_tracked")})
    check("fp module S=%d offset=%+.0f" % (S, offset), got, want, yard, 3 * sr.PER_CONTRACTION)


def test_feature_propagation_refuses_two_sources(dev):
    layer, x1, x2, p1, pts2, _ = _fp_module(dev, 2, 0.0)
    with pytest.raises(ValueError):
        layer.to(dev)(x1.to(dev), x2.to(dev), p1.to(dev), pts2.to(dev))


# ----------------------------------------------------------------------------- the folded first layer
def _load(conv, bn, L, W=None):
    with torch.no_grad():
        conv.weight.copy_((L["W"] if W is None else W).reshape(conv.weight.shape))
        conv.bias.copy_(L["b"])
        bn.weight.copy_(L["gamma"]); bn.bias.copy_(L["beta"])
        bn.running_mean.copy_(L["run_mean"]); bn.running_var.copy_(L["run_var"])


def _layer_got(q, convs, bns, training, unpermute=None):
    for i, (conv, bn) in enumerate(zip(convs, bns)):
        dW = conv.weight.grad.flatten(1)
        q["dW%d" % i] = unpermute(dW) if (unpermute is not None and i == 0) else dW
        q["dgamma%d" % i], q["dbeta%d" % i] = bn.weight.grad, bn.bias.grad
        if training:
            q["run_mean%d" % i], q["run_var%d" % i] = bn.running_mean, bn.running_var
        else:
            q["db%d" % i] = conv.bias.grad
    return q


@pytest.mark.parametrize("name", list(sr.FOLD_CASES))
def test_fold_first_layer_vs_float64(dev, name):
    """pointnet2._fold_first_layer (the two per-point GEMMs, mlsp_sa_fold_fwd/bwd_f32, the compact reverse lists) on forced centres and
    neighbourhoods against sa_restatement.fold_first_layer in float64: the activated edge rows Z, d xyz, d new_xyz, d feat, d W0, d gamma,
    d beta, the conv bias gradient in eval mode and the BatchNorm buffers in training mode.  Every first-conv width (every tpr / nel / nen
    split), ns 1 .. 64, E below 256 and no multiple of 256, BatchNorm scales of both signs; ball-query groups that are mostly padding, kNN
    groups without any, and a caller's own rows with a repeat of slot 0 mid-row and another point in the last slot (`[5, 5, 7, 9]`): only
    the TRAILING copies of slot 0 are padding.  The loss weights meet the premise of the compact lists and vanish at ReLU kinks
    (sa_restatement.fold_weights).  One contraction: floor 2e-6."""
    from mlsp_amd import model_utils, pointnet2 as p2
    c = sr.FOLD_CASES[name]
    xyz, feat, fps_idx, idx = sr.fold_input(c)
    wgt, _ = sr.fold_weights(c)
    want, yard = sr.fold_quantities(c, F64, wgt), sr.fold_quantities(c, F32, wgt)
    conv, bn = torch.nn.Conv2d(3 + c.D, c.C, 1), torch.nn.BatchNorm2d(c.C)
    _load(conv, bn, sr.fold_layers(c, [c.C])[0])
    conv, bn = conv.to(dev), bn.to(dev)
    xg = xyz.to(dev).requires_grad_(True)
    qg = sr.gather(xyz, fps_idx).to(dev).requires_grad_(True)
    fg = feat.to(dev).requires_grad_(True) if c.D else None
    Z = p2._fold_first_layer(xg, qg, fg, idx.to(dev), conv.weight.view(c.C, 3 + c.D), conv, bn, c.training)
    model_utils.flush_bn_counters()
    (Z * wgt.to(dev)).sum().backward()
    got = {"Z": Z, "dxyz": xg.grad, "dnew_xyz": qg.grad}
    if c.D:
        got["dfeat"] = fg.grad
    check("fold " + name, _layer_got(got, [conv], [bn], c.training), want, yard, sr.PER_CONTRACTION)


@pytest.mark.parametrize("name", list(sr.MODULE_CASES))
def test_folded_module_vs_float64(dev, name):
    """PointNetSetAbstraction (sa-*: centres and neighbourhoods pinned through fps_idx= / idx=) and PointNetSetAbstractionMsg (msg-*: seed_idx=,
    its own bit-exact ball query / kNN search; first-conv columns in the reference's [feat | xyz] order) with fold_first=True, the
    neighbourhood max forced to the float64 run's slots (padding slots expressed as slot 0) on the HIP path and the fp32 yardstick alike:
    output, d feat, d xyz (through the neighbours and through the centres), every parameter gradient but the conv biases in front of batch
    statistics, the BatchNorm buffers.  Two chained contractions: floor 4e-6."""
    from mlsp_amd import functional as Fh, pointnet2 as p2
    c = sr.MODULE_CASES[name]
    xyz, feat, fps_idx, idx = sr.fold_input(c)
    _, sel = sr.module_quantities(c, F64)
    sel = sr.pads_to_slot0(sel, idx)
    want, _ = sr.module_quantities(c, F64, sel)
    yard, _ = sr.module_quantities(c, F32, sel)
    layers = sr.fold_layers(c, [c.C, sr.MODULE_WIDTH2])
    msg, knn = name.startswith("msg"), c.kind == "knn"
    unpermute = None
    if msg:
        mod = p2.PointNetSetAbstractionMsg(c.S, [sr.FOLD_RADIUS], [c.ns], c.D, [[c.C, sr.MODULE_WIDTH2]], knn=knn)
        convs, bns = mod.conv_blocks[0], mod.bn_blocks[0]
        W0 = layers[0]["W"]
        _load(convs[0], bns[0], layers[0], W=torch.cat([W0[:, 3:], W0[:, :3]], 1))      # the reference's column order: [feat | xyz]
        unpermute = lambda dW: torch.cat([dW[:, c.D:], dW[:, :c.D]], 1)
    else:
        mod = p2.PointNetSetAbstraction(c.S, sr.FOLD_RADIUS, c.ns, 3 + c.D, [c.C, sr.MODULE_WIDTH2], False, knn=knn)
        convs, bns = mod.mlp_convs, mod.mlp_bns
        _load(convs[0], bns[0], layers[0])
    _load(convs[1], bns[1], layers[1])
    mod = mod.to(dev).train(c.training)
    assert mod.fold_first
    xg = xyz.to(dev).requires_grad_(True)
    fg = feat.to(dev).requires_grad_(True) if c.D else None
    with Fh.forced_selections([sel]):
        if msg:
            new_xyz, out = mod(xg, fg, seed_idx=fps_idx.to(dev))
        else:
            used = []
            new_xyz, out = mod(xg, fg, fps_idx=fps_idx.to(dev), idx=idx.to(dev), chosen=used)
            assert torch.equal(used[0][1].cpu(), idx)
    assert torch.equal(new_xyz.detach().cpu(), sr.gather(xyz, fps_idx))
    (out * sr.module_weights(c).to(dev)).sum().backward()
    got = {"out": out, "dxyz": xg.grad}
    if c.D:
        got["dfeat"] = fg.grad
    check("module " + name, _layer_got(got, convs, bns, c.training, unpermute), want, yard, 2 * sr.PER_CONTRACTION)
