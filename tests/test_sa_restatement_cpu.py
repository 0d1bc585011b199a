"""tests/sa_restatement.py pinned on the CPU: its float-valued functions in fp32 against oracle/ref_sa_cpu.py and the reference's own outputs
(tests/golden/sa_*.npz); on every lattice input fp32 and float64 give IDENTICAL indices (the condition under which the GPU file's bit-exact
index assertions are legitimate); and, per case of tests/test_gpu_sa_paths.py, the condition the case is there for -- so that the GPU file
cannot pass vacuously after a changed seed or kernel constant.  Every test prints what it guarantees (pytest -s shows it)."""
import os
import re

import numpy as np
import pytest
import torch

import sa_restatement as sr
from oracle import ref_sa_cpu as sa
from test_sa_oracle_cpu import GOLD, load_case, split_state

SA_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlsp_amd", "csrc")
F32, F64 = torch.float32, torch.float64


# ----------------------------------------------------------------------------- the restatement against the oracle and the goldens
def test_group_and_branch_match_the_reference_golden():
    """sa_s0_B4_N256.npz (ball-query groups, D > 0, training): sa_branch on the golden's own indices reproduces the reference's output, BN
    buffers and feature gradient at the oracle's tolerances; group() equals the oracle's centred gather bit for bit."""
    g, cfg, params, buffers = load_case("sa_s0_B4_N256.npz")
    xyz, pts = torch.from_numpy(g["xyz"]), torch.from_numpy(g["points"]).requires_grad_(True)
    fps_idx, idx = torch.from_numpy(g["fps_idx"]).long(), torch.from_numpy(g["group_idx"]).long()
    new_xyz = sr.gather(xyz, fps_idx)
    assert np.array_equal(new_xyz.numpy(), g["new_xyz"])
    G = sr.group(xyz, new_xyz, pts.detach(), idx)
    want = torch.cat([sa.gather_rows(xyz, idx) - new_xyz[:, :, None], sa.gather_rows(pts.detach(), idx)], -1)
    assert torch.equal(G, want.reshape(G.shape))
    layers = [{"W": params["mlp_convs.%d.weight" % i].flatten(1), "b": params["mlp_convs.%d.bias" % i],
               "gamma": params["mlp_bns.%d.weight" % i], "beta": params["mlp_bns.%d.bias" % i],
               "run_mean": buffers["mlp_bns.%d.running_mean" % i], "run_var": buffers["mlp_bns.%d.running_var" % i]}
              for i in range(len(cfg["mlp"]))]
    out, _, bufs = sr.sa_branch(xyz, new_xyz, pts, idx, layers, True)
    np.testing.assert_allclose(out.detach().numpy(), g["new_points"], rtol=1e-5, atol=1e-5)
    for i, (m, v) in enumerate(bufs):
        np.testing.assert_allclose(m.numpy(), g["state_after/mlp_bns.%d.running_mean" % i], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(v.numpy(), g["state_after/mlp_bns.%d.running_var" % i], rtol=1e-5, atol=1e-6)
    (out * torch.from_numpy(g["wgt"])).sum().backward()
    np.testing.assert_allclose(pts.grad.numpy(), g["d_points"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", ["sa_fp_s13_B2_N200.npz", "sa_fp1_s13_B2_N200.npz"])
def test_interp3_matches_the_oracle_and_the_reference_golden(name):
    """interp3 in fp32 is, bit for bit, the interpolation inside oracle.fp_forward (which reproduces the golden's output exactly:
    tests/test_sa_oracle_cpu.py); fed into the fixture's MLP it reproduces the reference's output."""
    g = dict(np.load(os.path.join(GOLD, name)))
    params, buffers = split_state(g)
    x1, x2 = torch.from_numpy(g["xyz1"]).permute(0, 2, 1), torch.from_numpy(g["xyz2"]).permute(0, 2, 1)
    p1, p2 = torch.from_numpy(g["points1"]).permute(0, 2, 1), torch.from_numpy(g["points2"]).permute(0, 2, 1)
    interp, idx, d = sr.interp3(p2.contiguous(), x1.contiguous(), x2.contiguous())
    if idx is not None:
        d_or, idx_or = torch.sort(sa.square_distance(x1, x2), dim=-1, stable=True)
        assert torch.equal(idx, idx_or[:, :, :3]) and torch.equal(d, d_or[:, :, :3]) and float(d.min()) >= 0
    h = torch.cat([p1, interp], -1).reshape(-1, p1.shape[-1] + interp.shape[-1])
    for i in range(2):
        h, _, _ = sr._bn_relu(h @ params["mlp_convs.%d.weight" % i].squeeze(-1).t() + params["mlp_convs.%d.bias" % i],
                              params["mlp_bns.%d.weight" % i], params["mlp_bns.%d.bias" % i], buffers["mlp_bns.%d.running_mean" % i],
                              buffers["mlp_bns.%d.running_var" % i], True, 0.1, 1e-5)
    out = h.view(x1.shape[0], x1.shape[1], -1).permute(0, 2, 1)
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=1e-5, atol=1e-5)


def test_fold_first_layer_matches_the_oracle_layer():
    """fold_first_layer in fp32 against oracle.sa_forward with a one-layer MLP before its max (conv2d + F.batch_norm + relu on the grouped
    tensor): the same edge rows, training and eval, and the same buffers."""
    c = sr.FOLD_CASES[next(n for n in sr.FOLD_CASES if "ball" in n and "D5" in n)]
    xyz, feat, fps_idx, idx = sr.fold_input(c)
    L = sr.fold_layers(c, [c.C])[0]
    for training in (True, False):
        z, m, v = sr.fold_first_layer(xyz, sr.gather(xyz, fps_idx), feat, idx, L["W"], L["b"], L["gamma"], L["beta"], L["run_mean"],
                                      L["run_var"], training)
        params = {"mlp_convs.0.weight": L["W"][:, :, None, None], "mlp_convs.0.bias": L["b"], "mlp_bns.0.weight": L["gamma"],
                  "mlp_bns.0.bias": L["beta"]}
        bufs = {"mlp_bns.0.running_mean": L["run_mean"], "mlp_bns.0.running_var": L["run_var"]}
        cfg = dict(npoint=c.S, radius=None, nsample=c.ns, D=c.D, mlp=[c.C], group_all=False)
        _, out, _, _, nb = sa.sa_forward(params, bufs, cfg, xyz, feat, None, training=training, groups=(fps_idx, idx))
        np.testing.assert_allclose(z.view(c.B, c.S, c.ns, c.C).max(2)[0].numpy(), out.numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(m.numpy(), nb["mlp_bns.0.running_mean"].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(v.numpy(), nb["mlp_bns.0.running_var"].numpy(), rtol=1e-5, atol=1e-6)


def test_direct_form_distance_is_the_ball_query_expression():
    """for C = 3, fp32: torch's sum((a - b)^2, -1) is bit-identical to (dx*dx + dy*dy) + dz*dz, the expression of both kernels"""
    g = sr.gen(1)
    a, b = sr.cloud(g, (2, 300, 3), 20.0), sr.cloud(g, (2, 200, 3), 20.0)
    dx, dy, dz = ((a[:, :, None, i] - b[:, None, :, i]) for i in range(3))
    assert torch.equal(sr.square_distance(a, b), (dx * dx + dy * dy) + dz * dz)
    assert torch.equal(sr.square_distance(a, b), sa.square_distance(a, b))


# ----------------------------------------------------------------------------- FPS
def test_fps_plan_table_matches_the_library_and_its_source():
    from mlsp_amd import _lib
    lib = _lib.load()
    for N, plan in sr.FPS_PLAN.items():
        assert lib.mlsp_fps_plan(N) == plan, N
    assert lib.mlsp_fps_plan(0) == 0 and lib.mlsp_fps_plan(-3) == 0
    # every N of a case is a row of the table, both kernels and both edges of the switch are reached, N = 8192 is past 64 KB of LDS
    assert {c.N for c in sr.FPS_CASES.values()} <= set(sr.FPS_PLAN)
    assert {sr.FPS_PLAN[c.N] for c in sr.FPS_CASES.values()} == {1, 2}
    assert sr.FPS_PLAN[63] == 1 and sr.FPS_PLAN[64] == 2 and sr.FPS_PLAN[2048] == 2 and sr.FPS_PLAN[2049] == 1
    assert (3 * 8192 + 32) * 4 > 64 * 1024 >= (3 * 2049 + 32) * 4
    src = open(os.path.join(SA_HIP, "sa.hip")).read()
    assert "const int plan = fps_plan(N);" in src and "if (plan == FPS_PLAN_KERNEL2) {" in src
    hdr = open(os.path.join(SA_HIP, "fps_plan.h")).read()
    assert re.search(r"#define FPS2_MIN_N 64\b", hdr) and re.search(r"#define FPS2_MAX_N 2048\b", hdr)
    assert re.search(r"#define FPS_T 1024\b", hdr) and re.search(r"#define FPS_PPT 8\b", hdr)


@pytest.mark.parametrize("name", list(sr.FPS_CASES))
def test_fps_case(name):
    c = sr.FPS_CASES[name]
    xyz, start = sr.fps_input(c)
    assert xyz.shape == (sr.FPS_B, c.N, 3) and int(start[-1]) == c.N - 1 and c.S <= c.N
    want = sa.fps(xyz, c.S, start)
    note = ""
    if c.kind in ("lattice", "lattice4", "identical"):
        assert torch.equal(sa.fps(xyz.double(), c.S, start), want)          # fp32 and float64 choose alike: exact arithmetic
        if c.N >= 63:
            # exact ties in the arg-max that decides a sample: the maximum of the running distances is attained more than once
            run = torch.full((c.N,), 1e10)
            tied = 0
            for i in want[0, :-1]:
                run = torch.minimum(run, ((xyz[0] - xyz[0, i]) ** 2).sum(-1))
                tied += int((run == run.max()).sum() > 1)
            assert tied > 0, name
            note = "%d of %d arg-maxima of cloud 0 exactly tied" % (tied, c.S - 1)
    if c.kind == "identical":
        assert bool((want[:, 1:] == 0).all())
    if c.kind == "pitch6":
        assert xyz.stride(1) == 6 and xyz.stride(2) == 1
    if c.kind == "noncontiguous":
        assert xyz.stride(0) != c.N * xyz.stride(1)                          # forces the copy in pointnet2._xyz_rows
    print("fps %-28s kernel %d  %s" % (name, sr.FPS_PLAN[c.N], note))


# ----------------------------------------------------------------------------- ball query
def _ball_check(c):
    xyz, new_xyz = sr.ball_input(c)
    hits = sr.ball_hits(c, xyz, new_xyz)
    cnt = hits.sum(-1)
    lattice = c.kind not in ("random",)
    if lattice:
        assert torch.equal(sr.ball_hits(c, xyz, new_xyz, F64), hits), c.name
        assert torch.equal(sa.ball_query(c.radius, c.nsample, xyz.double(), new_xyz.double()), sa.ball_query(c.radius, c.nsample, xyz, new_xyz))
    return xyz, new_xyz, hits, cnt


@pytest.mark.parametrize("name", list(sr.BALL_CASES))
def test_ball_case(name):
    c = sr.BALL_CASES[name]
    xyz, new_xyz, hits, cnt = _ball_check(c)
    first = torch.where(cnt > 0, hits.int().argmax(-1), torch.full_like(cnt, -1))
    rank = hits.long().cumsum(-1)
    nth = ((rank == c.nsample) & hits).int().argmax(-1)                     # index of the nsample-th hit (0 where there is none)
    note = "hits per query %d..%d" % (int(cnt.min()), int(cnt.max()))
    if name == "many-in-first-chunk":
        assert bool((hits[:, :, :64].sum(-1) > c.nsample).any())
    elif name == "nsample-th-hit-is-lane-63":
        assert (cnt >= c.nsample + 2).all() and nth[:, 0].tolist() == [63, 63] and nth[:, 1].tolist() == [127, 127]
    elif name == "first-hit-beyond-128":
        assert int(first.min()) > 128
    elif name == "one-hit":
        assert bool((cnt == 1).all())
    elif name.startswith("nsample-"):
        assert c.nsample > c.N and bool((cnt < c.nsample).all()) and bool((cnt >= 1).any())
    elif name == "on-the-sphere-r0.5":
        d = sr.square_distance(new_xyz, xyz)
        on = d == 0.25
        assert int(on.sum()) > 0 and bool(hits[on].all())
        note += ", %d pairs with d == r^2 exactly (inside)" % int(on.sum())
    elif name in ("r0.1", "r0.2"):
        r2 = c.radius ** 2
        assert float(torch.tensor(r2, dtype=F32)) != r2                     # r^2 rounds in fp32
        assert bool((cnt < c.nsample).any())
    elif name == "pitch6-xyz":
        assert xyz.stride(1) == 6 and new_xyz.stride(1) == 3
    elif name == "pitch6-new_xyz":
        assert xyz.stride(1) == 3 and new_xyz.stride(1) == 6
    elif name == "zero-hit":
        assert bool((cnt[:, 1] == 0).all()) and bool((cnt[:, 0] > 0).all()) and bool((cnt[:, 2] > 0).all())
    else:
        raise AssertionError(name)
    if name != "zero-hit":
        assert int(cnt.min()) >= 1                                           # the reference indexes out of range otherwise
    pads = int((c.nsample - cnt.clamp(max=c.nsample)).sum())
    print("ball %-28s %s, %d padding slots" % (name, note, pads))


def test_ball_sweep_cases():
    seen_pad = seen_full = 0
    for N in sr.BALL_SWEEP_N:
        for ns in sr.BALL_SWEEP_NS:
            _, _, _, cnt = _ball_check(sr.ball_sweep_case(N, ns))
            assert int(cnt.min()) >= 1                                       # every query is a point of its cloud
            seen_pad += int((cnt < ns).any())
            seen_full += int((cnt > ns).any())
    assert seen_pad >= 10 and seen_full >= 5
    print("ball sweep: %d of 30 cases with padded groups, %d with more hits than slots; fp32 and float64 indices identical" % (seen_pad, seen_full))


# ----------------------------------------------------------------------------- query kNN
@pytest.mark.parametrize("k", sr.KNN_K)
def test_knn_lattice_cases(k):
    ties = dups = 0
    for Nr in sr.knn_nr(k):
        for Nq in sr.KNN_NQ:
            ref, q, n_own = sr.knn_lattice_input(k, Nr, Nq)
            idx, d = sr.knn_oracle(k, ref, q)
            idx64, d64 = sr.knn_oracle(k, ref.double(), q.double())
            assert torch.equal(idx, idx64) and torch.equal(d.double(), d64)
            assert torch.equal(idx, sa.knn_group(k, ref, q))
            assert bool((d[:, :n_own, 0] == 0).all()) and torch.equal(sr.gather(ref, idx[:, :n_own, 0]), q[:, :n_own])
            full = sr.square_distance(q, ref)
            if Nr > k:                                                        # the k-th and (k+1)-th candidates exactly tied in some row
                s = torch.sort(full, -1)[0]
                ties += int((s[:, :, k - 1] == s[:, :, k]).sum())
            dups += int((full == 0).sum(-1).gt(1).sum())
    assert ties > 0 or k == max(sr.KNN_K) and dups > 0
    assert dups > 0
    print("knn k=%d: %d rows with the k-th / (k+1)-th distance exactly tied, %d queries on duplicated references; fp32 == float64" % (k, ties, dups))


def test_knn_c6_lattice_case():
    ref, q, _ = sr.knn_lattice_input(16, 300, 255, C=6)
    idx, d = sr.knn_oracle(16, ref, q)
    idx64, d64 = sr.knn_oracle(16, ref.double(), q.double())
    assert torch.equal(idx, idx64) and torch.equal(d.double(), d64)


def test_knn_offset_case_separates_the_two_distance_forms():
    """the random cloud shifted by +20: the expanded form -2ab + a^2 + b^2 ranks differently from the direct form there (and goes
    negative at coincident points), so the GPU test on this input fails on a kernel that computes the expanded form"""
    g = sr.gen(3100)
    ref = sr.cloud(g, (2, 600, 3), 20.0)
    q = torch.cat([ref[:, :100], sr.cloud(g, (2, 157, 3), 20.0)], 1)
    idx, d = sr.knn_oracle(16, ref, q)
    ex = -2 * torch.matmul(q, ref.permute(0, 2, 1))
    ex = (ex + (q ** 2).sum(-1, keepdim=True)) + (ref ** 2).sum(-1).unsqueeze(1)
    de, order = torch.sort(ex, dim=-1, stable=True)
    differ = int((order[:, :, :16] != idx).any(-1).sum())
    assert differ > 0 and float(d.min()) == 0.0 and bool((d[:, :100, 0] == 0).all())
    assert not torch.equal(de[:, :, :16], d)
    print("knn +20: %d of %d rows rank differently under the expanded form" % (differ, idx.shape[0] * idx.shape[1]))


# ----------------------------------------------------------------------------- grouping
def test_group_idx_has_the_lists_it_is_there_for():
    B, N, S, ns = sr.GROUP_DIMS
    idx = sr.group_idx()
    assert idx.shape == (B, S, ns) and int(idx.min()) == 0 and int(idx.max()) < N
    for b in range(B):
        n = torch.bincount(idx[b].reshape(-1), minlength=N)
        assert n[:5].tolist() == [70, 4, 5, 6, 7] and bool((n[30:] == 0).all())
        assert {int(v) % 4 for v in n[1:5]} == {0, 1, 2, 3} and int(n.max()) > 64
    assert idx[0, 0].tolist() == [0] * ns                                     # repeats inside a row
    _, n = sr.group_backward_bounds(idx, torch.ones(B * S * ns, 3 + 5), N)
    assert torch.equal(n, torch.stack([torch.bincount(idx[b].reshape(-1), minlength=N) for b in range(B)]).double())
    print("group: list lengths 70 / 4 / 5 / 6 / 7, points 30..39 unnamed")


# ----------------------------------------------------------------------------- interpolation
@pytest.mark.parametrize("offset", sr.INTERP_OFFSETS)
@pytest.mark.parametrize("S", sr.INTERP_S)
def test_interp_case(S, offset):
    B, N = sr.INTERP_DIMS
    xyz1, xyz2 = sr.interp_input(S, offset)
    feat = torch.randn(B, S, 4, generator=sr.gen(1))
    out, idx, d = sr.interp3(feat, xyz1, xyz2)
    out64, idx64, d64 = sr.interp3(feat.double(), xyz1.double(), xyz2.double())
    assert torch.equal(idx, idx64)                                            # the same three sources in both precisions
    coincident = int((d[:, :, 0] == 0).sum())
    assert coincident >= B * (S - 1 - (4 if S == 64 else 0)) and float(d.min()) == 0.0     # (source 1 left its own point for source 0's)
    # a point that sits on the two identical sources: weights 1/2 and 1/2
    on_pair = (d[:, :, 0] == 0) & (d[:, :, 1] == 0)
    assert int(on_pair.sum()) >= B and bool((idx[on_pair][:, :2] == torch.tensor([0, 1])).all())
    want = 0.5 * (feat[:, 0] + feat[:, 1])
    assert sr.dist(out[on_pair], want.repeat_interleave(on_pair.sum(1), 0)) < 1e-5
    named = torch.stack([torch.bincount(idx[b].reshape(-1), minlength=S) for b in range(B)])
    if S == 64:
        assert bool((named[:, 60:] == 0).all())
    print("interp S=%d offset=%+.0f: %d coincident points, %d on the identical pair, %d unnamed sources; fp32 yardstick %.2e"
          % (S, offset, coincident, int(on_pair.sum()), int((named == 0).sum()), sr.dist(out, out64)))


# ----------------------------------------------------------------------------- folded first layer
def _fold_conditions(c):
    xyz, feat, fps_idx, idx = sr.fold_input(c)
    pads = sr.trailing_pads(idx)
    E = c.B * c.S * c.ns
    assert idx.shape == (c.B, c.S, c.ns) and int(idx.min()) >= 0 and int(idx.max()) < c.N <= 300
    assert E % 256 != 0 and c.S <= c.N
    groups_with_pads = int(pads.any(-1).sum())
    if c.kind == "ball":
        if c.ns >= 16:
            assert groups_with_pads > c.B * c.S // 2, c.name                  # pads in most groups
        elif c.ns > 1:
            assert groups_with_pads >= 1, c.name
        assert torch.equal(pads[:, :, 1:], idx[:, :, 1:] == idx[:, :, :1])   # ball-query rows: every repeat of slot 0 is trailing
    elif c.kind == "knn":
        assert groups_with_pads == 0 and c.ns <= c.N
        assert all(len(set(r.tolist())) == c.ns for r in idx.reshape(-1, c.ns))
    else:
        rep = (idx[:, :, 1] == idx[:, :, 0]) & (idx[:, :, -1] != idx[:, :, 0])
        assert int(rep.sum()) >= c.B * c.S // 2 and idx[0, 0, :3].tolist() == [5, 5, 7]
        assert not bool(pads[:, :, 1][rep].any())                             # that repeat is NOT padding
        assert groups_with_pads >= c.B * (c.S // 2)                           # ... and the rows between end in padding
    widths = [c.C] if c.name in sr.FOLD_CASES else [c.C, sr.MODULE_WIDTH2]
    kappa = sr.fold_kappa(c, widths)
    assert kappa <= sr.FOLD_KAPPA_MAX * len(widths), (c.name, kappa)          # BatchNorm amplifies the rounding of u - w by no more
    return E, groups_with_pads, int(pads.sum()), kappa


@pytest.mark.parametrize("name", list(sr.FOLD_CASES) + list(sr.MODULE_CASES))
def test_fold_case(name):
    c = sr.FOLD_CASES.get(name) or sr.MODULE_CASES[name]
    E, gp, npad, kappa = _fold_conditions(c)
    print("fold %-34s E = %4d, %3d of %3d groups with trailing pads (%d slots), kappa %.1f" % (name, E, gp, c.B * c.S, npad, kappa))


def test_fold_cases_cover_the_grid():
    cs = list(sr.FOLD_CASES.values())
    assert {c.C for c in cs} == {16, 32, 64, 128, 256} and {c.ns for c in cs} == set(sr.FOLD_NS)
    assert {c.D for c in cs} == {0, 5} and {c.training for c in cs} == {True, False}
    assert {(c.C, c.kind) for c in cs} == {(C, k) for C in (16, 32, 64, 128, 256) for k in ("ball", "knn", "pinned")}
    assert any(c.B * c.S * c.ns < 256 for c in cs) and any(c.B * c.S * c.ns > 256 for c in cs)
    for c in cs:
        g = sr.fold_layers(c, [c.C])[0]["gamma"]
        assert bool((g < 0).any()) and bool((g > 0).any())


def test_trailing_pads_on_a_hand_written_row():
    idx = torch.tensor([[[5, 5, 7, 9], [5, 7, 5, 5], [5, 5, 5, 5], [5, 6, 7, 8]]])
    assert sr.trailing_pads(idx)[0].tolist() == [[False] * 4, [False, False, True, True], [False, True, True, True], [False] * 4]
    sel = torch.tensor([[1, 3], [2, 3], [3, 0], [1, 2]])
    assert sr.pads_to_slot0(sel, idx).tolist() == [[1, 3], [0, 0], [0, 0], [1, 2]]


@pytest.mark.parametrize("name", list(sr.MODULE_CASES))
def test_module_case_has_no_relu_argument_within_rounding_of_zero(name):
    """The loss of a whole module reaches every ReLU of both layers; one whose argument lies within rounding of 0 has its derivative decided
    by rounding, and the gradients of two correct implementations then differ by a whole term.  None of these cases has one: every argument
    (float64, forced selections) is at least KINK_MARGIN of its layer's largest away from 0 -- ten times the 1e-5 that separates the fp32
    paths from float64.  Forcing the float64 selections (padding slots expressed as slot 0) changes no value of the fp32 run beyond rounding."""
    c = sr.MODULE_CASES[name]
    _, sel = sr.module_quantities(c, F64)
    _, _, _, idx = sr.fold_input(c)
    sel = sr.pads_to_slot0(sel, idx)
    pre = []
    q64, _ = sr.module_quantities(c, F64, sel, pre_out=pre)
    margins = [float(p.abs().min() / p.abs().max()) for p in pre]
    assert len(pre) == 2 and min(margins) > sr.KINK_MARGIN, (name, margins)
    q32, _ = sr.module_quantities(c, F32, sel)
    free, _ = sr.module_quantities(c, F32)
    assert sr.dist(q32["out"], free["out"]) < 1e-6 and sr.dist(q32["out"], q64["out"]) < 1e-5
    print("module %-16s ReLU-argument margins %s; fp32 yardstick of the output %.2e" % (name, ["%.1e" % m for m in margins], sr.dist(q32["out"], q64["out"])))


@pytest.mark.parametrize("name", list(sr.FOLD_CASES))
def test_fold_weights_meet_the_premise_of_the_compact_lists(name):
    c = sr.FOLD_CASES[name]
    w, nkink = sr.fold_weights(c)
    _, _, _, idx = sr.fold_input(c)
    pads = sr.trailing_pads(idx).view(c.B * c.S, c.ns)
    w3 = w.view(c.B * c.S, c.ns, c.C)
    assert torch.equal(w3[pads], w3[:, -1:, :].expand(-1, c.ns, -1)[pads])
    assert nkink < 0.01 * w.numel() and float(w.abs().max()) > 0
    if c.kind == "pinned":                                                    # the mid-row repeat carries its OWN weights, unlike the last row's
        assert not torch.equal(w3[0::2, 1], w3[0::2, -1])
    q32, q64 = sr.fold_quantities(c, F32, w), sr.fold_quantities(c, F64, w)
    assert sorted(q32) == sorted(q64)
    print("fold %-34s %d weights zeroed at ReLU kinks; fp32 yardsticks %s" % (name, nkink, {k: "%.1e" % sr.dist(q32[k], q64[k]) for k in q64}))
