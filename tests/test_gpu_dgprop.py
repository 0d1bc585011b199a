"""functional.gn_edge_max (csrc/gnedge.hip) and DGCNN_Propagation (mlsp_amd/propagation.py) against the float64 restatement
(tests/dgprop_restatement.py) fed the same fp32 inputs.

Distance: max|a - b| / max|b|.  Bar per quantity: max(floor, 3 x the distance of the fp32 restatement run on the same device) -- 3 because
the summation order differs.  Floor: the GEMM family's 2e-6 per chained contraction (DESIGN.md section 19's rule): 2e-6 for gn_edge_max
alone (no contraction of its own; its sums over a group count as one), 4e-6 for the module (two stages).  Gradients are compared with the
float64 backward routed through the kernel's recorded slots (functional.recorded_selections); that every recorded slot attains the float64
optimum of its (point, channel) within the forward bar is asserted separately.  No entry is left out of any comparison.

The shapes are the smallest at which each thing can go wrong, not the workload's.  (The off-centre case runs at C = 32: C = 24 with four
groups is outside the kernels' limits and is one of the refusal cases.)"""
import pytest
import torch

import dgprop_restatement as R
from test_dgprop_cpu import NARROW, REF, load_case

pytestmark = pytest.mark.gpu

GN_FLOOR, MODULE_FLOOR = 2e-6, 4e-6
MODES = ("fp32", "f16x3")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def check(name, got, want64, want32, floor):
    """assert dist(got, want64) <= max(floor, 3 dist(want32, want64)); the figures are printed first"""
    d, y = rel(got, want64), rel(want32, want64)
    bar = max(floor, 3 * y)
    print("  %-22s distance %.2e  fp32 restatement %.2e  bar %.2e" % (name, d, y, bar))
    assert torch.isfinite(got).all() and d <= bar, (name, d, y, bar)
    return bar


def make_idx(g, B, Nk, Nq, k):
    if k <= Nk:                                            # k distinct neighbours per query
        return torch.rand(B, Nq, Nk, generator=g).argsort(dim=-1)[:, :, :k].int()
    return torch.randint(0, Nk, (B, Nq, k), generator=g).int()


def gn_inputs(seed, B, Nk, Nq, k, C):
    g = torch.Generator().manual_seed(seed)
    return {"u": torch.randn(B * Nk, C, generator=g), "w": torch.randn(B * Nq, C, generator=g), "idx": make_idx(g, B, Nk, Nq, k),
            "gamma": torch.randn(C, generator=g), "beta": 0.3 * torch.randn(C, generator=g), "R": torch.randn(B * Nq, C, generator=g)}


def gn_gpu(t, groups, dev, eps=1e-5, slope=0.2):
    """-> (out, argk [B Nq, C], {grads}) of the kernel path, and the autograd handles for further backward passes"""
    from mlsp_amd import functional as Fh
    leaf = {n: t[n].to(dev).requires_grad_(True) for n in ("u", "w", "gamma", "beta")}
    with Fh.recorded_selections() as rec:
        out = Fh.gn_edge_max(leaf["u"], leaf["w"], t["idx"].to(dev), leaf["gamma"], leaf["beta"], groups, eps, slope)
    assert len(rec.sel) == 1 and rec.sel[0].dtype == torch.uint8 and rec.sel[0].shape == out.shape
    loss = (out * t["R"].to(dev)).sum()
    grads = dict(zip(leaf, torch.autograd.grad(loss, list(leaf.values()), retain_graph=True)))
    return out.detach(), rec.sel[0], grads, (loss, leaf)


def gn_restated(t, groups, dev, dtype, argk, eps=1e-5, slope=0.2):
    B, Nq, k = t["idx"].shape
    C = t["u"].shape[1]
    leaf = {n: t[n].to(dev).to(dtype).requires_grad_(True) for n in ("u", "w", "gamma", "beta")}
    idx = t["idx"].to(dev).long()
    kw = dict(groups=groups, eps=eps, slope=slope, dtype=dtype)
    free = R.gn_edge_max(leaf["u"].view(B, -1, C), leaf["w"].view(B, Nq, C), idx, leaf["gamma"], leaf["beta"], **kw)
    routed = R.gn_edge_max(leaf["u"].view(B, -1, C), leaf["w"].view(B, Nq, C), idx, leaf["gamma"], leaf["beta"], argk=argk.view(B, Nq, C), **kw)
    grads = dict(zip(leaf, torch.autograd.grad((routed.reshape(B * Nq, C) * t["R"].to(dev).to(dtype)).sum(), list(leaf.values()))))
    return free.detach().reshape(B * Nq, C), routed.detach().reshape(B * Nq, C), grads


def gn_compare(t, groups, dev, floor=GN_FLOOR, **kw):
    """the whole comparison of one gn_edge_max call; -> (out, argk, grads, float64 grads)"""
    k = t["idx"].shape[2]
    out, argk, grads, _ = gn_gpu(t, groups, dev, **kw)
    assert int(argk.max()) < k
    free64, routed64, g64 = gn_restated(t, groups, dev, torch.float64, argk, **kw)
    free32, _, g32 = gn_restated(t, groups, dev, torch.float32, argk, **kw)
    bar = check("out", out, free64, free32, floor)
    # the recorded slot attains the float64 optimum of its (point, channel)
    gap = float((free64 - routed64).abs().max() / free64.abs().max())
    print("  recorded slots: worst distance from the float64 optimum %.2e" % gap)
    assert gap <= bar, (gap, bar)
    for n in ("u", "w", "gamma", "beta"):
        check("d" + n, grads[n], g64[n], g32[n], floor)
    return out, argk, grads, g64


GN_CASES = [(1, 4, 4, 4, 16, 4), (2, 8, 16, 1, 16, 4), (2, 5, 67, 3, 48, 4), (2, 16, 8, 4, 32, 4), (1, 8, 16, 16, 512, 4), (1, 8, 16, 4, 384, 4),
            (1, 64, 64, 64, 16, 4)]


@pytest.mark.parametrize("shape", GN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_gn_edge_max_against_float64(dev, shape):
    B, Nk, Nq, k, C, groups = shape
    t = gn_inputs(sum(shape), B, Nk, Nq, k, C)
    _, _, grads, _ = gn_compare(t, groups, dev)
    if Nq < Nk:                                            # source points that no edge names: exactly 0
        named = torch.zeros(B * Nk, dtype=torch.bool)
        named[(torch.arange(B).view(B, 1, 1) * Nk + t["idx"].long()).flatten()] = True
        assert not bool(named.all())
        assert bool((grads["u"].cpu()[~named] == 0).all())


def test_gn_edge_max_repeated_neighbour(dev):
    """one query names the same source twice: the first slot wins, du receives both edges' dense terms"""
    B, Nk, Nq, k, C, groups = 1, 6, 5, 3, 16, 4
    t = gn_inputs(11, B, Nk, Nq, k, C)
    t["idx"][0, 2] = torch.tensor([4, 4, 1])
    t["u"][4] += 3.0                                       # source 4 wins wherever gamma > 0
    _, argk, _, _ = gn_compare(t, groups, dev)
    a = argk.view(B, Nq, C)[0, 2].cpu()
    assert bool((a != 1).all()) and bool((a[t["gamma"] > 0] == 0).all())


def test_gn_edge_max_negative_and_zero_gamma(dev):
    B, Nk, Nq, k, C, groups = 2, 8, 16, 4, 32, 4
    t = gn_inputs(12, B, Nk, Nq, k, C)
    t["gamma"][::3] = -t["gamma"][::3].abs()
    t["gamma"][5] = 0.0
    out, argk, grads, g64 = gn_compare(t, groups, dev)
    want = torch.nn.functional.leaky_relu(t["beta"][5], 0.2)
    assert bool((out[:, 5].cpu() == want).all())
    assert g64["gamma"][5] != 0 and int(argk.max()) < k


def test_gn_edge_max_constant_group(dev):
    """variance 0 in one (cloud, group): rstd = 1 / sqrt(eps), everything finite"""
    B, Nk, Nq, k, C, groups = 2, 8, 16, 4, 32, 4
    t = gn_inputs(13, B, Nk, Nq, k, C)
    t["u"][:Nk, 8:16] = 1.5
    t["w"][:Nq, 8:16] = 0.25
    out, _, grads, _ = gn_compare(t, groups, dev)
    want = torch.nn.functional.leaky_relu(t["beta"][8:16], 0.2)
    assert bool((out[:Nq, 8:16].cpu() == want).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_gn_edge_max_off_centre(dev):
    """u + w with mean 100 and standard deviation 1: a one-pass fp32 variance is 1e-3 off here, a centred one 5e-6"""
    B, Nk, Nq, k, C, groups = 2, 8, 16, 4, 32, 4
    t = gn_inputs(14, B, Nk, Nq, k, C)
    t["u"] = t["u"] * (0.5 ** 0.5) + 60.0
    t["w"] = t["w"] * (0.5 ** 0.5) + 40.0
    gn_compare(t, groups, dev)


def test_gn_edge_max_one_nan(dev):
    B, Nk, Nq, k, C, groups = 2, 8, 16, 4, 32, 4
    t = gn_inputs(15, B, Nk, Nq, k, C)
    t["idx"][0, 3, 1] = 5
    t["u"][5, 9] = float("nan")
    out, argk, _, _ = gn_gpu(t, groups, dev)
    free64, _, _ = gn_restated(t, groups, dev, torch.float64, argk)
    assert int(argk.max()) < k
    assert torch.equal(torch.isnan(out), torch.isnan(free64))
    assert bool(torch.isnan(out[:Nq, 8:16]).all()) and not bool(torch.isnan(out[Nq:]).any()) and not bool(torch.isnan(out[:, :8]).any())
    ok = ~torch.isnan(free64)
    assert rel(out[ok], free64[ok]) <= GN_FLOOR * 3


def test_gn_edge_max_refuses_what_it_cannot_do(dev):
    from mlsp_amd import _lib, functional as Fh
    for (B, Nk, Nq, k, C, groups) in ((1, 8, 8, 4, 24, 4), (1, 8, 8, 65, 16, 4)):
        t = gn_inputs(16, B, Nk, Nq, k, C)
        with pytest.raises(_lib.MlspLibraryError):
            Fh.gn_edge_max(t["u"].to(dev), t["w"].to(dev), t["idx"].to(dev), t["gamma"].to(dev), t["beta"].to(dev), groups)
    torch.cuda.synchronize()


def test_gn_edge_max_backward_is_deterministic(dev):
    B, Nk, Nq, k, C, groups = 2, 16, 67, 4, 48, 4
    t = gn_inputs(17, B, Nk, Nq, k, C)
    _, _, first, (loss, leaf) = gn_gpu(t, groups, dev)
    again = dict(zip(leaf, torch.autograd.grad(loss, list(leaf.values()))))
    _, _, second, _ = gn_gpu(t, groups, dev)
    for n in first:
        assert torch.equal(first[n], again[n]) and torch.equal(first[n], second[n]), n


# ---------------------------------------------------------------------------------------------
def make_module(params, k, dev):
    from mlsp_amd.propagation import DGCNN_Propagation
    mid, two_in = params["layer1.0.weight"].shape[:2]
    m = DGCNN_Propagation(k=k, in_dim=two_in // 2, mid_dim=mid)
    m.load_state_dict({n: v.clone() for n, v in params.items()}, strict=True)
    return m.to(dev)


def module_inputs(seed, B, G, N, cin):
    g = torch.Generator().manual_seed(seed)
    return {"coor": torch.randn(B, 3, G, generator=g), "f": torch.randn(B, cin, G, generator=g), "coor_q": torch.randn(B, 3, N, generator=g),
            "f_q": torch.randn(B, cin, N, generator=g), "R": torch.randn(B, cin, N, generator=g)}


def narrow_params(seed, cin=16, mid=32):
    g = torch.Generator().manual_seed(seed)
    return {"layer1.0.weight": torch.randn(mid, 2 * cin, 1, 1, generator=g) / (2 * cin) ** 0.5, "layer1.1.weight": torch.randn(mid, generator=g),
            "layer1.1.bias": 0.3 * torch.randn(mid, generator=g), "layer2.0.weight": torch.randn(cin, 2 * mid, 1, 1, generator=g) / (2 * mid) ** 0.5,
            "layer2.1.weight": torch.randn(cin, generator=g), "layer2.1.bias": 0.3 * torch.randn(cin, generator=g)}


def module_graphs(m, t, dev):
    from mlsp_amd import pointnet2
    q = t["coor_q"].to(dev).transpose(1, 2).contiguous()
    return pointnet2.knn_point(m.k, t["coor"].to(dev).transpose(1, 2).contiguous(), q), pointnet2.knn_point(m.k, q, q)


def module_restated(params, t, graphs, argk, dev, dtype):
    p = {n: v.to(dev).to(dtype).requires_grad_(True) for n, v in params.items()}
    f, f_q = (t[n].to(dev).to(dtype).requires_grad_(True) for n in ("f", "f_q"))
    args = (t["coor"].to(dev), f, t["coor_q"].to(dev), f_q, graphs[0], graphs[1])
    free = R.forward(p, *args, dtype=dtype).detach()
    routed = R.forward(p, *args, dtype=dtype, argk=argk)
    (routed * t["R"].to(dev).to(dtype)).sum().backward()
    grads = {n: v.grad for n, v in p.items()}
    grads["f"], grads["f_q"] = f.grad, f_q.grad
    return free, routed.detach(), grads


def module_compare(m, params, t, dev, mode, rows16=False):
    """one forward + backward of the module in `mode` against the restatement; -> out"""
    from mlsp_amd import functional as Fh
    B, _, N = t["f_q"].shape
    m.zero_grad(set_to_none=True)
    f, f_q = (t[n].to(dev).requires_grad_(True) for n in ("f", "f_q"))
    with Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = m(t["coor"].to(dev), f, t["coor_q"].to(dev), f_q)
        (out * t["R"].to(dev)).sum().backward()
    argk = [a.view(B, N, -1) for a in rec.sel]
    assert len(argk) == 2 and all(int(a.max()) < m.k for a in argk)
    graphs = module_graphs(m, t, dev)
    free64, routed64, g64 = module_restated(params, t, graphs, argk, dev, torch.float64)
    free32, _, g32 = module_restated(params, t, graphs, argk, dev, torch.float32)
    print(" mode", mode)
    bar = check("out", out.detach(), free64, free32, MODULE_FLOOR)
    gap = float((free64 - routed64).abs().max() / free64.abs().max())
    print("  recorded slots: worst distance from the float64 optimum %.2e" % gap)
    assert gap <= bar, (gap, bar)
    got = {n: p.grad for n, p in m.named_parameters()}
    got["f"], got["f_q"] = f.grad, f_q.grad
    assert set(got) == set(g64)
    for n in sorted(got):
        sl = slice(None, None, 16) if rows16 and got[n].dim() == 4 else slice(None)
        check("d " + n, got[n][sl], g64[n][sl], g32[n][sl], MODULE_FLOOR)
    return out.detach()


@pytest.mark.parametrize("name", [NARROW, REF])
def test_module_on_the_reference_fixtures(dev, name):
    """both fixtures, both product modes: the output, the input gradients and every stored parameter gradient (or its stored rows)"""
    c, params = load_case(name)
    B, G, N, k, cin, mid = (int(v) for v in c["dims"])
    t = {n: torch.from_numpy(c[n]) for n in ("coor", "f", "coor_q", "f_q", "R")}
    m = make_module(params, k, dev)
    g1, g2 = module_graphs(m, t, dev)
    assert torch.equal(g1.cpu().int(), torch.from_numpy(c["idx1"])) and torch.equal(g2.cpu().int(), torch.from_numpy(c["idx2"]))
    for mode in MODES:
        out = module_compare(m, params, t, dev, mode, rows16=name == REF)
        d = rel(out.cpu(), torch.from_numpy(c["out"]))
        print("  out against the reference's own fp32 result: %.2e" % d)
        assert d <= 1e-5, d


@pytest.mark.parametrize("shape", [(2, 8, 16, 4), (2, 16, 33, 16), (1, 4, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_module_narrow_against_float64(dev, shape):
    B, G, N, k = shape
    params, t = narrow_params(sum(shape)), module_inputs(100 + sum(shape), B, G, N, 16)
    m = make_module(params, k, dev)
    for mode in MODES:
        module_compare(m, params, t, dev, mode)


def test_module_forward_rows_is_forward(dev):
    B, G, N, k = 2, 8, 16, 4
    params, t = narrow_params(5), module_inputs(105, B, G, N, 16)
    m = make_module(params, k, dev)
    g = {n: v.to(dev) for n, v in t.items()}
    with torch.no_grad():
        a = m(g["coor"], g["f"], g["coor_q"], g["f_q"])
        b = m.forward_rows(g["coor"].transpose(1, 2).contiguous(), g["f"].transpose(1, 2).reshape(B * G, 16),
                           g["coor_q"].transpose(1, 2).contiguous(), g["f_q"].transpose(1, 2).reshape(B * N, 16))
    assert a.shape == (B, 16, N) and b.shape == (B * N, 16)
    assert torch.equal(a, b.view(B, N, 16).transpose(1, 2))


def test_module_after_two_flat_adam_steps(dev):
    from mlsp_amd.optim import FlatAdam
    B, G, N, k = 2, 8, 16, 4
    params, t = narrow_params(6), module_inputs(106, B, G, N, 16)
    m = make_module(params, k, dev)
    opt = FlatAdam(m.parameters(), lr=1e-2)
    g = {n: v.to(dev) for n, v in t.items()}
    for _ in range(2):
        opt.zero_grad()
        (m(g["coor"], g["f"], g["coor_q"], g["f_q"]) * g["R"]).sum().backward()
        opt.step()
    now = {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
    assert not torch.equal(now["layer1.0.weight"], params["layer1.0.weight"]) and not torch.equal(now["layer2.1.bias"], params["layer2.1.bias"])
    module_compare(m, now, t, dev, "f16x3")


def test_fps_downsample_is_exact(dev):
    from mlsp_amd.propagation import DGCNN_Propagation
    g = torch.Generator().manual_seed(7)
    coor, x = torch.randn(2, 3, 32, generator=g), torch.randn(2, 16, 32, generator=g)
    idx, want_c, want_x = R.fps_downsample(coor, x, 8)
    assert idx.shape == (2, 8) and bool((idx[:, 0] == 0).all())
    got_c, got_x = DGCNN_Propagation.fps_downsample(coor.to(dev), x.to(dev), 8)
    assert torch.equal(got_c.cpu(), want_c) and torch.equal(got_x.cpu(), want_x)
