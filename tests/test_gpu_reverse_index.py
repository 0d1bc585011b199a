"""The reverse neighbour index and the sa.hip gathers that walk it, on every kernel path.

a. knn_reverse_kernel (mlsp_group_reverse, mlsp_group_reverse_compact, mlsp_knn_reverse) against the host sort of
   tests/reverse_restatement.py: integer data, compared exactly, between guard words, twice (atomics decide the fill order).
   tests/test_reverse_restatement_cpu.py proves which case of the table reaches which path of the kernel.
b. - d. mlsp_sa_group_bwd_f32, mlsp_interp3_{fwd,bwd}_f32 and mlsp_sa_fold_bwd_f32 (compact and full index) against float64, fed the
   HOST-built index: a failure belongs to the gather.  Bound per output element, derived from the kernel's expression and not from
   what it returns:  |got - ref64| <= (L + r) 2^-24 A  with L the terms summed into the element (padding rows count), r the fp32
   roundings the kernel applies to one term (counted beside each test) and A the reference sum over the terms' absolute values.
e. the index contract of the query kNN (mlsp_knn_query_f32): non-finite distances never produce an index outside [0, Nr)."""
import numpy as np
import pytest
import torch

import reverse_restatement as rr
from oracle import ref_sa_cpu as sa

pytestmark = pytest.mark.gpu

GUARD, FILL = 1024, -7
U = 2.0 ** -24
MLSP_ERR_ARG, MLSP_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from mlsp_amd import _lib as L
    return L


# ----------------------------------------------------------------------------- a. the builder, exactly
_refs = {}


def _reference(name, skip_pad):
    """(idx, host reference) of one case of the table, computed once and left unchanged"""
    key = (name, skip_pad)
    if key not in _refs:
        idx = rr.case_idx(name)
        _refs[key] = (idx, rr.reverse_reference(idx, rr.CASES[name].N, skip_pad))
    return _refs[key]


def _guarded(n, dev):
    big = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    return big, big[GUARD:GUARD + n]


def _build(api, idx_dev, c, dev):
    """one call of the builder into fresh guarded buffers -> (return code, {name: (whole buffer on the host, payload length)})"""
    L = _lib()
    lib = L.load()
    E = c.B * c.S * c.k
    bufs = {"rev_off": _guarded(c.B * c.N + 1, dev), "rev_ent": _guarded(E, dev), "rev_cnt": _guarded(c.B * c.N, dev),
            "pad_cnt": _guarded(c.B * c.S, dev)}
    p = {n: v[1].data_ptr() for n, v in bufs.items()}
    if api == "group":
        rc = lib.mlsp_group_reverse(idx_dev.data_ptr(), c.B, c.S, c.N, c.k, p["rev_off"], p["rev_ent"], L.stream())
    elif api == "compact":
        rc = lib.mlsp_group_reverse_compact(idx_dev.data_ptr(), c.B, c.S, c.N, c.k, p["rev_off"], p["rev_cnt"], p["rev_ent"], p["pad_cnt"],
                                            L.stream())
    else:
        rc = lib.mlsp_knn_reverse(idx_dev.data_ptr(), c.B, c.N, c.k, p["rev_off"], p["rev_ent"], L.stream())
    torch.cuda.synchronize()
    return rc, {n: (v[0].cpu().numpy(), v[1].numel()) for n, v in bufs.items()}


_BUILDS = [(n, api) for n in rr.CASES for api in ("group", "compact", "knn") if api != "knn" or rr.CASES[n].S == rr.CASES[n].N]


@pytest.mark.parametrize("name,api", _BUILDS, ids=["%s-%s" % na for na in _BUILDS])
def test_reverse_index_equals_host_sort(dev, name, api):
    """rev_off / rev_cnt / pad_cnt equal the reference; rev_ent equals it on every list position and keeps its prefill everywhere else (compact
    mode: the unfilled tail of each cloud's region); no guard word on either side of any buffer is touched; a second call gives the same."""
    c = rr.CASES[name]
    compact = api == "compact"
    idx, ref = _reference(name, compact)
    idx_dev = torch.from_numpy(idx).to(dev)
    want = {"rev_off": ref.rev_off, "rev_ent": np.where(ref.listed, ref.rev_ent, FILL).astype(np.int32),
            "rev_cnt": ref.rev_cnt if compact else np.full(c.B * c.N, FILL, dtype=np.int32),
            "pad_cnt": ref.pad_cnt if compact else np.full(c.B * c.S, FILL, dtype=np.int32)}
    assert compact or ref.listed.all()
    runs = []
    for _ in range(2):
        rc, got = _build(api, idx_dev, c, dev)
        assert rc == 0
        for n, (whole, length) in got.items():
            assert (whole[:GUARD] == FILL).all() and (whole[GUARD + length:] == FILL).all(), "guard words of %s written" % n
            body = whole[GUARD:GUARD + length]
            bad = np.flatnonzero(body != want[n])
            assert bad.size == 0, "%s: %d wrong words, first at %d: got %d, want %d" % (n, bad.size, bad[0], body[bad[0]], want[n][bad[0]])
        runs.append(got)
    for n in runs[0]:
        assert np.array_equal(runs[0][n][0], runs[1][n][0]), n


def test_reverse_index_error_paths(dev):
    """Refused before any launch: nothing is written."""
    L = _lib()
    lib = L.load()
    idx = torch.zeros(8, dtype=torch.int32, device=dev)
    off, ent, pad = (torch.full((n,), FILL, dtype=torch.int32, device=dev) for n in (50001, 300, 8))
    st = L.stream()
    assert lib.mlsp_group_reverse(idx.data_ptr(), 1, 1, 4, 257, off.data_ptr(), ent.data_ptr(), st) == MLSP_ERR_ARG
    assert lib.mlsp_knn_reverse(idx.data_ptr(), 1, 1, 257, off.data_ptr(), ent.data_ptr(), st) == MLSP_ERR_ARG
    assert lib.mlsp_group_reverse(idx.data_ptr(), 1, 1, 50000, 1, off.data_ptr(), ent.data_ptr(), st) == MLSP_ERR_UNSUPPORTED
    assert lib.mlsp_group_reverse_compact(idx.data_ptr(), 1, 2, 4, 4, off.data_ptr(), None, ent.data_ptr(), pad.data_ptr(), st) == MLSP_ERR_ARG
    torch.cuda.synchronize()
    for t in (off, ent, pad):
        assert bool((t == FILL).all())


# ----------------------------------------------------------------------------- b. - d. the gathers, against float64
def _check(what, got, ref, bound):
    """|got - ref| <= bound elementwise (float64 on the host); prints and returns the worst error-to-bound ratio"""
    got, ref, bound = got.detach().cpu().double(), ref.double(), bound.double()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert bool((err[~live] == 0).all()), "%s: an element with no term is not exactly 0" % what
    assert worst <= 1.0, (what, worst)
    return worst


def _to_dev(ref, dev, names=("rev_off", "rev_ent", "rev_cnt", "pad_cnt")):
    return {n: torch.from_numpy(np.ascontiguousarray(getattr(ref, n))).to(dev) for n in names}


_graph = {}


def _degree_graph():
    """B = 2 clouds of S = 64 groups x ns = 16 slots over N = 40 points.  Cloud 0: point t has in-degree t for t = 0..9 (every remainder of the
    4-unrolled entry loop, the empty list included), point 10 has 600 (above 512), the other slots are uniform over the points 11..39.
    Cloud 1 is uniform.  -> (idx, host reverse index, in-degrees [B*N])"""
    if not _graph:
        B, S, N, ns = 2, 64, 40, 16
        rng = np.random.default_rng(11)
        dest = [t for t in range(10) for _ in range(t)] + [10] * 600
        dest += rng.integers(11, N, size=S * ns - len(dest)).tolist()
        idx = np.stack([rng.permutation(np.array(dest)).reshape(S, ns), rng.integers(0, N, size=(S, ns))]).astype(np.int32)
        ref = rr.reverse_reference(idx, N)
        deg = ref.rev_cnt.astype(np.int64)
        assert deg[:10].tolist() == list(range(10)) and deg[10] == 600 and deg.max() > 512
        _graph["g"] = (idx, ref, deg)
    return _graph["g"]


@pytest.mark.parametrize("col", [0, 3])
@pytest.mark.parametrize("D", [1, 3, 64, 65, 130])
def test_sa_group_bwd_vs_float64(dev, D, col):
    """sa_group_bwd_kernel: dfeat[j] = sum of the rows dG[(i, s)][col : col + D] that name j.  D = 65 and 130 take the `c0 += 64` column loop
    twice and three times with a ragged last pass; in-degrees 0..9 take every remainder of the 4-unrolled entry loop.
    r = 0: a term is a loaded value, the kernel only adds (every add is one of the L)."""
    L = _lib()
    lib = L.load()
    idx, ref, deg = _degree_graph()
    B, S, ns = idx.shape
    N = 40
    ldg = col + D + 2
    g = torch.Generator().manual_seed(100 * D + col)
    dG = torch.randn(B * S * ns, ldg, generator=g)
    dst = torch.from_numpy((idx.astype(np.int64) + np.arange(B)[:, None, None] * N).reshape(-1))
    terms = dG[:, col:col + D].double()
    want = torch.zeros(B * N, D, dtype=torch.float64).index_add_(0, dst, terms)
    A = torch.zeros(B * N, D, dtype=torch.float64).index_add_(0, dst, terms.abs())
    R = 0
    bound = (torch.from_numpy(deg).double()[:, None] + R) * U * A
    r = _to_dev(ref, dev, ("rev_off", "rev_ent"))
    dGd = dG.to(dev)
    got = torch.full((B * N, D), float("nan"), device=dev)
    L.check(lib.mlsp_sa_group_bwd_f32(dGd.data_ptr(), ldg, col, D, r["rev_off"].data_ptr(), r["rev_ent"].data_ptr(), B, N, S, ns,
                                      got.data_ptr(), L.stream()), "mlsp_sa_group_bwd_f32")
    assert bool((got[0] == 0).all()) and deg[0] == 0           # the point nothing names: exactly 0
    _check("sa_group_bwd D=%d col=%d" % (D, col), got, want, bound)


@pytest.mark.parametrize("D", [1, 4, 7, 64, 67])
@pytest.mark.parametrize("S", [3, 50])
def test_interp3_fwd_bwd_vs_float64(dev, S, D):
    """interp3_fwd_kernel / interp3_bwd_kernel: weights w_t / sum w, w_t = 1 / (d_t + 1e-8f), on distances of exactly 0, 1e-9 and ordinary
    ones (all >= 0); channel quads with D % 4 != 0.  The reference evaluates the same fp32 distances (and the fp32 constant) in float64.
    r = 8 per term f * (w_u / ws): w_u carries 2 roundings (the add of 1e-8f, the reciprocal); ws its three w's (2, weighted by w_v / ws)
    plus its 2 inexact adds = 4; the division 1; the product with the feature 1.  L: forward 3, backward the source's in-degree."""
    L = _lib()
    lib = L.load()
    B, N = 2, 130
    rng = np.random.default_rng(10 * S + D)
    if S == 50:                                               # source 13 is in no row: no entry, gradient exactly 0
        idx = rng.integers(0, S - 1, size=(B, N, 3))
        idx = (idx + (idx >= 13)).astype(np.int32)
    else:
        idx = rng.integers(0, S, size=(B, N, 3)).astype(np.int32)
    kind = rng.integers(0, 10, size=(B, N, 3))
    dist = np.where(kind < 2, 0.0, np.where(kind < 4, 1e-9, rng.uniform(1e-4, 1.0, size=(B, N, 3)))).astype(np.float32)
    dist[0, 0], dist[0, 1], dist[0, 2] = (0.0, 0.0, 0.0), (0.0, 1e-9, 0.5), (1e-9, 1e-9, 1e-9)
    assert (dist >= 0).all() and (dist == 0).any() and (dist == np.float32(1e-9)).any()
    g = torch.Generator().manual_seed(7 * S + D)
    feat, dout = torch.randn(B, S, D, generator=g), torch.randn(B, N, D, generator=g)
    w = 1.0 / (torch.from_numpy(dist).double() + float(np.float32(1e-8)))
    wn = (w / w.sum(-1, keepdim=True)).reshape(B * N, 3)                                      # [B*N, 3]
    src = torch.from_numpy((idx.astype(np.int64) + np.arange(B)[:, None, None] * S).reshape(B * N, 3))
    f64, do64 = feat.double().reshape(B * S, D), dout.double().reshape(B * N, D)
    want_f = sum(wn[:, t:t + 1] * f64[src[:, t]] for t in range(3))
    A_f = sum(wn[:, t:t + 1] * f64[src[:, t]].abs() for t in range(3))
    want_b, A_b = torch.zeros(B * S, D, dtype=torch.float64), torch.zeros(B * S, D, dtype=torch.float64)
    for t in range(3):
        want_b.index_add_(0, src[:, t], wn[:, t:t + 1] * do64)
        A_b.index_add_(0, src[:, t], wn[:, t:t + 1] * do64.abs())
    ref = rr.reverse_reference(idx, S)                        # the roles of mlsp_group_reverse: S <- N rows of k = 3 slots over N <- S sources
    deg = torch.from_numpy(ref.rev_cnt.astype(np.int64)).double()
    R = 8
    idx_d, dist_d, feat_d, dout_d = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a.to(dev) for a in (idx, dist, feat, dout))
    out = torch.full((B * N, D), float("nan"), device=dev)
    L.check(lib.mlsp_interp3_fwd_f32(feat_d.data_ptr(), idx_d.data_ptr(), dist_d.data_ptr(), B, N, S, D, out.data_ptr(), L.stream()),
            "mlsp_interp3_fwd_f32")
    _check("interp3_fwd S=%d D=%d" % (S, D), out, want_f, (3 + R) * U * A_f)
    r = _to_dev(ref, dev, ("rev_off", "rev_ent"))
    dfeat = torch.full((B * S, D), float("nan"), device=dev)
    L.check(lib.mlsp_interp3_bwd_f32(dout_d.data_ptr(), dist_d.data_ptr(), r["rev_off"].data_ptr(), r["rev_ent"].data_ptr(), B, N, S, D,
                                     dfeat.data_ptr(), L.stream()), "mlsp_interp3_bwd_f32")
    if S == 50:
        assert ref.rev_cnt[13] == 0 and ref.rev_cnt[S + 13] == 0 and bool((dfeat[13] == 0).all()) and bool((dfeat[S + 13] == 0).all())
    _check("interp3_bwd S=%d D=%d" % (S, D), dfeat, want_b, (deg[:, None] + R) * U * A_b)


@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("ns", [8, 32])
@pytest.mark.parametrize("C", [16, 64, 256])
def test_sa_fold_bwd_both_index_forms_vs_float64(dev, C, ns, training):
    """mlsp_sa_fold_bwd_f32 (sa_fold_edge_kernel<2>, sa_fold_bwd_centre_kernel, sa_fold_bwd_point_kernel) in three forms:
    (1) the compact index (rev_cnt / pad_cnt) with a dZ whose padding rows equal their group's last-slot row -- THE PREMISE OF THE COMPACT
        FORM: the kernel adds a group's padding rows as pad_cnt times the row of its last slot, which is right only when those rows carry
        the same incoming gradient (they do behind the layer's own forward: identical rows in, identical rows out);
    (2) the full index (rev_cnt = pad_cnt = NULL: two entries in flight, a branch no Python path reaches) with the same dZ;
    (3) the full index with an unconstrained dZ.
    C = 16 / 64 / 256: 16 / 4 / 1 entry lanes per wave.  One point is the first hit of every group and collects most of the padding.
    The reference works in float64 on the kernel's fp32 inputs (y = fp32(u - w) and the four fp32 BatchNorm vectors); its ReLU gate is the
    sign of the exact y * scale + shift, which is the sign of the fmaf the kernel rounds: no kink exclusions.
    Roundings, from saf_dy  sc * (d - m1 - (y - mu) * is * m2)  (y is the reference's own fp32 value, d is exact):
      dbeta   L = C/4 (sa_fold_edge_kernel: 256 edges per workgroup over 256 / (C/4) edge lanes -> a run of C/4 fp32 adds per thread, then
              double partials), r = 1 (the cast of the double sum to fp32);
      dgamma  the same L; r = 3: yhat = (y - mu) * is is 2 roundings, the fmaf adds none beyond the run, the cast 1;
      du, dw  eval: r = 1 (m1 = m2 = 0: only the product with sc rounds).  Training: the worst leaf is yhat * m2 with 5 roundings
              ((y - mu), * is, * m2, the subtraction, * sc) and m2 = dgamma / E carries dgamma's own (C/4 + 3): r = C/4 + 8.
              A takes |m1|, |m2| from the absolute sums as well.  L = edges that name the point (padding rows included) / ns."""
    L = _lib()
    lib = L.load()
    B, N, S = 2, 96, 24
    E = B * S * ns
    rng = np.random.default_rng(1000 * C + 10 * ns + training)
    idx = rr.with_hub(rr.ball_like(rng, B, S, N, ns))
    pad = np.zeros(idx.shape, dtype=bool)
    pad[:, :, 1:] = idx[:, :, 1:] == idx[:, :, :1]
    assert pad.sum() > E // 4 and (rr.reverse_reference(idx, N).rev_cnt[[0, N]] > pad.sum() // 4).all()      # the hub of either cloud
    g = torch.Generator().manual_seed(C + ns + training)
    u, w = torch.randn(B * N, C, generator=g), 0.5 * torch.randn(B * S, C, generator=g)
    flat = torch.from_numpy((idx.astype(np.int64) + np.arange(B)[:, None, None] * N).reshape(-1))           # source row of every edge
    ctr = torch.arange(B * S).repeat_interleave(ns)
    y = (u[flat] - w[ctr]).double()                                                                          # fp32(u - w), exactly
    mean, var = y.mean(0), y.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    gamma = (0.5 + torch.rand(C, generator=g).double()) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0).double()
    beta = (torch.rand(C, generator=g).double() - 0.5) * 0.6
    assert (gamma < 0).any() and (gamma > 0).any()
    scale = gamma * invstd
    bn = torch.stack([scale, beta - mean * scale, mean, invstd]).float()                                     # bn_save [4][C], fp32
    sc, sh, mu, is_ = bn.double()
    gate = (y * sc + sh) > 0
    yhat = (y - mu) * is_
    dz_free = torch.randn(E, C, generator=g)
    padm = torch.from_numpy(pad).reshape(B * S, ns, 1)
    dz3 = dz_free.view(B * S, ns, C)
    dz_tied = torch.where(padm, dz3[:, -1:, :].expand(-1, ns, -1), dz3).reshape(E, C).contiguous()            # a group with padding ends in it
    lstat = C // 4
    r_point = lstat + 8 if training else 1

    def reference(dz):
        d = torch.where(gate, dz.double(), torch.zeros((), dtype=torch.float64))
        dbeta, dgamma, a_beta, a_gamma = d.sum(0), (d * yhat).sum(0), d.abs().sum(0), (d * yhat).abs().sum(0)
        m1, m2, m1a, m2a = (dbeta / E, dgamma / E, a_beta / E, a_gamma / E) if training else (torch.zeros(C, dtype=torch.float64),) * 4
        dy, dya = sc * (d - m1 - yhat * m2), sc.abs() * (d.abs() + m1a + yhat.abs() * m2a)
        du = torch.zeros(B * N, C, dtype=torch.float64).index_add_(0, flat, dy)
        dua = torch.zeros(B * N, C, dtype=torch.float64).index_add_(0, flat, dya)
        ldu = torch.bincount(flat, minlength=B * N).double()[:, None]
        return {"du": (du, (ldu + r_point) * U * dua), "dw": (-dy.view(B * S, ns, C).sum(1), (ns + r_point) * U * dya.view(B * S, ns, C).sum(1)),
                "dgamma": (dgamma, (lstat + 3) * U * a_gamma), "dbeta": (dbeta, (lstat + 1) * U * a_beta)}

    full, comp = rr.reverse_reference(idx, N), rr.reverse_reference(idx, N, skip_pad=True)
    assert comp.pad_cnt.sum() == pad.sum()
    rf, rc = _to_dev(full, dev, ("rev_off", "rev_ent")), _to_dev(comp, dev)
    ud, wd, idxd, bnd = u.to(dev), w.to(dev), torch.from_numpy(idx).to(dev), bn.to(dev)
    ws, wsn = L.workspace(dev, E, C, C)
    refs = {"tied": reference(dz_tied), "free": reference(dz_free)}
    for form, dz, r, which in (("compact", dz_tied, rc, "tied"), ("full", dz_tied, rf, "tied"), ("full-free", dz_free, rf, "free")):
        dzd = dz.to(dev)
        out = {"du": torch.full((B * N, C), float("nan"), device=dev), "dw": torch.full((B * S, C), float("nan"), device=dev),
               "dgamma": torch.full((C,), float("nan"), device=dev), "dbeta": torch.full((C,), float("nan"), device=dev)}
        L.check(lib.mlsp_sa_fold_bwd_f32(dzd.data_ptr(), ud.data_ptr(), wd.data_ptr(), idxd.data_ptr(), r["rev_off"].data_ptr(),
                                         r["rev_ent"].data_ptr(), L.ptr(r.get("rev_cnt")), L.ptr(r.get("pad_cnt")), B, N, S, ns, C,
                                         bnd.data_ptr(), training, out["du"].data_ptr(), out["dw"].data_ptr(), out["dgamma"].data_ptr(),
                                         out["dbeta"].data_ptr(), ws, wsn, L.stream()), "mlsp_sa_fold_bwd_f32")
        for n in ("du", "dw", "dgamma", "dbeta"):
            _check("sa_fold_bwd C=%d ns=%d training=%d %s %s" % (C, ns, training, form, n), out[n], *refs[which][n])


# ----------------------------------------------------------------------------- e. the query kNN's index contract
def _grid(shape, gen):
    """coordinates on the grid of eighths in [-1, 1]: every difference, square and sum of the distance is exact in fp32, whatever its
    association -- the kernel, the oracle and the host restatement compute the same numbers, and exact ties abound"""
    return torch.randint(-8, 9, shape, generator=gen).float() / 8


@pytest.mark.parametrize("k", [3, 16, 32, 64])
@pytest.mark.parametrize("C", [3, 8])
def test_knn_point_indices_stay_in_range_on_non_finite_input(dev, C, k):
    """mlsp_knn_query_f32's contract (include/mlsp_hip.h): a NaN or overflowed distance counts as +inf, +inf candidates fill the slots no
    finite candidate took, lowest index first, so every index lies in [0, Nr) -- the gathers behind it (index_points, the 3-NN
    interpolation) do not range-check.  The indices are read on the host only; nothing here gathers with them.
    Rows whose query and whole cloud are finite are bit-identical to oracle.ref_sa_cpu.knn_group; every row equals the contract's own host
    restatement (the fp32 distances with non-finite ones set to +inf, stable argsort), and the returned distances are those."""
    from mlsp_amd import pointnet2 as p2
    B, Nr, Nq = 2, 200, 70
    nan = float("nan")
    for kind in ("nan_query", "nan_reference", "k_minus_1_finite", "overflow"):
        gen = torch.Generator().manual_seed(100 * C + k)
        x, q = _grid((B, Nr, C), gen), _grid((B, Nq, C), gen)
        rows_ok = torch.ones(B, Nq, dtype=torch.bool)          # rows whose query and whole cloud are finite
        if kind == "nan_query":
            q[1, 5, C // 2] = nan
            rows_ok[1, 5] = False
        elif kind == "nan_reference":
            x[1, 17, 0] = nan
            rows_ok[1] = False
        elif kind == "k_minus_1_finite":
            x[1, k - 1:, C - 1] = nan
            rows_ok[1] = False
        else:
            x[1, 17, 0] = 1e30                                 # finite, but its squared difference overflows: d = +inf in fp32
        got, dist = p2.knn_point(k, x.to(dev), q.to(dev), return_dist=True)
        got, dist = got.cpu(), dist.cpu().numpy()
        assert int(got.min()) >= 0 and int(got.max()) < Nr, (kind, int(got.min()), int(got.max()))
        want = sa.knn_group(k, x, q)
        assert torch.equal(got[rows_ok], want[rows_ok]), kind
        xn, qn = x.numpy(), q.numpy()
        with np.errstate(all="ignore"):
            d = ((qn[:, :, None, :] - xn[:, None, :, :]) ** 2).sum(-1)          # the kernel's form: the difference first
        assert d.dtype == np.float32
        d = np.where(np.isfinite(d), d, np.float32(np.inf))
        order = np.argsort(d, axis=-1, kind="stable")[:, :, :k]
        assert np.array_equal(got.numpy(), order), kind
        assert np.array_equal(dist, np.take_along_axis(d, order, -1)), kind
        if kind == "nan_query":
            assert got[1, 5].tolist() == list(range(k))
        if kind == "k_minus_1_finite":
            assert sorted(got[1, 0, :k - 1].tolist()) == list(range(k - 1)) and int(got[1, 0, k - 1]) == k - 1
