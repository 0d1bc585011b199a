"""Fh.pointmlp_colmax (csrc/colmax.hip, mlsp_pointmlp_colmax_fwd_f32 / _bwd_f32, the sel_gamma block of gemm_epilogue) against its float64
restatement (tests/colmax_restatement.py) on every launch path.  The GPU run records its own selection (Fh.recorded_selections) and the
float64 run is given that selection, so every element of every quantity is compared and nothing is excluded; the selection itself is
checked against float64's Y (check_selection).  Every case states its path through mlsp_pointmlp_colmax_panel_rows.

Distance: max|a - b| / max|b| against float64.  Yardstick: the distance of the same restatement run in torch fp32 on the CPU with the same
selection forced.  Bar: max(floor, 3 x yardstick) per quantity -- 3 because the summation order differs.  Floor: 2e-6 (the GEMM family's
bar, test_gemm_split_bf16_accuracy) times the number of chained contractions that feed the quantity:

    quantity                    training                      eval
    out, running statistics     1 (Y)                         1
    dgamma, dbeta               1 (Y)                         1
    dW                          3 (Y, G = X^T X, W G)         1 (Y: the rows gathered by its selection)
    dX                          3 (Y, Mneg, X Mneg)           1
(test_grad_accum: a second consumer's dgrad is added into the same dX buffer -- a parallel addend, not a further link of the chain: the
same floors)
"""
import contextlib
import ctypes
import sys

import pytest
import torch
import torch.nn.functional as F

import colmax_restatement as cr

pytestmark = pytest.mark.gpu

from colmax_restatement import (FIVE_POINTS, FUSED_1x128, FUSED_2x64, FUSED_3x64, FUSED_FAST, FUSED_MULTI128, LDS_BIG, MANY_CLOUDS,
                                ONE_POINT, OUTLIER, UNFUSED_RAGGED, UNFUSED_SPLITK, panel_rows)

FLOOR = 2e-6
MODES = list(cr.MODES)
SPLIT_MODES = ["default", "bf16x6"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mode(mode):
    from mlsp_amd import functional as Fh
    return contextlib.nullcontext() if mode == "default" else Fh.gemm_precision(mode)


def make_inputs(shape, seed, family="randn", gamma=None):
    """family: "randn"; "dyadic" / "dup" (cr.dyadic_inputs); "lrelu" (X = leaky_relu(randn, 0.2): what the layer really receives, mean / std
    about 0.5) and "shift3" (X = randn + 3), both with a W whose rows do not sum to zero; "outlier" (one row of 50x the norm per cloud).
    gamma: both signs (rand * 2 - 0.6: ~30 % of the channels take the min branch) unless given."""
    B, N, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    P = B * N
    if family in ("dyadic", "dup"):
        X, W = cr.dyadic_inputs(B, N, Cin, Cout, seed, dup=family == "dup")
    else:
        X = torch.randn(P, Cin, generator=g)
        W = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
        if family == "lrelu":
            X = F.leaky_relu(X, 0.2)
        elif family == "shift3":
            X = X + 3
        elif family == "outlier":
            X.view(B, N, Cin)[torch.arange(B), torch.randint(0, N, (B,), generator=g)] *= 50
        if family in ("lrelu", "shift3"):
            W = W + torch.randn(Cout, 1, generator=g) / Cin ** 0.5            # row sums of order sqrt(Cin), either sign
    if gamma is None:
        gamma = torch.rand(Cout, generator=g) * 2 - 0.6
    beta = torch.randn(Cout, generator=g)
    rm, rv = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    dOut = torch.randn(B, Cout, generator=g)
    return dict(X=X, W=W, gamma=gamma, beta=beta, rm=rm, rv=rv, dOut=dOut)


def gpu_run(dev, inp, shape, training, mode, act=cr.ACT_LRELU, eps=1e-5, wslice=False, backward=True):
    """One forward (+ backward) of Fh.pointmlp_colmax.  wslice: W is a column slice of a wider weight (ldw > Cin).
    -> dict of cr.NAMES (CPU tensors) + sel (the recorded arg) + kinds (mlsp_profile_split_kinds of the call) + leaves / out (for a
    later backward)."""
    from mlsp_amd import _lib, functional as Fh
    lib = _lib.load()
    B, N, Cin, Cout = shape
    Xg = inp["X"].to(dev).requires_grad_(True)
    if wslice:
        Wleaf = torch.full((Cout, Cin + 8), 3.0)
        Wleaf[:, 4:4 + Cin] = inp["W"]
        Wleaf = Wleaf.to(dev).requires_grad_(True)
        Wg = Wleaf[:, 4:4 + Cin]
    else:
        Wleaf = Wg = inp["W"].to(dev).requires_grad_(True)
    gg, bg = inp["gamma"].to(dev).requires_grad_(True), inp["beta"].to(dev).requires_grad_(True)
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    buf, kinds = (ctypes.c_double * 4)(), (ctypes.c_double * 16)()
    with _mode(mode), Fh.recorded_selections() as rec:
        lib.mlsp_profile_begin()
        try:
            out = Fh.pointmlp_colmax(Xg, Wg, gg, bg, rm, rv, B, N, training=training, act=act, slope=0.2, eps=eps)
            if backward:
                out.backward(inp["dOut"].to(dev))
            torch.cuda.synchronize()
        finally:
            lib.mlsp_profile_end(buf)                      # (a case that raises must not leave the hook armed for the next one)
        lib.mlsp_profile_split_kinds(kinds)
    res = dict(out=out.detach().cpu(), run_mean=rm.cpu(), run_var=rv.cpu(), sel=rec.sel[0].cpu(), kinds=list(kinds),
               leaves=(Xg, Wleaf, gg, bg), out_gpu=out)
    if backward:
        dW = Wleaf.grad
        if wslice:
            assert not dW[:, :4].any() and not dW[:, 4 + Cin:].any()
            dW = dW[:, 4:4 + Cin]
        res.update(dX=Xg.grad.cpu(), dW=dW.cpu(), dgamma=gg.grad.cpu(), dbeta=bg.grad.cpu())
    return res


def check_selection(tag, inp, shape, sel, Y64):
    """every arg in [0, N); the selected value within 2 * delta of float64's column extreme, delta = 2e-6 * max|Y64| (one contraction on
    either side of the comparison); among the rows of the cloud that are bit-identical to the selected one, the smallest index"""
    B, N, Cin, Cout = shape
    sel = sel.long()
    assert sel.shape == (B, Cout) and int(sel.min()) >= 0 and int(sel.max()) < N, (tag, int(sel.min()), int(sel.max()))
    delta = 2e-6 * Y64.abs().max()
    s = torch.where(inp["gamma"] >= 0, 1.0, -1.0).double()
    ys = (Y64 * s).gather(1, sel.view(B, 1, Cout)).view(B, Cout)
    short = ((Y64 * s).max(dim=1)[0] - ys).max().item()
    assert short <= 2 * delta, (tag, short, delta.item())
    Xb = inp["X"].view(B, N, Cin)
    for b in range(B):
        _, inv = torch.unique(Xb[b], dim=0, return_inverse=True)
        first = torch.full((int(inv.max()) + 1,), N, dtype=torch.long).scatter_reduce(0, inv, torch.arange(N), "amin")
        assert torch.equal(first[inv][sel[b]], sel[b]), (tag, b)


def floors(training):
    f = {n: 1 for n in cr.NAMES}
    f["dW"] = f["dX"] = 3 if training else 1
    return f


def measure(tag, got, want, yard, training):
    """prints one line per quantity -- distance, yardstick, bar -- and one with the kink count; -> {quantity: (distance, yardstick, bar)}"""
    rows = {}
    print()
    for n, k in floors(training).items():
        assert torch.isfinite(got[n]).all(), (tag, n)
        assert got[n].shape == want[n].shape, (tag, n)
        d, y = cr.dist(got[n], want[n]), cr.dist(yard[n], want[n])
        rows[n] = (d, y, max(k * FLOOR, 3 * y))
        print("colmax %s %-8s distance %.3e  yardstick %.3e  bar %.3e" % ((tag, n) + rows[n]))
    print("colmax %s nkink    %d of %d" % (tag, want["nkink"], want["out"].numel()))
    # |z| <= 1e-6 max|z| holds for about 2e-6 * max|z| * (the density of z at 0) of the elements, of order 1e-5: two, or a thousandth
    assert want["nkink"] <= 2 + want["out"].numel() // 1000, (tag, want["nkink"])
    return rows


def check(tag, got, want, yard, training):
    """every quantity under its bar"""
    bad = [(n, d, bar) for n, (d, _, bar) in measure(tag, got, want, yard, training).items() if not d <= bar]
    assert not bad, (tag, bad)


def references(inp, shape, training, got, act=cr.ACT_LRELU, eps=1e-5):
    B, N = shape[:2]
    a = (inp["X"], inp["W"], inp["gamma"], inp["beta"], inp["rm"], inp["rv"], B, N, training, inp["dOut"])
    want = cr.colmax_f64(*a, act=act, eps=eps, sel=got["sel"], out_gpu=got["out"])
    yard = cr.colmax_f64(*a, act=act, eps=eps, sel=got["sel"], out_gpu=got["out"], dtype=torch.float32)
    return want, yard


def assert_path(tag, shape, mode, rows=None):
    """the shape query says `rows` (None: what cr.PATHS lists for the shape and mode), and N // rows panels per cloud -> (rows, panels)"""
    want_rows, want_panels = cr.PATHS[shape][MODES.index(mode)]
    assert rows is None or rows == want_rows
    q = panel_rows(shape, mode)
    assert q == want_rows and (shape[1] // q if q else 0) == want_panels and q * want_panels == (shape[1] if q else 0), (tag, q, want_rows)
    return q, want_panels


def against_float64(dev, tag, shape, mode, rows=None, training=True, family="randn", act=cr.ACT_LRELU, eps=1e-5, gamma=None, wslice=False,
                    inp=None, seed=None, assert_bars=True):
    """rows: what the shape query must say (None: cr.PATHS).  assert_bars=False: -> also the measured {quantity: (distance, yardstick, bar)}"""
    q, panels = assert_path(tag, shape, mode, rows)
    inp = inp or make_inputs(shape, sum(shape) if seed is None else seed, family, gamma)
    got = gpu_run(dev, inp, shape, training, mode, act=act, eps=eps, wslice=wslice)
    want, yard = references(inp, shape, training, got, act, eps)
    tag = "%s %s %s[%s] rows %d x %d" % (tag, "x".join(map(str, shape)), "train" if training else "eval", mode, q, panels)
    check_selection(tag, inp, shape, got["sel"], want["Y"])
    if not assert_bars:
        return inp, got, want, measure(tag, got, want, yard, training)
    check(tag, got, want, yard, training)
    return inp, got, want


def assert_split_forward(got, mode):
    """the forward GEMM (the bracket's only A B^T launch) ran on the split kernel"""
    if mode != "fp32":
        assert int(got["kinds"][1]) == 1, got["kinds"]
    else:
        assert not any(got["kinds"]), got["kinds"]


# ----------------------------------------------------------------------------- the launch paths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(UNFUSED_SPLITK, 0), (UNFUSED_RAGGED, 0), (FUSED_2x64, 64), (FUSED_3x64, 64), (FUSED_1x128, 128),
                                        (FUSED_FAST, None), (FUSED_MULTI128, None)])
def test_paths_training(dev, shape, rows, mode):
    _, got, _ = against_float64(dev, "path", shape, mode, rows)
    if shape in (FUSED_FAST, FUSED_MULTI128):
        assert_split_forward(got, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(FUSED_2x64, 64), (UNFUSED_RAGGED, 0), (FUSED_FAST, None)])
def test_paths_eval(dev, shape, rows, mode):
    """eval mode: the running statistics, untouched; on the fused shapes stat_part is null while sel_* is live"""
    inp, got, _ = against_float64(dev, "eval", shape, mode, rows, training=False)
    assert torch.equal(got["run_mean"], inp["rm"]) and torch.equal(got["run_var"], inp["rv"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(FUSED_2x64, 64), (UNFUSED_RAGGED, 0)])
@pytest.mark.parametrize("act", [cr.ACT_NONE, cr.ACT_LRELU])
def test_seg_identity_bn(dev, act, shape, rows, mode):
    """what the seg models call: eval, eps = 0, gamma = ones, beta = the conv bias, run_mean = 0, run_var = 1 (a conv + bias [+ LeakyReLU]
    + max).  Every column takes the max branch."""
    Cout = shape[3]
    inp = make_inputs(shape, 11, gamma=torch.ones(Cout))
    inp["rm"], inp["rv"] = torch.zeros(Cout), torch.ones(Cout)
    against_float64(dev, "seg act%d" % act, shape, mode, rows, training=False, act=act, eps=0.0, inp=inp)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(FUSED_2x64, 64), (UNFUSED_RAGGED, 0)])
def test_relu_training(dev, shape, rows, mode):
    """act = ReLU; a gradient that arrives at dead outputs only leaves every gradient exactly zero"""
    inp, got, _ = against_float64(dev, "relu", shape, mode, rows, act=cr.ACT_RELU)
    dead = got["out"] == 0
    assert 0 < int(dead.sum()) < dead.numel()
    inp2 = dict(inp, dOut=inp["dOut"] * dead)
    got2 = gpu_run(dev, inp2, shape, True, mode, act=cr.ACT_RELU)
    for n in ("dX", "dW", "dgamma", "dbeta"):
        assert not got2[n].any(), n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_gamma_zero_columns(dev, zero, mode):
    """gamma == 0 resp. -0.0 in a few columns (both take the max branch: gamma >= 0); out is act(beta) there and no gradient reaches W"""
    shape = FUSED_2x64
    inp = make_inputs(shape, 13)
    inp["gamma"][[0, 5, 33, 95]] = zero
    _, got, _ = against_float64(dev, "gamma %s" % zero, shape, mode, 64, inp=inp)
    assert not got["dW"][[0, 5, 33, 95]].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(FUSED_2x64, 64), (UNFUSED_RAGGED, 0)])
def test_weight_column_slice(dev, shape, rows, mode):
    """W a column slice of a wider weight (ldw = Cin + 8); the other columns of its gradient stay zero (gpu_run)"""
    against_float64(dev, "ldw", shape, mode, rows, wslice=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [MANY_CLOUDS, ONE_POINT, FIVE_POINTS])
def test_many_clouds_and_tiny_clouds(dev, shape, mode):
    """B = 70: the b += 64 loop of colmax_bwd_coef_kernel.  N = 1, N = 5: rows_per_part = 1 and scatter workgroups past N."""
    against_float64(dev, "tiny", shape, mode, 0)


@pytest.mark.parametrize("mode", MODES)
def test_outlier_point_long_lists(dev, mode):
    """one point of 50x the norm per cloud: the channels on whose side of zero its product falls select it -- about half of the 512 --,
    so the scatter's cooperative long-list branch runs with a list far longer than its 16 waves"""
    shape = OUTLIER
    _, got, _ = against_float64(dev, "outlier", shape, mode, 64, family="outlier")
    for b in range(shape[0]):
        assert int(torch.bincount(got["sel"][b].long(), minlength=shape[1]).max()) > 128


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_scatter_lds_above_64k(dev, mode):
    """N = 8192: the scatter's dynamic LDS is (2 * 8192 + 1 + 3 * 32 + 4096) * 4 = 82 KB: the mlsp_lds_limit branch"""
    against_float64(dev, "lds", LDS_BIG, mode, 64)


# ----------------------------------------------------------------------------- exact inputs: the first-occurrence rule
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", ["dyadic", "dup"])
@pytest.mark.parametrize("shape,rows", [(FUSED_2x64, 64), (FUSED_3x64, 64), (FUSED_MULTI128, None), (UNFUSED_RAGGED, 0)])
def test_dyadic_selection_is_float64s(dev, shape, rows, family, mode):
    """fp32, the split modes and float64 see the same Y (cr.dyadic_inputs asserts the premise), so the recorded arg must EQUAL float64's
    first extreme: across the half-waves, the two wm halves of a tile, and the panels of a cloud.  (FUSED_MULTI128 has Cin = 128: every
    partial sum is a multiple of 1/128 below 128 * 225 / 128, still exact in fp32.)"""
    inp, got, want = against_float64(dev, family, shape, mode, rows, family=family)
    first = cr.first_extreme(want["Y"], inp["gamma"])
    assert torch.equal(got["sel"].long(), first), int((got["sel"].long() != first).sum())
    tied = ((want["Y"] == want["Y"].gather(1, first.view(shape[0], 1, -1))).sum(dim=1) > 1).float().mean().item()
    assert tied > (0.9 if family == "dup" else 0.1), tied


# ----------------------------------------------------------------------------- off-centre inputs: where the Gram form cancels
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,rows", [(FUSED_FAST, None), (FUSED_MULTI128, None), (UNFUSED_SPLITK, 0)])
def test_off_centre_lrelu(dev, shape, rows, mode):
    """X = leaky_relu(randn, 0.2), W with non-zero row sums: W G - mean (x) sum_x is a difference of two large terms"""
    against_float64(dev, "lrelu-X", shape, mode, rows, family="lrelu")


_shift3_runs = {}


def shift3_case(dev, shape, mode):
    """one run per (shape, mode), shared by the three tests below: the path and the selection asserted, every quantity measured
    -> {quantity: (distance, yardstick, bar)}"""
    if (shape, mode) not in _shift3_runs:
        _shift3_runs[shape, mode] = against_float64(dev, "randn+3", shape, mode, family="shift3", assert_bars=False)[3]
    return _shift3_runs[shape, mode]


# X = randn + 3: the (quantity, shape, mode) triples measured over their bars on MI355X (profiles/colmax_float64_distances.txt),
# "distance against bar".  Everything not listed holds and is asserted.
SHIFT3_GRAM = {            # W G and mean (x) sum_x (X Mneg and r) are far larger than their difference, each rounded to fp32
    ("dW", FUSED_FAST, "default"): "3.900e-5 against 2.891e-5", ("dW", FUSED_FAST, "fp32"): "3.764e-5 against 2.891e-5",
    ("dW", FUSED_FAST, "bf16x6"): "3.900e-5 against 2.891e-5",
    ("dW", FUSED_MULTI128, "default"): "3.290e-5 against 2.736e-5", ("dW", FUSED_MULTI128, "fp32"): "3.487e-5 against 2.736e-5",
    ("dW", FUSED_MULTI128, "bf16x6"): "3.267e-5 against 2.736e-5",
    ("dW", UNFUSED_SPLITK, "default"): "2.248e-5 against 1.265e-5", ("dW", UNFUSED_SPLITK, "fp32"): "2.248e-5 against 1.265e-5",
    ("dW", UNFUSED_SPLITK, "bf16x6"): "2.248e-5 against 1.265e-5",
    ("dX", FUSED_FAST, "default"): "7.755e-6 against 6e-6", ("dX", FUSED_FAST, "fp32"): "6.871e-6 against 6e-6",
    ("dX", FUSED_FAST, "bf16x6"): "7.755e-6 against 6e-6"}
SHIFT3_STATS = {           # the GEMM epilogue's fused statistics add y and y^2 of a panel in fp32 before the fp64 partials
    ("run_var", FUSED_FAST, "default"): "1.738e-5 against 2e-6", ("run_var", FUSED_FAST, "fp32"): "2.049e-5 against 2e-6",
    ("run_var", FUSED_FAST, "bf16x6"): "1.738e-5 against 2e-6",
    ("run_var", FUSED_MULTI128, "default"): "8.921e-6 against 2e-6", ("run_var", FUSED_MULTI128, "fp32"): "4.238e-6 against 2e-6",
    ("run_var", FUSED_MULTI128, "bf16x6"): "8.167e-6 against 2e-6",
    ("dgamma", FUSED_FAST, "default"): "9.176e-6 against 5.538e-6", ("dgamma", FUSED_FAST, "fp32"): "1.543e-5 against 5.538e-6",
    ("dgamma", FUSED_FAST, "bf16x6"): "9.176e-6 against 5.538e-6",
    ("dgamma", FUSED_MULTI128, "default"): "8.742e-6 against 4.608e-6", ("dgamma", FUSED_MULTI128, "bf16x6"): "8.041e-6 against 4.608e-6",
    ("out", FUSED_FAST, "default"): "1.582e-5 against 9.637e-6", ("out", FUSED_FAST, "fp32"): "1.413e-5 against 9.637e-6",
    ("out", FUSED_FAST, "bf16x6"): "1.582e-5 against 9.637e-6",
    ("out", FUSED_MULTI128, "default"): "1.520e-5 against 1.058e-5", ("out", FUSED_MULTI128, "bf16x6"): "1.233e-5 against 1.058e-5"}
SHIFT3_SHAPES = (FUSED_FAST, FUSED_MULTI128, UNFUSED_SPLITK)


def _shift3_params(quantities, over, cause):
    return [pytest.param(q, shape, mode, marks=pytest.mark.xfail(strict=True, reason="%s: %s" % (cause, over[q, shape, mode]))
                         if (q, shape, mode) in over else ())
            for q in quantities for shape in SHIFT3_SHAPES for mode in MODES]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHIFT3_SHAPES)
def test_off_centre_shift3(dev, shape, mode):
    """X = randn + 3 (mean / std = 3), the same W: columns of Y with |mean| up to 10 standard deviations.  The path, the selection and
    the quantities that neither the Gram form nor the batch variance enters: dbeta, run_mean."""
    rows = shift3_case(dev, shape, mode)
    for q in ("dbeta", "run_mean"):
        assert rows[q][0] <= rows[q][2], (q, rows[q])


@pytest.mark.parametrize("quantity,shape,mode", _shift3_params(("dW", "dX"), SHIFT3_GRAM, "Gram form cancels in fp32"))
def test_off_centre_shift3_gram_terms(dev, quantity, shape, mode):
    """dW = S - A (x) sum_x - diag(Bc) (W G - mean (x) sum_x) and dX = X Mneg - 1 (x) r + ...: on this input both differences are far smaller
    than their terms, and each term is rounded to fp32 (stock fp32 autograd is itself 4e-6 ... 1e-5 from float64 on dW here).  dW is over
    its bar on every shape, dX at Cin 256; dX holds on the other two shapes.  The cure is to form the Gram terms on X - xbar
    (Y - mean = (X - xbar) W^T); it changes launches of the timed step and is not made here."""
    d, _, bar = shift3_case(dev, shape, mode)[quantity]
    assert d <= bar, (quantity, d, bar)


@pytest.mark.parametrize("quantity,shape,mode", _shift3_params(("run_var", "dgamma", "out"), SHIFT3_STATS, "fused BatchNorm statistics in fp32"))
def test_off_centre_shift3_batch_statistics(dev, quantity, shape, mode):
    """A defect of its own, in the epilogue every pointmlp layer shares: the fused statistics add y and y^2 of a row panel in fp32 before
    the fp64 partials, so the variance of a column ten standard deviations off zero loses digits; dgamma and out follow through invstd.  The
    shape whose K is split takes colstats instead and holds (run_var 2.2e-7, dgamma 1.7e-6, out 1.4e-6), as do dgamma and out on
    32x256x128x1024 in fp32 (4.376e-6 against 4.608e-6, 5.647e-6 against 1.058e-5).  The cure is a shifted sum of squares in the epilogue: a change to the timed step, not made here."""
    d, _, bar = shift3_case(dev, shape, mode)[quantity]
    assert d <= bar, (quantity, d, bar)


# ----------------------------------------------------------------------------- a shared input gradient
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("colmax_last", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_grad_accum(dev, training, colmax_last, mode, monkeypatch):
    """Fh.fan_out(X, 2) into a pointmlp and a pointmlp_colmax: dX is the float64 sum of both consumers' input gradients.  colmax_last:
    its backward runs second and ADDS (dx_accumulate = 1; in eval mode the memset is skipped); otherwise it writes and the pointmlp adds.
    autograd runs the node created last first; who claimed the shared buffer, in which order and with which flag, is asserted."""
    from mlsp_amd import functional as Fh
    claims, claim = [], Fh.SharedInputGrad.claim

    def recording_claim(self, shape_, device):
        buf, accumulate = claim(self, shape_, device)
        claims.append(("ColMax" in type(sys._getframe(1).f_locals["ctx"]).__name__, accumulate))      # (the caller: a Function's backward)
        return buf, accumulate
    monkeypatch.setattr(Fh.SharedInputGrad, "claim", recording_claim)
    shape = FUSED_2x64
    B, N, Cin, Cout = shape
    assert_path("accum", shape, mode, 64)
    inp = make_inputs(shape, 17)
    g = torch.Generator().manual_seed(18)
    W2, R2 = torch.randn(48, Cin, generator=g) / Cin ** 0.5, torch.randn(B * N, 48, generator=g) * 0.05
    Xg, Wg, gg, bg, W2g = [t.to(dev).requires_grad_(True) for t in (inp["X"], inp["W"], inp["gamma"], inp["beta"], W2)]
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    with _mode(mode), Fh.recorded_selections() as rec:
        (a0, a1), acc = Fh.fan_out(Xg, 2)
        if not colmax_last:
            o1 = Fh.pointmlp(a0, W2g, training=training, grad_accum=acc)
        o2 = Fh.pointmlp_colmax(a1, Wg, gg, bg, rm, rv, B, N, training=training, grad_accum=acc)
        if colmax_last:
            o1 = Fh.pointmlp(a0, W2g, training=training, grad_accum=acc)
        ((o1 * R2.to(dev)).sum() + (o2 * inp["dOut"].to(dev)).sum()).backward()
    assert claims == [(not colmax_last, 0), (colmax_last, 1)], claims
    got = dict(out=o2.detach().cpu(), dX=Xg.grad.cpu(), dW=Wg.grad.cpu(), dgamma=gg.grad.cpu(), dbeta=bg.grad.cpu(), run_mean=rm.cpu(),
               run_var=rv.cpu(), sel=rec.sel[0].cpu())
    want, yard = references(inp, shape, training, got)
    want["dX"] = want["dX"] + R2.double() @ W2.double()
    yard["dX"] = yard["dX"] + R2 @ W2
    tag = "accum %s %s[%s]" % ("adds" if colmax_last else "writes", "train" if training else "eval", mode)
    check_selection(tag, inp, shape, got["sel"], want["Y"])
    check(tag, got, want, yard, training)


# ----------------------------------------------------------------------------- NaN: arg stays in range
@pytest.mark.parametrize("shape,rows,mode", [(FUSED_2x64, 64, "fp32"), (UNFUSED_RAGGED, 0, "fp32"), (FUSED_MULTI128, 128, "bf16x6")])
@pytest.mark.parametrize("whole_cloud", [True, False])
def test_nan_rows_are_defined_and_in_range(dev, whole_cloud, shape, rows, mode):
    """A cloud of NaN (whole_cloud) or one NaN row in a cloud, eval mode (the statistics do not spread it).  A column of NaN takes no row
    in any panel: arg is 0 there, never the no-row sentinel.  The forward never dereferences arg, so it runs first and alone; the
    backward -- which indexes X and LDS by arg -- runs only after arg is known to be in range.  Both fused cases: the f32-MFMA kernel
    (K = 64 stays on it in every mode) and the split kernel on three bf16 pieces, whose NaN operand rows stay inside their own rows of Y
    (the two-piece f16 mode scales by a bound of the whole operand, which a NaN takes with it: not a case of this contract)."""
    B, N, Cin, Cout = shape
    assert_path("nan", shape, mode, rows)
    inp = make_inputs(shape, 19)
    if whole_cloud:
        inp["X"].view(B, N, Cin)[1] = float("nan")
    else:
        inp["X"].view(B, N, Cin)[1, 7] = float("nan")
    got = gpu_run(dev, inp, shape, False, mode, backward=False)
    sel = got["sel"].long()
    assert int(sel.min()) >= 0 and int(sel.max()) < N, (int(sel.min()), int(sel.max()))
    if mode != "fp32":
        assert_split_forward(got, mode)
    bad = ~torch.isfinite(got["out"])
    want_bad = torch.zeros(B, Cout, dtype=torch.bool)
    want_bad[1] = whole_cloud
    assert torch.equal(bad, want_bad)
    if whole_cloud:
        assert not sel[1].any()
    else:
        assert not (sel[1] == 7).any()                        # a NaN is never the extreme
    got["out_gpu"].backward(inp["dOut"].to(dev))
    torch.cuda.synchronize()
    dX = got["leaves"][0].grad.cpu().view(B, N, Cin)
    others = [b for b in range(B) if b != 1]
    assert torch.isfinite(dX[others]).all()


# ----------------------------------------------------------------------------- run to run
@pytest.mark.parametrize("mode", SPLIT_MODES)
def test_bit_reproducible(dev, mode):
    inp = make_inputs(FUSED_FAST, 23, "lrelu")
    a, b = (gpu_run(dev, inp, FUSED_FAST, True, mode) for _ in range(2))
    for n in cr.NAMES + ("sel",):
        assert torch.equal(a[n], b[n]), n
