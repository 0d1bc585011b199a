"""The contract of mlsp_operand_bounds_next (include/mlsp_hip.h), driven through mlsp_gemm_f32 and _lib.Bound directly: the table is
handed to ONE following entry point that takes a `precision` -- a shape query or a rejected call included --, a valid entry is used as it
is, an unmeasured one is measured into and marked.  Every call is precision 3 (f16x3) on a workspace of _lib.workspace(dev, M, K, N).

SMALL (128 x 128 x 256) is the shape the contract was first written down for; with the split-K slab that this workspace always holds, the
launch splits its 8 K-tiles four ways, two tiles per workgroup, and stays on the f32 kernel (gemm.hip gemm_pick_split / gemm_split_pays):
no bound is read there.  BIG (2048 x 1024 x 1024) keeps 8 K-tiles per workgroup and runs on the two-piece f16 products; measuring its
operands pays under launch_gemm's own rule (0.33 * 2MNK / 150e6 = 9.4 us against 3 + 4 (MK + KN) / 3e6 = 7.2 us)."""
import pytest
import torch

from mlsp_amd import _lib

pytestmark = pytest.mark.gpu

SMALL = (128, 128, 256)         # M, N, K
BIG = (2048, 1024, 1024)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def disarm():
    yield
    _lib.load().mlsp_operand_bounds_next(None, 0)         # whatever a failing case left armed points at this test's memory


def gemm(A, B, tab=None, precision=3):
    """C = A B through mlsp_gemm_f32, `tab` armed for it -> (return code, C)"""
    lib = _lib.load()
    (M, K), N = A.shape, B.shape[1]
    C = torch.zeros(M, N, device=A.device)
    ws, wsn = _lib.workspace(A.device, M, K, N)
    if tab is not None:
        assert lib.mlsp_operand_bounds_next(tab, len(tab)) == 0
    rc = lib.mlsp_gemm_f32(0, 0, M, N, K, A.data_ptr(), K, B.data_ptr(), N, C.data_ptr(), N, None, precision, ws, wsn, _lib.stream())
    torch.cuda.synchronize()
    return rc, C


def table(A, B, bufs, valid, n):
    tab = (_lib.Bound * 2)()
    for e, X, buf in zip(tab, (A, B), bufs):
        e.ptr, e.rows, e.cols, e.ld, e.partials, e.valid, e.n = X.data_ptr(), X.shape[0], X.shape[1], X.stride(0), buf.data_ptr(), valid, n
    return tab


def rel_l2(C, want):
    return ((C.double() - want).norm() / want.norm()).item()


@pytest.fixture(scope="module")
def cases(dev):
    """per shape: the operands, the unoffered result and the float64 product (computed once, never written again)"""
    out = {}
    for shape in (SMALL, BIG):
        M, N, K = shape
        g = torch.Generator(device="cpu").manual_seed(M + K)
        A, B = torch.randn(M, K, generator=g).to(dev), torch.randn(K, N, generator=g).to(dev)
        rc, C0 = gemm(A, B)
        assert rc == 0
        out[shape] = (A, B, C0, A.double() @ B.double())
    return out


def inflated(A, B):
    """valid bounds that overstate both operands by 2^30: scaled by them, the operands fall into the f16 subnormals"""
    return [torch.full((256,), float(X.abs().max()) * 2.0 ** 30, device=X.device) for X in (A, B)]


def check_valid_entry_is_used(cases, shape, bar):
    A, B, C0, want = cases[shape]
    bufs = inflated(A, B)
    keep = [b.clone() for b in bufs]
    tab = table(A, B, bufs, 1, 256)
    rc, C1 = gemm(A, B, tab)
    d0, d1 = rel_l2(C0, want), rel_l2(C1, want)
    print("%s: relative L2 to float64: unoffered %.3e, with bounds 2^30 too large %.3e, ratio %.3g" % (shape, d0, d1, d1 / d0))
    assert rc == 0 and all(e.valid == 1 and e.n == 256 for e in tab) and all(torch.equal(b, k) for b, k in zip(bufs, keep))
    assert d1 >= bar * d0, (d0, d1)
    return tab


def test_a_valid_entry_is_used_as_it_is(cases):
    """Case a as first written down, at SMALL.  Measured on an MI355X, the same figures on the parent of the CallCtx refactor and after
    it: relative L2 to float64 1.512e-07 unoffered, 1.512e-07 with the inflated bounds, ratio 1 -- this launch never reads a bound (module
    docstring).  The ratio being nowhere near 100, the 2^30 construction stays and the bar is a tenth of the measured ratio, 0.1, as the
    case's own rule for that outcome says: at this shape it only pins that offering a table does no harm.  The factor 100 is held where
    the bounds are read, by test_a_valid_entry_is_used_on_the_split_path."""
    check_valid_entry_is_used(cases, SMALL, 0.1)


def test_a_valid_entry_is_used_on_the_split_path(cases):
    """The same at BIG, on the two-piece f16 products: about 8 significant bits remain of about 22.  Measured on an MI355X, the same figures
    on the parent of the CallCtx refactor and after it: relative L2 to float64 1.948e-07 unoffered, 6.373e-03 with the inflated bounds,
    ratio 3.27e+04 -- comfortably above the bar, the factor 100 of case a."""
    check_valid_entry_is_used(cases, BIG, 100.0)


@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_b_the_table_is_for_one_call_only(cases, shape):
    A, B, C0, _ = cases[shape]
    rc, _ = gemm(A, B, table(A, B, inflated(A, B), 1, 256))
    assert rc == 0
    rc, C2 = gemm(A, B)                                   # not re-armed
    assert rc == 0 and torch.equal(C2, C0)


def test_c_an_unmeasured_entry_is_measured_into(cases):
    A, B, C0, _ = cases[BIG]
    bufs = [torch.full((256,), -1.0, device=A.device) for _ in range(2)]
    tab = table(A, B, bufs, 0, 0)
    rc, C1 = gemm(A, B, tab)
    assert rc == 0 and [(e.valid, e.n) for e in tab] == [(1, 256), (1, 256)]
    for X, buf in zip((A, B), bufs):
        assert buf.min().item() >= 0.0 and buf.max().item() == X.abs().max().item()
    assert torch.equal(C1, C0)                            # (the same maxima, wherever they were measured into)
    rc, C2 = gemm(A, B, tab)                              # the same table, now valid
    assert rc == 0 and torch.equal(C2, C1) and [(e.valid, e.n) for e in tab] == [(1, 256), (1, 256)]


def unarmed_call_leaves(cases, tab, bufs):
    A, B, C0, _ = cases[BIG]
    rc, C1 = gemm(A, B)
    assert rc == 0 and torch.equal(C1, C0)
    assert [(e.valid, e.n) for e in tab] == [(0, 0), (0, 0)] and all((b == -1.0).all().item() for b in bufs)


def test_d_a_shape_query_consumes_the_table(cases):
    A, B, _, _ = cases[BIG]
    lib = _lib.load()
    bufs = [torch.full((256,), -1.0, device=A.device) for _ in range(2)]
    tab = table(A, B, bufs, 0, 0)
    assert lib.mlsp_operand_bounds_next(tab, len(tab)) == 0
    M, N, K = BIG
    assert lib.mlsp_pointmlp_bwd_stats_parts(M, K, N, K, K, 3) >= 0
    unarmed_call_leaves(cases, tab, bufs)


def test_e_a_rejected_call_consumes_the_table(cases):
    """(the one behaviour the CallCtx refactor changed: before it a call rejected for its `precision` left the table armed for the next one)"""
    A, B, _, _ = cases[BIG]
    bufs = [torch.full((256,), -1.0, device=A.device) for _ in range(2)]
    tab = table(A, B, bufs, 0, 0)
    rc, _ = gemm(A, B, tab, precision=7)
    assert rc == -1
    unarmed_call_leaves(cases, tab, bufs)
