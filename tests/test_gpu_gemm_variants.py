"""Every launch of tests/gemm_shapes.py on the GPU, in the row's product mode, bracketed by the measurement hook:

  a. the launch that ran is the one the row pins (mlsp_profile_launches: family, tile height, splits, grid, bf16 or f16 pieces, the slab
     reducer; a row that thin.hip or skinny.hip takes records no tile-kernel launch);
  b. the result is EXACT on integer operands -- the addressing test.  Operands and bias are integers in [-8, 8] held as fp32: one bf16
     piece, one f16 piece, every product and partial sum an integer below 2^24 (64 K <= 2^24 for K <= 262144; [-4, 4] beyond), so all four
     modes return exactly the float64 product whatever the summation order or power-of-two scale.  Pitches of dim + 1 and dim + 4, operands
     and a bias 4 bytes off a 16-byte boundary, a pitched C: every float of the buffers outside the operands is NaN, and `out` is NaN before
     the call -- the launch must overwrite all of C (the slab sum of a split-K launch too) and nothing beside it.  A second tier holds one
     operand up to 2^12 (two pieces in both piece modes; the dropped lo * lo term is zero) where every sum of |a b| stays below 2^24;
  c. rounding on wide-range operands: test_gemm_split_bf16_accuracy's criterion, unchanged, on the newly pinned split-kernel rows and on
     the bf16-kernel rows (there against the float64 product of the bf16-rounded operands);
  d. every split-K and folded launch run twice on unit-normal operands, where the summation order shows in the bits, is bit-identical
     (on the integer operands a repeat proves only that no stale slab is read: every order gives the same integers)."""
import ctypes
import functools

import pytest
import torch

import gemm_shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mlsp_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fh():
    from mlsp_amd import functional as Fh
    return Fh


def _rid(r):
    return "%s-%d%d-%dx%dx%d-p%d.%d.%d-o%d%d-b%d" % ((r.mode, r.ta, r.tb, r.M, r.N, r.K) + tuple(r.pad) + tuple(r.off) + (r.bias,))


ROWS = list(dict.fromkeys(r for _, r in gemm_shapes.rows()))            # (a launch two tests make is launched once here)
COLS = 14                                                                # MLSP_PROF_LAUNCH_COLS


def _recorded(fn):
    """fn() under the measurement hook -> (its value, the rows of mlsp_profile_launches)"""
    lib = _fh()._lib.load()
    table = (ctypes.c_int32 * (COLS * 8))()
    assert lib.mlsp_profile_begin() == 0
    try:
        val = fn()
        torch.cuda.synchronize()
    finally:
        lib.mlsp_profile_end((ctypes.c_double * 4)())                   # (a case that raises must not leave the hook armed for the next one)
    n = lib.mlsp_profile_launches(table, 8)
    assert 0 <= n <= 8, n
    return val, [tuple(table[i * COLS:(i + 1) * COLS]) for i in range(n)]


def _assert_pinned(r, recs):
    if r.via in ("thin", "skinny"):
        assert recs == [], recs                                          # the offer was taken: no tile kernel
        return
    assert len(recs) == 1, recs
    M, N, K, ta, tb, ns, bm, _epi, split, _extra, fam, gx, gy, red = recs[0]
    family, lbm, lns, _xcd = gemm_shapes.parse(r.label)
    assert (M, N, K, ta, tb) == (r.M, r.N, r.K, r.ta, r.tb), recs            # (a folded launch is listed as the 64 x 64 x K product it is)
    assert gemm_shapes.FAMILIES[fam] == ("FOLD64" if r.via == "fold" else family), recs
    assert (bm, ns, (gx, gy)) == (lbm, lns, gemm_shapes.grid(r)), recs
    assert split == (0 if family != "SPLIT" else 2 if "/pieces/" in r.label else 1), recs       # f16 pieces only where the row says so
    assert red == (gemm_shapes.REDUCERS.index(r.reduce) if r.reduce != "-" else -1), recs


def _place(dev, vals, pad, off):
    """vals [rows][cols] (CPU) as a device row view of pitch cols + pad that starts `off` floats off a 16-byte boundary, every float around
    it NaN"""
    rows, cols = vals.shape
    ld = cols + pad
    buf = torch.full((off + rows * ld + 64,), float("nan"), device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals)
    assert view.data_ptr() % 16 == 4 * off and view.stride() == (ld, 1)
    return buf, view


@functools.lru_cache(maxsize=2)
def _integers(ta, tb, M, N, K, bias, big):
    """integer operands (CPU fp32) and the float64 product rounded to fp32.  big: 0 both in [-lim, lim]; 1 / 2: A / B up to 2^12."""
    g = torch.Generator().manual_seed(1000 * big + 7 * M + 3 * N + K)
    lim = 8 if K <= 262144 else 4

    def ints(shape, hi):
        return torch.randint(-hi, hi + 1, shape, generator=g).float()
    A = ints((K, M) if ta else (M, K), 4096 if big == 1 else lim)
    B = ints((N, K) if tb else (K, N), 4096 if big == 2 else lim)
    bv = ints((N,), lim) if bias else None
    opA, opB = (A.t() if ta else A).double(), (B.t() if tb else B).double()
    bound = (opA.abs() @ opB.abs()).max().item() if big else float(K * lim * lim)
    assert bound + lim <= 2 ** 24, bound                                 # every partial sum is an integer the fp32 accumulators hold
    want = opA @ opB
    if bias:
        want = want + bv.double()
    assert torch.equal(want.float().double(), want)
    return A, B, bv, want.float()


def _launch_exact(dev, r, big=0):
    """the row's launch on integer operands -> (C's columns, C's pad columns, the recorded launches)"""
    Fh = _fh()
    A, B, bv, want = _integers(r.ta, r.tb, r.M, r.N, r.K, bool(r.bias), big)
    keepA, dA = _place(dev, A, r.pad[0], r.off[0])
    keepB, dB = _place(dev, B, r.pad[1], r.off[1])
    bias = None
    if r.bias:
        keepb, bias = _place(dev, bv.view(1, -1), 0, r.bias - 1)
        bias = bias.view(-1)
    keepC, out = _place(dev, torch.full((r.M, r.N), float("nan")), r.pad[2], 0)
    assert (dA.stride(0), dB.stride(0), out.stride(0)) == gemm_shapes.pitches(r)
    with Fh.gemm_precision(r.mode):
        got, recs = _recorded(lambda: Fh.gemm(dA, dB, bool(r.ta), bool(r.tb), bias=bias, out=out))
        assert got.data_ptr() == out.data_ptr()
        first = out.cpu()
        if r.reduce != "-" or r.via == "fold":                          # a slab is overwritten, not added to: the repeat is the same
            out.fill_(float("nan"))
            Fh.gemm(dA, dB, bool(r.ta), bool(r.tb), bias=bias, out=out)
            assert torch.equal(out.cpu(), first)
    beside = keepC[:r.M * out.stride(0)].view(r.M, -1)[:, r.N:].cpu()
    tail = keepC[r.M * out.stride(0):].cpu()
    assert torch.isnan(beside).all() and torch.isnan(tail).all()         # nothing written beside C
    return first, want, recs


@pytest.mark.parametrize("r", ROWS, ids=_rid)
def test_the_pinned_kernel_ran_and_is_exact_on_integers(dev, r):
    got, want, recs = _launch_exact(dev, r)
    _assert_pinned(r, recs)
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("big", [1, 2], ids=["A-to-4096", "B-to-4096"])
@pytest.mark.parametrize("r", gemm_shapes.PIECE_TIER, ids=_rid)
def test_two_piece_operands_are_exact_on_integers(dev, r, big):
    got, want, recs = _launch_exact(dev, r, big)
    _assert_pinned(r, recs)
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (len(bad), bad[:4].tolist())


SPLIT_K = [r for r in ROWS if r.reduce != "-" or r.via == "fold" or (r.via == "thin" and r.ta)]      # (thin.hip's A^T B kernel sums slabs too)


@pytest.mark.parametrize("r", SPLIT_K, ids=_rid)
def test_split_k_repeats_bit_for_bit(dev, r):
    """d.  Unit-normal operands in the row's pitches, offsets and bias: partial sums round, so a reducer or a K split that summed in an
    order of its own choosing (atomics, a race) would differ between two runs; the result is also held to test_gemm's bar for K."""
    Fh = _fh()
    g = torch.Generator().manual_seed(5 + r.M + r.N + r.K)
    A = torch.randn((r.K, r.M) if r.ta else (r.M, r.K), generator=g)
    B = torch.randn((r.N, r.K) if r.tb else (r.K, r.N), generator=g)
    bv = torch.randn(r.N, generator=g) if r.bias else None
    keepA, dA = _place(dev, A, r.pad[0], r.off[0])
    keepB, dB = _place(dev, B, r.pad[1], r.off[1])
    bias = _place(dev, bv.view(1, -1), 0, r.bias - 1)[1].view(-1) if r.bias else None
    runs = []
    with Fh.gemm_precision(r.mode):
        for _ in range(3):
            keepC, out = _place(dev, torch.full((r.M, r.N), float("nan")), r.pad[2], 0)
            runs.append(Fh.gemm(dA, dB, bool(r.ta), bool(r.tb), bias=bias, out=out).cpu())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    if r.mode != "bf16":
        want = (A.t() if r.ta else A).double() @ (B.t() if r.tb else B).double()
        if r.bias:
            want = want + bv.double()
        err = (runs[0].double() - want).abs().max().item()
        assert err < 2e-6 * r.K ** 0.5 * 4 + 1e-6, err


def _rounding_cases():
    new = [r for r in gemm_shapes.NEW if r.label.startswith("SPLIT/")]
    bf16 = [r for r in ROWS if r.label.startswith("BF16/") and r.via == "tile"]
    return [(r, s) for r in new for s in ((1.0, 1e-6, 3e5) if r.mode == "f16x3" else (1.0,))] + [(r, 1.0) for r in bf16]


@pytest.mark.parametrize("r,scale", _rounding_cases(), ids=lambda v: _rid(v) if isinstance(v, tuple) else "%g" % v)
def test_rounding_on_wide_range_operands(dev, r, scale):
    """test_gemm_split_bf16_accuracy's criterion on the row's shape and layout (contiguous operands: the same plan): against float64 the
    relative L2 error is below 2e-6 and at most twice the fp32 kernel's own on the same operands, the largest error at most twice its
    largest.  A bf16-kernel row is held against the float64 product of the bf16-rounded operands, which the fp32 kernel is given."""
    Fh = _fh()
    ta, tb, M, N, K = bool(r.ta), bool(r.tb), r.M, r.N, r.K
    g = torch.Generator().manual_seed(11)
    shpA, shpB = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    A = (torch.randn(shpA, generator=g) * torch.exp(2.0 * torch.randn(shpA, generator=g))).to(dev) * scale
    B = (torch.randn(shpB, generator=g) * torch.exp(2.0 * torch.randn(shpB, generator=g))).to(dev) * scale
    on_bf16 = r.label.startswith("BF16/")
    Ar, Br = (A.bfloat16().float(), B.bfloat16().float()) if on_bf16 else (A, B)
    ref = (Ar.double().t() if ta else Ar.double()) @ (Br.double().t() if tb else Br.double())
    zero = torch.zeros(N, device=dev) if r.bias else None              # (a row that only its bias keeps from skinny.hip keeps one)
    with Fh.gemm_precision("fp32"):
        exact = Fh.gemm(Ar, Br, ta, tb, bias=zero).double()
    with Fh.gemm_precision(r.mode):
        split, recs = _recorded(lambda: Fh.gemm(A, B, ta, tb, bias=zero))
        split = split.double()
    family, bm, ns, _ = gemm_shapes.parse(r.label)
    assert len(recs) == 1 and (gemm_shapes.FAMILIES[recs[0][10]], recs[0][6], recs[0][5]) == (family, bm, ns), recs
    assert recs[0][8] == (0 if on_bf16 else 2 if "/pieces/" in r.label else 1), recs
    e32 = ((exact - ref).norm() / ref.norm()).item()
    e6 = ((split - ref).norm() / ref.norm()).item()
    m32 = ((exact - ref).abs().max() / ref.abs().max()).item()
    m6 = ((split - ref).abs().max() / ref.abs().max()).item()
    print("rel-L2 vs float64: fp32 MFMA %.2e, %s %.2e | max-abs / max: %.2e, %.2e" % (e32, r.mode, e6, m32, m6))
    assert e6 < 2e-6 and e6 < 2.0 * e32 + 1e-8, (e6, e32)
    assert m6 < 2.0 * m32 + 1e-7, (m6, m32)
