"""Every kernel of csrc/loss.hip -- masked Chamfer (fused and one-direction), |cos| normal loss, cardinality tail, density loss -- against
the float64 restatements of tests/loss_restatement.py, at the shapes and mask edges where the kernels take another path.

Distance: max|a - b| / max|b|.  Yardstick: the distance from float64 of the reference run in fp32 on the CPU.
Bar per quantity: min(1e-4, max(2e-6, 3 x yardstick)) -- the floor is the GEMM family's (test_gemm_split_bf16_accuracy), 3 is for the
differing summation order, 1e-4 is the tolerance of test_losses_vs_golden, kept as a cap.  tests/test_loss_restatement_cpu.py shows for
the same seeds that every yardstick is <= 3e-5, that no masked row is a near-tie (gap >= 1e-3) outside the tie case, and that the fp32
reference selects the float64 columns -- so the selection is compared exactly.

Largest measured distance per kernel (MI355X), beside the yardstick and bar of that quantity; every selection equal to float64's:
  kernel                      quantity                                    distance   yardstick   bar
  Chamfer, fused              loss      uneven (1 / 40 / 200 rows)        1.72e-07   1.12e-07    2.0e-06
                              d pred    tiny (3, 2)                       1.11e-07   1.11e-07    2.0e-06
                              N = 1638 / 1639 / 3840, any quantity     <= 6.9e-08  <= 1.3e-07    2.0e-06
  Chamfer, one direction      loss      wave (2, 65)                      1.14e-07   1.55e-08    2.0e-06
                              d p2      wide                              9.90e-08   9.90e-08    2.0e-06
                              N = 2730 / 2731 / 6400, any quantity     <= 7.9e-08  <= 9.4e-08    2.0e-06
  non-finite masked rows      cloud 0's gradient against the finite case: 0 (the same bits), both forms, all three cases
  normal loss                 loss      P = 1, x 1e6                      7.11e-08   7.11e-08    2.0e-06
                              d pred    P = 257, w = 26 m + 1             2.47e-07   1.81e-07    2.0e-06
  cardinality tail            dens      (300, 64), x 1                    2.75e-07   1.42e-07    2.0e-06
                              d logits  (257, 5), x 60, from dens         8.34e-07   8.34e-07    2.5e-06
  density loss                kl        p_vec with exact zeros            9.50e-08   1.38e-07    2.0e-06
                              d p_vec   P = 65537, nc = 64, 0/1 mask      8.64e-08   8.64e-08    2.0e-06
  tail feeding density loss   d logits  (300, 64), no mask                3.46e-07   1.61e-07    2.0e-06
The distance closest to its bar is a third of it (the tail's gradients at x 60, where the yardstick sets the bar).
"""
import pytest
import torch

import loss_restatement as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fh():
    from mlsp_amd import functional as Fh
    return Fh


def _leaf(t, dev, need=True):
    return t.detach().clone().to(dev).requires_grad_(need)


def compare(tag, got, want64, ref32):
    """got / want64 / ref32: dicts name -> tensor; every quantity of want64 within its bar"""
    bad = []
    for name in sorted(want64):
        g, w = got[name].detach().cpu(), want64[name]
        assert torch.isfinite(g).all(), (tag, name)
        d, y = lr.dist(g, w), lr.dist(ref32[name], w)
        b = lr.bar(y)
        print("%-34s %-12s distance %.3e  yardstick %.3e  bar %.3e" % (tag, name, d, y, b))
        if not d <= b:
            bad.append((name, d, y, b))
    assert not bad, (tag, bad)


# --------------------------------------------------------------------------------------------- Chamfer
def fused_run(case, dev):
    """-> (dict(loss, d_pred), argA, argB) of mlsp.reconstruction_loss; the args are the backward's saved tensors"""
    from mlsp_amd import mlsp
    pred = _leaf(case.pred, dev)
    loss = mlsp.reconstruction_loss(pred, case.gold.to(dev), case.mask.to(dev))
    argA, argB = (t.cpu().long() for t in loss.grad_fn.saved_tensors[4:6])
    loss.backward()
    return dict(loss=loss.detach().cpu(), d_pred=pred.grad.cpu()), argA, argB


def dir_run(case, dev, need=(True, True), swap=False):
    """-> (dict(loss, d_p1, d_p2), arg) of mlsp.chamfer_distance(pred, gold^T, mask^T) (swap: rows from gold^T, columns from pred)"""
    from mlsp_amd import mlsp
    a, b = case.pred, case.gold.permute(0, 2, 1).contiguous()
    if swap:
        a, b = b, a
    p1, p2 = _leaf(a, dev, need[0]), _leaf(b, dev, need[1])
    loss = mlsp.chamfer_distance(p1, p2, case.mask.permute(0, 2, 1).contiguous().to(dev))
    arg = loss.grad_fn.saved_tensors[4].cpu().long()
    loss.backward()
    out = dict(loss=loss.detach().cpu())
    if need[0]:
        out["d_p1"] = p1.grad.cpu()
    if need[1]:
        out["d_p2"] = p2.grad.cpu()
    return out, arg


def _bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def _selected(arg, masked, N):
    """[B, N] bool: columns that some masked row selected"""
    hit = torch.zeros_like(masked)
    for b in range(arg.shape[0]):
        hit[b, arg[b][masked[b]]] = True
    return hit


def check_chamfer_case(case, dev):
    gt, mc = case.gold.permute(0, 2, 1).contiguous(), case.mask[:, 0, :]
    masked = mc != 0
    selA, _ = lr.selection(gt.double(), case.pred.double(), mc.double())       # gold rows, pred columns
    selB, _ = lr.selection(case.pred.double(), gt.double(), mc.double())       # pred rows, gold columns
    form = lr.fp32_form(case.N)

    got, argA, argB = fused_run(case, dev)
    assert torch.equal(argA[masked], selA[masked]) and torch.equal(argB[masked], selB[masked]), case.name
    compare(case.name + " fused", got, lr.fused_reference(case), lr.fused_reference(case, torch.float32, form))
    idle = ~masked & ~_selected(argA, masked, case.N)           # pred rows that are unmasked and that no gold row selected
    assert (got["d_pred"][idle] == 0).all(), case.name
    again, _, _ = fused_run(case, dev)
    assert _bits_equal(got, again), case.name + ": the fused form is not bit-reproducible"

    want, ref32 = lr.dir_reference(case), lr.dir_reference(case, torch.float32, form)
    got, arg = dir_run(case, dev)
    assert torch.equal(arg[masked], selB[masked]), case.name
    compare(case.name + " one-direction", got, want, ref32)
    assert (got["d_p1"][~masked] == 0).all(), case.name
    assert (got["d_p2"][~_selected(arg, masked, case.N)] == 0).all(), case.name
    again, _ = dir_run(case, dev)
    assert _bits_equal(got, again), case.name + ": the one-direction form is not bit-reproducible"
    only2, _ = dir_run(case, dev, need=(False, True))
    assert torch.equal(only2["d_p2"], got["d_p2"]) and torch.equal(only2["loss"], got["loss"]), case.name
    return got


@pytest.mark.parametrize("case", lr.chamfer_cases(), ids=lambda c: c.name)
def test_chamfer_vs_float64(dev, case):
    got = check_chamfer_case(case, dev)
    if case.ties:
        # every column j < 48 has a copy at j + 48 at exactly the same distance: the lower index is selected (checked above against
        # the float64 first minimum) and takes the whole gradient -- nothing lands on the copy
        assert (got["d_p2"][:, case.N // 2:] == 0).all()
        half = lr.ties_case(12, duplicates=False)
        h, _ = dir_run(half, dev)
        # Against the duplicate-free half (N = 48, 12 masked rows), which selects the same columns.  A row's gradient is
        # (2 g / count) (p1_i - p2_t): the count doubles, a power of two, so the rows compare bitwise, and the copies equal their originals.
        half_n = case.N // 2
        assert torch.equal(got["d_p1"][:, :half_n], 0.5 * h["d_p1"]) and torch.equal(got["d_p1"][:, half_n:], got["d_p1"][:, :half_n])
        # A column's gradient and the loss sum every row twice over 24 rows where the half sums it once over 12: the same real number in
        # another order of additions, so these two compare to the floor of the bar
        assert lr.dist(got["d_p2"][:, :half_n], h["d_p2"]) <= lr.FLOOR
        assert lr.dist(got["loss"], h["loss"]) <= lr.FLOOR


def test_chamfer_large_n(dev):
    """the dynamic-LDS path above 64 KB: the fused forward crosses it between N = 1638 and 1639 and ends at 3840, the one-direction
    forward crosses between 2730 and 2731 and ends at 6400"""
    from mlsp_amd import _lib
    for N in lr.LARGE_FUSED_N:
        case = lr.large_case(N)
        mc = case.mask[:, 0, :]
        masked = mc != 0
        gt = case.gold.permute(0, 2, 1).contiguous()
        got, argA, argB = fused_run(case, dev)
        assert torch.equal(argA[masked], lr.selection(gt.double(), case.pred.double(), mc.double())[0][masked]), N
        assert torch.equal(argB[masked], lr.selection(case.pred.double(), gt.double(), mc.double())[0][masked]), N
        compare(case.name + " fused", got, lr.fused_reference(case), lr.fused_reference(case, torch.float32, lr.fp32_form(N)))
    for N in lr.LARGE_DIR_N:
        case = lr.large_case(N)
        mc = case.mask[:, 0, :]
        masked = mc != 0
        got, arg = dir_run(case, dev)
        assert torch.equal(arg[masked], lr.selection(case.pred.double(), case.gold.permute(0, 2, 1).double(), mc.double())[0][masked]), N
        compare(case.name + " one-direction", got, lr.dir_reference(case), lr.dir_reference(case, torch.float32, lr.fp32_form(N)))
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        fused_run(lr.large_case(3841), dev)
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        dir_run(lr.large_case(6401), dev)


def test_chamfer_nonfinite_masked_rows(dev):
    """A NaN or an infinity in a masked point, or coordinates whose squared distances overflow: the arg arrays stay in [0, N) and the loss
    is non-finite (include/mlsp_hip.h).  Forward first; the arg arrays are checked on the host BEFORE any backward runs, so a wrong index
    fails here and the kernel that would read through it is never launched."""
    from mlsp_amd import mlsp
    base, cases = lr.nonfinite_cases()
    N, masked = base.N, base.mask[:, 0, :] != 0
    want_fused = fused_run(base, dev)[0]["d_pred"][0]
    base_dir = {"pred": dir_run(base, dev)[0], "gold": dir_run(base, dev, swap=True)[0]}
    yard = {"fused": lr.dist(lr.fused_reference(base, torch.float32, "ref_cpu")["d_pred"][0], lr.fused_reference(base)["d_pred"][0])}
    for tag, case, rows_cloud in cases:
        # fused form
        pred = _leaf(case.pred, dev)
        loss = mlsp.reconstruction_loss(pred, case.gold.to(dev), case.mask.to(dev))
        argA, argB = (t.cpu().long() for t in loss.grad_fn.saved_tensors[4:6])
        for a in (argA, argB):
            assert ((a[masked] >= 0) & (a[masked] < N)).all(), (tag, a[masked])
        assert not torch.isfinite(loss).item(), (tag, loss.item())
        loss.backward()
        d = lr.dist(pred.grad[0].cpu(), want_fused)
        print("nonfinite %-12s fused cloud 0 gradient: distance %.3e  bar %.3e" % (tag, d, lr.bar(yard["fused"])))
        assert d <= lr.bar(yard["fused"]), (tag, d)
        # one-direction form, rows from the cloud that holds the spoilt point
        swap = rows_cloud == "gold"
        a, b = case.pred, case.gold.permute(0, 2, 1).contiguous()
        if swap:
            a, b = b, a
        p1, p2 = _leaf(a, dev), _leaf(b, dev)
        loss = mlsp.chamfer_distance(p1, p2, case.mask.permute(0, 2, 1).contiguous().to(dev))
        arg = loss.grad_fn.saved_tensors[4].cpu().long()
        assert ((arg[masked] >= 0) & (arg[masked] < N)).all(), (tag, arg[masked])
        assert not torch.isfinite(loss).item(), (tag, loss.item())
        loss.backward()
        want = base_dir[rows_cloud]
        for name, g in (("d_p1", p1.grad), ("d_p2", p2.grad)):
            d = lr.dist(g[0].cpu(), want[name][0])
            print("nonfinite %-12s one-direction cloud 0 %s: distance %.3e" % (tag, name, d))
            assert d <= lr.FLOOR, (tag, name, d)


# --------------------------------------------------------------------------------------------- normal loss
def normal_run(pred, gt, w, dev, weight=1.0):
    Fh = _fh()
    p = _leaf(pred, dev)
    loss = Fh.normal_loss(p, gt.to(dev), None if w is None else w.to(dev), weight)
    loss.backward()
    return dict(loss=loss.detach().cpu(), d_pred=p.grad.cpu())


@pytest.mark.parametrize("P", lr.NORMAL_P)
def test_normal_loss_vs_float64(dev, P):
    """P = 65537 is one past the 256 x 256 grid of the partial kernel: the grid-stride loop takes a second trip"""
    for kind in lr.WEIGHT_KINDS:
        for scale in (1e-6, 1.0, 1e6):
            pred, gt, w = lr.normal_case(20 + P % 7, P, kind, scale)
            got = normal_run(pred, gt, w, dev)
            if kind == "zero":                                  # 0 / 0, as the reference
                assert torch.isnan(got["loss"]) and torch.isnan(lr.normal_reference(pred, gt, w)["loss"])
                continue
            compare("normal P=%d w=%s x%g" % (P, kind, scale), got, lr.normal_reference(pred, gt, w),
                    lr.normal_reference(pred, gt, w, torch.float32))
            assert _bits_equal(got, normal_run(pred, gt, w, dev))
            if kind == "01":
                assert (got["d_pred"][0][w == 0] == 0).all()


def test_normal_loss_hand_rows(dev):
    """Rows whose gradient is known in closed form, placed in front of random rows.  With c = cos(pred, gt), n = |pred| and hats for the
    unit vectors, d loss / d pred = -(w / sum w) sign(c) (gt^ - c pred^) / n."""
    pred, gt, w = lr.normal_case(27, 257, "26m+1", 1.0)
    pred[0, 0] = 0.0                                                       # pred exactly zero: |cos| = 0, gradient zero and finite
    gt[0, 1] = 0.0                                                         # gt exactly zero: the same
    pred[0, 2], gt[0, 2] = torch.tensor([0.0, 3.0, 0.0]), torch.tensor([2.0, 0.0, 0.0])      # perpendicular on the axes: cos = 0 exactly
    gt[0, 3] = torch.tensor([0.5, -1.0, 2.0])
    pred[0, 3] = -2 * gt[0, 3]                                             # anti-parallel: |cos| = 1, gt^ - c pred^ = 0
    pred[0, 4], gt[0, 4] = torch.tensor([0.0, 0.0, 2.0]), torch.tensor([3.0, 0.0, 4.0])      # c = 0.8, gradient -(w/sw) (0.6, 0, 0) / 2
    got = normal_run(pred, gt, w, dev)
    want = lr.normal_reference(pred, gt, w)
    compare("normal hand rows", got, want, lr.normal_reference(pred, gt, w, torch.float32))
    g = got["d_pred"][0]
    assert torch.isfinite(g).all()
    assert (g[0] == 0).all() and (g[1] == 0).all() and (g[2] == 0).all()
    scale = want["d_pred"].abs().max().item()
    assert g[3].abs().max().item() <= lr.FLOOR * scale                     # zero up to the rounding of c = -(gt^ . gt^)
    k = (w[4] / w.sum()).item()
    expect = torch.tensor([-k * 0.6 / 2, 0.0, 0.0], dtype=torch.float64)
    assert (g[4].double() - expect).abs().max().item() <= lr.FLOOR * scale and g[4][1] == 0


# --------------------------------------------------------------------------------------------- cardinality tail
def tail_run(logits, Rp, Rd, dev):
    Fh = _fh()
    w = lr.fc2w(logits.shape[1]).view(1, -1).to(dev)
    out = {}
    for tag, use_p, use_d in (("d_from_pvec", True, False), ("d_from_dens", False, True), ("d_from_both", True, True)):
        lg = _leaf(logits, dev)
        p, d = Fh.density_tail(lg, w)
        loss = ((p * Rp.to(dev)).sum() if use_p else 0) + ((d * Rd.to(dev)).sum() if use_d else 0)
        loss.backward()
        out[tag] = lg.grad.cpu()
    out["pvec"], out["dens"] = p.detach().cpu(), d.detach().cpu()
    return out


@pytest.mark.parametrize("P,nc", lr.TAIL_SHAPES)
@pytest.mark.parametrize("scale", [1.0, 60.0])
def test_density_tail_vs_float64(dev, P, nc, scale):
    """x 60: one class dominates the row and the other probabilities underflow -- only the max subtraction keeps the exponentials finite"""
    c = lr.tail_case(lr.tail_seed(P, nc), P, nc, scale)
    got = tail_run(*c, dev)
    compare("tail P=%d nc=%d x%g" % (P, nc, scale), got, lr.tail_reference(*c), lr.tail_reference(*c, dtype=torch.float32))
    assert (got["pvec"].double().sum(1) - 1).abs().max().item() <= 1e-6
    assert _bits_equal(got, tail_run(*c, dev))


# --------------------------------------------------------------------------------------------- density loss
def density_run(pvec, dens, tvec, target, m, dev):
    Fh = _fh()
    p, d = _leaf(pvec, dev), _leaf(dens, dev)
    kl, mae = Fh.density_loss(p, d, tvec.to(dev), target.to(dev), None if m is None else m.to(dev), 1.0)
    out = dict(kl=kl.detach().cpu(), mae=mae.detach().cpu())
    for tag, l in (("kl", kl), ("mae", mae), ("both", kl + mae)):
        gp, gd = torch.autograd.grad(l, (p, d), retain_graph=True)
        out["d_pvec_" + tag], out["d_dens_" + tag] = gp.cpu(), gd.cpu()
    return out


@pytest.mark.parametrize("P", [1, 257, 65537])
@pytest.mark.parametrize("nc", [1, 16, 64])
def test_density_loss_vs_float64(dev, P, nc):
    """Hand-made p_vec.  (At nc = 1 a softmax gives exactly 1, and log(1 + 1e-10) is below what fp32 resolves: the reference's own fp32 kl
    is then 0 against 1e-10 in float64.  So the nc = 1 rows hold values in (0.03, 0.7) instead.)"""
    for kind in lr.WEIGHT_KINDS:
        c = lr.density_case(40 + nc, P, nc, kind)
        got = density_run(*c, dev)
        want = lr.density_reference(*c)
        if kind == "zero":
            assert torch.isnan(got["kl"]) and torch.isnan(got["mae"]) and torch.isnan(want["kl"]) and torch.isnan(want["mae"])
            continue
        compare("density P=%d nc=%d m=%s" % (P, nc, kind), got, want, lr.density_reference(*c, dtype=torch.float32))
        same = c[1] == c[3]                                          # dens == target: sign(0) = 0
        assert same.any() and (got["d_dens_mae"][same] == 0).all() and (got["d_dens_both"][same] == 0).all()
        assert (got["d_dens_kl"] == 0).all() and (got["d_pvec_mae"] == 0).all()
        assert _bits_equal(got, density_run(*c, dev))


def test_density_loss_zero_probabilities(dev):
    c = lr.density_zero_case(50)
    assert (c[0] == 0).any()
    compare("density zeros", density_run(*c, dev), lr.density_reference(*c), lr.density_reference(*c, dtype=torch.float32))


@pytest.mark.parametrize("P,nc", [(257, 16), (300, 64)])
def test_density_loss_fed_by_tail(dev, P, nc):
    Fh = _fh()
    g = torch.Generator().manual_seed(51)
    logits = torch.randn(P, nc, generator=g)
    tvec, target = lr.soft_labels(P, nc, g)
    for kind in lr.WEIGHT_KINDS[:3]:
        m = lr.make_weight(kind, P, g)
        lg = _leaf(logits, dev)
        p, d = Fh.density_tail(lg, lr.fc2w(nc).view(1, -1).to(dev))
        kl, mae = Fh.density_loss(p, d, tvec.to(dev), target.to(dev), None if m is None else m.to(dev), 1.0)
        (kl + mae).backward()
        got = dict(kl=kl.detach().cpu(), mae=mae.detach().cpu(), d_logits=lg.grad.cpu())
        compare("tail+density P=%d nc=%d m=%s" % (P, nc, kind), got, lr.tail_density_reference(logits, tvec, target, m),
                lr.tail_density_reference(logits, tvec, target, m, torch.float32))


# --------------------------------------------------------------------------------------------- dtypes
@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16])
def test_wrappers_refuse_non_fp32_differentiable_inputs(dev, dtype):
    """the kernels read fp32; another dtype must raise, not be reinterpreted or silently converted"""
    Fh = _fh()
    case = lr.random_case("dtype", 60, 2, 70, 12)
    pred, gold, mask = case.pred.to(dev), case.gold.to(dev), case.mask.to(dev)
    with pytest.raises(TypeError, match="float32"):
        Fh.chamfer_masked(pred.to(dtype).requires_grad_(True), gold, mask, 0.5)
    npred, ngt, w = (t.to(dev) for t in lr.normal_case(61, 70, "26m+1", 1.0))
    with pytest.raises(TypeError, match="float32"):
        Fh.normal_loss(npred.to(dtype).requires_grad_(True), ngt, w)
    logits = lr.tail_case(62, 70, 16, 1.0)[0].to(dev)
    with pytest.raises(TypeError, match="float32"):
        Fh.density_tail(logits.to(dtype).requires_grad_(True), lr.fc2w(16).to(dev))
    pvec, dens, tvec, target, m = (t.to(dev) for t in lr.density_case(63, 70, 16, "26m+1"))
    with pytest.raises(TypeError, match="float32"):
        Fh.density_loss(pvec.to(dtype).requires_grad_(True), dens, tvec, target, m)
    with pytest.raises(TypeError, match="float32"):
        Fh.density_loss(pvec, dens.to(dtype).requires_grad_(True), tvec, target, m)


def test_wrappers_convert_targets_and_masks(dev):
    """float64 / int targets, masks and weights are converted: the same bits as with float ones, and an fp32 gradient"""
    Fh = _fh()
    case = lr.random_case("dtype", 60, 2, 70, 12)

    def chamfer(gold, mask):
        p = _leaf(case.pred, dev)
        Fh.chamfer_masked(p, gold.to(dev), mask.to(dev), 0.5).backward()
        return p.grad
    want = chamfer(case.gold, case.mask)
    assert want.dtype == torch.float32
    assert torch.equal(chamfer(case.gold.double(), case.mask.double()), want)
    assert torch.equal(chamfer(case.gold, case.mask.int()), want) and torch.equal(chamfer(case.gold, case.mask.bool()), want)

    npred, ngt, w = lr.normal_case(61, 70, "26m+1", 1.0)

    def normal(gt, w):
        return normal_run(npred, gt, w, dev)
    want = normal(ngt, w)
    assert _bits_equal(normal(ngt.double(), w.double()), want) and _bits_equal(normal(ngt, w.long()), want)

    pvec, dens, tvec, target, m = lr.density_case(63, 70, 16, "26m+1")
    want = density_run(pvec, dens, tvec, target, m, dev)
    assert _bits_equal(density_run(pvec, dens, tvec.double(), target.double(), m.double(), dev), want)
    assert _bits_equal(density_run(pvec, dens, tvec, target.long(), m.int(), dev), want)       # the targets are whole counts
    assert want["d_pvec_both"].dtype == torch.float32 and want["d_dens_both"].dtype == torch.float32
