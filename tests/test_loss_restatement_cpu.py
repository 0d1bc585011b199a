"""The input conditions of tests/test_gpu_losses.py, checked without a GPU for the committed seeds:

  - the masked-row form of tests/loss_restatement.py equals oracle/ref_cpu.py in float64 wherever both fit (dist <= 1e-12 on the value and
    on every gradient);
  - except in the deliberate tie case every masked row's float64 gap between its best and second-best column is >= 1e-3 (relative), and
    the fp32 reference selects the same columns as float64 -- so a selection that differs on the GPU is a wrong kernel, not a near-tie;
  - the yardstick (dist from float64 of the reference run in fp32 on the CPU) is <= 3e-5 for every quantity of every case, so the bar
    min(1e-4, max(2e-6, 3 x yardstick)) is never set by its cap;
  - in the wide-cloud case at least one masked row of each direction selects an UNMASKED column in float64;
  - the restatement reproduces the recorded values of tests/golden/loss_s0_N256.npz and chamfer_dir_s4_B3_N256.npz to the tolerances
    of tests/test_gpu_kernels.py.

A seed that misses a condition is replaced in loss_restatement.chamfer_cases; the condition stays."""
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import loss_restatement as lr

CASES = lr.chamfer_cases()
LARGE = sorted(set(lr.LARGE_FUSED_N + lr.LARGE_DIR_N))
_, _NONFINITE = lr.nonfinite_cases()
NONFINITE_BASE = lr.nonfinite_base()


def _clouds_of(case):
    """the (rows, columns, mask_cord) of the two directions: A = gold rows against pred columns, B = the converse"""
    gt, mc = case.gold.permute(0, 2, 1).contiguous(), case.mask[:, 0, :]
    return {"A": (gt, case.pred, mc), "B": (case.pred, gt, mc)}


@pytest.mark.parametrize("case", CASES + [NONFINITE_BASE], ids=lambda c: c.name)
def test_masked_row_form_equals_ref_cpu(case):
    for make in (lr.fused_reference, lr.dir_reference):
        rows, ref = make(case, torch.float64, "rows"), make(case, torch.float64, "ref_cpu")
        for k in ref:
            d = lr.dist(rows[k], ref[k])
            print(case.name, make.__name__, k, "%.2e" % d)
            assert d <= 1e-12, (case.name, make.__name__, k, d)


@pytest.mark.parametrize("N", [1638, 2731])
def test_masked_row_form_equals_ref_cpu_large(N):
    """(float64 ref_cpu at N = 2731 holds [1, N, N, 3] in about 180 MB a copy; the larger N are left to the row form)"""
    case = lr.large_case(N)
    rows, ref = lr.dir_reference(case, torch.float64, "rows"), lr.dir_reference(case, torch.float64, "ref_cpu")
    for k in ref:
        assert lr.dist(rows[k], ref[k]) <= 1e-12, (N, k)


@pytest.mark.parametrize("case", CASES + [NONFINITE_BASE] + [lr.large_case(N) for N in LARGE], ids=lambda c: c.name)
def test_gap_and_fp32_selection(case):
    for tag, (p1, p2, mc) in _clouds_of(case).items():
        a64, gap = lr.selection(p1.double(), p2.double(), mc.double())
        a32, _ = lr.selection(p1, p2, mc)
        assert torch.equal(a64, a32), (case.name, tag)
        masked = mc != 0
        assert ((a64 >= 0) == masked).all()
        if case.ties:
            assert (gap[masked] == 0).all(), "every masked row of the tie case has an exact tie"
            assert (a64[masked] < case.N // 2).all(), "and the first minimum is the lower copy"
            continue
        print(case.name, tag, "smallest gap %.2e" % gap.min().item())
        assert gap.min().item() >= lr.GAP_MIN, (case.name, tag, gap.min().item())


def _yardsticks(ref64, ref32):
    return {k: lr.dist(ref32[k], ref64[k]) for k in ref64}


@pytest.mark.parametrize("case", CASES + [NONFINITE_BASE], ids=lambda c: c.name)
def test_chamfer_yardstick(case):
    for make in (lr.fused_reference, lr.dir_reference):
        y = _yardsticks(make(case, torch.float64, "rows"), make(case, torch.float32, lr.fp32_form(case.N)))
        print(case.name, make.__name__, " ".join("%s %.2e" % kv for kv in y.items()))
        assert max(y.values()) <= lr.YARD_MAX, (case.name, y)


@pytest.mark.parametrize("N", LARGE)
def test_chamfer_yardstick_large(N):
    case = lr.large_case(N)
    make = lr.fused_reference if N in lr.LARGE_FUSED_N else lr.dir_reference
    y = _yardsticks(make(case, torch.float64, "rows"), make(case, torch.float32, lr.fp32_form(N)))
    print(case.name, " ".join("%s %.2e" % kv for kv in y.items()))
    assert max(y.values()) <= lr.YARD_MAX, (N, y)


def test_wide_case_selects_unmasked_columns():
    case = next(c for c in CASES if c.name == "wide")
    for tag, (p1, p2, mc) in _clouds_of(case).items():
        arg, _ = lr.selection(p1.double(), p2.double(), mc.double())
        n_un = n_m = 0
        for b in range(case.B):
            a = arg[b][mc[b] != 0]
            n_un += int((mc[b][a] == 0).sum())
            n_m += int((mc[b][a] != 0).sum())
        print("wide", tag, "rows selecting an unmasked column", n_un, "a masked one", n_m)
        assert n_un >= 1, tag


@pytest.mark.parametrize("P", lr.NORMAL_P)
@pytest.mark.parametrize("kind", lr.WEIGHT_KINDS[:3])
@pytest.mark.parametrize("scale", [1e-6, 1.0, 1e6])
def test_normal_yardstick(P, kind, scale):
    pred, gt, w = lr.normal_case(20 + P % 7, P, kind, scale)
    y = _yardsticks(lr.normal_reference(pred, gt, w), lr.normal_reference(pred, gt, w, torch.float32))
    assert max(y.values()) <= lr.YARD_MAX, y


@pytest.mark.parametrize("P,nc", lr.TAIL_SHAPES)
@pytest.mark.parametrize("scale", [1.0, 60.0])
def test_tail_yardstick(P, nc, scale):
    c = lr.tail_case(lr.tail_seed(P, nc), P, nc, scale)
    y = _yardsticks(lr.tail_reference(*c), lr.tail_reference(*c, dtype=torch.float32))
    assert max(y.values()) <= lr.YARD_MAX, y
    assert (lr.tail_reference(*c)["pvec"].sum(1) - 1).abs().max().item() <= 1e-12


@pytest.mark.parametrize("P", [1, 257, 65537])
@pytest.mark.parametrize("nc", [1, 16, 64])
@pytest.mark.parametrize("kind", lr.WEIGHT_KINDS[:3])
def test_density_yardstick(P, nc, kind):
    c = lr.density_case(40 + nc, P, nc, kind)
    y = _yardsticks(lr.density_reference(*c), lr.density_reference(*c, dtype=torch.float32))
    assert max(y.values()) <= lr.YARD_MAX, y


def test_density_yardstick_zeros_and_tail():
    c = lr.density_zero_case(50)
    y = _yardsticks(lr.density_reference(*c), lr.density_reference(*c, dtype=torch.float32))
    assert max(y.values()) <= lr.YARD_MAX, y
    for P, nc in ((257, 16), (300, 64)):
        g = torch.Generator().manual_seed(51)
        logits = torch.randn(P, nc, generator=g)
        tvec, target = lr.soft_labels(P, nc, g)
        y = _yardsticks(lr.tail_density_reference(logits, tvec, target, None),
                        lr.tail_density_reference(logits, tvec, target, None, torch.float32))
        assert max(y.values()) <= lr.YARD_MAX, y


def test_all_zero_weights_give_nan():
    pred, gt, w = lr.normal_case(21, 257, "zero", 1.0)
    assert torch.isnan(lr.normal_reference(pred, gt, w)["loss"])
    r = lr.density_reference(*lr.density_case(41, 257, 16, "zero"))
    assert torch.isnan(r["kl"]) and torch.isnan(r["mae"])


def test_restatement_reproduces_recorded_losses(golden_dir):
    """the float64 restatement against the fp32 recordings of the unmodified reference, at test_losses_vs_golden's tolerances"""
    g = dict(np.load(os.path.join(golden_dir, "loss_s0_N256.npz")))
    args = gc.make_args()
    inp = gc.make_inputs(0, 2, 256)
    case = lr._case("golden", torch.from_numpy(g["pred"]), inp["gold"], inp["mask"][:, 0, :])
    r = lr.fused_reference(case)
    k = args.DefRec_weight * 20.0                                         # calc_loss: weight * DefRec_SCALER (MLSP/mlsp.py:7)
    np.testing.assert_allclose(k * r["loss"].item(), g["loss_DefRec"], rtol=1e-4)
    np.testing.assert_allclose((k * r["d_pred"]).numpy(), g["g_pred"], rtol=1e-3, atol=1e-6)
    mask_cord = inp["mask"].permute(0, 2, 1)[:, :, 0] * 26 + 1
    normal = torch.from_numpy(g["normal"])
    # the normal gradient is recorded for the whole loss: only the normal loss reaches `normal`
    rn = lr.normal_reference(normal, inp["normal_gt"], mask_cord)
    np.testing.assert_allclose(args.normal_pred_weight * rn["loss"].item(), g["loss_normal"], rtol=1e-4)
    np.testing.assert_allclose((args.normal_pred_weight * rn["d_pred"]).numpy(), g["g_normal"], rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(args.normal_pred_weight * lr.normal_reference(normal, inp["normal_gt"], None)["loss"].item(),
                               g["normal_unmasked"], rtol=1e-4)
    lg = torch.from_numpy(g["dlogits"])
    rd = lr.tail_density_reference(lg, inp["dens_vec"], inp["dens_val"], mask_cord.reshape(-1))
    np.testing.assert_allclose(args.Density_weight * rd["kl"].item(), g["loss_kl"], rtol=1e-4)
    np.testing.assert_allclose(args.Density_weight * rd["mae"].item(), g["loss_mae"], rtol=1e-4)
    np.testing.assert_allclose((args.Density_weight * rd["d_logits"]).numpy(), g["g_dlogits"], rtol=1e-3, atol=1e-7)
    ru = lr.tail_density_reference(lg, inp["dens_vec"], inp["dens_val"], None)
    np.testing.assert_allclose(args.Density_weight * ru["kl"].item(), g["kl_unmasked"], rtol=1e-4)
    np.testing.assert_allclose(args.Density_weight * ru["mae"].item(), g["mae_unmasked"], rtol=1e-4)


def test_restatement_reproduces_recorded_one_direction(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "chamfer_dir_s4_B3_N256.npz")))
    p1, p2 = torch.from_numpy(g["p1"]), torch.from_numpy(g["p2"])
    case = lr._case("golden_dir", p1, p2.permute(0, 2, 1), torch.from_numpy(g["mask"])[:, :, 0])
    r = lr.dir_reference(case)
    np.testing.assert_allclose(r["loss"].item(), g["dist"], rtol=1e-5)
    np.testing.assert_allclose(r["d_p1"].numpy(), g["g_p1"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(r["d_p2"].numpy(), g["g_p2"], rtol=1e-4, atol=1e-7)


def test_nonfinite_cases_overflow_fp32():
    """case (c): every squared distance of cloud 1 is beyond fp32 (so no column compares below the kernels' start value), and cloud 0
    of every non-finite case is the base case's cloud 0"""
    for tag, case, _ in _NONFINITE:
        assert torch.equal(case.pred[0], NONFINITE_BASE.pred[0]) and torch.equal(case.gold[0], NONFINITE_BASE.gold[0]), tag
        assert torch.equal(case.mask, NONFINITE_BASE.mask), tag
    case = next(c for t, c, _ in _NONFINITE if t == "overflow")
    d = case.pred[1].unsqueeze(1) - case.gold[1].t().unsqueeze(0)
    assert torch.isinf((d * d).sum(-1)).all()
    assert (d.double() ** 2).min().item() > float(torch.finfo(torch.float32).max)
