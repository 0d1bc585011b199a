"""The segmentation-supervision kernels (csrc/segsup.hip) through functional.seg_cross_entropy / seg_metrics_device and mlsp_amd.seg_train,
against the float64 restatement of tests/segsup_restatement.py and the recorded torch / sklearn values of tests/golden/segsup_*.npz.

Shapes: B in {1, 3}; N in {1, 255, 256, 257, 513} -- a chunk is 256 points up to N = 16384, so 513 is two chunks and a partial one --
plus N = 16641, where a thread takes two points; C in {1, 2, 8} (logits in registers; 8 read as 16-byte quads), {10, 13} (rows off the
16-byte grid, walked twice) and 64 (walked twice as quads).

Exact: preds = np.argmax of the same fp32 logits; mIoU and accuracy within 4 float64 ulps of the restatement on those preds (bit equality
is expected and printed).  Loss and gradient: distance = max |got - float64|, bar = max(floor, 3 x the same distance of torch's own fp32
F.cross_entropy on the CPU), floor = 2^-22 max(1, max |lse|) for a loss (per point or mean) and 2^-22 max |g| for gradient entries.

Measured on an MI355X: every mIoU and accuracy, on computed and on given predictions and against sklearn's recorded values, has the
restatement's bits (0 ulps).  Per input and quantity, the case closest to its bar:
  input     reduction  quantity  shape             distance    torch fp32  bar
  3 randn   mean       loss      B1 N257 C64       2.023e-07   2.023e-07   2.789e-06
            mean       grad      B1 N255 C8        5.304e-10   5.948e-10   1.784e-09
            none       loss      B1 N257 C13       8.717e-07   8.717e-07   2.615e-06
            none       grad      B3 N1 C13         2.084e-07   1.127e-07   7.550e-07
  + 1e4     mean       loss      B3 N257 C13       1.050e-07   3.718e-07   2.387e-03
            mean       grad      B3 N257 C2        1.007e-10   1.414e-10   4.243e-10
            none       loss      B1 N16641 C8      8.618e-07   8.618e-07   2.387e-03
            none       grad      B3 N257 C8        1.883e-07   3.245e-07   9.735e-07
  +- 80     mean       loss      B3 N257 C10       1.588e-06   6.041e-06   1.920e-05
            mean       grad      B3 N257 C2        7.429e-11   1.018e-10   3.092e-10
            none       loss      B3 N257 C2        7.629e-06   7.629e-06   2.289e-05
            none       grad      B3 N257 C8        1.857e-07   2.443e-07   8.805e-07
No distance is above a third of its bar.  (An fp32 loss is half an fp32 ulp from float64 at best, which is where it coincides with torch's.)
"""
import glob
import itertools
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import segsup_restatement as sr

pytestmark = pytest.mark.gpu

BS, NS, CS = (1, 3), (1, 255, 256, 257, 513), (1, 2, 8, 10, 13, 64)
N_TWO_PER_THREAD = 64 * 256 + 257
SHAPES = list(itertools.product(BS, NS, CS)) + [(1, N_TWO_PER_THREAD, 8)]
EDGE_SHAPES = [(3, 257, C) for C in CS] + [(1, 513, 8), (1, N_TWO_PER_THREAD, 8)]     # every kernel path, for the harder inputs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "segsup_*.npz")))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fh():
    from mlsp_amd import functional as Fh
    return Fh


_cases = {}


def case(kind, B, N, C):
    """seeded inputs and their float64 / torch-fp32 references, computed once per module"""
    key = (kind, B, N, C)
    if key not in _cases:
        seed = 100 * B + N + 7 * C
        logits = sr.make_logits(kind, B, N, C, seed)
        labels = sr.make_labels(B, N, C, seed)
        right = np.random.RandomState(seed + 1).uniform(size=(B, N)) < 0.5
        labels[right] = logits.argmax(axis=2)[right]
        up = np.random.RandomState(seed + 2).randn(B, N).astype(np.float32)
        c = dict(logits=logits, labels=labels, upstream=up)
        for red, u in (("mean", None), ("none", up)):
            c["want_" + red] = sr.cross_entropy(logits, labels, red, upstream=u)
            c["torch_" + red] = sr.torch_fp32(logits, labels, red, upstream=u)
        _cases[key] = c
    return _cases[key]


def run(dev, logits, labels, reduction="mean", upstream=None):
    """-> dict(loss, grad, preds, miou, acc, pcl) as numpy, from functional.seg_cross_entropy(with_metrics=True) and its backward"""
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    y = torch.from_numpy(labels).to(dev)
    loss, preds, miou, acc, pcl = _fh().seg_cross_entropy(x, y, reduction, with_metrics=True)
    assert not preds.requires_grad and not miou.requires_grad and not acc.requires_grad and not pcl.requires_grad
    if reduction == "mean":
        loss.backward(None if upstream is None else torch.tensor(float(upstream), device=dev))
    else:
        loss.backward(torch.ones_like(loss) if upstream is None else torch.from_numpy(upstream).to(dev))
    assert miou.dtype == acc.dtype == torch.float64 and preds.dtype == torch.int64 and loss.dtype == torch.float32
    return dict(loss=loss.detach().cpu().numpy().astype(np.float64), grad=x.grad.cpu().numpy().astype(np.float64), preds=preds.cpu().numpy(),
                miou=miou.cpu().numpy(), acc=acc.cpu().numpy(), pcl=pcl.cpu().numpy())


def check_exact(tag, got, logits, labels):
    C = logits.shape[2]
    assert np.array_equal(got["preds"], logits.argmax(axis=2)), tag
    miou, acc = sr.batch_metrics(labels, got["preds"], C)
    u = max(sr.ulps(got["miou"], miou), sr.ulps(got["acc"], acc))
    if u:
        print("%-28s metrics %g ulps from the restatement (not the same bits)" % (tag, u))
    assert u <= sr.METRIC_ULPS, (tag, got["miou"], miou, got["acc"], acc)
    return u


def check_close(tag, got, c, reduction):
    want, t32 = c["want_" + reduction], c["torch_" + reduction]
    out = []
    for name, bar_of in (("loss", sr.loss_bar), ("grad", sr.grad_bar)):
        d, y = sr.adist(got[name], want[name]), sr.adist(t32[name], want[name])
        b = bar_of(want, y)
        print("%-28s %-5s %-4s distance %.3e  torch fp32 %.3e  bar %.3e" % (tag, reduction, name, d, y, b))
        out.append((name, d, y, b))
    bad = [o for o in out if not o[1] <= o[3]]
    assert not bad, (tag, reduction, bad)


# --------------------------------------------------------------------------------------------- 1. predictions and counts
@pytest.mark.parametrize("kind", ["randn3", "ties"])
def test_preds_and_metrics_are_exact(dev, kind):
    worst = 0.0
    for B, N, C in SHAPES:
        c = case(kind, B, N, C)
        got = run(dev, c["logits"], c["labels"])
        worst = max(worst, check_exact("%s B%d N%d C%d" % (kind, B, N, C), got, c["logits"], c["labels"]))
        pcl = c["want_mean"]["cloud_sum"] / N
        assert sr.adist(got["pcl"], pcl) <= sr.loss_bar(c["want_mean"], 0.0), (B, N, C)
    print("%s: %d shapes, metrics at most %g ulps from the restatement" % (kind, len(SHAPES), worst))


def test_metrics_of_given_predictions(dev):
    from mlsp_amd import seg_train
    for B, N, C in [(1, 1, 2), (3, 255, 8), (3, 257, 13), (1, 513, 64), (1, N_TWO_PER_THREAD, 8)]:
        rs = np.random.RandomState(B + N + C)
        absent = C - 2 if C > 2 else None                   # a class in neither labels nor predictions
        classes = np.array([k for k in range(C) if k != absent])
        labels = classes[rs.randint(0, len(classes), (B, N))].astype(np.int64)
        preds = np.where(rs.uniform(size=(B, N)) < 0.6, labels, classes[rs.randint(0, len(classes), (B, N))]).astype(np.int64)
        y, p = torch.from_numpy(labels).to(dev), torch.from_numpy(preds).to(dev)
        miou, acc = _fh().seg_metrics_device(y, p, C)
        wm, wa = sr.batch_metrics(labels, preds, C)
        u = max(sr.ulps(miou.cpu().numpy(), wm), sr.ulps(acc.cpu().numpy(), wa))
        print("given preds B%d N%d C%d: %g ulps" % (B, N, C, u))
        assert u <= sr.METRIC_ULPS
        m, a = seg_train.seg_metrics(y, p)                    # the trainer's form: class ids below 64, Python sums over the batch
        tm, ta = sr.trainer_metrics(labels, preds, 64)
        assert isinstance(m, float) and isinstance(a, float)
        assert sr.ulps(m, tm) <= sr.METRIC_ULPS * B and sr.ulps(a, ta) <= sr.METRIC_ULPS * B, (m, tm, a, ta)
        assert seg_train.seg_metrics(y, p, num_classes=C) == (m, a)         # (no class id reaches C here)


def test_shapes_out_of_range_raise(dev):
    from mlsp_amd import _lib
    y = torch.zeros(2, 5, dtype=torch.int64, device=dev)
    for C in (65, 0):
        with pytest.raises(_lib.MlspLibraryError):
            _fh().seg_cross_entropy(torch.zeros(2, 5, C, device=dev), y)
        with pytest.raises(_lib.MlspLibraryError):
            _fh().seg_metrics_device(y, y, C)


# --------------------------------------------------------------------------------------------- 2. loss and gradient against float64
@pytest.mark.parametrize("reduction", ["mean", "none"])
@pytest.mark.parametrize("kind", ["randn3", "shift1e4", "spread80"])
def test_loss_and_gradient_vs_float64(dev, kind, reduction):
    for B, N, C in (SHAPES if kind == "randn3" else EDGE_SHAPES):
        c = case(kind, B, N, C)
        got = run(dev, c["logits"], c["labels"], reduction, c["upstream"] if reduction == "none" else None)
        check_close("%s B%d N%d C%d" % (kind, B, N, C), got, c, reduction)


# --------------------------------------------------------------------------------------------- 3. the trainer's call shape
def test_trainer_call_shape_reads_the_logits_in_place(dev):
    from mlsp_amd.seg_train import SegCrossEntropy
    B, N, C = 3, 257, 8
    c = case("randn3", B, N, C)
    for reduction in ("mean", "none"):
        x = torch.from_numpy(c["logits"]).to(dev).requires_grad_(True)
        y = torch.from_numpy(c["labels"]).to(dev)
        view = x.permute(0, 2, 1)
        assert view.stride() == (N * C, 1, C)
        loss = SegCrossEntropy(reduction=reduction)(view, y)
        fn = loss.grad_fn
        assert "SegCE" in type(fn).__name__, type(fn).__name__
        assert fn.saved_tensors[0].data_ptr() == x.data_ptr()              # what the kernels read is the head's own tensor: no copy
        up = torch.from_numpy(c["upstream"]).to(dev)
        loss.backward(up if reduction == "none" else None)
        assert x.grad.shape == (B, N, C) and x.grad.is_contiguous()
        got = dict(loss=loss.detach().cpu().numpy().astype(np.float64), grad=x.grad.cpu().numpy().astype(np.float64))
        assert got["loss"].shape == ((B, N) if reduction == "none" else ())
        check_close("module, permuted view", got, c, reduction)
    # a [B, C, N] tensor that is no view of [B, N, C]: one copy, same values
    x = torch.from_numpy(np.ascontiguousarray(c["logits"].transpose(0, 2, 1))).to(dev).requires_grad_(True)
    loss = SegCrossEntropy()(x, y)
    loss.backward()
    got = dict(loss=loss.detach().cpu().numpy().astype(np.float64), grad=x.grad.cpu().numpy().astype(np.float64).transpose(0, 2, 1))
    check_close("module, [B, C, N] contiguous", got, c, "mean")


def test_plain_rows_equal_torch(dev):
    from mlsp_amd.seg_train import SegCrossEntropy
    R, C = 5, 10
    logits = sr.make_logits("randn3", 1, R, C, 11)
    labels = sr.make_labels(1, R, C, 11)
    up = np.random.RandomState(3).randn(1, R).astype(np.float32)
    for reduction, u in (("mean", None), ("none", up)):
        c = {"want_" + reduction: sr.cross_entropy(logits, labels, reduction, upstream=u)}
        x32 = torch.from_numpy(logits[0]).clone().requires_grad_(True)
        l32 = torch.nn.functional.cross_entropy(x32, torch.from_numpy(labels[0]), reduction=reduction)
        l32.backward(None if u is None else torch.from_numpy(u[0]))
        c["torch_" + reduction] = dict(loss=l32.detach().numpy().astype(np.float64).reshape(c["want_" + reduction]["loss"].shape),
                                       grad=x32.grad.numpy().astype(np.float64)[None])
        x = torch.from_numpy(logits[0]).to(dev).requires_grad_(True)
        loss = SegCrossEntropy(reduction=reduction)(x, torch.from_numpy(labels[0]).to(dev))
        assert loss.shape == l32.shape
        loss.backward(None if u is None else torch.from_numpy(u[0]).to(dev))
        got = dict(loss=loss.detach().cpu().numpy().astype(np.float64).reshape(c["want_" + reduction]["loss"].shape),
                   grad=x.grad.cpu().numpy().astype(np.float64)[None])
        check_close("[R, C] rows", got, c, reduction)


# --------------------------------------------------------------------------------------------- 4. ignored labels
def test_ignored_labels(dev):
    for B, N, C in [(3, 257, 8), (1, 513, 13)]:
        c = case("randn3", B, N, C)
        logits, labels = c["logits"], c["labels"].copy()
        rs = np.random.RandomState(5)
        gone = rs.uniform(size=(B, N)) < 0.1
        gone[0, 0] = gone[B - 1, N - 1] = True
        labels[gone] = -100
        only100 = labels.copy()
        labels[0, 0] = C + 3                                  # out of range, not ignore_index: torch raises, the kernels ignore it
        for reduction, up in (("mean", None), ("none", c["upstream"])):
            got = run(dev, logits, labels, reduction, up)
            want = sr.cross_entropy(logits, labels, reduction, upstream=up)
            assert want["n_valid"] == int((~gone).sum())
            t32 = sr.torch_fp32(logits, only100, reduction, upstream=up)      # torch, ignore_index = -100 (its default)
            check_close("ignored B%d N%d C%d" % (B, N, C), got, {"want_" + reduction: want, "torch_" + reduction: t32}, reduction)
            assert not got["grad"][gone].any()                                # exact zeros
            check_exact("ignored", got, logits, labels)
            if reduction == "mean":                                           # n_valid leaves them out: the mean is over the valid points
                assert abs(got["loss"] - want["per_point"].sum() / (~gone).sum()) <= sr.loss_bar(want, 0.0)


def test_every_label_ignored(dev):
    B, N, C = 2, 257, 8
    c = case("randn3", B, N, C)
    labels = np.full((B, N), -100, dtype=np.int64)
    got = run(dev, c["logits"], labels)
    assert np.isnan(got["loss"]) and not got["grad"].any()
    assert np.isnan(got["miou"]).all() and np.isnan(got["acc"]).all()
    assert np.array_equal(got["preds"], c["logits"].argmax(axis=2))
    torch.cuda.synchronize()


def test_nan_logit(dev):
    B, N, C = 1, 257, 10
    logits = case("randn3", B, N, C)["logits"].copy()
    labels = case("randn3", B, N, C)["labels"]
    logits[0, 3, 4] = np.nan
    logits[0, 200, 0] = np.nan
    x = torch.from_numpy(logits).to(dev)
    loss, preds, _, _, _ = _fh().seg_cross_entropy(x, torch.from_numpy(labels).to(dev), "none", with_metrics=True)
    loss, preds = loss.cpu().numpy(), preds.cpu().numpy()
    assert np.isnan(loss[0, 3]) and np.isnan(loss[0, 200]) and np.isfinite(np.delete(loss[0], [3, 200])).all()
    assert ((preds >= 0) & (preds < C)).all()


# --------------------------------------------------------------------------------------------- 5. golden fixtures
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_golden_fixtures(dev, path):
    z = np.load(path)
    logits, labels, up = z["logits"], z["labels"], z["upstream"]
    lse = sr.lse64(logits)
    for reduction, u in (("mean", None), ("none", up)):
        got = run(dev, logits, labels, reduction, u)
        t32 = sr.torch_fp32(logits, labels, reduction, upstream=u)
        nv = float((labels != -100).sum())
        g = np.full(labels.shape, 1.0 / nv) if reduction == "mean" else up.astype(np.float64)
        want = dict(loss=z["loss_" + reduction], lse=lse, g=g)
        names = ["loss"]
        if "grad_" + reduction in z.files:
            want["grad"] = z["grad_" + reduction]
            names.append("grad")
        for name in names:
            d, y = sr.adist(got[name], want[name]), sr.adist(t32[name], want[name])
            b = (sr.loss_bar if name == "loss" else sr.grad_bar)(want, y)
            print("%-16s %-5s %-4s distance %.3e  torch fp32 %.3e  bar %.3e" % (os.path.basename(path), reduction, name, d, y, b))
            assert d <= b, (path, reduction, name, d, y, b)
        assert np.array_equal(got["preds"], z["preds"])
        u_m = max(sr.ulps(got["miou"], z["miou"]), sr.ulps(got["acc"], z["acc"]))
        print("%-16s metrics %g ulps from sklearn's" % (os.path.basename(path), u_m))
        assert u_m <= sr.METRIC_ULPS


# --------------------------------------------------------------------------------------------- 6. determinism
def test_two_runs_give_the_same_bits(dev):
    for B, N, C in [(3, 513, 8), (3, 257, 13), (1, N_TWO_PER_THREAD, 8)]:
        c = case("randn3", B, N, C)
        for reduction, up in (("mean", None), ("none", c["upstream"])):
            a, b = (run(dev, c["logits"], c["labels"], reduction, up) for _ in range(2))
            for name in ("loss", "grad", "miou", "acc", "pcl", "preds"):
                assert a[name].tobytes() == b[name].tobytes(), (B, N, C, reduction, name)


# --------------------------------------------------------------------------------------------- 7. end to end
def test_seg_step_under_the_segmentation_model(dev):
    """DGCNN_DefRec's parameter gradients under seg_step, under torch's F.cross_entropy on the device, and under the float64 gradient of
    the loss with respect to the logits (rounded to fp32) pushed through the same backward: the model's backward is the same fp32 linear
    map in all three, so the distance to the float64-anchored gradients measures the loss kernels alone.  distance = max |g - g64| /
    max |g64| over all parameters; bar = max(2e-6, 3 x torch's distance) -- 2e-6 is the floor the project holds quantities to that have
    passed through its GEMMs (tests/loss_restatement.py FLOOR)."""
    from mlsp_amd import seg_models, seg_train
    B, N, C = 2, 128, 8
    m = seg_models.DGCNN_DefRec(gc.make_seg_args(dropout=0.0, gpu=True), in_size=3, num_classes=C)
    gc.perturb_params(m, 4)
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(9)
    x = ((torch.rand(B, 3, N, generator=g) * 2 - 1) * 0.66).to(dev)
    labels = torch.randint(0, C, (B, N), generator=g).to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    anchor = {}

    def grads(kind):
        m.load_state_dict(state)                                 # (the running statistics move with every forward)
        m.zero_grad(set_to_none=True)
        logits = m(x, make_seg=True, activate_DefRec=False)["seg"]
        assert logits.shape == (B, N, C)
        if kind == "ours":
            loss, preds, miou, acc = seg_train.seg_step(logits, labels)
            assert torch.equal(preds, logits.max(dim=2)[1])
            loss.backward()
        elif kind == "torch":
            loss = torch.nn.functional.cross_entropy(logits.permute(0, 2, 1), labels)
            loss.backward()
        else:
            want = anchor["want"] = sr.cross_entropy(logits.detach().cpu().numpy(), labels.cpu().numpy(), "mean")
            loss = torch.tensor(want["loss"])
            logits.backward(torch.from_numpy(want["grad"].astype(np.float32)).to(dev))
        ps = [n for n, p in m.named_parameters() if p.grad is not None]     # (the heads that activate_DefRec=False leaves out get none)
        assert len(ps) > 20, ps
        return float(loss.detach()), ps, torch.cat([p.grad.detach().double().reshape(-1) for p in m.parameters() if p.grad is not None]).cpu()

    l64, n64, g64 = grads("float64")
    lo, no, go = grads("ours")
    lt, nt, gt = grads("torch")
    assert no == n64 == nt
    scale = g64.abs().max().item()
    d, y = (go - g64).abs().max().item() / scale, (gt - g64).abs().max().item() / scale
    bar = max(2e-6, 3 * y)
    print("end to end: loss %.7f (float64 %.7f, torch %.7f); parameter gradients: distance %.3e  torch %.3e  bar %.3e" % (lo, l64, lt, d, y, bar))
    assert abs(lo - l64) <= sr.loss_bar(anchor["want"], abs(lt - l64))
    assert d <= bar
