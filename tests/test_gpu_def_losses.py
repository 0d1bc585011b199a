"""The index-matched losses on the deformed region (MLSP/mlsp.py:184-427) on the MI355X: findindexs against the reference's indices
and a float64 restatement, the three losses and their gradients against tests/golden/def_losses_*.npz (made by
tools/make_golden_def_losses.py), bit-reproducible backward scatters, a finite-difference check, and both models end to end."""
import os

import numpy as np
import pytest
import torch

import golden_common as gc

pytestmark = pytest.mark.gpu

CASES = ["def_losses_s0_B4_N1024.npz", "def_losses_s1_B2_N2048.npz", "def_losses_tie_s2_B2_N256.npz"]
NC = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mlsp_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _load(golden_dir, fname):
    return dict(np.load(os.path.join(golden_dir, fname)))


def _args(defpart):
    import argparse
    return argparse.Namespace(Density_normal_defpart=defpart, normal_pred_weight=0.5, Density_weight=0.05, density_num_class=NC)


def _ref_dist32(p1, p2, pen):
    """the reference's fp32 expression (MLSP/mlsp.py:205-215) for one cloud: torch.norm(p1_i - p2_j)**2 + pen_j, [N,N], CPU"""
    return torch.norm(p1[:, None, :] - p2[None, :, :], 2, dim=2) ** 2 + pen[None, :]


def _penalty(m):
    pen = m.clone()
    pen[m == 0] = 100
    pen[m == 1] = 0
    return pen


def _directions(g):
    """(rows, columns, penalty) per direction and cloud: index1 rows = pred, columns = gold; index2 the converse"""
    pred = torch.from_numpy(g["pred"])
    gold = torch.from_numpy(g["gold"]).permute(0, 2, 1).contiguous()
    pen = _penalty(torch.from_numpy(g["mask"])[:, 0])
    return [(pred, gold, pen), (gold, pred, pen)]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("fname", CASES)
def test_indices_match_reference(dev, golden_dir, fname):
    """Equal to the reference's indices on every row, except where the two candidates tie in the reference's own fp32 expression;
    on exact ties the lowest index is chosen (torch.min)."""
    from mlsp_amd import mlsp
    g = _load(golden_dir, fname)
    i1, i2 = mlsp.findindexs(torch.from_numpy(g["pred"]).to(dev), torch.from_numpy(g["gold"]).to(dev), torch.from_numpy(g["mask"]).to(dev))
    assert i1.dtype == torch.int64 and i2.dtype == torch.int64
    ours = [i1.cpu(), i2.cpu()]
    gold_idx = [torch.from_numpy(g["index1"]), torch.from_numpy(g["index2"])]
    ties = 0
    for d, (rows, cols, pen) in enumerate(_directions(g)):
        for b in range(rows.shape[0]):
            D = _ref_dist32(rows[b], cols[b], pen[b])
            o, r = ours[d][b], gold_idx[d][b]
            assert ((o >= 0) & (o < D.shape[1])).all()
            diff = (o != r).nonzero().flatten()
            if len(diff):
                assert torch.equal(D[diff, o[diff]], D[diff, r[diff]]), (d, b, diff[:8])
            if "tie" in fname:
                mins = D.min(dim=1).values
                first = (D == mins[:, None]).int().argmax(dim=1)          # lowest index attaining the minimum
                ties += int(((D == mins[:, None]).sum(1) > 1).sum())
                assert torch.equal(o, first), (d, b)
    if "tie" in fname:
        assert ties > 0


@pytest.mark.parametrize("fname", CASES[:2])
def test_indices_vs_float64(dev, golden_dir, fname):
    """Against a float64 restatement: at most 0.1 % of rows differ, each within 2 fp32 ulp of the float64 minimum."""
    from mlsp_amd import mlsp
    g = _load(golden_dir, fname)
    i1, i2 = mlsp.findindexs(torch.from_numpy(g["pred"]).to(dev), torch.from_numpy(g["gold"]).to(dev), torch.from_numpy(g["mask"]).to(dev))
    ours = [i1.cpu(), i2.cpu()]
    bad = total = 0
    for d, (rows, cols, pen) in enumerate(_directions(g)):
        for b in range(rows.shape[0]):
            D = ((rows[b].double()[:, None, :] - cols[b].double()[None, :, :]) ** 2).sum(-1) + pen[b].double()[None, :]
            want = D.argmin(dim=1)
            o = ours[d][b]
            diff = (o != want).nonzero().flatten()
            bad += len(diff)
            total += D.shape[0]
            if len(diff):
                got_d, want_d = D[diff, o[diff]].numpy(), D[diff, want[diff]].numpy()
                ulp = np.spacing(want_d.astype(np.float32)).astype(np.float64)
                assert (np.abs(got_d - want_d) <= 2 * ulp).all(), (d, b, got_d, want_d)
    assert bad <= 1e-3 * total, (bad, total)


def _inputs(g, dev):
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    return {k: t(k) for k in ("pred", "gold", "mask", "normal_pred", "normal_labels", "density", "density_mse", "density_labels",
                              "density_mse_label", "density_cls", "index1", "index2")}


@pytest.mark.parametrize("fname", CASES)
@pytest.mark.parametrize("defpart", [0, 1])
def test_losses_and_grads_vs_golden(dev, golden_dir, fname, defpart):
    """calc_def_normal_loss and deform_densityloss given the reference's indices: losses within 1e-5, gradients within 1e-4
    (relative, max-norm)."""
    from mlsp_amd import mlsp
    g = _load(golden_dir, fname)
    x = _inputs(g, dev)
    args = _args(bool(defpart))
    idx = [x["index1"], x["index2"]]
    npd = x["normal_pred"].clone().requires_grad_(True)
    loss = mlsp.calc_def_normal_loss(args, {"Normal": npd}, x["normal_labels"], x["mask"], idx, dev)
    loss.backward()
    np.testing.assert_allclose(loss.item(), g["normal_loss_dp%d" % defpart], rtol=1e-5)
    assert _rel(npd.grad.cpu().numpy(), g["d_normal_dp%d" % defpart]) < 1e-4
    pv, dn = x["density"].clone().requires_grad_(True), x["density_mse"].clone().requires_grad_(True)
    kl, mae = mlsp.deform_densityloss(args, {"density": pv, "density_mse": dn}, x["density_labels"], x["density_mse_label"], x["mask"],
                                      idx, dev)
    (kl + mae).backward()
    np.testing.assert_allclose(kl.item(), g["kl_dp%d" % defpart], rtol=1e-5)
    np.testing.assert_allclose(mae.item(), g["mae_dp%d" % defpart], rtol=1e-5)
    assert _rel(pv.grad.cpu().numpy(), g["dkl_density_dp%d" % defpart]) < 1e-4
    assert _rel(dn.grad.cpu().numpy(), g["dkl_density_mse_dp%d" % defpart]) < 1e-4


@pytest.mark.parametrize("fname", CASES)
@pytest.mark.parametrize("all_", [False, True])
def test_calc_def_density_loss_vs_golden(dev, golden_dir, fname, all_):
    """calc_def_density_loss with nn.NLLLoss(reduction='none') (the fixture's criterion), both `all` settings."""
    from mlsp_amd import mlsp
    g = _load(golden_dir, fname)
    assert int(g["criterion_nll"]) == 1
    x = _inputs(g, dev)
    pv = x["density"].clone().requires_grad_(True)
    loss = mlsp.calc_def_density_loss(_args(False), {"density": pv}, x["density_cls"], x["mask"], [x["index1"], x["index2"]], dev,
                                      torch.nn.NLLLoss(reduction='none'), all=all_)
    loss.backward()
    np.testing.assert_allclose(loss.item(), g["cdl_loss_all%d" % int(all_)], rtol=1e-5)
    assert _rel(pv.grad.cpu().numpy(), g["d_cdl_density_all%d" % int(all_)]) < 1e-4


@pytest.mark.parametrize("fname", CASES[:2])
def test_end_to_end_with_own_indices(dev, golden_dir, fname):
    """findindexs on the GPU feeding the losses: the same losses and gradients as the reference's chain (no ties in these clouds)."""
    from mlsp_amd import mlsp
    g = _load(golden_dir, fname)
    x = _inputs(g, dev)
    idx = mlsp.findindexs(x["pred"], x["gold"], x["mask"])
    assert torch.equal(idx[0], x["index1"]) and torch.equal(idx[1], x["index2"])
    args = _args(False)
    npd = x["normal_pred"].clone().requires_grad_(True)
    pv, dn = x["density"].clone().requires_grad_(True), x["density_mse"].clone().requires_grad_(True)
    ln = mlsp.calc_def_normal_loss(args, {"Normal": npd}, x["normal_labels"], x["mask"], idx, dev)
    kl, mae = mlsp.deform_densityloss(args, {"density": pv, "density_mse": dn}, x["density_labels"], x["density_mse_label"], x["mask"],
                                      idx, dev)
    (ln + kl + mae).backward()
    np.testing.assert_allclose(ln.item(), g["normal_loss_dp0"], rtol=1e-5)
    np.testing.assert_allclose(kl.item(), g["kl_dp0"], rtol=1e-5)
    assert _rel(npd.grad.cpu().numpy(), g["d_normal_dp0"]) < 1e-4
    assert _rel(pv.grad.cpu().numpy(), g["dkl_density_dp0"]) < 1e-4


def test_unsupported_size_is_an_error(dev):
    from mlsp_amd import mlsp
    N = 4097
    with pytest.raises(RuntimeError, match="unsupported"):
        mlsp.findindexs(torch.zeros(1, N, 3, device=dev), torch.zeros(1, 3, N, device=dev), torch.ones(1, 3, N, device=dev))


def test_backward_is_bit_reproducible(dev):
    """Half of gold sits in a tight cluster around one point, so hundreds of gold points share one nearest prediction: the scatter
    through index2 sums many terms into one row.  Two backward passes give identical bits."""
    from mlsp_amd import mlsp, functional as Fh
    g = torch.Generator().manual_seed(7)
    B, N = 2, 1024
    gold = torch.rand(B, 3, N, generator=g) * 2 - 1
    gold[:, :, : N // 2] = 0.3 + 1e-3 * torch.randn(B, 3, N // 2, generator=g)
    pred = (gold.permute(0, 2, 1) + 0.05 * torch.randn(B, N, 3, generator=g)).contiguous()
    mask = (torch.rand(B, 1, N, generator=g) < 0.3).float().expand(B, 3, N).contiguous()
    pred, gold, mask = pred.to(dev), gold.to(dev), mask.to(dev)
    idx = mlsp.findindexs(pred, gold, mask)
    counts = torch.stack([torch.bincount(idx[1][b], minlength=N) for b in range(B)])
    assert counts.max().item() >= 100
    normal_pred, normal_lab = torch.randn(B, N, 3, generator=g).to(dev), torch.randn(B, N, 3, generator=g).to(dev)
    pvec = torch.softmax(torch.randn(B * N, NC, generator=g), 1).to(dev)
    dens, dval = (torch.rand(B * N, generator=g) * 30).to(dev), (torch.rand(B, N, generator=g) * 30).round().to(dev)
    dlab = torch.softmax(torch.randn(B * N, NC, generator=g), 1).to(dev)
    feat = torch.randn(B, N, 7, generator=g).to(dev)

    def run():
        npd = normal_pred.clone().requires_grad_(True)
        pv, dn = pvec.clone().requires_grad_(True), dens.clone().requires_grad_(True)
        ft = feat.clone().requires_grad_(True)
        for dp in (False, True):
            mlsp.calc_def_normal_loss(_args(dp), {"Normal": npd}, normal_lab, mask, idx, dev).backward()
            kl, mae = mlsp.deform_densityloss(_args(dp), {"density": pv, "density_mse": dn}, dlab, dval, mask, idx, dev)
            (kl + 3 * mae).backward()
        (Fh.gather_rows(ft, idx[1]) * torch.arange(7, device=dev)).sum().backward()
        return npd.grad.clone(), pv.grad.clone(), dn.grad.clone(), ft.grad.clone()
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    # the gather's scatter is the plain sum (float64 restatement)
    want = torch.zeros(B, N, 7, dtype=torch.float64, device=dev)
    for bb in range(B):
        want[bb].index_add_(0, idx[1][bb], torch.arange(7, device=dev, dtype=torch.float64).expand(N, 7))
    assert torch.allclose(a[3].double(), want, rtol=1e-6, atol=1e-5)


def test_gather_rows_matches_indexing(dev):
    from mlsp_amd import functional as Fh
    g = torch.Generator().manual_seed(3)
    B, N = 3, 300
    idx = torch.randint(0, N, (B, N), generator=g).to(dev)
    x = torch.randn(B, N, 5, generator=g).to(dev)
    lab = torch.randint(0, 1 << 40, (B, N, 1), generator=g).to(dev)
    ar = torch.arange(B, device=dev)[:, None]
    assert torch.equal(Fh.gather_rows(x, idx), x[ar, idx])
    assert torch.equal(Fh.gather_rows_bits(lab, idx), lab[ar, idx])


def test_normal_loss_finite_differences(dev):
    """B = 1, N = 64, fp32 central differences of calc_def_normal_loss (step 5e-3) on 24 coordinates against the kernel's gradient.
    Labels are near the predictions so no |cos| sits at its kink.  Tolerance: 2e-2 of the largest gradient entry (fp32 rounding of
    a loss of order 1 over a 1e-2 step is ~1e-5; the second-order term of the step is well below that)."""
    from mlsp_amd import mlsp
    g = torch.Generator().manual_seed(11)
    B, N = 1, 64
    pred3 = torch.rand(B, N, 3, generator=g)
    gold = (pred3 + 0.05 * torch.randn(B, N, 3, generator=g)).permute(0, 2, 1).contiguous()
    mask = (torch.rand(B, 1, N, generator=g) < 0.4).float().expand(B, 3, N).contiguous()
    npred = torch.randn(B, N, 3, generator=g)
    nlab = npred + 0.3 * torch.randn(B, N, 3, generator=g)
    pred3, gold, mask, npred, nlab = (t.to(dev) for t in (pred3, gold, mask, npred, nlab))
    idx = mlsp.findindexs(pred3, gold, mask)
    args = _args(False)
    p = npred.clone().requires_grad_(True)
    mlsp.calc_def_normal_loss(args, {"Normal": p}, nlab, mask, idx, dev).backward()
    an = p.grad.flatten().cpu()
    h = 5e-3
    picks = torch.randperm(N * 3, generator=g)[:24]
    fd = []
    for k in picks.tolist():
        e = torch.zeros(N * 3, device=dev)
        e[k] = h
        lp = mlsp.calc_def_normal_loss(args, {"Normal": npred + e.view(B, N, 3)}, nlab, mask, idx, dev).item()
        lm = mlsp.calc_def_normal_loss(args, {"Normal": npred - e.view(B, N, 3)}, nlab, mask, idx, dev).item()
        fd.append((lp - lm) / (2 * h))
    fd = torch.tensor(fd)
    tol = 2e-2 * an.abs().max().item()
    assert (fd - an[picks]).abs().max().item() <= tol, (fd, an[picks])


def _train_step(model, x, gold, mask, dev, B, N, opt, **fwd):
    from mlsp_amd import mlsp
    g = torch.Generator().manual_seed(5)
    normal_gt = torch.randn(B, N, 3, generator=g).to(dev)
    dlab = torch.softmax(torch.randn(B * N, NC, generator=g), 1).to(dev)
    dval = (torch.rand(B, N, generator=g) * 30).round().to(dev)
    args = _args(False)
    args.density_num_class = NC
    logits = model(x, activate_density_normal_ondef=True, **fwd)
    assert logits["DefRec"].shape == (B, N, 3)
    idx = mlsp.findindexs(logits["DefRec"], gold, mask)
    loss = mlsp.calc_def_normal_loss(args, logits, normal_gt, mask, idx, dev)
    kl, mae = mlsp.deform_densityloss(args, logits, dlab, dval, mask, idx, dev)
    loss = loss + kl + mae
    opt.zero_grad()
    loss.backward()
    assert torch.isfinite(loss).item()
    n_grad = 0
    for p in model.parameters():
        if p.grad is not None:
            n_grad += 1
            assert torch.isfinite(p.grad).all().item()
    assert n_grad > 0
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all().item() for p in model.parameters())


def test_dgcnn_end_to_end(dev):
    """DGCNN at B = 8, N = 1024: deform_input, the model's deformed-part heads, findindexs, calc_def_normal_loss + deform_densityloss,
    backward and one FlatAdam step."""
    from mlsp_amd import Models, mlsp, pc_utils
    from mlsp_amd.optim import FlatAdam
    B, N = 8, 1024
    torch.manual_seed(0)
    np.random.seed(0)
    model = Models.DGCNN(gc.make_args(dropout=0.5, cuda=True)).to(dev).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(1)
    x = ((torch.rand(B, 3, N, generator=g) * 2 - 1) * 0.66).to(dev)       # the centre voxel holds >= 40 points
    gold = x.clone()
    lookup = torch.Tensor(pc_utils.region_mean(3)).to(dev)
    x, mask = mlsp.deform_input(x, lookup, 'volume_based_voxels', dev)
    assert (mask[:, 0].sum(1) >= 40).all()
    _train_step(model, x, gold, mask, dev, B, N, opt)


def test_segda_end_to_end(dev):
    """The PointSegDA model at N = 2048, k = 40 through the same losses."""
    from mlsp_amd import seg_models, mlsp, pc_utils
    from mlsp_amd.optim import FlatAdam
    B, N, K = 2, 2048, 40
    torch.manual_seed(2)
    np.random.seed(2)
    m = seg_models.DGCNN_DefRec(gc.make_seg_args(dropout=0.0, gpu=True), in_size=3, num_classes=8)
    m.k = m.shared_layers.k = K
    m = m.to(dev).train()
    opt = FlatAdam(m.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    x = ((torch.rand(B, 3, N, generator=g) * 2 - 1) * 0.66).to(dev)
    gold = x.clone()
    lookup = torch.Tensor(pc_utils.region_mean(3)).to(dev)
    x, mask = mlsp.deform_input(x, lookup, 'volume_based_voxels', dev)
    _train_step(m, x, gold, mask, dev, B, N, opt, make_seg=False, activate_DefRec=False)
