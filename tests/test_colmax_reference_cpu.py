"""The float64 restatement that tests/test_gpu_colmax.py measures the colmax kernels against (tests/colmax_restatement.py), pinned on the
CPU against stock autograd: F.batch_norm -> activation -> max over the points."""
import pytest
import torch
import torch.nn.functional as F

import colmax_restatement as cr


def _inputs(B, N, Cin, Cout, seed, sign):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B * N, Cin, generator=g, dtype=torch.float64)
    W = torch.randn(Cout, Cin, generator=g, dtype=torch.float64) * 0.2
    gamma = torch.rand(Cout, generator=g, dtype=torch.float64) + 0.2
    gamma = gamma if sign > 0 else -gamma if sign < 0 else gamma * (torch.arange(Cout) % 3 - 0.5).sign()
    beta = torch.randn(Cout, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1, torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5
    dOut = torch.randn(B, Cout, generator=g, dtype=torch.float64)
    return X, W, gamma, beta, rm, rv, dOut


def _stock(X, W, gamma, beta, rm, rv, B, N, training, dOut, act, eps):
    x, w, g, b = [t.clone().requires_grad_(True) for t in (X, W, gamma, beta)]
    rm, rv = rm.clone(), rv.clone()
    z = F.batch_norm(x @ w.t(), rm, rv, g, b, training, 0.1, eps)
    z = z if act == cr.ACT_NONE else F.relu(z) if act == cr.ACT_RELU else F.leaky_relu(z, 0.2)
    o = z.view(B, N, -1).max(dim=1)[0]
    o.backward(dOut)
    return dict(out=o.detach(), dX=x.grad, dW=w.grad, dgamma=g.grad, dbeta=b.grad, run_mean=rm, run_var=rv)


@pytest.mark.parametrize("sign", [1, -1, 0])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act,eps", [(cr.ACT_LRELU, 1e-5), (cr.ACT_NONE, 1e-3), (cr.ACT_RELU, 1e-5)])
def test_restatement_equals_stock_autograd(training, sign, act, eps):
    """sel=None: the first extreme of Y per column is the arg-max of act(BN(Y)), both signs of gamma (sign 0: mixed); a forced selection
    equal to that arg-max reproduces it.  (ReLU: a dead maximum is tied with every other dead row in stock torch, which then may name
    another row -- the values and every gradient are zero there either way.)"""
    B, N, Cin, Cout = 3, 37, 12, 20
    X, W, gamma, beta, rm, rv, dOut = _inputs(B, N, Cin, Cout, 5 + sign, sign)
    want = _stock(X, W, gamma, beta, rm, rv, B, N, training, dOut, act, eps)
    got = cr.colmax_f64(X, W, gamma, beta, rm, rv, B, N, training, dOut, act=act, eps=eps)
    assert got["nkink"] == 0 or act == cr.ACT_NONE
    for n in cr.NAMES:
        assert cr.dist(got[n], want[n]) <= 1e-12, (n, cr.dist(got[n], want[n]))
    forced = cr.colmax_f64(X, W, gamma, beta, rm, rv, B, N, training, dOut, act=act, eps=eps, sel=got["sel"])
    for n in cr.NAMES:
        assert torch.equal(forced[n], got[n]), n
    assert torch.equal(got["sel"], cr.first_extreme(got["Y"], gamma))
    if sign:
        y = got["Y"] * sign
        assert torch.equal(y.gather(1, got["sel"].view(B, 1, Cout)).view(B, Cout), y.max(dim=1)[0])


def test_restatement_in_fp32_is_close():
    """the yardstick run: the same ops in fp32, with the float64 run's selection forced"""
    B, N, Cin, Cout = 2, 50, 16, 24
    X, W, gamma, beta, rm, rv, dOut = [t.float() for t in _inputs(B, N, Cin, Cout, 9, 0)]
    want = cr.colmax_f64(X, W, gamma, beta, rm, rv, B, N, True, dOut)
    yard = cr.colmax_f64(X, W, gamma, beta, rm, rv, B, N, True, dOut, sel=want["sel"], dtype=torch.float32)
    for n in cr.NAMES:
        assert yard[n].dtype == torch.float32 and cr.dist(yard[n], want[n]) < 1e-5, n


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("shape", [(2, 128, 64, 96), (3, 192, 40, 70), (32, 256, 128, 1024), (4, 100, 64, 96)])
def test_dyadic_premise(shape, dup):
    """fp32 == float64 on X W^T for the dyadic shapes of the GPU file (asserted inside dyadic_inputs), and ties between DIFFERENT rows
    are frequent: the first-occurrence rule decides more than a tenth of the columns (the sparse channels of dyadic_inputs)."""
    B, N, Cin, Cout = shape
    X, W = cr.dyadic_inputs(B, N, Cin, Cout, seed=sum(shape), dup=dup)
    assert Cin * 225 < 2 ** 24
    Y = (X @ W.t()).view(B, N, Cout)
    tied = ((Y == Y.max(dim=1, keepdim=True)[0]).sum(dim=1) > 1).float().mean().item()
    assert tied > (0.9 if dup else 0.1), tied
    if dup:
        assert all(len(torch.unique(X.view(B, N, Cin)[b], dim=0)) <= 3 for b in range(B))


def test_query_reaches_every_answer():
    """The shape query launches nothing: its answers for the shapes of the GPU file (cr.PATHS) hold on any machine.  0, 64 and 128 in
    every product mode; both panel heights on the multi-panel shape across the modes; every cloud a whole number of panels; junk is 0."""
    from mlsp_amd import _lib
    lib = _lib.load()
    for shape, per_mode in cr.PATHS.items():
        for mode, (rows, panels) in zip(cr.MODES, per_mode):
            assert cr.panel_rows(shape, mode) == rows, (shape, mode)
            assert rows * panels == (shape[1] if rows else 0), (shape, mode)
    for i in range(3):
        assert {per_mode[i][0] for per_mode in cr.PATHS.values()} == {0, 64, 128}
    assert {rows for rows, _ in cr.PATHS[cr.FUSED_MULTI128]} == {64, 128}
    assert lib.mlsp_pointmlp_colmax_panel_rows(2, 128, 64, 96, 7) == 0 and lib.mlsp_pointmlp_colmax_panel_rows(0, 128, 64, 96, 0) == 0
