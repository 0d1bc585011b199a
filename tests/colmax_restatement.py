"""pointmlp_colmax restated with plain torch ops: a bias-free 1x1 conv, BatchNorm1d, an activation and the max over the N points of each
cloud (PointDA/Models.py:132-136, PointDA/model_utils.py:116-117), in float64 -- or in fp32, the yardstick of tests/test_gpu_colmax.py.
Shared by tests/test_gpu_colmax.py and tests/test_colmax_reference_cpu.py."""
import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
NAMES = ("out", "dX", "dW", "dgamma", "dbeta", "run_mean", "run_var")

MODES = ("default", "fp32", "bf16x6")
# (B, N, Cin, Cout): the smallest shape of each forward path, derived from BM = BN = 128, BK = 32, gemm_pick_split and gemm_pick_bm
UNFUSED_SPLITK = (3, 128, 128, 256)        # 6 output tiles, 4 K tiles: K is split
UNFUSED_RAGGED = (4, 100, 64, 96)          # 64-row panels, N % 64 != 0
FUSED_2x64 = (2, 128, 64, 96)              # 64-row panels, two per cloud, short K, ragged column tile (the bounds-checked epilogue)
FUSED_3x64 = (3, 192, 40, 70)              # three per cloud, K no multiple of the K tile
FUSED_1x128 = (1, 128, 64, 160)            # P < 256 keeps the 128-row tile: one panel per cloud
FUSED_FAST = (16, 256, 256, 1024)          # 256 tiles, 8 K tiles: interior epilogue, the split kernel in the split modes; 256 < 512 tiles: 64 rows
FUSED_MULTI128 = (32, 256, 128, 1024)      # 512 tiles: 128-row panels where the split kernel takes the launch, 64-row ones in fp32
MANY_CLOUDS = (70, 4, 32, 48)
ONE_POINT, FIVE_POINTS = (3, 1, 16, 24), (3, 5, 16, 24)
OUTLIER = (2, 128, 64, 512)
LDS_BIG = (1, 8192, 8, 32)
# shape -> (panel rows the query returns, panels per cloud) in each of MODES; (0, 0): the unfused forward
PATHS = {UNFUSED_SPLITK: ((0, 0),) * 3, UNFUSED_RAGGED: ((0, 0),) * 3, MANY_CLOUDS: ((0, 0),) * 3, ONE_POINT: ((0, 0),) * 3,
         FIVE_POINTS: ((0, 0),) * 3, FUSED_2x64: ((64, 2),) * 3, FUSED_3x64: ((64, 3),) * 3, FUSED_1x128: ((128, 1),) * 3,
         FUSED_FAST: ((64, 4),) * 3, FUSED_MULTI128: ((128, 2), (64, 4), (128, 2)), OUTLIER: ((64, 2),) * 3, LDS_BIG: ((64, 128),) * 3}


def panel_rows(shape, mode):
    """mlsp_pointmlp_colmax_panel_rows for (B, N, Cin, Cout) in product mode `mode` ("default": the process default)"""
    import contextlib
    from mlsp_amd import _lib, functional as Fh
    with contextlib.nullcontext() if mode == "default" else Fh.gemm_precision(mode):
        return _lib.load().mlsp_pointmlp_colmax_panel_rows(*shape, Fh.gemm_precision.code())


def colmax_f64(X, W, gamma, beta, rm, rv, B, N, training, dOut, act=ACT_LRELU, slope=0.2, eps=1e-5, momentum=0.1, sel=None, out_gpu=None,
               kink=1e-6, dtype=torch.float64):
    """X [B*N, Cin], W [Cout, Cin], dOut [B, Cout].  Y = X W^T; BatchNorm with the batch statistics over all B*N rows (training) or the
    running ones (eval); the activation (0 none, 1 ReLU, 2 LeakyReLU with `slope`); out[b, c] = the value at row sel[b, c] of cloud b, by
    gather; the gradients by autograd.  sel=None takes the FIRST extreme of Y per column -- the first maximum where gamma >= 0, the first
    minimum otherwise (act(BN(.)) is monotone per channel).  Where the pre-activation z lies within kink * max|z| of 0 it may round to
    either side in fp32: there the restatement takes the branch of `out_gpu` (the kernel's output, `out > 0`) when given.
    -> dict: out, dX, dW, dgamma, dbeta, run_mean, run_var (after the update), sel [B, Cout], nkink (elements where that happened),
    Y [B, N, Cout] (detached)."""
    P, Cin = X.shape
    Cout = W.shape[0]
    assert P == B * N and W.shape[1] == Cin
    x, w, g, b = [t.detach().to(torch.device("cpu"), dtype).requires_grad_(True) for t in (X, W, gamma, beta)]
    y = (x @ w.t()).view(B, N, Cout)
    rm_, rv_ = rm.detach().to("cpu", dtype), rv.detach().to("cpu", dtype)
    if training:
        mean, var = y.mean(dim=(0, 1)), y.var(dim=(0, 1), unbiased=False)
    else:
        mean, var = rm_, rv_
    if sel is None:
        sel = torch.where(g.detach() >= 0, y.detach(), -y.detach()).argmax(dim=1)          # (argmax: the first maximal index)
    sel = sel.to("cpu").long().view(B, 1, Cout)
    ysel = y.gather(1, sel).view(B, Cout)
    z = (ysel - mean) / torch.sqrt(var + eps) * g + b
    zd = z.detach()
    near = zd.abs() <= kink * zd.abs().max()
    pos = zd > 0
    if out_gpu is not None:
        pos = torch.where(near, out_gpu.detach().to("cpu") > 0, pos)
    o = z if act == ACT_NONE else torch.where(pos, z, z * (0.0 if act == ACT_RELU else slope))
    o.backward(dOut.detach().to("cpu", dtype))
    if training:
        rm_ = (1 - momentum) * rm_ + momentum * mean.detach()
        rv_ = (1 - momentum) * rv_ + momentum * var.detach() * P / (P - 1)
    return dict(out=o.detach(), dX=x.grad, dW=w.grad, dgamma=g.grad, dbeta=b.grad, run_mean=rm_, run_var=rv_, sel=sel.view(B, Cout),
                nkink=int(near.sum()) if act else 0, Y=y.detach())


def dist(a, b):
    """max|a - b| / max|b| in float64"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def dyadic_inputs(B, N, Cin, Cout, seed, dup=False):
    """X in i/8 and W in j/16 (|i|, |j| <= 15): every partial sum of X W^T is a multiple of 1/128 below Cin * 225 / 128, exact in fp32 while
    Cin * 225 < 2^24 -- and in the split product modes, whose pieces hold such values exactly.  fp32, the split modes and float64 then see
    the same Y and make the same choices, exact ties between different rows included.  Every fourth channel has ONE small tap only
    (|j| <= 2, on input c % Cin), so its column of Y takes at most 31 values and its extreme is shared by several different rows.
    dup: every cloud is made of three distinct points.  The premise is asserted here, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-15, 16, (B * N, Cin), generator=g).float() / 8
    W = torch.randint(-15, 16, (Cout, Cin), generator=g).float() / 16
    c4 = torch.arange(0, Cout, 4)
    W[c4] = 0
    W[c4, c4 % Cin] = torch.randint(-2, 3, (len(c4),), generator=g).float() / 16
    if dup:
        X = X.view(B, N, Cin)[:, :3][torch.arange(B)[:, None], torch.randint(0, 3, (B, N), generator=g)].reshape(B * N, Cin).contiguous()
    assert torch.equal((X @ W.t()).double(), X.double() @ W.double().t())
    return X, W


def first_extreme(Y, gamma):
    """[B, N, C] -> [B, C]: the first row of each cloud attaining the column's maximum (gamma >= 0) or minimum"""
    return torch.where(gamma >= 0, Y, -Y).argmax(dim=1)
