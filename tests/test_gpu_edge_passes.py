"""What the leaner EdgeConv passes can newly break (csrc/edge.hip), at the smallest shapes that
reach them.  When all three backward passes are vectorised (Cout in {64, 128, 256}, aligned operands, pitches that are multiples of 4)
the reduce stores gz, the reverse gather writes dv_j next to du_j and raises the bound of duv for both, and no point pass runs; the
forward keeps ysel = v + the extreme; the T-Net's first stage hands the forward reduce no ysel / argsel buffers at all.
The yardsticks are those of tests/test_gpu_kernels.py (float64 evaluation of the reference's op sequence, dyadic inputs, the common
bars) and of tests/test_gpu_tnet.py (the float64 restatement, its bars)."""
import pytest
import torch

import test_gpu_tnet as tg
import tnet_restatement as tr
from test_gpu_kernels import _EC_L2, _EC_MAX, _edgeconv_errors, _edgeconv_f64, _edgeconv_gpu, _edgeconv_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mlsp_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _against_float64(dev, shape, seed, training, act, graph="rand"):
    """the procedure of test_edgeconv_fwd_bwd for one case: selections equal to float64's first-occurrence slots, every quantity at the
    common bars -> (got, want)"""
    B, N, C, Cout, k = shape
    x, idx, W, gamma, beta, rm, rv, dOut = _edgeconv_inputs(B, N, C, Cout, k, seed=seed, graph=graph)
    idx = idx.to(dev)
    got = _edgeconv_gpu(dev, x, idx, W, gamma, beta, rm, rv, training, dOut, act=act)
    want = _edgeconv_f64(x, idx, W, gamma, beta, rm, rv, training, dOut, act=act, out_gpu=got["out"])
    err = _edgeconv_errors(got, want)
    print("edge passes", shape, training, act, graph, " ".join("%s %.1e/%.1e" % (n, *e) for n, e in err.items()))
    assert want["nkink"] <= 1e-4 * B * N * Cout + 2, want["nkink"]
    assert torch.equal(got["sel"].long(), want["sel"]), (got["sel"].long() != want["sel"]).sum().item()
    for name, (l2, mx) in err.items():
        assert l2 <= _EC_L2 and mx <= _EC_MAX, (name, l2, mx)
    return got, want


def test_dv_of_a_destination_nobody_points_to(dev):
    """graph "hub": the upper half of each cloud is in no neighbour list, so its waves of the gather walk an empty reverse list -- and
    still owe dv (point 0 has in-degree N).  vec<32> forward, edge_bwd_gather_vec_kernel<32, DV>; the <16> and <64> hubs are in _EDGE_CASES.
    A missing dv row shows in dx and dW."""
    _against_float64(dev, (2, 256, 8, 128, 20), seed=11, training=True, act=2, graph="hub")


@pytest.mark.parametrize("shape,act", [pytest.param((1, 200, 128, 256, 20), 0, id="1-200-128-256-20-none"),
                                       pytest.param((3, 64, 64, 128, 20), 1, id="3-64-64-128-20-relu")])
def test_fused_backward_in_eval_mode(dev, shape, act):
    """eval mode on the fused path: no batch statistics flow back, dv = gz (the gather copies the row the reduce stored) and du is the
    plain sum of the selected gz"""
    _against_float64(dev, shape, seed=sum(shape), training=False, act=act)


def _duv_f64(x, idx, W, gamma, beta, sel, dOut):
    """the point-space gradient [du | dv] of a training-mode call without activation, by autograd in float64 on idx's device (sel: the
    slots taken)"""
    B, N, k = idx.shape
    C, Cout = x.shape[1], W.shape[0]
    dv = idx.device
    x64, W64, g64, b64, d64 = (t.to(dv, torch.float64) for t in (x, W, gamma, beta, dOut))
    uv = (x64 @ torch.cat((W64[:, :C], W64[:, C:] - W64[:, :C])).t()).requires_grad_(True)
    u, v = uv[:, :Cout].view(B, N, Cout), uv[:, Cout:].view(B, N, 1, Cout)
    y = u[torch.arange(B, device=dv)[:, None, None], idx] + v
    mean, var = y.mean(dim=(0, 1, 2)), y.var(dim=(0, 1, 2), unbiased=False)
    ysel = y.gather(2, sel.to(dv).view(B, N, 1, Cout)).view(B * N, Cout)
    ((ysel - mean) / torch.sqrt(var + 1e-5) * g64 + b64).backward(d64)
    return uv.grad[:, :Cout], uv.grad[:, Cout:]


def test_the_bound_of_duv_covers_dv(dev):
    """Mode "f16x3" with C a multiple of 128: the backward passes leave the bound of duv for the two products that read it, and dv now comes
    from the gather.  The inputs make du small while dv is not: all k slots of points 2m and 2m + 1 name point m of their cloud (in-degree
    2k in the lower half of a cloud, 0 in the upper half), there is no activation, and dOut's row 2m + 1 is minus its row 2m -- the two
    selected gz that reach du_m cancel exactly, mean(dz) is zero, and what is left of du is the BatchNorm term of mean(dz yhat), a sum
    of P/2 terms of random sign divided by P k.  The split pieces place the bound in [2^14, 2^15) of f16's 65504 (gemm.hip), so a bound
    more than 4 x too small overflows them: float64 must show max|dv| > 16 max|du| (checked below; 59 measured), and then a bound
    raised from du alone leaves no finite dx or dW.
    The rule of test_edgeconv_backward_f16x3_follows_the_gradient_magnitude: the f16 pieces ran all three products, every output is
    finite, every quantity is at the fp32 bars and within 2 x the fp32 mode's distance.
    Shape: that test's (32, 1024, 128, 256, 20), not a smaller one -- P = 32768 is the smallest row count at which the dgrad (P x 128 x 512)
    and the wgrad (512 x 128 x P) go to the split kernel at all (gemm_plan.h: 256 output tiles, or eight K tiles per split-K slice); at
    P = 512 all three products stay on the fp32 kernel and nothing reads the bound."""
    B, N, C, Cout, k = 32, 1024, 128, 256, 20
    x, idx, W, gamma, beta, rm, rv, dOut = _edgeconv_inputs(B, N, C, Cout, k, seed=23)
    idx = (torch.arange(N) // 2).view(1, N, 1).expand(B, N, k).contiguous().to(dev)
    dOut = torch.stack((dOut[0::2], -dOut[0::2]), dim=1).view(B * N, Cout)
    got = {mode: _edgeconv_gpu(dev, x, idx, W, gamma, beta, rm, rv, True, dOut, act=0, mode=mode) for mode in ("fp32", "f16x3")}
    want = _edgeconv_f64(x, idx, W, gamma, beta, rm, rv, True, dOut, act=0)
    du, dv = _duv_f64(x, idx, W, gamma, beta, want["sel"], dOut)
    print("edge passes bound: float64 max|du| %.3e max|dv| %.3e" % (du.abs().max().item(), dv.abs().max().item()))
    assert dv.abs().max().item() > 16 * du.abs().max().item()
    assert int(got["f16x3"]["kinds"][13]) == 3 and int(got["fp32"]["kinds"][13]) == 0, (got["f16x3"]["kinds"], got["fp32"]["kinds"])
    err = {}
    for mode, r in got.items():
        assert torch.equal(r["sel"].long(), want["sel"]), mode
        assert all(torch.isfinite(r[n]).all() for n in ("out", "dx", "dW", "dgamma", "dbeta", "run_mean", "run_var")), mode
        err[mode] = _edgeconv_errors(r, want)
        print("edge passes bound", mode, " ".join("%s %.1e/%.1e" % (n, *e) for n, e in err[mode].items()))
    for name, (l2, mx) in err["f16x3"].items():
        assert l2 <= _EC_L2 and mx <= _EC_MAX, (name, l2, mx)
        assert l2 <= 2 * err["fp32"][name][0] + 1e-9 and mx <= 2 * err["fp32"][name][1] + 1e-8, (name, err["f16x3"][name], err["fp32"][name])


def test_two_calls_agree_to_the_bit(dev):
    """the fused passes keep a fixed summation order: two identical calls, every output equal"""
    B, N, C, Cout, k = 2, 512, 16, 64, 20
    x, idx, W, gamma, beta, rm, rv, dOut = _edgeconv_inputs(B, N, C, Cout, k, seed=3, dyadic=False)
    a, b = (_edgeconv_gpu(dev, x, idx.to(dev), W, gamma, beta, rm, rv, True, dOut) for _ in range(2))
    for name in ("out", "dx", "dW", "dgamma", "dbeta", "run_mean", "run_var", "sel"):
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("B,N,k,training", [pytest.param(2, 128, 20, True, id="2-128-20-train"), pytest.param(2, 128, 20, False, id="2-128-20-eval"),
                                            pytest.param(1, 1024, 36, True, id="1-1024-36-train")])
def test_tnet_first_stage_without_selection_buffers(dev, B, N, k, training):
    """Fh.tnet_edge: its first stage calls the forward reduce with null ysel / argsel (it reads s1 and the statistics only).  Against
    the float64 restatement at the bars of tests/test_gpu_tnet.py, in training and in eval mode.  N = 128 reaches edge_reduce_vec_kernel's
    uniform branch, (1, 1024, 36) the template flag of edge_reduce_lds_kernel (k = 36: the wide kernel refuses); the wide kernel's is
    reached by the larger clouds of test_tnet_forward_kernels_vs_float64."""
    inp = tr.dyadic_case(B, N, k, 0, training=training)
    m1, m2 = tr.kink_margins(inp)
    assert m1 >= 0.999 * tr.KINK1 and m2 >= tr.KINK2, (m1, m2)
    got = tg.gpu_run(dev, inp, "fp32")
    tag = "null-buffers %dx%dx%d %s" % (B, N, k, "train" if training else "eval")
    print()
    assert int(got["sel"].max()) < k, tag
    want = tr.reference(inp, got["sel"])
    yard = tr.reference(inp, got["sel"], dtype=torch.float32)
    rows = tg.measure(tag, inp, got, want, yard, True)
    tg.check_selection(tag, inp, got["sel"], want["z"], rows["out"][2])
    if not training:
        for n, t in zip(tr.STATS, inp.rs):
            assert torch.equal(got[n], t), (tag, n)
    bad = [(n, d, bar) for n, (d, _, bar) in rows.items() if not d <= bar]
    assert not bad, (tag, bad)
