"""Fh.tnet_edge (csrc/tnet.hip: launch_tnet_edge_fwd / launch_tnet_edge_bwd and what follows them) against its float64 restatement
(tests/tnet_restatement.py) on every kernel the two launchers choose among.  The case table, with the kernel each case reaches, is
tr.CASES ("T-Net test matrix"); tests/test_tnet_restatement_cpu.py checks the table and the inputs on the CPU.

Every case: the GPU run records its own arg-max slots (Fh.recorded_selections); every slot is < k and names a value within the forward
bar x the channel's range of float64's extreme of z (the maximum where gamma2 >= 0, the minimum otherwise); the float64 run is given
those slots, so every element of every quantity is compared and nothing is excluded.

Distance: relative L2 for forward values (out, the running statistics), max|a - b| / max|b| for gradients.  Modes "fp32", "bf16x6" and
"f16x3": bar = max(project bar, 3 x yardstick), project bar 4e-7 forward and 1e-4 backward (test_tnet_forward_kernels_vs_float64,
test_tnet_backward_kernels_vs_float64 in tests/test_gpu_kernels.py), yardstick = the restatement in fp32 on the CPU with the same slots
against float64; 3 because the summation order differs.  Mode "bf16" (operands rounded to bf16: 2^-9 per value): the method of
test_tnet_edge_bf16_operands_vs_fp32_products -- the forward against the "bf16x6" forward, and the SAME "bf16" forward taken back once
with single and once with six products: below 1e-2, and above 1e-5 where operands really were rounded.
Measured distances: profiles/tnet_float64_distances.txt."""
import contextlib

import pytest
import torch

import tnet_restatement as tr

pytestmark = pytest.mark.gpu

FWD_BAR, BWD_BAR = 4e-7, 1e-4
BF16_BAR, BF16_FLOOR = 1e-2, 1e-5
SPECIAL = ("forced-", "repro-")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mlsp_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def gpu_run(dev, inp, mode, xgrad=True, bwd_mode=None):
    """One forward + backward of Fh.tnet_edge in product mode `mode` ("default": the process default); bwd_mode: the backward's products
    (the Function hands its forward's mode to its backward: overridden).  -> dict of CPU tensors: out, sel, the gradients (dx: None without
    xgrad), the running statistics after the call."""
    from mlsp_amd import _lib, functional as Fh
    leaves = [t.to(dev).requires_grad_(xgrad or i > 0) for i, t in enumerate((inp.xp, inp.W1, inp.g1, inp.b1, inp.W2, inp.g2, inp.b2))]
    rs = [t.clone().to(dev) for t in inp.rs]
    graph = Fh.graph_from_indices(inp.idx.to(dev), inp.B, inp.N, inp.k)
    with contextlib.nullcontext() if mode == "default" else Fh.gemm_precision(mode), Fh.recorded_selections() as rec:
        out = Fh.tnet_edge(leaves[0], graph, leaves[1], leaves[2], leaves[3], rs[0], rs[1], leaves[4], leaves[5], leaves[6], rs[2], rs[3],
                           inp.training, slope=inp.slope)
    assert out.grad_fn.prec == _lib.GEMM_PRECISION_MODES[tr.resolve_mode(mode)]
    if bwd_mode is not None:
        out.grad_fn.prec = _lib.GEMM_PRECISION_MODES[bwd_mode]
    out.backward(inp.w.to(dev))
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu(), sel=rec.sel[0].cpu())
    res.update(zip(tr.GRADS, (None if t.grad is None else t.grad.cpu() for t in leaves)))
    res.update(zip(tr.STATS, (t.cpu() for t in rs)))
    assert (res["dx"] is None) == (not xgrad)
    return res


def check_selection(tag, inp, sel, z, bar):
    """sel [P, 128] uint8, z [B, 128, N, k] (float64, pre-BN): every slot < k; the value at the slot within bar x (the channel's range) of the
    channel's extreme over the point's k edges"""
    B, N, k = inp.B, inp.N, inp.k
    sel = sel.long()
    assert sel.shape == (B * N, 128) and int(sel.max()) < k, (tag, int(sel.max()), k)
    zs = z * torch.where(inp.g2 >= 0, 1.0, -1.0).double().view(1, 128, 1, 1)
    at = zs.gather(-1, sel.view(B, N, 128).transpose(2, 1)[..., None])[..., 0]
    short = zs.max(dim=-1)[0] - at
    rng = (z.amax(dim=(0, 2, 3)) - z.amin(dim=(0, 2, 3))).view(1, 128, 1)
    worst = (short / rng).max().item()
    print("tnet %s selection shortfall %.3e of the range, bar %.3e" % (tag, worst, bar))
    assert worst <= bar, (tag, worst, bar)


def measure(tag, inp, got, want, yard, xgrad):
    """prints one line per quantity -- distance, yardstick, bar; -> {quantity: (distance, yardstick, bar)}"""
    rows = {}
    names = ("out",) + (tr.STATS if inp.training else ()) + tr.GRADS[0 if xgrad else 1:]
    for n in names:
        assert got[n].shape == want[n].shape and torch.isfinite(got[n]).all(), (tag, n)
        fwd = n == "out" or n in tr.STATS
        d, y = (tr.rel_l2 if fwd else tr.dist)(got[n], want[n]), (tr.rel_l2 if fwd else tr.dist)(yard[n], want[n])
        rows[n] = (d, y, max(FWD_BAR if fwd else BWD_BAR, 3 * y))
        print("tnet %s %-4s distance %.3e  yardstick %.3e  bar %.3e" % ((tag, n) + rows[n]))
    return rows


def case_tag(c, inp):
    return "%s %dx%dx%d %s[%s] slope %g %s -> %s" % (c.name, c.B, c.N, c.k, "train" if inp.training else "eval", c.mode, inp.slope, c.fwd, c.bwd)


def assert_path(c, inp):
    """the kernels this case's shape, slope and product mode reach, from the launchers' conditions"""
    mode = tr.resolve_mode(c.mode)
    assert (c.k, inp.slope) == (inp.k, c.opt.get("slope", 0.2))
    assert tr.fwd_kernel(c.k, mode) == c.fwd and tr.bwd_kernel(c.k, mode, inp.slope) == c.bwd, (c.name, mode)


def against_float64(dev, name, split_centre=False):
    """modes "fp32", "bf16x6", "f16x3": the whole procedure for one case -> (inp, got, want)"""
    c = tr.CASES[name]
    inp = tr.case_inputs(name)
    assert_path(c, inp)
    xgrad = c.opt.get("xgrad", True)
    got = gpu_run(dev, inp, c.mode, xgrad)
    tag = case_tag(c, inp)
    print()
    assert int(got["sel"].max()) < inp.k, tag                      # before anything indexes with it
    want = tr.reference(inp, got["sel"], split_centre=split_centre)
    yard = tr.reference(inp, got["sel"], dtype=torch.float32)
    rows = measure(tag, inp, got, want, yard, xgrad)
    check_selection(tag, inp, got["sel"], want["z"], rows["out"][2])
    if not inp.training:
        for n, t in zip(tr.STATS, inp.rs):
            assert torch.equal(got[n], t), (tag, n)                 # eval mode leaves the running statistics alone
    bad = [(n, d, bar) for n, (d, _, bar) in rows.items() if not d <= bar]
    assert not bad, (tag, bad)
    return inp, got, want


def bf16_against_six_products(dev, name):
    """mode "bf16" -> (one, six): the runs with single and with six products in the backward"""
    c = tr.CASES[name]
    inp = tr.case_inputs(name)
    assert_path(c, inp)
    tag = case_tag(c, inp)
    ref_f, one, six = gpu_run(dev, inp, "bf16x6"), gpu_run(dev, inp, "bf16"), gpu_run(dev, inp, "bf16", bwd_mode="bf16x6")
    print()
    assert torch.equal(one["out"], six["out"]) and torch.equal(one["sel"], six["sel"]), tag
    rel_out = tr.rel_l2(one["out"], ref_f["out"])
    print("tnet %s out  against the bf16x6 forward %.3e" % (tag, rel_out))
    assert rel_out < BF16_BAR, (tag, rel_out)
    if "ONEP" in c.fwd:                                             # (any other k: one forward kernel for every mode)
        assert rel_out > BF16_FLOOR, (tag, rel_out)
    check_selection(tag, inp, one["sel"], tr.reference(inp)["z"], BF16_BAR)
    for n in tr.GRADS:
        assert torch.isfinite(one[n]).all(), (tag, n)
        rel = tr.rel_l2(one[n], six[n])
        print("tnet %s %-4s single against six products %.3e" % (tag, n, rel))
        assert rel < BF16_BAR, (tag, n, rel)
        if n == "dW2":
            assert rel > BF16_FLOOR, (tag, n, rel)
    return one, six


@pytest.mark.parametrize("name", [n for n in tr.CASES if not n.startswith(SPECIAL)])
def test_case(dev, name):
    """every launch path: the bwdg instantiations at both ends of their k ranges, bwds with three products and one, the round-1 kernel, the
    forward kernels on partial tiles, both tile walks past the grid caps, negative BatchNorm scales, eval mode, a small slope"""
    if tr.resolve_mode(tr.CASES[name].mode) == "bf16":
        bf16_against_six_products(dev, name)
    else:
        against_float64(dev, name)


@pytest.mark.parametrize("name", [n for n in tr.CASES if n.startswith("forced-")])
def test_forced_indices(dev, name):
    """indices from the first half of each cloud, one hub point in every row, a repeated entry per row: with a gradient on x
    (tnet_edge_bwd2_kernel over the reverse index) and without (tnet_bwd_tmom / xmom / w1_finish).  The dx rows of the points that are
    nobody's neighbour carry their centre share only."""
    inp, got, want = against_float64(dev, name, split_centre=True)
    deg0 = inp.deg0
    assert int(deg0.sum()) == inp.B * (inp.N - inp.N // 2)
    assert not want["dx_nbr"][deg0].any()
    if got["dx"] is not None:
        d = ((got["dx"][deg0].double() - want["dx_ctr"][deg0]).abs().max() / want["dx"].abs().max()).item()
        print("tnet %s dx of degree-0 points against their centre share %.3e" % (name, d))
        assert d <= BWD_BAR, (name, d)


@pytest.mark.parametrize("name", [n for n in tr.CASES if n.startswith("repro-")])
def test_bit_reproducible(dev, name):
    """the file states a fixed summation order: two identical calls agree to the bit"""
    inp, a, _ = against_float64(dev, name)
    b = gpu_run(dev, inp, tr.CASES[name].mode)
    for n in ("out", "sel") + tr.GRADS + tr.STATS:
        assert torch.equal(a[n], b[n]), (name, n)
