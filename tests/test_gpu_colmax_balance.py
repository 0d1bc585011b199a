"""The backward of Fh.pointmlp_colmax where its two sparse products (csrc/colmax.hip: colmax_gather_rows_kernel, one wave per channel and
64-column chunk of Cin with the clouds' rows loaded 16 at a time; colmax_scatter_rows_kernel, whose waves take the entries of a row's list
in batches) can go wrong, at the smallest shapes that show it: one list as long as the whole cloud, lists of length one, Cin around the
64-column chunk of the gather and below the 256-column chunk of the scatter, list lengths that are multiples of the batch and of the 16
waves, and lists that are not.

Everything goes through Fh.pointmlp_colmax forward + backward against the float64 restatement, with the helpers and the bars of
tests/test_gpu_colmax.py: max(floor * 2e-6, 3 x the fp32 yardstick) per quantity, the float64 run given the recorded selection."""
import pytest
import torch

import colmax_restatement as cr
from test_gpu_colmax import check, check_selection, gpu_run, make_inputs, references

pytestmark = pytest.mark.gpu

MODE = "default"
RAGGED = (3, 192, 72, 70)             # Cin = one 64-column chunk + 8 columns, Cout no multiple of the 16 waves


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_case(dev, tag, shape, inp, training=True, wslice=False):
    """one forward + backward, every quantity under its bar -> (got, want)"""
    got = gpu_run(dev, inp, shape, training, MODE, wslice=wslice)
    want, yard = references(inp, shape, training, got)
    tag = "%s %s %s" % (tag, "x".join(map(str, shape)), "train" if training else "eval")
    check_selection(tag, inp, shape, got["sel"], want["Y"])
    check(tag, got, want, yard, training)
    return got, want


def list_lengths(sel, b, N):
    return torch.bincount(sel[b].long(), minlength=N)


def one_row_inputs(shape, seed):
    """the "outlier" family with both clouds given the same outlier point x_r and gamma_c = sign(x_r . W_c): every channel's extreme is
    that point.  (x_r . W_c is N(0, 50^2): a twentieth of the channels would have it inside the other rows' range, so each W_c is moved
    along x_r by 0.05 |x_r| ~ 20 away from zero; the other rows' products move by 0.05 N(0, 1).)"""
    B, N, Cin, Cout = shape
    inp = make_inputs(shape, seed, "outlier")
    Xb = inp["X"].view(B, N, Cin)
    r = Xb.norm(dim=2).argmax(dim=1)
    for b in range(1, B):
        Xb[b, r[b]] = Xb[0, r[0]]
    xr = Xb[0, r[0]]
    p = inp["W"] @ xr
    inp["W"] = inp["W"] + 0.05 * torch.sign(p)[:, None] * (xr / xr.norm())[None, :]
    inp["gamma"] = torch.where(inp["W"] @ xr >= 0, 1.0, -1.0)
    return inp, r


def planted_columns_inputs(shape, seed, cols_per_row):
    """W_c = w_c e_(c % Cin) with w_c > 0 and gamma > 0: channel c selects the row with the largest X[:, c % Cin].  cols_per_row: how many
    consecutive columns have their maximum planted in row 3 * i of every cloud, so that row's list has cols_per_row[i] * Cout / Cin
    channels and the lists follow each other in this order in the sorted entries."""
    B, N, Cin, Cout = shape
    assert sum(cols_per_row) == Cin and Cout % Cin == 0 and 3 * len(cols_per_row) <= N
    inp = make_inputs(shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    W = torch.zeros(Cout, Cin)
    W[torch.arange(Cout), torch.arange(Cout) % Cin] = torch.rand(Cout, generator=g) + 0.5
    inp["W"], inp["gamma"] = W, torch.rand(Cout, generator=g) + 0.5
    Xb = inp["X"].view(B, N, Cin)
    j = 0
    for i, m in enumerate(cols_per_row):
        Xb[:, 3 * i, j:j + m] = 10.0
        j += m
    return inp


def test_every_channel_selects_the_same_row(dev):
    """one list of Cout = 512 entries per cloud: every wave of one workgroup takes 32 of them, the other workgroups of the cloud none"""
    shape = cr.OUTLIER
    B, N, Cin, Cout = shape
    inp, r = one_row_inputs(shape, 31)
    got, want = run_case(dev, "one-row", shape, inp)
    for b in range(B):
        assert int(list_lengths(got["sel"], b, N).max()) == Cout
    first = cr.first_extreme(want["Y"], inp["gamma"])
    assert torch.equal(first, r.view(B, 1).expand(B, Cout)) and torch.equal(got["sel"].long(), first)


def test_every_channel_selects_a_different_row(dev):
    """N = 256 >= Cout = 96 and a point planted per channel (10 W_c / |W_c| towards the channel's extreme, at a row of its own; the other
    channels see 10 |W| N(0, 1) / 8 of it): all lists have length one"""
    shape = (2, 256, 64, 96)
    B, N, Cin, Cout = shape
    inp = make_inputs(shape, 37)
    g = torch.Generator().manual_seed(38)
    Xb = inp["X"].view(B, N, Cin)
    s = torch.where(inp["gamma"] >= 0, 1.0, -1.0)
    for b in range(B):
        rows = torch.randperm(N, generator=g)[:Cout]
        Xb[b, rows] = 10.0 * s[:, None] * inp["W"] / inp["W"].norm(dim=1, keepdim=True)
    got, want = run_case(dev, "distinct", shape, inp)
    for b in range(B):
        assert int(list_lengths(got["sel"], b, N).max()) == 1
    assert torch.equal(got["sel"].long(), cr.first_extreme(want["Y"], inp["gamma"]))


@pytest.mark.parametrize("Cin", [8, 40, 64, 72, 130])
def test_cin_around_the_column_chunk(dev, Cin):
    """Cin below one 64-column chunk, one chunk, a ragged second and a ragged third chunk"""
    shape = (3, 192, Cin, 70)
    run_case(dev, "chunk", shape, make_inputs(shape, 41 + Cin))


def test_weight_column_slice(dev):
    """ldw = Cin + 8"""
    run_case(dev, "ldw", RAGGED, make_inputs(RAGGED, 43), wslice=True)


def test_list_lengths_in_multiples_of_eight(dev):
    """(2, 64, 64, 512): eight channels share each column, so a row given m columns has a list of 8 m entries: lists of exactly 8 (the
    longest a single wave takes), of 16 (one entry per wave) and of 24 ... 96 (whole batches and ragged ones per wave)."""
    shape = (2, 64, 64, 512)
    B, N, Cin, Cout = shape
    cols = [4, 8, 4, 1, 1, 1, 1, 4, 2, 2, 12, 1, 3, 4, 8, 2, 2, 4]
    inp = planted_columns_inputs(shape, 47, cols)
    got, _ = run_case(dev, "aligned", shape, inp)
    for b in range(B):
        n = list_lengths(got["sel"], b, N)
        assert n[n > 0].tolist() == [8 * m for m in cols]


@pytest.mark.parametrize("case", ["ragged", "one-row"])
def test_eval_mode(dev, case):
    """dX is zero-filled, then scattered: every row without a list stays zero"""
    shape = RAGGED if case == "ragged" else cr.OUTLIER
    inp = make_inputs(shape, 53) if case == "ragged" else one_row_inputs(shape, 53)[0]
    got, _ = run_case(dev, "eval " + case, shape, inp, training=False)
    B, N, Cin, _ = shape
    for b in range(B):
        empty = list_lengths(got["sel"], b, N) == 0
        assert empty.any() and not got["dX"].view(B, N, Cin)[b][empty].any()


@pytest.mark.parametrize("training", [True, False])
def test_accumulates_into_a_shared_gradient(dev, training):
    """Fh.fan_out as in test_gpu_colmax.test_grad_accum, the colmax backward second: it adds its rows to the pointmlp's input gradient"""
    from mlsp_amd import functional as Fh
    shape = RAGGED
    B, N, Cin, Cout = shape
    inp = make_inputs(shape, 59)
    g = torch.Generator().manual_seed(60)
    W2, R2 = torch.randn(48, Cin, generator=g) / Cin ** 0.5, torch.randn(B * N, 48, generator=g) * 0.05
    Xg, Wg, gg, bg, W2g = [t.to(dev).requires_grad_(True) for t in (inp["X"], inp["W"], inp["gamma"], inp["beta"], W2)]
    rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
    with Fh.recorded_selections() as rec:
        (a0, a1), acc = Fh.fan_out(Xg, 2)
        o2 = Fh.pointmlp_colmax(a1, Wg, gg, bg, rm, rv, B, N, training=training, grad_accum=acc)
        o1 = Fh.pointmlp(a0, W2g, training=training, grad_accum=acc)
        ((o1 * R2.to(dev)).sum() + (o2 * inp["dOut"].to(dev)).sum()).backward()
    got = dict(out=o2.detach().cpu(), dX=Xg.grad.cpu(), dW=Wg.grad.cpu(), dgamma=gg.grad.cpu(), dbeta=bg.grad.cpu(), run_mean=rm.cpu(),
               run_var=rv.cpu(), sel=rec.sel[0].cpu())
    want, yard = references(inp, shape, training, got)
    want["dX"] = want["dX"] + R2.double() @ W2.double()
    yard["dX"] = yard["dX"] + R2 @ W2
    tag = "accum adds %s" % ("train" if training else "eval")
    check_selection(tag, inp, shape, got["sel"], want["Y"])
    check(tag, got, want, yard, training)


@pytest.mark.parametrize("case", ["one-row", "chunk130"])
def test_two_runs_are_bit_identical(dev, case):
    shape = cr.OUTLIER if case == "one-row" else (3, 192, 130, 70)
    inp = one_row_inputs(shape, 61)[0] if case == "one-row" else make_inputs(shape, 61)
    a, b = (gpu_run(dev, inp, shape, True, MODE) for _ in range(2))
    assert torch.equal(a["sel"], b["sel"])
    for n in ("dX", "dW"):
        assert torch.equal(a[n], b[n]), n
