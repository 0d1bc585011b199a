"""The float64 restatement that tests/test_gpu_tnet.py measures the T-Net per-edge kernels against (tests/tnet_restatement.py), pinned on
the CPU: (a) against the reference's own modules (oracle/ref_torch_modules.py: two Conv2d + BatchNorm2d + LeakyReLU blocks and the max
over k), and the conditions the GPU file's inputs must meet so that fp32 and float64 take the same LeakyReLU branches -- (b) on every
first-layer pre-activation, (c) on the second-layer pre-activation of every selected slot, (d) both in the slope = 0 cases as well."""
import pytest
import torch

import tnet_restatement as tr
from oracle import ref_torch_modules

KEYS = list(dict.fromkeys(tr.input_key(c) for c in tr.CASES.values()))
_refs = {}


def _case(key):
    """the inputs of one row of the case table and their float64 restatement (sel=None), computed once"""
    if key not in _refs:
        name = next(c.name for c in tr.CASES.values() if tr.input_key(c) == key)
        inp = tr.case_inputs(name)
        _refs[key] = (inp, tr.reference(inp))
    return _refs[key]


def _ids(key):
    return "%dx%dx%d-slope%g-%s-%s%s" % (key[:4] + ("train" if key[4] else "eval", key[5], "-neg" if key[6] else ""))


def _stock(inp):
    """the reference's blocks themselves (Conv2d -> BatchNorm2d -> LeakyReLU, twice) on its edge features, then the max over k, in float64"""
    b1, b2 = ref_torch_modules._conv2d_block(6, 64).double(), ref_torch_modules._conv2d_block(64, 128).double()
    x = inp.xp.double().requires_grad_(True)
    for blk, W, g, b, rm, rv in ((b1, inp.W1, inp.g1, inp.b1, inp.rs[0], inp.rs[1]), (b2, inp.W2, inp.g2, inp.b2, inp.rs[2], inp.rs[3])):
        conv, bn, act = blk.conv
        with torch.no_grad():
            conv.weight.copy_(W.double()[:, :, None, None])
            for dst, src in ((bn.weight, g), (bn.bias, b), (bn.running_mean, rm), (bn.running_var, rv)):
                dst.copy_(src.double())
        act.negative_slope = inp.slope
        blk.train(inp.training)
    f = ref_torch_modules.edge_features(x.view(inp.B, inp.N, 3).transpose(2, 1), inp.k, lambda *_: inp.idx)
    out = b2(b1(f)).max(dim=-1)[0].transpose(2, 1).reshape(inp.B * inp.N, 128)
    out.backward(inp.w.double())
    p1, p2 = b1.conv, b2.conv
    res = dict(out=out.detach(), dx=x.grad, dW1=p1[0].weight.grad[:, :, 0, 0], dg1=p1[1].weight.grad, db1=p1[1].bias.grad,
               dW2=p2[0].weight.grad[:, :, 0, 0], dg2=p2[1].weight.grad, db2=p2[1].bias.grad, rm1=p1[1].running_mean, rv1=p1[1].running_var,
               rm2=p2[1].running_mean, rv2=p2[1].running_var)
    return res


@pytest.mark.parametrize("key", KEYS, ids=_ids)
def test_restatement_equals_the_reference_modules(key):
    """(a): sel=None -- the value, the seven gradients, the running statistics; forcing its own arg-max changes nothing; the split into
    neighbour and centre shares adds up to dx"""
    inp, ref = _case(key)
    want = _stock(inp)
    for n in ("out",) + tr.GRADS + tr.STATS:
        assert ref[n].shape == want[n].shape and tr.dist(ref[n], want[n]) <= 1e-12, (n, tr.dist(ref[n], want[n]))
    if not inp.training:
        for n, t in zip(tr.STATS, inp.rs):
            assert torch.equal(ref[n], t.double()), n
    act = torch.where(ref["a2"] > 0, ref["a2"], ref["a2"] * inp.slope)
    sel = act.argmax(dim=-1).transpose(2, 1).reshape(inp.B * inp.N, 128)
    forced = tr.reference(inp, sel=sel, split_centre=True)
    for n in ("out",) + tr.GRADS:
        assert tr.dist(forced[n], ref[n]) <= 1e-12, n
    assert not forced["dx_nbr"][inp.deg0].any()


@pytest.mark.parametrize("key", KEYS, ids=_ids)
def test_no_pre_activation_near_the_kink(key):
    """(b), (c), (d): a condition on the inputs, slope = 0 cases included; nothing is masked out of any comparison"""
    inp, ref = _case(key)
    m1, m2 = tr.kink_margins(inp, ref)
    assert m1 >= 0.999 * tr.KINK1, m1           # (beta1 is rounded to fp32: 2^-13 less a rounding of 1e-11)
    assert m2 >= tr.KINK2, m2
    # the same in the yardstick's precision: the first conv's outputs are exact in fp32
    y32 = tr.reference(inp, dtype=torch.float32)["y"]
    assert torch.equal(y32.double(), ref["y"])


def test_restatement_in_fp32_is_close():
    """the yardstick run: the same ops in fp32, with the float64 run's selection forced"""
    inp, ref = _case(KEYS[0])
    sel = ref["a2"].argmax(dim=-1).transpose(2, 1).reshape(inp.B * inp.N, 128)
    yard = tr.reference(inp, sel=sel, dtype=torch.float32)
    assert yard["out"].dtype == torch.float32 and tr.rel_l2(yard["out"], ref["out"]) < 1e-5
    for n in tr.GRADS:
        assert yard[n].dtype == torch.float32 and tr.dist(yard[n], ref[n]) < 1e-4, n


def test_forced_indices_have_degree_zero_points_a_hub_and_repeats():
    inp = tr.case_inputs("forced-k24-dx")
    B, N, k = inp.B, inp.N, inp.k
    assert torch.equal(inp.deg0.view(B, N), (torch.arange(N) >= N // 2).expand(B, N))
    assert (inp.idx[:, :, 0] == 1).all() and torch.equal(inp.idx[:, :, 2], inp.idx[:, :, 1])


def test_case_table_reaches_every_dispatch_row():
    """Every row of the launchers' dispatch ("T-Net test matrix") is some case's path, each case states the path its shape
    and mode take, every multi-point tile is partial, and the tile-walk cases have more tiles than workgroups on either walk."""
    fwd, bwd = set(), set()
    for c in tr.CASES.values():
        mode = tr.resolve_mode(c.mode)
        slope = c.opt.get("slope", 0.2)
        assert tr.fwd_kernel(c.k, mode) == c.fwd and tr.bwd_kernel(c.k, mode, slope) == c.bwd, c.name
        fwd.add(c.fwd)
        bwd.add(c.bwd)
        assert 1 <= c.k <= 128 and c.N > c.k or c.opt.get("graph") == "forced"
        if not c.name.startswith(("forced", "walk-")):         # (the walk cases are sized by their tile counts)
            # (fwd-k40-*: N = 42 leaves 2 of the forward's 4 points; the backward's 3-point tiles are partial in bwdg-k40)
            for t in {tr.points_per_tile(c.k, True)} | ({tr.points_per_tile(c.k)} if not c.name.startswith("fwd-k40") else set()):
                assert t == 1 or c.N % t, c.name
        assert c.B * c.N * c.k <= 70000, c.name
    assert fwd == {"fwd", "fwd2<20>", "fwd2<40>", "fwd3<20>", "fwd3<40>", "fwd3<20,ONEP>", "fwd3<40,ONEP>"}
    assert bwd == {"bwd", "bwds", "bwds<ONEP>", "bwdg<0,20>", "bwdg<0,24>", "bwdg<0,32>", "bwdg<1,40>", "bwdg<2,32>"}
    assert {c.opt.get("xgrad", True) for c in tr.CASES.values()} == {True, False}
    for name, forward, xcd in (("walk-gram-xcd", False, True), ("walk-gram-plain", False, False), ("walk-fwd-xcd", True, True),
                               ("walk-fwd-plain", True, False)):
        c = tr.CASES[name]
        n = tr.tiles(c.B, c.N, c.k)
        assert (c.B % 8 == 0) == xcd and tr.grid(n, gram=not forward) < n <= tr.grid(n, gram=not forward) + 16, (name, n)
