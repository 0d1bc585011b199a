"""mlsp_amd.optim with several parameter groups and with AdamW: FlatAdamW / FlatAdam / FlatSGD over the reference's "no weight decay on
BatchNorm and biases" split (utils/optimizer.py add_weight_decay), per-group learning rates and options, against torch.optim.AdamW(fused=True) /
Adam(fused=True) / SGD step by step: ONE launch per step (flat_steps), bit-identical parameters and state, one step counter per group."""
import copy
import warnings

import pytest
import torch
from torch import nn

import golden_common as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _Net(nn.Module):
    """a used trunk with BatchNorm, a head that never runs (no gradient, never stepped, no state), a late head, a tensor that does not end
    on a tile boundary, parameters of 1 / 3 / 2048 / 2049 elements (one lane, an unaligned tail, exactly one 2048-element tile, one tile
    plus one element) and, with `many`, 100 five-element vectors (more than the 96 segments of one launch)"""

    def __init__(self, many=False):
        super().__init__()
        self.a = nn.Linear(37, 129)
        self.bn = nn.BatchNorm1d(129)
        self.unused = nn.Linear(129, 5)
        self.b = nn.Linear(129, 70001 // 129)
        self.late = nn.Linear(129, 3)
        self.one = nn.Parameter(torch.randn(1, 1))             # 2-D: decayed
        self.three = nn.Parameter(torch.randn(3))
        self.tile = nn.Parameter(torch.randn(2048))
        self.tile1 = nn.Parameter(torch.randn(1, 2049))        # 2-D: decayed
        self.vecs = nn.ParameterList([nn.Parameter(torch.randn(5)) for _ in range(100)]) if many else None

    def forward(self, x, late=False):
        h = torch.relu(self.bn(self.a(x)))
        out = self.b(h).sum()
        extras = [self.one, self.three, self.tile, self.tile1] + (list(self.vecs) if self.vecs is not None else [])
        out = out + h.mean() * sum((p * p).sum() for p in extras)
        return out + self.late(h).sum() if late else out


def _no_decay(name, p):
    return p.dim() == 1 or name.endswith(".bias")                # the reference's add_weight_decay


def _split(m, wd, skip=(), **decayed):
    named = [(n, p) for n, p in m.named_parameters() if not n.startswith(tuple(skip))]
    return [dict(params=[p for n, p in named if _no_decay(n, p)], weight_decay=0.0),
            dict(params=[p for n, p in named if not _no_decay(n, p)], weight_decay=wd, **decayed)]


def _groups(m, cfg):
    """the parameter groups of configuration `cfg` for model m (m.parameters() for the one-group case)"""
    if cfg == "a_one_group":
        return list(m.parameters())
    if cfg == "b_two_groups":
        return _split(m, 1e-2)
    if cfg == "c_three_groups":                                  # different lr / betas / eps; the third holds only the head that never runs
        g = _split(m, 1e-2, skip=("unused.",), lr=3e-3, betas=(0.8, 0.99), eps=1e-6)
        g[0].update(lr=5e-4, betas=(0.95, 0.9999), eps=1e-10)
        return g + [dict(params=list(m.unused.parameters()), lr=1e-2, betas=(0.5, 0.9), eps=1e-3)]
    if cfg == "d_momentum_0.9_and_0":
        g = _split(m, 5e-5, momentum=0.9)
        g[0]["momentum"] = 0.0
        return g
    if cfg == "e_nesterov_on_and_off":
        g = _split(m, 5e-5, nesterov=True)
        g[0]["nesterov"] = False
        return g
    assert cfg == "f_hundred_vectors"                            # the list alternately over two groups, the rest with the first
    vecs = list(m.vecs)
    rest = [p for n, p in m.named_parameters() if not n.startswith("vecs.")]
    return [dict(params=rest + vecs[0::2], weight_decay=0.0), dict(params=vecs[1::2], weight_decay=1e-2, lr=4e-3)]


def _make(kind, groups, ours):
    from mlsp_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    if kind == "adamw":
        return FlatAdamW(groups, lr=1e-3, weight_decay=1e-2) if ours else torch.optim.AdamW(groups, lr=1e-3, weight_decay=1e-2, fused=True)
    if kind == "adam":
        return FlatAdam(groups, lr=1e-3, weight_decay=5e-5) if ours else torch.optim.Adam(groups, lr=1e-3, weight_decay=5e-5, fused=True)
    return (FlatSGD if ours else torch.optim.SGD)(groups, lr=2e-2, momentum=0.9, weight_decay=5e-5)


def _pair(dev, many=False):
    torch.manual_seed(3)
    m1 = _Net(many).to(dev)
    m2 = copy.deepcopy(m1)
    return m1, m2


def _same(m1, o1, m2, o2):
    """bit-identical parameters and state tensors, the same step count per parameter (so per group); no state where torch has none"""
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), (n, (p != q).sum().item(), p.numel())
        s1, s2 = o1.state.get(p, {}), o2.state.get(q, {})
        assert set(s1) == set(s2), (n, set(s1), set(s2))
        for k in s2:
            if k == "step":
                assert float(s1[k]) == float(s2[k]), (n, float(s1[k]), float(s2[k]))
            else:
                assert torch.equal(s1[k], s2[k]), (n, k, (s1[k] != s2[k]).sum().item())


def _x(dev, it, rows=64):
    return torch.randn(rows, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(it))


def _step(m, o, x, late=False):
    o.zero_grad()
    m(x, late=late).backward()
    o.step()


CASES = [("adamw", "a_one_group"), ("adamw", "b_two_groups"), ("adam", "b_two_groups"), ("sgd", "b_two_groups"),
         ("adamw", "c_three_groups"), ("adam", "c_three_groups"), ("sgd", "d_momentum_0.9_and_0"), ("sgd", "e_nesterov_on_and_off"),
         ("adamw", "f_hundred_vectors"), ("adam", "f_hundred_vectors"), ("sgd", "f_hundred_vectors")]


@pytest.mark.parametrize("kind,cfg", CASES, ids=["%s-%s" % c for c in CASES])
def test_grouped_flat_step_is_bit_identical_to_torch(dev, kind, cfg):
    """six steps under CosineAnnealingLR (it scales every group's lr): one launch per step, one layout, torch's results bit for bit"""
    m1, m2 = _pair(dev, many=cfg == "f_hundred_vectors")
    o1, o2 = _make(kind, _groups(m1, cfg), True), _make(kind, _groups(m2, cfg), False)
    assert isinstance(o1, type(o2))
    s1, s2 = torch.optim.lr_scheduler.CosineAnnealingLR(o1, 10), torch.optim.lr_scheduler.CosineAnnealingLR(o2, 10)
    for it in range(6):
        x = _x(dev, it)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)       # (the hand-over to torch's path warns)
            for m, o, s in ((m1, o1, s1), (m2, o2, s2)):
                _step(m, o, x)
                s.step()
        assert [g["lr"] for g in o1.param_groups] == [g["lr"] for g in o2.param_groups]
        _same(m1, o1, m2, o2)
    assert o1.flat_steps == 6 and o1.layouts_built == 1
    assert not o1.state.get(m1.unused.weight) and not o1.state.get(m1.late.bias)
    if kind != "sgd":                                             # one device-side counter per group that steps, shared by its parameters
        for g in o1.param_groups:
            ptrs = {o1.state[p]["step"].data_ptr() for p in g["params"] if o1.state.get(p)}
            assert len(ptrs) <= 1
    if cfg == "d_momentum_0.9_and_0":
        assert not any(o1.state.get(p) for p in o1.param_groups[0]["params"])
        assert all("momentum_buffer" in o1.state[p] for p in o1.param_groups[1]["params"] if p.grad is not None)


def test_parameters_of_one_storage_in_different_groups(dev):
    """two Parameter views of one tensor, back to back (what functional.rehome_adjacent makes of merged layers; the bias of such a layer
    sits in the no-decay group): the flat layout keeps their distance, and each steps with its own group's weight decay"""
    from mlsp_amd.optim import FlatAdamW
    torch.manual_seed(5)
    base = torch.randn(129 * 37 + 129, device=dev) * 0.1
    w1, b1 = nn.Parameter(base[:129 * 37].view(129, 37)), nn.Parameter(base[129 * 37:])
    assert b1.data_ptr() - w1.data_ptr() == 4 * 129 * 37 and w1.untyped_storage().data_ptr() == b1.untyped_storage().data_ptr()
    w2, b2 = nn.Parameter(w1.detach().clone()), nn.Parameter(b1.detach().clone())
    o1 = FlatAdamW([dict(params=[w1], weight_decay=1e-2), dict(params=[b1], weight_decay=0.3, lr=2e-3)], lr=1e-3)
    o2 = torch.optim.AdamW([dict(params=[w2], weight_decay=1e-2), dict(params=[b2], weight_decay=0.3, lr=2e-3)], lr=1e-3, fused=True)
    for it in range(4):
        x = _x(dev, it)
        for w, b, o in ((w1, b1, o1), (w2, b2, o2)):
            o.zero_grad()
            torch.nn.functional.linear(x, w, b).pow(2).sum().backward()
            o.step()
        assert torch.equal(w1, w2) and torch.equal(b1, b2), it
        assert b1.data_ptr() - w1.data_ptr() == 4 * 129 * 37
    f = o1._flat
    assert o1.flat_steps == 4 and o1.layouts_built == 1
    assert f["offs"][1] - f["offs"][0] == 129 * 37 and list(f["seg_group"]) == [0, 1]
    # (the decay is what separates the groups: with the other group's value the bias would have moved elsewhere)
    assert torch.equal(o1.state[b1]["exp_avg"], o2.state[b2]["exp_avg"])


def _steps_of(sd):
    return {k: float(v["step"]) for k, v in sd["state"].items()}


def test_flat_adamw_state_dict_is_interchangeable_with_torch_adamw(dev):
    from mlsp_amd.optim import FlatAdamW
    m1, m2 = _pair(dev)
    o1, o2 = _make("adamw", _groups(m1, "b_two_groups"), True), _make("adamw", _groups(m2, "b_two_groups"), False)
    for it in range(3):
        _step(m1, o1, _x(dev, it))
        _step(m2, o2, _x(dev, it))
    _same(m1, o1, m2, o2)
    sd1, sd2 = copy.deepcopy(o1.state_dict()), copy.deepcopy(o2.state_dict())
    assert sd1["param_groups"] == sd2["param_groups"]
    assert sorted(sd1["state"]) == sorted(sd2["state"]) and all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in sd1["state"].values())
    m3, m4 = copy.deepcopy(m2), copy.deepcopy(m2)
    o3 = _make("adamw", _groups(m3, "b_two_groups"), False)
    o3.load_state_dict(sd1)                                   # FlatAdamW -> torch
    o4 = _make("adamw", _groups(m4, "b_two_groups"), True)
    o4.load_state_dict(sd2)                                   # torch -> FlatAdamW
    for it in range(3, 6):
        for m, o in ((m1, o1), (m2, o2), (m3, o3), (m4, o4)):
            _step(m, o, _x(dev, it))
        _same(m1, o1, m2, o2)
        _same(m3, o3, m2, o2)
        _same(m4, o4, m2, o2)
    assert isinstance(o4, FlatAdamW) and o1.flat_steps == 6 and o4.flat_steps == 3


def test_loaded_state_with_groups_at_different_steps(dev):
    """a step count per GROUP is what the flat step keeps: loaded state whose groups are at different steps stays on the flat path, state
    with two step counts inside one group goes to torch's per-tensor path; identical to torch either way"""
    m0, m2 = _pair(dev)
    o2 = _make("adamw", _groups(m2, "b_two_groups"), False)
    for it in range(3):
        _step(m2, o2, _x(dev, it))
    sd = copy.deepcopy(o2.state_dict())
    group1 = set(sd["param_groups"][1]["params"])
    for k, v in sd["state"].items():
        if k in group1:
            v["step"] = v["step"] + 7.0                       # group 1 at step 10, group 0 at step 3
    for inside_one_group in (False, True):
        sdx = copy.deepcopy(sd)
        if inside_one_group:
            k = sorted(group1 & set(sdx["state"]))[0]
            sdx["state"][k]["step"] = sdx["state"][k]["step"] - 2.0
        ma, mb = copy.deepcopy(m2), copy.deepcopy(m2)
        oa, ob = _make("adamw", _groups(ma, "b_two_groups"), True), _make("adamw", _groups(mb, "b_two_groups"), False)
        oa.load_state_dict(copy.deepcopy(sdx))
        ob.load_state_dict(copy.deepcopy(sdx))
        for it in range(3, 6):
            _step(ma, oa, _x(dev, it))
            _step(mb, ob, _x(dev, it))
            _same(ma, oa, mb, ob)
        assert oa.flat_steps == (0 if inside_one_group else 3), inside_one_group
        want = {3.0 + 3, 10.0 + 3} | ({8.0 + 3} if inside_one_group else set())
        assert set(_steps_of(oa.state_dict()).values()) == want


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_add_param_group_after_two_steps(dev, kind):
    """the late head joins as a third group after two steps: ONE rebuild of the layout, the existing state carried over, the new group's
    counter starts at 0 (its first update is step 1)"""
    m1, m2 = _pair(dev)
    o1, o2 = (_make(kind, _split(m, 1e-2, skip=("late.", "unused.")), ours) for m, ours in ((m1, True), (m2, False)))
    for it in range(5):
        if it == 2:
            for m, o in ((m1, o1), (m2, o2)):
                o.add_param_group(dict(params=list(m.late.parameters()), lr=5e-3, weight_decay=0.1))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            _step(m1, o1, _x(dev, it), late=it >= 2)
            _step(m2, o2, _x(dev, it), late=it >= 2)
        _same(m1, o1, m2, o2)
        assert o1.layouts_built == (1 if it < 2 else 2)
    assert o1.flat_steps == 5 and len(o1.param_groups) == 3
    if kind == "adamw":
        assert float(o1.state[m1.late.weight]["step"]) == 3.0 and float(o1.state[m1.a.weight]["step"]) == 5.0
    base, n = o1._flat["p"].data_ptr(), o1._flat["p"].numel()
    assert all(base <= p.data_ptr() < base + 4 * n for g in o1.param_groups for p in g["params"])


def test_more_than_eight_groups_hand_over_to_torch(dev):
    """nine groups: torch's own path from the first step, same results"""
    m1, m2 = _pair(dev)
    mk = lambda m: [dict(params=[p], weight_decay=1e-3 * i) for i, p in enumerate(list(m.parameters())[:9])]
    o1, o2 = _make("adamw", mk(m1), True), _make("adamw", mk(m2), False)
    for it in range(2):
        _step(m1, o1, _x(dev, it))
        _step(m2, o2, _x(dev, it))
        _same(m1, o1, m2, o2)
    assert o1.flat_steps == 0


def _dgcnn(dev, seed=3):
    from mlsp_amd import Models
    torch.manual_seed(seed)
    return Models.DGCNN(gc.make_args(cuda=True)).to(dev).train()


def _dgcnn_backward(m, x):
    out = m(x, activate_density_normal_ondef=True)
    sum(v.float().sum() for v in out.values()).backward()


def test_two_group_step_publishes_weight_bounds(dev):
    """tiles are numbered segment by segment in address order whatever the groups: after a two-group step weight_bounds hands a GEMM the
    tiles of a decayed weight (maxima that bound |W| and are reached by it) and one run of tiles for the merged first-layer operand, whose
    neighbours' biases live in the other group; withdrawn after a write torch sees"""
    from mlsp_amd import functional as Fh, _lib
    from mlsp_amd.optim import FlatAdamW
    m = _dgcnn(dev)
    opt = FlatAdamW(_split(m, 1e-2), lr=1e-3)
    x = (torch.rand(2, 3, 128, device=dev) * 2 - 1)
    assert opt.weight_bounds(m.conv5.weight.view(1024, -1)) is None        # nothing published before the first step
    for _ in range(2):
        opt.zero_grad()
        _dgcnn_backward(m, x)
        opt.step()
    assert opt.flat_steps == 2 and opt in _lib.weight_bound_providers
    assert any(p is m.conv5.weight for p in opt.param_groups[1]["params"])
    W5 = m.conv5.weight.view(1024, -1)
    ptr, n = opt.weight_bounds(W5)
    f = opt._flat
    t0 = (ptr - f["tile_amax"].data_ptr()) // 4
    j = [f["params"][i] is m.conv5.weight for i in opt._active].index(True)
    assert (t0, t0 + n) == (f["tile_begin"][j], f["tile_begin"][j + 1]) and n == (W5.numel() + 2047) // 2048
    assert f["tile_amax"][t0:t0 + n].max().item() == W5.abs().max().item()
    Wm = Fh.row_blocks([h.conv1.weight.view(h.conv1.out_channels, -1) for h in (m.DefRec, m.Norm_pred, m.Density_cls)], rehome=False)
    r = opt.weight_bounds(Wm[:, :512])
    assert r is not None and r[1] > 1
    t0 = (r[0] - f["tile_amax"].data_ptr()) // 4
    assert f["tile_amax"][t0:t0 + r[1]].max().item() >= Wm[:, :512].abs().max().item()
    with torch.no_grad():
        m.conv5.weight.mul_(1.5)                                            # torch sees this write: conv5's bounds are withdrawn ...
    assert opt.weight_bounds(m.conv5.weight.view(1024, -1)) is None
    assert opt.weight_bounds(Wm[:, :512]) is not None                       # ... the others stand
    opt.invalidate_bounds()
    assert opt.weight_bounds(Wm[:, :512]) is None


def test_two_group_step_reads_the_exchange_bucket_in_place(dev):
    """with FlatGradSync the step reads the packed (all-reduced) gradients where the bucket holds them, whatever their groups"""
    from mlsp_amd.ddp import FlatGradSync
    m1, m2 = _pair(dev)
    sync = FlatGradSync(m1, force=True, align=4)
    o1 = sync.wrap(_make("sgd", _groups(m1, "d_momentum_0.9_and_0"), True))
    o2 = _make("sgd", _groups(m2, "d_momentum_0.9_and_0"), False)
    for it in range(3):
        _step(m1, o1, _x(dev, it))
        _step(m2, o2, _x(dev, it))
        _same(m1, o1, m2, o2)
        lo, hi = sync.flat.data_ptr(), sync.flat.data_ptr() + 4 * sync.flat.numel()
        assert all(p.grad is None or lo <= p.grad.data_ptr() < hi for p in m1.parameters())
    assert o1.flat_steps == 3


def test_flat_adamw_steps_dgcnn_like_torch_adamw(dev):
    """Models.DGCNN with the three heads active and the reference's split -- the merged heads' weights and their biases are parameters of
    ONE storage in different groups -- four FlatAdamW steps against torch.optim.AdamW(fused=True) on a copy of the model that is fed the
    SAME gradient tensors (so the forward's rounding does not enter): bit-identical parameters, one launch per step"""
    from mlsp_amd import functional as Fh
    from mlsp_amd.optim import FlatAdamW
    m1 = _dgcnn(dev)
    m2 = copy.deepcopy(m1)
    o1 = FlatAdamW(_split(m1, 1e-2), lr=1e-3)
    o2 = torch.optim.AdamW(_split(m2, 1e-2), lr=1e-3, fused=True)
    s1, s2 = torch.optim.lr_scheduler.CosineAnnealingLR(o1, 10), torch.optim.lr_scheduler.CosineAnnealingLR(o2, 10)
    for it in range(4):
        x = torch.rand(2, 3, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(it)) * 2 - 1
        o1.zero_grad()
        _dgcnn_backward(m1, x)
        for p, q in zip(m1.parameters(), m2.parameters()):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        o1.step()
        o2.step()
        s1.step()
        s2.step()
        _same(m1, o1, m2, o2)
    assert o1.flat_steps == 4
    # the merged first layers stayed adjacent in one storage although their members belong to different groups
    heads = (m1.DefRec, m1.Norm_pred, m1.Density_cls)
    assert Fh._adjacent([h.conv1.weight for h in heads]) and Fh._adjacent([h.bn1.weight for h in heads])
    gid = {id(p): g for g, grp in enumerate(o1.param_groups) for p in grp["params"]}
    assert {gid[id(h.conv1.weight)] for h in heads} == {1} and {gid[id(h.bn1.weight)] for h in heads} == {0}
    assert o1.layouts_built <= 2


@pytest.mark.parametrize("which", ["adam", "sgd", "sgd_first"])
def test_one_group_entry_points_equal_the_group_entry_points(dev, which):
    """mlsp_adam_flat_f32 / mlsp_sgd_flat_f32 keep their signatures and results: one step through each equals one step through the
    groups entry point with a single group (which the tests above hold to torch), on an aligned segment of one tile plus a tail and an
    unaligned segment -- parameters, state, step counter and tile maxima, bit for bit"""
    import ctypes
    from mlsp_amd import _lib
    lib = _lib.load()
    offs, numels = [0, 2117], [2051, 130]                        # the second segment starts off 16 bytes: the element-wise path
    n = 2304
    gen = torch.Generator(device=dev).manual_seed(11)
    P0, M0, B0 = (torch.randn(n, device=dev, generator=gen) * s for s in (0.1, 0.01, 0.01))
    V0 = torch.rand(n, device=dev, generator=gen) * 1e-4
    grads = [torch.randn(k, device=dev, generator=gen) * 0.01 for k in numels]
    off, numel = (ctypes.c_uint32 * 2)(*offs), (ctypes.c_uint32 * 2)(*numels)
    gp = (ctypes.c_void_p * 2)(*[g.data_ptr() for g in grads])
    lr, wd, step = 7.3e-4, 5e-5, 3
    out = []
    for grouped in (False, True):
        P, M, V, B = P0.clone(), M0.clone(), V0.clone(), B0.clone()
        amax, step_out = torch.zeros(3, device=dev), torch.zeros((), device=dev)
        if which == "adam":
            if grouped:
                t = (_lib.MlspAdamGroup * 1)()
                t[0].lr, t[0].beta1, t[0].beta2, t[0].weight_decay, t[0].eps, t[0].step, t[0].decoupled = lr, 0.9, 0.999, wd, 1e-8, step, 0
                t[0].step_out = step_out.data_ptr()
                rc = lib.mlsp_adam_flat_groups_f32(P.data_ptr(), M.data_ptr(), V.data_ptr(), off, numel, gp, None, 2, t, 1, amax.data_ptr(),
                                                   _lib.stream())
            else:
                rc = lib.mlsp_adam_flat_f32(P.data_ptr(), M.data_ptr(), V.data_ptr(), off, numel, gp, 2, lr, 0.9, 0.999, wd, 1e-8, step,
                                            step_out.data_ptr(), amax.data_ptr(), _lib.stream())
        else:
            first = int(which == "sgd_first")
            if grouped:
                t = (_lib.MlspSgdGroup * 1)()
                t[0].lr, t[0].momentum, t[0].dampening, t[0].weight_decay, t[0].nesterov, t[0].maximize, t[0].first = lr, 0.9, 0.1, wd, 0, 0, first
                rc = lib.mlsp_sgd_flat_groups_f32(P.data_ptr(), B.data_ptr(), off, numel, gp, None, 2, t, 1, amax.data_ptr(), _lib.stream())
            else:
                rc = lib.mlsp_sgd_flat_f32(P.data_ptr(), B.data_ptr(), off, numel, gp, 2, lr, 0.9, 0.1, wd, 0, 0, first, amax.data_ptr(),
                                           _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        out.append((P, M, V, B, amax, step_out))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    P = out[0][0]
    assert not torch.equal(P[:2051], P0[:2051]) and not torch.equal(P[2117:2247], P0[2117:2247])      # both segments stepped ...
    assert torch.equal(P[2051:2117], P0[2051:2117]) and torch.equal(P[2247:], P0[2247:])              # ... and nothing around them
    assert out[0][4][0].item() == P[:2048].abs().max().item() and out[0][4][2].item() == P[2117:2247].abs().max().item()
    if which == "adam":
        assert out[0][5].item() == step
