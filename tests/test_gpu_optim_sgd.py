"""mlsp_amd.optim.FlatSGD against torch.optim.SGD (its default multi-tensor path on GPU tensors): the trainers' `--optimizer SGD`
(momentum 0.9, weight decay 5e-5, CosineAnnealingLR) as one launch over flat buffers -- the foreach arithmetic restated type by type and
lowering by lowering (tools/sgd_probe): bit-identical parameters and momentum buffers."""
import copy
import warnings

import numpy as np
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
    """a used trunk, a head that never runs (no gradient, never stepped, no state) and a late head"""

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(37, 129)
        self.bn = nn.BatchNorm1d(129)
        self.unused = nn.Linear(129, 5)
        self.b = nn.Linear(129, 70001 // 129)       # a tensor that does not end on a tile boundary; odd sizes take the element-wise path
        self.late = nn.Linear(129, 3)

    def forward(self, x, late=False):
        h = torch.relu(self.bn(self.a(x)))
        out = self.b(h).sum()
        return out + self.late(h).sum() if late else out


def _pair(dev):
    torch.manual_seed(3)
    m1 = _Net().to(dev)
    m2 = copy.deepcopy(m1)
    return m1, m2


def _same(m1, o1, m2, o2):
    """bit-identical parameters and momentum buffers; a parameter without state in torch has none here either"""
    for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), (n, (p != q).sum().item(), p.numel())
        b1, b2 = o1.state.get(p, {}).get("momentum_buffer"), o2.state.get(q, {}).get("momentum_buffer")
        assert (b1 is None) == (b2 is None), n
        if b1 is not None:
            assert torch.equal(b1, b2), (n, (b1 != b2).sum().item())


def _step(m, o, x, late=False):
    o.zero_grad()
    m(x, late=late).backward()
    o.step()


CONFIGS = {
    "trainers": dict(momentum=0.9, weight_decay=5e-5),
    "momentum0": dict(momentum=0.0, weight_decay=5e-5),
    "nesterov": dict(momentum=0.9, weight_decay=5e-5, nesterov=True),
    "dampening": dict(momentum=0.9, weight_decay=5e-5, dampening=0.1),
    "maximize": dict(momentum=0.9, weight_decay=5e-5, maximize=True),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_flat_sgd_is_bit_identical_to_torch_sgd(dev, name):
    """6 steps under CosineAnnealingLR: a parameter that leaves the buffer is re-homed (one rebuild, state carried over); a head that
    starts late hands over to torch's own path (one warning) and identity continues"""
    from mlsp_amd.optim import FlatSGD
    kw = CONFIGS[name]
    m1, m2 = _pair(dev)
    o1 = FlatSGD(m1.parameters(), lr=2e-2, **kw)
    o2 = torch.optim.SGD(m2.parameters(), lr=2e-2, **kw)
    s1 = torch.optim.lr_scheduler.CosineAnnealingLR(o1, 10)
    s2 = torch.optim.lr_scheduler.CosineAnnealingLR(o2, 10)
    for it in range(6):
        if it == 2:
            m1.a.weight.data = m1.a.weight.data.clone()       # leaves the flat buffer: laid out again at the next step
        late = it >= 4
        x = torch.randn(64, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(it))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for m, o, s in ((m1, o1, s1), (m2, o2, s2)):
                _step(m, o, x, late)
                s.step()
        ours = [str(r.message) for r in w if "FlatSGD" in str(r.message)]
        assert len(ours) == (1 if it == 4 else 0), (it, ours)
        _same(m1, o1, m2, o2)
        assert o1.flat_steps == min(it + 1, 4)
    assert o1.layouts_built == 2
    assert not o1.state.get(m1.unused.weight)
    if kw["momentum"] == 0:
        assert not any(o1.state.values()) and not any(o2.state.values())
    else:
        assert o1.state[m1.late.weight]["momentum_buffer"] is not None


def test_flat_sgd_keeps_shared_storages_together(dev):
    """Models.DGCNN with the three heads' merged first layers (parameters re-homed back to back): the flat layout moves each shared
    storage as a unit, so the merged operands stay views, with at most one rebuild of the layout"""
    from mlsp_amd import Models, functional as Fh
    from mlsp_amd.optim import FlatSGD
    torch.manual_seed(3)
    m = Models.DGCNN(gc.make_args(cuda=True)).to(dev).train()
    opt = FlatSGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-5)
    x = (torch.rand(4, 3, 256, device=dev) * 2 - 1)
    heads = (m.DefRec, m.Norm_pred, m.Density_cls)
    for _ in range(3):
        opt.zero_grad()
        out = m(x, activate_density_normal_ondef=True)
        sum(v.float().sum() for v in out.values()).backward()
        opt.step()
        assert Fh._adjacent([h.conv1.weight for h in heads]) and Fh._adjacent([h.bn1.weight for h in heads])
        assert all(torch.isfinite(p).all().item() for p in m.parameters())
    assert opt.flat_steps == 3 and opt.layouts_built <= 2
    base, n = opt._flat["p"].data_ptr(), opt._flat["p"].numel()
    assert all(base <= p.data_ptr() < base + 4 * n for p in m.parameters() if p.requires_grad)


def test_flat_sgd_state_dict_round_trips_with_torch_sgd(dev):
    """a FlatSGD state dict loads into torch.optim.SGD and a torch state dict into FlatSGD; stepping stays bit-identical both ways"""
    from mlsp_amd.optim import FlatSGD
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=5e-5)
    m1, m2 = _pair(dev)
    o1, o2 = FlatSGD(m1.parameters(), **kw), torch.optim.SGD(m2.parameters(), **kw)
    xs = [torch.randn(64, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(it)) for it in range(6)]
    for x in xs[:3]:
        _step(m1, o1, x)
        _step(m2, o2, x)
    _same(m1, o1, m2, o2)
    sd1, sd2 = copy.deepcopy(o1.state_dict()), copy.deepcopy(o2.state_dict())
    assert sd1["param_groups"] == sd2["param_groups"]
    assert sorted(sd1["state"]) == sorted(sd2["state"]) and all(set(v) == {"momentum_buffer"} for v in sd1["state"].values())
    m3, m4 = copy.deepcopy(m2), copy.deepcopy(m2)
    o3 = torch.optim.SGD(m3.parameters(), **kw)
    o3.load_state_dict(sd1)                                   # FlatSGD -> torch
    o4 = FlatSGD(m4.parameters(), **kw)
    o4.load_state_dict(sd2)                                   # torch -> FlatSGD
    for x in xs[3:]:
        for m, o in ((m1, o1), (m2, o2), (m3, o3), (m4, o4)):
            _step(m, o, x)
        _same(m1, o1, m2, o2)
        _same(m3, o3, m2, o2)
        _same(m4, o4, m2, o2)
    assert o1.flat_steps == 6 and o4.flat_steps == 3


def test_flat_sgd_falls_back_for_good_on_partial_state(dev):
    """loaded state in which only some stepped parameters have a momentum buffer: torch's own path from the first step on"""
    from mlsp_amd.optim import FlatSGD
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=5e-5)
    m1, m2 = _pair(dev)
    o2 = torch.optim.SGD(m2.parameters(), **kw)
    x = torch.randn(64, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    _step(m2, o2, x)
    sd = copy.deepcopy(o2.state_dict())
    del sd["state"][0]                                        # a.weight loses its buffer
    m1.load_state_dict(m2.state_dict())
    o1 = FlatSGD(m1.parameters(), **kw)
    o1.load_state_dict(sd)
    o2.load_state_dict(copy.deepcopy(sd))
    for it in range(1, 3):
        x = torch.randn(64, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(it))
        _step(m1, o1, x)
        _step(m2, o2, x)
        _same(m1, o1, m2, o2)
    assert o1.flat_steps == 0


def test_flat_sgd_reads_the_exchange_bucket_in_place(dev):
    """with FlatGradSync the step reads the packed (all-reduced) gradients where the bucket holds them: no second copy"""
    from mlsp_amd.ddp import FlatGradSync
    from mlsp_amd.optim import FlatSGD
    m1, m2 = _pair(dev)
    sync = FlatGradSync(m1, force=True, align=4)
    o1 = sync.wrap(FlatSGD(m1.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-5))
    o2 = torch.optim.SGD(m2.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-5)
    for it in range(3):
        x = torch.randn(64, 37, device=dev, generator=torch.Generator(device=dev).manual_seed(it))
        _step(m1, o1, x)
        _step(m2, o2, x)
        _same(m1, o1, m2, o2)
        lo, hi = sync.flat.data_ptr(), sync.flat.data_ptr() + 4 * sync.flat.numel()
        assert all(p.grad is None or lo <= p.grad.data_ptr() < hi for p in m1.parameters())
    assert o1.flat_steps == 3


def test_flat_sgd_publishes_weight_bounds(dev):
    """the step kernel leaves the largest magnitude of every updated 2048-element parameter tile, as FlatAdam's does: weight_bounds hands
    a GEMM exactly the tiles of the parameter its weight operand is, one run of tiles for the merged first-layer operand; withdrawn after
    a write torch sees and after invalidate_bounds()"""
    from mlsp_amd import Models, functional as Fh, _lib
    from mlsp_amd.optim import FlatSGD
    torch.manual_seed(3)
    m = Models.DGCNN(gc.make_args(cuda=True)).to(dev).train()
    opt = FlatSGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-5)
    x = (torch.rand(4, 3, 256, device=dev) * 2 - 1)
    assert opt.weight_bounds(m.conv5.weight.view(1024, -1)) is None        # nothing published before the first step
    for _ in range(2):
        opt.zero_grad()
        out = m(x, activate_density_normal_ondef=True)
        sum(v.float().sum() for v in out.values()).backward()
        opt.step()
    assert opt in _lib.weight_bound_providers
    W5 = m.conv5.weight.view(1024, -1)
    ptr, n = opt.weight_bounds(W5)
    f = opt._flat
    t0 = (ptr - f["tile_amax"].data_ptr()) // 4
    ps = f["params"]
    j = [ps[i] is m.conv5.weight for i in opt._active].index(True)
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


def _trainer_loss(args, logits, inp):
    from mlsp_amd import mlsp
    mask_cord = inp["mask"].permute(0, 2, 1)[:, :, 0] * 26 + 1
    loss = mlsp.calc_loss(args, logits, inp["gold"], inp["mask"])
    loss = loss + mlsp.calc_masked_normal_loss(args, logits["Normal"], inp["normal_gt"], mask_cord)
    kl, mae = mlsp.densityloss(args, logits, inp["dens_val"], inp["dens_vec"], mask=mask_cord.reshape(-1))
    return loss + kl + mae + torch.nn.functional.cross_entropy(logits["cls"], inp["cls_label"])


def test_flat_sgd_trains_dgcnn_like_torch_sgd(dev):
    """a trainer-shaped DGCNN step on the default f16x3 GEMMs (forward with activate_density_normal_ondef, backward, SGD), four times:
    FlatSGD (whose published bounds the GEMMs read) and torch SGD (the GEMMs measure their weights) give the same finite outputs to the
    suite's f16x3 tolerance"""
    from mlsp_amd import Models, _lib
    from mlsp_amd.optim import FlatSGD
    assert _lib.DEFAULT_GEMM_PRECISION == "f16x3"
    args = gc.make_args(dropout=0.0, cuda=True)
    inps = [{k: v.to(dev) for k, v in gc.make_inputs(s, 4, 256).items()} for s in range(4)]
    res = {}
    for flat in (True, False):
        torch.manual_seed(3)
        m = Models.DGCNN(gc.make_args(dropout=0.0, cuda=True))
        gc.perturb_params(m, 3)
        m = m.to(dev).train()
        kw = dict(lr=1e-3, momentum=0.9, weight_decay=5e-5)
        opt = FlatSGD(m.parameters(), **kw) if flat else torch.optim.SGD(m.parameters(), **kw)
        outs = []
        for inp in inps:
            opt.zero_grad()
            logits = m(inp["x"], activate_density_normal_ondef=True)
            loss = _trainer_loss(args, logits, inp)
            loss.backward()
            opt.step()
            outs.append(({k: v.detach().cpu().numpy() for k, v in logits.items()}, loss.item()))
        if flat:
            assert opt.flat_steps == len(inps)
        res[flat] = outs
    for (la, lossa), (lb, lossb) in zip(res[True], res[False]):
        assert np.isfinite(lossa)
        for k in la:
            assert np.isfinite(la[k]).all(), k
            np.testing.assert_allclose(la[k], lb[k], rtol=1e-3, atol=1e-3, err_msg=k)
        np.testing.assert_allclose(lossa, lossb, rtol=1e-3)
