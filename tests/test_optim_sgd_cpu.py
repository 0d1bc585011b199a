"""CPU checks of mlsp_amd.optim.FlatSGD: a torch.optim.SGD subclass with torch's constructor and validation; on CPU parameters it IS
torch's path (the flat step needs GPU parameters), so it must equal torch.optim.SGD exactly.  The C entry point is declared, bound and
refuses bad arguments before it launches anything."""
import copy
import ctypes
import re

import pytest
import torch
from torch import nn


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 33), nn.ReLU(), nn.Linear(33, 5))


@pytest.mark.parametrize("kw", [dict(momentum=0.9, weight_decay=5e-5), dict(), dict(momentum=0.9, nesterov=True),
                                dict(momentum=0.5, dampening=0.1, weight_decay=1e-2), dict(momentum=0.9, maximize=True)])
def test_flat_sgd_equals_torch_sgd_on_cpu(kw):
    from mlsp_amd.optim import FlatSGD
    m1 = _net()
    m2 = copy.deepcopy(m1)
    o1, o2 = FlatSGD(m1.parameters(), lr=0.05, **kw), torch.optim.SGD(m2.parameters(), lr=0.05, **kw)
    assert isinstance(o1, torch.optim.SGD)
    s1, s2 = torch.optim.lr_scheduler.CosineAnnealingLR(o1, 5), torch.optim.lr_scheduler.CosineAnnealingLR(o2, 5)
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        x = torch.randn(16, 7, generator=g)
        for m, o, s in ((m1, o1, s1), (m2, o2, s2)):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
            s.step()
        for p, q in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(p, q)
    assert o1.flat_steps == 0
    sd1, sd2 = o1.state_dict(), o2.state_dict()
    assert sd1["param_groups"] == sd2["param_groups"]
    assert sd1["state"].keys() == sd2["state"].keys()
    for k in sd2["state"]:
        assert torch.equal(sd1["state"][k]["momentum_buffer"], sd2["state"][k]["momentum_buffer"])
    if not kw.get("momentum"):
        assert not sd1["state"]


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(momentum=0.9, dampening=0.1, nesterov=True),
                                dict(nesterov=True), dict(fused=True, differentiable=True)])
def test_flat_sgd_rejects_what_torch_rejects(kw):
    from mlsp_amd.optim import FlatSGD
    with pytest.raises((ValueError, RuntimeError)) as want:
        torch.optim.SGD(_net().parameters(), **kw)
    with pytest.raises(type(want.value), match=re.escape(str(want.value))):
        FlatSGD(_net().parameters(), **kw)


def test_sgd_entry_point_is_bound_and_checks_its_arguments():
    from mlsp_amd import _lib
    assert "mlsp_sgd_flat_f32" in _lib.SIGNATURES
    lib = _lib.load()
    off, numel = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint32 * 1)(4)
    grads = (ctypes.c_void_p * 1)(256)
    call = lambda P, B, mom, nseg=1: lib.mlsp_sgd_flat_f32(P, B, off, numel, grads, nseg, 1e-3, mom, 0.0, 5e-5, 0, 0, 0, None, None)
    err = -1                                                   # MLSP_ERR_ARG: refused before any launch
    assert call(None, 512, 0.9) == err                         # no parameters
    assert call(256, None, 0.9) == err                         # momentum without a momentum buffer
    assert call(256, 520, 0.9) == err                          # a momentum buffer off 16 bytes
    assert call(260, None, 0.0) == err                         # parameters off 16 bytes
    assert call(256, None, 0.0, nseg=0) == err                 # nothing to step
