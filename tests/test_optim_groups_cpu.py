"""CPU checks of the parameter-group side of mlsp_amd.optim: FlatAdamW is a torch.optim.AdamW with torch's constructor and validation; on
CPU parameters FlatAdamW and two-group FlatAdam / FlatSGD ARE torch's path (the flat step needs GPU parameters), so they must equal
torch's optimizers exactly.  The two group entry points are declared, bound and refuse bad arguments before they launch anything."""
import copy
import ctypes
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(7, 33), nn.BatchNorm1d(33), nn.ReLU(), nn.Linear(33, 5))


def _split(m, weight_decay, **extra):
    """the reference's add_weight_decay (utils/optimizer.py:18-36): 1-D parameters and biases are not decayed"""
    no_decay = [p for n, p in m.named_parameters() if p.dim() == 1 or n.endswith(".bias")]
    decay = [p for n, p in m.named_parameters() if not (p.dim() == 1 or n.endswith(".bias"))]
    return [dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=weight_decay, **extra)]


def _make(kind, m, ours):
    from mlsp_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    if kind == "adamw":
        return (FlatAdamW if ours else torch.optim.AdamW)(m.parameters(), lr=2e-3)
    if kind == "adamw_groups":
        return (FlatAdamW if ours else torch.optim.AdamW)(_split(m, 1e-2, lr=5e-3), lr=2e-3)
    if kind == "adam_groups":
        groups = _split(m, 5e-5, betas=(0.8, 0.99))
        return FlatAdam(groups, lr=2e-3) if ours else torch.optim.Adam(groups, lr=2e-3, fused=False)
    groups = _split(m, 5e-5, momentum=0.9, nesterov=True)
    return (FlatSGD if ours else torch.optim.SGD)(groups, lr=0.05)


@pytest.mark.parametrize("kind", ["adamw", "adamw_groups", "adam_groups", "sgd_groups"])
def test_grouped_optimizers_equal_torch_on_cpu(kind):
    m1 = _net()
    m2 = copy.deepcopy(m1)
    o1, o2 = _make(kind, m1, True), _make(kind, m2, False)
    assert isinstance(o1, type(o2))
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
        assert sd1["state"][k].keys() == sd2["state"][k].keys()
        for name in sd2["state"][k]:
            assert torch.equal(sd1["state"][k][name], sd2["state"][k][name]), (k, name)


def test_flat_adamw_is_an_adamw_with_torch_defaults():
    from mlsp_amd.optim import FlatAdam, FlatAdamW
    o = FlatAdamW(_net().parameters())
    assert isinstance(o, torch.optim.AdamW) and isinstance(o, FlatAdam)
    want = torch.optim.AdamW(_net().parameters()).param_groups[0]
    got = o.param_groups[0]
    assert {k: v for k, v in got.items() if k != "params"} == {k: v for k, v in want.items() if k != "params"}
    assert got["weight_decay"] == 1e-2 and got["decoupled_weight_decay"] is True
    # FlatAdam takes torch.optim.Adam's flag and keeps it per group
    o = FlatAdam(_split(_net(), 1e-2, decoupled_weight_decay=True), lr=1e-3)
    assert [g["decoupled_weight_decay"] for g in o.param_groups] == [False, True]


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-1e-4), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)),
                                dict(betas=(-0.1, 0.999))])
def test_flat_adamw_rejects_what_torch_rejects(kw):
    from mlsp_amd.optim import FlatAdamW
    with pytest.raises(ValueError) as want:
        torch.optim.AdamW(_net().parameters(), **kw)
    with pytest.raises(ValueError, match=re.escape(str(want.value))):
        FlatAdamW(_net().parameters(), **kw)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlsp_hip.h")).read(), flags=re.S)


def test_group_structs_match_the_header():
    """the ctypes mirrors list the fields of mlsp_adam_group_t / mlsp_sgd_group_t in the header's order, with its sizes"""
    from mlsp_amd import _lib
    src = _header()
    for cname, cls in (("mlsp_adam_group_t", _lib.MlspAdamGroup), ("mlsp_sgd_group_t", _lib.MlspSgdGroup)):
        body = re.search(r"typedef struct \w+ \{([^}]*)\} %s;" % cname, src).group(1)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [n for n, _ in cls._fields_], (cname, names)
    assert ctypes.sizeof(_lib.MlspAdamGroup) == 64 and ctypes.sizeof(_lib.MlspSgdGroup) == 48
    assert "#define MLSP_FLAT_MAX_GROUPS 8" in src and _lib.FLAT_MAX_GROUPS == 8
    assert "#define MLSP_ABI_VERSION 14" in src


ERR_ARG = -1                                                   # MLSP_ERR_ARG: refused before any launch


def _segs(n):
    off = (ctypes.c_uint32 * n)(*[64 * i for i in range(n)])
    numel = (ctypes.c_uint32 * n)(*[5] * n)
    grads = (ctypes.c_void_p * n)(*[4096 + 256 * i for i in range(n)])
    return off, numel, grads


def test_adam_groups_entry_point_is_bound_and_checks_its_arguments():
    from mlsp_amd import _lib
    assert "mlsp_adam_flat_groups_f32" in _lib.SIGNATURES and "mlsp_adam_flat_groups_f32" in _header()
    lib = _lib.load()

    def call(P=256, M=512, V=768, nseg=3, ngroups=2, tags=(0, 1, 1), steps=(1, 4), seg_group=True):
        off, numel, grads = _segs(max(nseg, 1))
        sg = (ctypes.c_uint8 * max(nseg, 1))(*tags[:max(nseg, 1)])
        table = (_lib.MlspAdamGroup * max(ngroups, 1))()
        for g in range(max(ngroups, 1)):
            t = table[g]
            t.lr, t.beta1, t.beta2, t.weight_decay, t.eps, t.step, t.decoupled = 1e-3, 0.9, 0.999, 1e-2, 1e-8, steps[g % len(steps)], g % 2
        return lib.mlsp_adam_flat_groups_f32(P, M, V, off, numel, grads, sg if seg_group else None, nseg, table, ngroups, None, None)

    assert call(ngroups=0) == ERR_ARG                          # no group
    assert call(ngroups=9, tags=(0, 8, 1)) == ERR_ARG          # more than 8 groups
    assert call(tags=(0, 2, 1)) == ERR_ARG                     # a segment of a group that is not there
    assert call(tags=(0, 1, 255)) == ERR_ARG
    assert call(steps=(1, 0)) == ERR_ARG                       # a group whose step is not >= 1
    assert call(steps=(-3, 2)) == ERR_ARG
    assert call(P=None) == ERR_ARG and call(M=None) == ERR_ARG and call(V=None) == ERR_ARG
    assert call(P=260) == ERR_ARG and call(M=516) == ERR_ARG and call(V=776) == ERR_ARG        # off 16 bytes
    assert call(nseg=0) == ERR_ARG                             # nothing to step
    off, numel, grads = _segs(1)
    assert lib.mlsp_adam_flat_groups_f32(256, 512, 768, off, numel, grads, None, 1, None, 1, None, None) == ERR_ARG   # no group table


def test_sgd_groups_entry_point_is_bound_and_checks_its_arguments():
    from mlsp_amd import _lib
    assert "mlsp_sgd_flat_groups_f32" in _lib.SIGNATURES and "mlsp_sgd_flat_groups_f32" in _header()
    lib = _lib.load()

    def call(P=256, B=512, nseg=3, ngroups=2, tags=(0, 1, 1), momentum=(0.9, 0.0)):
        off, numel, grads = _segs(max(nseg, 1))
        sg = (ctypes.c_uint8 * max(nseg, 1))(*tags[:max(nseg, 1)])
        table = (_lib.MlspSgdGroup * max(ngroups, 1))()
        for g in range(max(ngroups, 1)):
            t = table[g]
            t.lr, t.momentum, t.dampening, t.weight_decay = 1e-3, momentum[g % len(momentum)], 0.0, 5e-5
        return lib.mlsp_sgd_flat_groups_f32(P, B, off, numel, grads, sg, nseg, table, ngroups, None, None)

    assert call(ngroups=0) == ERR_ARG
    assert call(ngroups=9) == ERR_ARG
    assert call(tags=(0, 1, 2)) == ERR_ARG                     # a segment of a group that is not there
    assert call(P=None) == ERR_ARG                             # no parameters
    assert call(P=260) == ERR_ARG and call(B=520) == ERR_ARG   # off 16 bytes
    assert call(B=None, momentum=(0.0, 0.9)) == ERR_ARG        # momentum in SOME group without a momentum buffer
    assert call(B=None, momentum=(0.9, 0.0)) == ERR_ARG
    assert call(nseg=0) == ERR_ARG
