"""CPU checks of the Point Transformer models: the fp32 restatement (tests/hengshuang_restatement.py) reproduces the reference's recorded
results (tests/golden/hsg_*.npz, tools/make_golden_hengshuang.py), the modules keep the reference's state_dict, the shim resolves to
them, and nothing runs without a GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import hengshuang_restatement as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"def": "hsg_def_B2_N48_nb2_k4.npz", "cls": "hsg_cls_B2_N64_nb2_k4.npz", "seg": "hsg_seg_B2_N64_nb1_k8.npz"}
CPU_BOUND = 1e-5          # what tests/test_pointbert_cpu.py holds the same kind of comparison to


def fixture(kind):
    return HR.load_fixture(os.path.join(ROOT, "tests", "golden", FIXTURES[kind]))


def make_cfg(z):
    num_point, nblocks, k, input_dim, tdim, num_class, _ = (int(v) for v in z["cfg"])
    cfg = types.SimpleNamespace(num_point=num_point, nblocks=nblocks, nneighbor=k, num_class=num_class, input_dim=input_dim,
                                transformer_dim=tdim, dropout=0.0)
    cfg.model = cfg
    return cfg


def make_model(kind, z):
    from mlsp_amd import hengshuang_model as hm
    return {"def": hm.PointTransformerDef, "cls": hm.PointTransformerCls, "seg": hm.PointTransformerSeg}[kind](make_cfg(z))


@pytest.mark.parametrize("kind", sorted(FIXTURES))
def test_constructors_and_state_dict_keys(kind):
    z, params, _ = fixture(kind)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", FIXTURES[kind])) < 1000000
    m = make_model(kind, z)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in params.values()]
    named = [n for n, _ in m.named_parameters()]
    assert named == [k for k in params if ("p." + k) in z.files or ("wseed." + k) in z.files]
    assert sum(p.numel() for p in m.parameters()) == sum(params[k].numel() for k in named)
    m.load_state_dict(params, strict=True)
    if kind != "cls":
        assert [k for k in sd if k.startswith("transition_ups.0.fc1.")][:4] == ["transition_ups.0.fc1.0.weight", "transition_ups.0.fc1.0.bias",
                                                                                 "transition_ups.0.fc1.2.weight", "transition_ups.0.fc1.2.bias"]
        assert not list(m.transition_ups[0].fp.parameters())
    if kind == "def":
        loss, acc = m.get_loss_acc(torch.tensor([[2.0, 0.0], [0.0, 1.0]]), torch.tensor([0, 0]))
        assert float(acc) == 50.0 and abs(float(loss) - float(torch.nn.functional.cross_entropy(torch.tensor([[2.0, 0.0], [0.0, 1.0]]), torch.tensor([0, 0])))) < 1e-7


def test_reference_reads_both_cfg_spellings():
    """Backbone and PointTransformerDef read cfg.nblocks / cfg.nneighbor / cfg.transformer_dim, PointTransformerCls / Seg read cfg.model.*
    for their own members: mirrored, not repaired"""
    from mlsp_amd import hengshuang_model as hm
    inner = types.SimpleNamespace(nblocks=1, nneighbor=8, transformer_dim=16)
    cfg = types.SimpleNamespace(num_point=64, nblocks=2, nneighbor=4, num_class=5, input_dim=3, transformer_dim=32, dropout=0.0, model=inner)
    seg = hm.PointTransformerSeg(cfg)
    assert seg.backbone.nblocks == 2 and seg.nblocks == 1 and len(seg.transition_ups) == 1
    assert seg.backbone.transformer1.k == 4 and seg.transformer2.k == 8 and seg.transformer2.fc1.out_features == 16
    assert seg.fc2[0].in_features == 64 and hm.PointTransformerCls(cfg).fc2[0].in_features == 64
    d = hm.PointTransformerDef(cfg)
    assert d.nblocks == 2 and d.DefRec.conv1.in_channels == 544


def test_shim_resolves_to_our_classes():
    import importlib
    from mlsp_amd import hengshuang_model as hm
    shims = os.path.join(ROOT, "mlsp_amd", "shims")
    added = shims not in sys.path
    if added:
        sys.path.insert(0, shims)
    try:
        mod = importlib.import_module("PointDA.hengshuang_transformer.hengshuang_model")
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(shims))
        for name in ("TransitionDown", "TransitionUp", "Backbone", "PointTransformerCls", "PointTransformerSeg", "PointTransformerDef"):
            assert getattr(mod, name) is getattr(hm, name), name
    finally:
        if added:
            sys.path.remove(shims)


def test_cpu_tensors_raise_and_refusals():
    from mlsp_amd import _lib, functional as Fh, hengshuang_model as hm
    z, _, _ = fixture("def")
    cfg = make_cfg(z)
    x = torch.zeros(2, 48, 3)
    for m in (hm.PointTransformerDef(cfg), hm.PointTransformerCls(cfg), hm.PointTransformerSeg(cfg), hm.Backbone(cfg)):
        with pytest.raises(_lib.MlspLibraryError):
            m(x)
    with pytest.raises(_lib.MlspLibraryError):
        hm.TransitionDown(4, 4, [35, 64, 64])(torch.zeros(1, 16, 3), torch.zeros(1, 16, 32))
    with pytest.raises(_lib.MlspLibraryError):
        hm.TransitionUp(64, 32, 32)(torch.zeros(1, 4, 3), torch.zeros(1, 4, 64), torch.zeros(1, 16, 3), torch.zeros(1, 16, 32))
    with pytest.raises(_lib.MlspLibraryError):
        Fh.cloud_mean(torch.zeros(8, 4), 2, 4)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.interp3_add(torch.zeros(1, 1, 4), torch.zeros(1, 5, 4))
    # a level of two points feeding a TransitionUp (32 / 8 / 2), alone and in the models that decode
    with pytest.raises(ValueError):
        hm.TransitionUp(64, 32, 32)(torch.zeros(1, 2, 3), torch.zeros(1, 2, 64), torch.zeros(1, 8, 3), torch.zeros(1, 8, 32))
    cfg2 = make_cfg(z)
    cfg2.num_point = 32
    with pytest.raises(ValueError):
        hm.PointTransformerSeg(cfg2)(torch.zeros(2, 32, 3))
    with pytest.raises(_lib.MlspLibraryError):
        hm.PointTransformerCls(cfg2)(torch.zeros(2, 32, 3))                   # (no TransitionUp: two points are fine)
    # nsample larger than the level's point count: 8 / 2 with nneighbor 4
    with pytest.raises(ValueError):
        hm.TransitionDown(1, 4, [35, 64, 64])(torch.zeros(1, 2, 3), torch.zeros(1, 2, 32))
    cfg3 = make_cfg(z)
    cfg3.num_point = 8
    with pytest.raises(ValueError):
        hm.PointTransformerCls(cfg3)(torch.zeros(2, 8, 3))
    # DefRec reads 32 + 512 channels: nblocks = 4 only
    with pytest.raises(ValueError):
        hm.PointTransformerDef(cfg)(x, activate_DefRec=True)


@pytest.mark.parametrize("kind", sorted(FIXTURES))
@pytest.mark.parametrize("tag", ["train", "eval"])
def test_restatement_reproduces_the_reference_fp32(kind, tag):
    """The fp32 restatement, fed the fixture's graph and the reference's own selections, against the reference's outputs and gradients.
    Bound 1e-5; a training-mode bias gradient that the reference itself cannot hold to half of that against its own float64 run on any
    draw (tools/make_golden_hengshuang.own_error: a small remainder of sums that a BatchNorm cancels) gets twice its stored own error."""
    z, params, graph = fixture(kind)
    nblocks = int(z["cfg"][1])
    training = tag == "train"
    assert float(z[tag + ".own_error"]) < CPU_BOUND / 2
    sel = [torch.from_numpy(z["%s.sel.%d" % (tag, i)]) for i in range(nblocks)]
    x, Rw = torch.from_numpy(z["x"]), torch.from_numpy(z[tag + ".R"])
    out, g, _ = HR.grads(kind, params, nblocks, x, graph, Rw, training=training, dtype=torch.float32, sel=sel)
    assert out.dtype == torch.float32
    stored = {k[len(tag) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + ".g.")}
    stored16 = {k[len(tag) + 5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + ".g16.")}
    assert set(stored) | set(stored16) == set(g) and len(g) > 30
    wants = dict(stored)
    wants.update(stored16)
    worst, over = {"out": HR.dist(out, z[tag + ".out"])}, {}
    assert worst["out"] <= CPU_BOUND, worst
    for key, got in g.items():
        want = wants[key]
        got = got[::16] if key in stored16 else got
        if HR.residue_bias(key, training, kind, nblocks) and key[:-4] + "weight" in stored16:
            wants_den = {key[:-4] + "weight": stored16[key[:-4] + "weight"]}
        else:
            wants_den = wants
        e = HR.grad_dist(key, got, want, wants_den, training, kind, nblocks)
        bound = CPU_BOUND
        if (tag + ".own." + key) in z.files:
            bound = max(bound, 2 * float(z[tag + ".own." + key]))
        worst[key] = e
        if e > bound:
            over[key] = (e, bound)
    print(kind, tag, "out %.2e, worst gradient %.2e" % (worst["out"], max(v for k, v in worst.items() if k != "out")))
    assert not over, over


def test_float64_ops_agree_with_plain_torch():
    g = torch.Generator().manual_seed(5)
    for B, N, S, C in ((1, 5, 1, 4), (2, 48, 3, 32), (3, 130, 17, 36)):
        feat, add = torch.randn(B, S, C, generator=g, dtype=torch.float64), torch.randn(B, N, C, generator=g, dtype=torch.float64)
        if S == 1:
            got, want = HR.interp3_add(feat, add), add + feat.repeat(1, N, 1)
        else:
            src, qry = torch.randn(B, S, 3, generator=g, dtype=torch.float64), torch.randn(B, N, 3, generator=g, dtype=torch.float64)
            d, idx = torch.cdist(qry, src).pow(2).sort(dim=-1)
            d, idx = d[:, :, :3], idx[:, :, :3]
            got = HR.interp3_add(feat, add, idx, d)
            want = add.clone()
            recip = 1.0 / (d + 1e-8)
            for b in range(B):
                for j in range(3):
                    want[b] += feat[b][idx[b, :, j]] * (recip[b, :, j] / recip[b].sum(-1)).unsqueeze(-1)
            assert HR.dist(HR.sq_dist_to(qry, src, idx), d) <= 1e-13
        assert HR.dist(got, want) <= 1e-13
    for B, N, C in ((1, 1, 4), (3, 130, 36), (2, 1024, 512)):
        x = torch.randn(B, N, C, generator=g, dtype=torch.float64)
        assert HR.dist(HR.cloud_mean(x), x.mean(1)) <= 1e-13
