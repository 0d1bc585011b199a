"""CPU checks of the Point-BERT PointTransformer: the restatement of tests/pointbert_restatement.py is pinned to the unmodified reference
(fixtures of tools/make_golden_pointbert.py), and mlsp_amd.pointbert's modules construct with the reference's state_dict and initial
values.  No GPU and no reference tree needed."""
import os
import types

import numpy as np
import pytest
import torch

import pointbert_restatement as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLS = os.path.join(GOLDEN, "ptrans_cls_s0_B2_N40_G5_M7_d24_h2_depth2.npz")
DEF = os.path.join(GOLDEN, "ptrans_def_s1_B2_N520_G8_M8_d32_h2_depth12_e32.npz")
TOL = 1e-5          # max|a - b| / max|b| between two fp32 evaluations of the same graph


@pytest.mark.parametrize("path,tag", [(CLS, "cls"), (DEF, "cls"), (DEF, "def")])
def test_restatement_reproduces_the_reference_fp32(path, tag):
    """fed the reference's own indices and selections, the fp32 restatement gives the reference's output and every stored gradient.

    The fixtures' draw is the first on which the reference's own fp32 gradients are within 5e-6 of its own float64 run
    (tools/make_golden_pointbert.py), so a second fp32 evaluation has room inside 1e-5.  Measured: classification path 2.3e-6 and 2.1e-6;
    DefRec path (depth 12) output 4.2e-6, worst gradient 5.5e-6 at 8 CPU threads, 6.6e-6 at 4, 5.1e-6 at 2 and 1."""
    z, cfg, params, graph = PR.load_fixture(path)
    pts, Rw = torch.from_numpy(z["pts"]), torch.from_numpy(z[tag + ".R"])
    sel = PR.stored_selections(path, z, tag)
    assert len(sel) == (8 if tag == "def" else 4)
    out, grads, _ = PR.grads(params, cfg, pts, graph, Rw, activate_DefRec=tag == "def", training=True, dtype=torch.float32, sel=sel)
    worst = {"out": PR.dist(out, z[tag + ".out"])}
    stored = [f for f in z.files if f.startswith(tag + ".g")]
    seen = 0
    for key, g in grads.items():
        pair = PR.stored_grad(z, tag, key, g)
        assert pair is not None, key
        seen += 1
        if PR.residue_bias(key):            # exactly 0 in exact arithmetic: both values are residue, measured against the layer's weight gradient
            scale = float(grads[key[:-len("bias")] + "weight"].abs().max())
            worst[key] = float((pair[1] - pair[0]).abs().max()) / scale
            continue
        worst[key] = PR.dist(pair[1], pair[0])
    assert seen == len(stored), (seen, len(stored))                # the restatement reaches exactly the parameters the reference reaches
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    print("worst", max(worst.values()))
    assert not bad, bad


def _ours(cfg):
    from mlsp_amd import pointbert
    return pointbert.PointTransformer(cfg)


@pytest.mark.parametrize("path", [CLS, DEF])
def test_module_state_dict_matches_the_fixture(path):
    """same key list and shapes as the reference's module (DGCNN_Propagation at (2 d -> 512, 1024 -> d)); under the stored seed every tensor
    drawn before the DGCNN_Propagation blocks has the reference's float64 sum exactly"""
    z, cfg, _, _ = PR.load_fixture(path)
    torch.manual_seed(int(z["seed"]))
    m = _ours(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    for (k, v), shape in zip(sd.items(), z["shapes"]):
        assert tuple(v.shape) == tuple(int(s) for s in shape if s > 0), k
    assert [n for n, _ in m.named_parameters()] == [k for k in sd if "running_" not in k and "num_batches" not in k]
    for k, s in zip(z["fresh.keys"], z["fresh.sums"]):
        assert float(sd[str(k)].double().sum()) == float(s), k


def test_module_at_the_reference_widths():
    """trans_dim 384 / depth 12: the key list, the shapes and, under the stored seed, every tensor's float64 sum equal the reference's own"""
    z = np.load(CLS)
    cfg = types.SimpleNamespace(trans_dim=384, depth=12, drop_path_rate=0.0, cls_dim=10, num_heads=6, group_size=32, num_group=64,
                                encoder_dims=256, encoder_type="Encoder", dropout=0.5, model="PointTransformer")
    torch.manual_seed(int(z["ref.seed"]))
    sd = _ours(cfg).state_dict()
    assert list(sd.keys()) == [str(k) for k in z["ref.keys"]] and len(sd) == 246
    for (k, v), shape, s in zip(sd.items(), z["ref.shapes"], z["ref.sums"]):
        assert tuple(v.shape) == tuple(int(x) for x in shape if x > 0), k
        assert float(v.double().sum()) == float(s), k


def test_group_and_encoder_construct_and_export():
    from mlsp_amd import Models, model_utils, mlsp, pointbert, _lib
    assert model_utils.Group is pointbert.Group and model_utils.Encoder is pointbert.Encoder
    assert Models.PointTransformer is pointbert.PointTransformer and Models.fps is pointbert.fps
    for name in ("PointNetFeaturePropagation", "square_distance", "index_points"):
        assert hasattr(model_utils, name), name
    assert callable(mlsp.calc_loss_ptrans)
    g = model_utils.Group(num_group=5, group_size=7)
    assert (g.num_group, g.group_size) == (5, 7) and not list(g.parameters())
    e = model_utils.Encoder(encoder_channel=32)
    assert list(e.state_dict().keys())[:3] == ["first_conv.0.weight", "first_conv.0.bias", "first_conv.1.weight"]
    assert e.second_conv[3].out_channels == 32
    with pytest.raises(_lib.MlspLibraryError):
        g(torch.zeros(1, 16, 3))
    with pytest.raises(_lib.MlspLibraryError):
        e(torch.zeros(1, 5, 7, 3))
    with pytest.raises(ValueError):
        model_utils.Group(num_group=4, group_size=65)
    for other in ("Pointnet_Encoder", "Dgcnn_Encoder", "Relative_Encoder"):
        cfg = types.SimpleNamespace(trans_dim=24, depth=2, drop_path_rate=0.0, cls_dim=10, num_heads=2, group_size=7, num_group=5,
                                    encoder_dims=32, encoder_type=other, dropout=0.0)
        with pytest.raises(NotImplementedError):
            pointbert.PointTransformer(cfg)


def test_thin_in_restatement_is_conv_batchnorm_act():
    """the restatement's thin_in against torch's own Conv1d + BatchNorm1d + ReLU modules (float64), running buffers included"""
    torch.manual_seed(3)
    conv, bn = torch.nn.Conv1d(3, 8, 1).double(), torch.nn.BatchNorm1d(8).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(8))
        bn.bias.copy_(torch.randn(8))
    X = torch.randn(33, 3, dtype=torch.float64)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    want = torch.relu(bn(conv(X.t().unsqueeze(0)))).squeeze(0).t()
    got = PR.thin_in(X, conv.weight.view(8, 3), conv.bias, bn.weight, bn.bias, rm0, rv0, training=True, act=PR.ACT_RELU)
    assert PR.dist(got["H"], want) < 1e-13
    assert PR.dist(got["run_mean"], bn.running_mean) < 1e-13 and PR.dist(got["run_var"], bn.running_var) < 1e-13
    bn.eval()
    want = torch.relu(bn(conv(X.t().unsqueeze(0)))).squeeze(0).t()
    got = PR.thin_in(X, conv.weight.view(8, 3), conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, training=False, act=PR.ACT_RELU)
    assert PR.dist(got["H"], want) < 1e-13
    lin = torch.nn.Linear(3, 8).double()
    got = PR.thin_in(X, lin.weight, lin.bias, act=PR.ACT_GELU)
    assert PR.dist(got["H"], torch.nn.functional.gelu(lin(X))) < 1e-13


def test_token_pool_and_group_restatements():
    torch.manual_seed(4)
    y = torch.randn(3, 6, 8, dtype=torch.float64)
    want = torch.cat([y[:, 0], y[:, 1:].max(1)[0]], dim=-1)
    arg = y[:, 1:].max(1)[1] + 1
    assert torch.equal(PR.token_pool(y), want) and torch.equal(PR.token_pool(y, arg), want)
    xyz = torch.randn(2, 40, 3)
    fps = PR.DG.fps_from_zero(xyz, 5)
    assert bool((fps[:, 0] == 0).all())
    center = PR.index_points(xyz, fps)
    idx = PR.DG.knn(7, xyz, center)[0]
    nb, c = PR.group(xyz, fps, idx)
    assert nb.shape == (2, 5, 7, 3) and torch.equal(c, center)
    assert bool((nb[:, :, 0].abs().sum(-1) == 0).all())            # a centre is its own nearest neighbour
