"""CPU checks of the Point-BERT transformer encoder: the fp32 restatement (tests/vit_restatement.py) reproduces the reference's recorded
results (tests/golden/vitblock_*.npz, vitenc_*.npz; tools/make_golden_vit.py), the modules keep the reference's state_dict, and nothing
runs without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import vit_restatement as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_FIXTURE = "vitblock_s0_B2_L65_d48_h6.npz"
ENCODER_FIXTURE = "vitenc_s1_B2_L9_d32_h4_depth4.npz"


def load_fixture(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    c = {k: torch.from_numpy(z[k]) for k in z.files if k != "keys"}
    c["keys"] = [str(k) for k in z["keys"]]
    c["params"] = {k[2:]: v for k, v in c.items() if k.startswith("p.")}
    c["grads"] = {k[2:]: v for k, v in c.items() if k.startswith("g.")}
    return c


def _fixture_is_small_and_numeric(name, c):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1000000
    assert all(v.dtype in (torch.float32, torch.int64) for v in c.values() if torch.is_tensor(v))
    assert sorted(c["params"]) == sorted(c["keys"])


def test_restatement_reproduces_the_reference_block_fp32():
    c = load_fixture(BLOCK_FIXTURE)
    _fixture_is_small_and_numeric(BLOCK_FIXTURE, c)
    B, L, dim, heads, _ = (int(v) for v in c["dims"])
    assert (B, L, dim, heads) == (2, 65, 48, 6) and c["keys"] == vr.block_keys(False)
    out, grads = vr.block_grads(c["params"], c["x"], c["R"], heads, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (B, L, dim)
    worst = {"out": vr.dist(out, c["out"])}
    for key, g in c["grads"].items():
        worst["d " + key] = vr.dist(grads[key], g)
    print(BLOCK_FIXTURE, worst)
    assert len(worst) == 1 + 1 + 11 and max(worst.values()) <= 1e-5, worst


def test_restatement_reproduces_the_reference_encoder_fp32():
    c = load_fixture(ENCODER_FIXTURE)
    _fixture_is_small_and_numeric(ENCODER_FIXTURE, c)
    B, L, dim, heads, depth = (int(v) for v in c["dims"])
    assert (B, L, dim, heads, depth) == (2, 9, 32, 4, 4)
    assert c["keys"] == ["blocks.%d.%s" % (i, k) for i in range(depth) for k in vr.block_keys(True)]
    out, feats, grads = vr.encoder_grads(c["params"], c["x"], c["pos"], c["R"], [c["R2"]], heads, depth, dtype=torch.float32)
    assert len(feats) == 1 and torch.equal(feats[0], out)                       # depth 4: block 3 is the last, its output is collected
    worst = {"out": vr.dist(out, c["out"]), "feat0": vr.dist(feats[0], c["feat0"])}
    for key, g in c["grads"].items():
        worst["d " + key] = vr.dist(grads[key], g)
    print(ENCODER_FIXTURE, worst)
    assert len(worst) == 2 + 2 + 12 * depth and max(worst.values()) <= 1e-5, worst


def test_state_dicts_are_the_reference_s():
    from mlsp_amd.vit import Block, TransformerEncoder
    c = load_fixture(BLOCK_FIXTURE)
    blk = Block(48, 6)
    assert list(blk.state_dict()) == c["keys"] == ["norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight",
                                                   "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "attn.qkv.weight",
                                                   "attn.proj.weight", "attn.proj.bias"]
    blk.load_state_dict(c["params"], strict=True)
    assert torch.equal(blk.attn.qkv.weight, c["params"]["attn.qkv.weight"]) and blk.attn.qkv.bias is None
    assert blk.attn.scale == 8 ** -0.5 and blk.mlp.fc1.out_features == 192 and isinstance(blk.drop_path, torch.nn.Identity)
    c = load_fixture(ENCODER_FIXTURE)
    enc = TransformerEncoder(embed_dim=32, depth=4, num_heads=4, qkv_bias=True)
    assert list(enc.state_dict()) == c["keys"]
    enc.load_state_dict(c["params"], strict=True)
    assert [n for n, _ in enc.named_parameters()] == c["keys"]                  # an optimiser sees the reference's parameter order
    # the reference's defaults and its per-block drop_path list
    enc = TransformerEncoder(depth=2, drop_path_rate=[0.0, 0.25])
    assert enc.blocks[0].attn.num_heads == 12 and enc.blocks[0].norm1.normalized_shape == (768,) and enc.blocks[0].attn.qkv.bias is None
    assert isinstance(enc.blocks[0].drop_path, torch.nn.Identity) and enc.blocks[1].drop_path.drop_prob == 0.25
    assert Block(16, 2, qk_scale=0.3, mlp_ratio=1.0).attn.scale == 0.3


def test_forward_on_cpu_tensors_raises():
    from mlsp_amd import _lib, functional as Fh
    from mlsp_amd.vit import Attention, Block, Mlp, TransformerEncoder
    x = torch.zeros(1, 8, 16)
    for mod in (Block(16, 2), Attention(16, 2), Mlp(16, 32)):
        with pytest.raises(_lib.MlspLibraryError):
            mod(x)
    with pytest.raises(_lib.MlspLibraryError):
        TransformerEncoder(embed_dim=16, depth=1, num_heads=2)(x, x)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.mhsa(torch.zeros(8, 48), 1, 8, 2, 0.5)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.layernorm(torch.zeros(8, 16), torch.ones(16), torch.zeros(16), 1e-5)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.gelu(torch.zeros(8, 16))


def test_dropout_is_refused_at_construction():
    from mlsp_amd.vit import Attention, Block, Mlp, TransformerEncoder
    for build in (lambda: Block(16, 2, drop=0.1), lambda: Block(16, 2, attn_drop=0.1), lambda: Mlp(16, drop=0.5),
                  lambda: Attention(16, 2, attn_drop=0.1), lambda: Attention(16, 2, proj_drop=0.1),
                  lambda: TransformerEncoder(embed_dim=16, depth=1, num_heads=2, drop_rate=0.1),
                  lambda: TransformerEncoder(embed_dim=16, depth=1, num_heads=2, attn_drop_rate=0.1)):
        with pytest.raises(NotImplementedError):
            build()


def test_drop_path_is_the_identity_in_eval_and_at_rate_zero():
    from mlsp_amd.vit import DropPath
    x = torch.randn(3, 4, 8)
    assert DropPath(0.0).train()(x) is x and DropPath(0.5).eval()(x) is x
    assert DropPath(0.5).train().eval().sample_scale(3, x.device) is None


def test_shim_resolves_to_our_classes():
    import importlib
    from mlsp_amd import model_utils, vit
    shims = os.path.join(ROOT, "mlsp_amd", "shims")
    added = shims not in sys.path
    if added:
        sys.path.insert(0, shims)
    try:
        mod = importlib.import_module("PointDA.model_utils")
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(shims))
        for name in ("Mlp", "Attention", "Block", "TransformerEncoder"):
            assert getattr(mod, name) is getattr(vit, name) is getattr(model_utils, name), name
    finally:
        if added:
            sys.path.remove(shims)
