"""CPU checks of the vector-attention block: the fp32 restatement (tests/vecattn_restatement.py) reproduces the reference's recorded
results (tests/golden/tblock_*.npz, tools/make_golden_transformer.py), the module keeps the reference's state_dict, and nothing runs
without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import vecattn_restatement as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("tblock_s0_B2_N64_k16.npz", "tblock_s1_B2_N8_k16.npz")


def load_fixture(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    c = {k: torch.from_numpy(z[k]) for k in z.files}
    c["params"] = {k[2:]: v for k, v in c.items() if k.startswith("p.")}
    c["grads"] = {k[2:]: v for k, v in c.items() if k.startswith("g.")}
    return c


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_fp32(name):
    c = load_fixture(name)
    B, N, k, d_points, d_model = (int(v) for v in c["dims"])
    assert sorted(c["params"]) == sorted(vr.PARAM_KEYS)
    assert all(v.dtype in (torch.float32, torch.int64) for v in c.values() if torch.is_tensor(v))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1000000
    idx = vr.knn_index(c["xyz"], k)
    assert idx.shape == (B, N, min(k, N)) and torch.equal(idx, c["knn_idx"])
    assert torch.equal(idx[:, :, 0], torch.arange(N).expand(B, N))           # nearest first: itself
    out, attn, grads = vr.block_grads(c["params"], c["xyz"], c["features"], idx, c["R"], dtype=torch.float32)
    assert out.dtype == torch.float32 and attn.shape == (B, N, min(k, N), d_model)
    worst = {"out": vr.dist(out, c["out"]), "attn": vr.dist(attn, c["attn"])}
    for key, g in c["grads"].items():
        worst["d " + key] = vr.dist(grads[key], g)
    print(name, worst)
    assert max(worst.values()) <= 1e-5, worst


def test_state_dict_is_the_reference_s():
    from mlsp_amd.transformer import TransformerBlock
    for name in FIXTURES:
        c = load_fixture(name)
        _, _, k, d_points, d_model = (int(v) for v in c["dims"])
        blk = TransformerBlock(d_points, d_model, k)
        assert blk.k == k
        assert list(blk.state_dict()) == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc_delta.0.weight", "fc_delta.0.bias",
                                          "fc_delta.2.weight", "fc_delta.2.bias", "fc_gamma.0.weight", "fc_gamma.0.bias",
                                          "fc_gamma.2.weight", "fc_gamma.2.bias", "w_qs.weight", "w_ks.weight", "w_vs.weight"]
        blk.load_state_dict(c["params"], strict=True)
        assert torch.equal(blk.fc_delta[0].weight, c["params"]["fc_delta.0.weight"])


def test_forward_on_cpu_tensors_raises():
    from mlsp_amd import _lib
    from mlsp_amd.transformer import TransformerBlock
    blk = TransformerBlock(8, 16, 4)
    with pytest.raises(_lib.MlspLibraryError):
        blk(torch.zeros(1, 8, 3), torch.zeros(1, 8, 8))
    with pytest.raises(_lib.MlspLibraryError):
        blk(torch.zeros(1, 8, 3), torch.zeros(1, 8, 8), knn_idx=torch.zeros(1, 8, 4, dtype=torch.long))


def test_shim_resolves_to_our_class():
    import importlib
    from mlsp_amd.transformer import TransformerBlock
    shims = os.path.join(ROOT, "mlsp_amd", "shims")
    added = shims not in sys.path
    if added:
        sys.path.insert(0, shims)
    try:
        mod = importlib.import_module("PointDA.hengshuang_transformer.transformer")
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(shims))
        assert mod.TransformerBlock is TransformerBlock
    finally:
        if added:
            sys.path.remove(shims)
