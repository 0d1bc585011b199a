"""CPU checks of DGCNN_Propagation's boundary: the plain-torch restatement (tests/dgprop_restatement.py) reproduces the fixtures captured
from the unmodified reference (tools/make_golden_propagation.py), the module mirrors the reference's constructor and state_dict, resolves
through the PointDA.Models shim, and refuses to run without a GPU."""
import os

import numpy as np
import pytest
import torch

import dgprop_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NARROW, REF = "dgprop_s0_B2_G8_N16_k4_c16_m32.npz", "dgprop_s1_B2_G8_N16_k4_ref.npz"
REF_SHAPES = {"layer1.0.weight": (512, 768, 1, 1), "layer1.1.weight": (512,), "layer1.1.bias": (512,),
              "layer2.0.weight": (384, 1024, 1, 1), "layer2.1.weight": (384,), "layer2.1.bias": (384,)}


def load_case(name):
    """-> (fixture arrays, parameters as torch tensors keyed like the state_dict)"""
    c = dict(np.load(os.path.join(GOLDEN, name)))
    B, G, N, k, cin, mid = (int(v) for v in c["dims"])
    params = {}
    for key in R.KEYS:
        if "p." + key in c:
            params[key] = torch.from_numpy(c["p." + key])
        else:
            shape = (mid, 2 * cin, 1, 1) if key.startswith("layer1") else (cin, 2 * mid, 1, 1)
            i = 0 if key.startswith("layer1") else 1
            params[key] = torch.from_numpy(R.hash_fill(shape, int(c["wseed"][i]), float(c["wscale"][i])))
    return c, params


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_hash_fill_is_unstructured_and_exact():
    w = R.hash_fill((64, 96), 7, 0.25)
    assert w.dtype == np.float32 and np.abs(w).max() < 0.25 and abs(float(w.mean())) < 0.01
    assert np.linalg.matrix_rank(w.astype(np.float64)) == 64
    assert np.array_equal(w.ravel()[:6000], R.hash_fill((6000,), 7, 0.25)) and not np.array_equal(w, R.hash_fill((64, 96), 8, 0.25))
    assert [int(v) for v in R.hash_fill((4,), 3, 1.0).astype(np.float64) * (1 << 23)] == [-346312, -5839447, -7490580, -4690750]      # the same integers on every machine


@pytest.mark.parametrize("name", [NARROW, REF])
def test_restatement_reproduces_the_reference_fixture(name):
    c, params = load_case(name)
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 1000000
    B, G, N, k, cin, mid = (int(v) for v in c["dims"])
    coor, coor_q = torch.from_numpy(c["coor"]), torch.from_numpy(c["coor_q"])
    idx1 = R.knn(k, coor.transpose(1, 2), coor_q.transpose(1, 2))[0]
    idx2 = R.knn(k, coor_q.transpose(1, 2), coor_q.transpose(1, 2))[0]
    assert np.array_equal(idx1.numpy(), c["idx1"]) and np.array_equal(idx2.numpy(), c["idx2"])
    assert c["idx1"].dtype == np.int32 and c["idx1"].shape == (B, N, k) and list(c["keys"]) == list(R.KEYS)
    p = {key: v.clone().requires_grad_(True) for key, v in params.items()}
    f, f_q = (torch.from_numpy(c[n]).requires_grad_(True) for n in ("f", "f_q"))
    out = R.forward(p, coor, f, coor_q, f_q, idx1, idx2, dtype=torch.float32)
    assert out.shape == (B, cin, N) and out.dtype == torch.float32
    (out * torch.from_numpy(c["R"])).sum().backward()
    dist = {"out": rel(out.detach(), c["out"]), "g.f": rel(f.grad, c["g.f"]), "g.f_q": rel(f_q.grad, c["g.f_q"])}
    for key in R.KEYS:
        if "g." + key in c:
            dist["g." + key] = rel(p[key].grad, c["g." + key])
        else:
            dist["g16." + key] = rel(p[key].grad[::16], c["g16." + key])
    print(name, {n: "%.2e" % v for n, v in dist.items()})
    assert len(dist) == 9 and max(dist.values()) <= 1e-5, dist
    # some GroupNorm weights are negative (the selection takes the minimum there) and the biases matter
    assert (params["layer1.1.weight"] < 0).any() and (params["layer2.1.weight"] < 0).any() and params["layer1.1.bias"].abs().min() > 0


def test_recorded_slots_route_the_restatement_like_its_own_max():
    c, params = load_case(NARROW)
    args = [torch.from_numpy(c[n]) for n in ("coor", "f", "coor_q", "f_q")] + [torch.from_numpy(c["idx1"]).long(), torch.from_numpy(c["idx2"]).long()]
    e1, e2 = R.forward(params, *args, return_edges=True)
    argk = [e.argmax(dim=-1).permute(0, 2, 1) for e in (e1, e2)]
    assert torch.equal(R.forward(params, *args, argk=argk), R.forward(params, *args))


def test_state_dict_and_constructor_are_the_reference_ones():
    import inspect
    from mlsp_amd.propagation import DGCNN_Propagation
    m = DGCNN_Propagation()
    assert m.k == 16 and {k: tuple(v.shape) for k, v in m.state_dict().items()} == REF_SHAPES and list(m.state_dict()) == list(R.KEYS)
    sig = inspect.signature(DGCNN_Propagation.__init__)
    assert list(sig.parameters) == ["self", "k", "in_dim", "mid_dim"] and sig.parameters["k"].default == 16
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("in_dim", "mid_dim"))
    assert list(inspect.signature(DGCNN_Propagation.forward).parameters) == ["self", "coor", "f", "coor_q", "f_q"]
    assert isinstance(m.layer1[1], torch.nn.GroupNorm) and m.layer1[1].num_groups == 4 and m.layer2[2].negative_slope == 0.2
    c, params = load_case(NARROW)
    narrow = DGCNN_Propagation(k=4, in_dim=16, mid_dim=32)
    narrow.load_state_dict(params, strict=True)
    assert torch.equal(narrow.layer2[0].weight, params["layer2.0.weight"])


def test_no_cpu_fallback_and_shim():
    from mlsp_amd import _lib, functional as Fh
    from mlsp_amd.propagation import DGCNN_Propagation
    import mlsp_amd.Models
    import sys
    shims = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlsp_amd", "shims")
    sys.path.insert(0, shims)
    try:
        import PointDA.Models as shim
    finally:
        sys.path.remove(shims)
    assert shim.DGCNN_Propagation is DGCNN_Propagation is mlsp_amd.Models.DGCNN_Propagation
    m = DGCNN_Propagation(k=4, in_dim=16, mid_dim=32)
    with pytest.raises(_lib.MlspLibraryError):
        m(torch.zeros(1, 3, 8), torch.zeros(1, 16, 8), torch.zeros(1, 3, 8), torch.zeros(1, 16, 8))
    with pytest.raises(_lib.MlspLibraryError):
        m.forward_rows(torch.zeros(1, 8, 3), torch.zeros(8, 16), torch.zeros(1, 8, 3), torch.zeros(8, 16))
    with pytest.raises(_lib.MlspLibraryError):
        DGCNN_Propagation.fps_downsample(torch.zeros(1, 3, 8), torch.zeros(1, 16, 8), 4)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.gn_edge_max(torch.zeros(8, 16), torch.zeros(8, 16), torch.zeros(1, 8, 4, dtype=torch.int32), torch.ones(16), torch.zeros(16), 4)
