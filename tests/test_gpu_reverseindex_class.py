"""functional.ReverseIndex: its scatter against a host index_add_, exactly, and how often each op that uses it builds the lists.

The edge rows hold small integers stored as float32, so every summation order gives the same bits and the comparison is torch.equal.
The launch counts wrap mlsp_group_reverse on the loaded library object: one build per object, none on a second backward over a
retained graph, none where an op needs no reverse index."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def builds(monkeypatch):
    """a one-element list counting the mlsp_group_reverse launches of the test"""
    from mlsp_amd import _lib
    lib = _lib.load()
    real, n = lib.mlsp_group_reverse, [0]

    def counting(*args):
        n[0] += 1
        return real(*args)

    monkeypatch.setattr(lib, "mlsp_group_reverse", counting)
    return n


def _idx(B, Nq, Nk, k, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, Nk, (B, Nq, k), generator=g, dtype=torch.int32)
    if (B, Nq, Nk, k) == (2, 5, 3, 4):
        idx[0] = 1                                           # every edge of cloud 0 names its row 1; rows 0 and 2 are named by none
        idx[1] = 2 * torch.randint(0, 2, (Nq, k), generator=g, dtype=torch.int32)      # cloud 1: row 1 is named by none
    return idx


SCATTERS = [((2, 5, 3, 4), [(4, 0, 4), (7, 2, 3)]),
            ((1, 1, 1, 1), [(4, 0, 4), (1, 0, 1)]),
            ((2, 70, 8, 2), [(16, c, w) for c in (0, 3) for w in (4, 12)])]


@pytest.mark.parametrize("shape,cuts", SCATTERS, ids=["x".join(map(str, s)) for s, _ in SCATTERS])
def test_scatter_equals_host_index_add(dev, builds, shape, cuts):
    from mlsp_amd import functional as Fh
    B, Nq, Nk, k = shape
    idx = _idx(B, Nq, Nk, k, 5)
    if shape == (2, 5, 3, 4):
        assert not (idx[0] == 0).any() and (idx[0] == 1).all() and not (idx[1] == 1).any()
    rows = (idx.long() + torch.arange(B)[:, None, None] * Nk).reshape(-1)
    rev = Fh.ReverseIndex(idx.to(dev), Nk)
    for n, (ld, col, width) in enumerate(cuts):
        dG = torch.randint(-8, 9, (B * Nq * k, ld), generator=torch.Generator().manual_seed(n)).float()
        want = torch.zeros(B * Nk, width).index_add_(0, rows, dG[:, col:col + width])
        got = rev.scatter(dG.to(dev), ld, col, width)
        assert got.shape == (B * Nk, width) and torch.equal(got.cpu(), want), (shape, ld, col, width)
    off, ent = rev.lists()
    assert builds[0] == 1 and rev.lists()[0] is off and rev.lists()[1] is ent
    assert off.shape == (B * Nk + 1,) and ent.shape == (B * Nq * k,) and off.dtype == ent.dtype == torch.int32
    assert torch.equal(off.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(rows, minlength=B * Nk).cumsum(0)]))


def _va_inputs(dev, d, B=2, N=8, k=4):
    g = torch.Generator().manual_seed(2)
    xyz = torch.rand(B * N, 3, generator=g).to(dev)
    idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32).to(dev)
    q, kk, v = (torch.randn(B * N, d, generator=g).to(dev).requires_grad_(True) for _ in range(3))
    shapes = [(d, 3), (d,), (d, d), (d,), (d, d), (d,), (d, d), (d,)]
    params = [(0.3 * torch.randn(s, generator=g)).to(dev).requires_grad_(True) for s in shapes]
    return xyz, idx, q, kk, v, params


def test_vector_attention_builds_once(dev, builds):
    from mlsp_amd import functional as Fh
    xyz, idx, q, kk, v, params = _va_inputs(dev, 8)
    res, _ = Fh.vector_attention(xyz, idx, q, kk, v, *params)
    assert builds[0] == 0
    res.sum().backward(retain_graph=True)
    assert builds[0] == 1 and all(t.grad is not None for t in (q, kk, v))
    res.sum().backward()
    assert builds[0] == 1


def test_gn_edge_max_builds_once(dev, builds):
    from mlsp_amd import functional as Fh
    B, Nk, Nq, k, C, groups = 2, 8, 8, 4, 16, 4
    g = torch.Generator().manual_seed(3)
    u = torch.randn(B * Nk, C, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(B * Nq, C, generator=g).to(dev).requires_grad_(True)
    idx = torch.randint(0, Nk, (B, Nq, k), generator=g, dtype=torch.int32).to(dev)
    gamma, beta = (torch.randn(C, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    out = Fh.gn_edge_max(u, w, idx, gamma, beta, groups)
    assert builds[0] == 0
    out.sum().backward(retain_graph=True)
    assert builds[0] == 1 and u.grad is not None and w.grad is not None
    out.sum().backward()
    assert builds[0] == 1


def test_group_builds_once_for_both_gathers(dev, builds):
    from mlsp_amd import pointnet2 as P
    B, N, S, ns, D = 2, 9, 4, 3, 5
    g = torch.Generator().manual_seed(4)
    xyz = torch.rand(B, N, 3, generator=g).to(dev).requires_grad_(True)
    feat = torch.randn(B, N, D, generator=g).to(dev).requires_grad_(True)
    idx = torch.randint(0, N, (B, S, ns), generator=g).to(dev)
    G = P._Group.apply(xyz, xyz[:, :S].detach(), feat, idx)
    G.sum().backward()
    assert builds[0] == 1 and xyz.grad.shape == xyz.shape and feat.grad.shape == feat.shape


@pytest.mark.parametrize("S,want", [(3, 1), (1, 0)])
def test_interp3_add_builds_once_per_backward(dev, builds, S, want):
    from mlsp_amd import functional as Fh
    B, N, C = 2, 6, 8
    g = torch.Generator().manual_seed(6)
    feat = torch.randn(B, S, C, generator=g).to(dev).requires_grad_(True)
    add = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
    idx = dist = None
    if S > 1:
        idx = torch.stack([torch.randperm(S, generator=g) for _ in range(B * N)]).view(B, N, 3).to(torch.int32).to(dev)
        dist = torch.rand(B, N, 3, generator=g).to(dev)
    out = Fh.interp3_add(feat, add, idx, dist)
    out.sum().backward(retain_graph=True)
    assert builds[0] == want and feat.grad.shape == feat.shape
    out.sum().backward()
    assert builds[0] == 2 * want


def test_interp3_builds_once_per_backward(dev, builds):
    from mlsp_amd import pointnet2 as P
    B, N, S, D = 2, 6, 4, 5
    g = torch.Generator().manual_seed(7)
    feat = torch.randn(B, S, D, generator=g).to(dev).requires_grad_(True)
    idx = torch.stack([torch.randperm(S, generator=g)[:3] for _ in range(B * N)]).view(B, N, 3).to(torch.int32).to(dev)
    out = P._Interp3.apply(feat, idx, torch.rand(B, N, 3, generator=g).to(dev))
    out.sum().backward()
    assert builds[0] == 1 and feat.grad.shape == feat.shape


def test_unsupported_shape_keeps_its_message(dev):
    from mlsp_amd import _lib
    from mlsp_amd import functional as Fh
    xyz, idx, q, kk, v, params = _va_inputs(dev, 6)
    with pytest.raises(_lib.MlspLibraryError) as e:
        Fh.vector_attention(xyz, idx, q, kk, v, *params)
    assert str(e.value).startswith("mlsp_vecattn_delta_fwd_f32: ")
    assert str(e.value).endswith(" (needs d % 4 == 0, 1 <= k <= 64, 16-byte-aligned rows)")
