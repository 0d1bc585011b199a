"""on-device label generators vs the numpy restatement (parity unpinned: no python-pcl) and closed forms."""
import numpy as np
import pytest
import torch

from oracle import knn_canon, labels_np
import test_corrupt_oracle_cpu as cases            # the edge-case inputs; their conditions are proven there, on the CPU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_cloud = cases.ball_cloud


def _check_counts(got, x, radius, K):
    """got [B,N] device counts against the float64 bracket and the fp32 oracle: inside [lo, hi] everywhere, equal to the oracle wherever
    no pair of the point is within fp32 rounding of the radius (lo == hi); -> the mask of those points"""
    sure = np.zeros(got.shape, bool)
    for b in range(len(x)):
        lo, hi = labels_np.radius_count_bounds(x[b], radius, K)
        assert (lo <= got[b]).all() and (got[b] <= hi).all()
        sure[b] = lo == hi
        assert np.array_equal(got[b][sure[b]], labels_np.radius_count(x[b], radius, K)[sure[b]])
    assert (~sure).mean() <= 0.01                      # a condition on the inputs (asserted on the CPU as well)
    return sure


@pytest.mark.parametrize("B,N,radius", cases.DENSITY_CASES)
def test_cal_density_vs_numpy(dev, B, N, radius):
    from mlsp_amd import labels
    x = _cloud(1, B, N)
    raw = labels.radius_count(x.to(dev), radius).cpu().numpy()
    assert raw.dtype == np.int32 and raw.shape == (B, N)
    sure = _check_counts(raw, x.numpy(), radius, 100)
    cls, row = labels.cal_density(x.to(dev), radius=radius, num_cls=16, pergroup=2)
    wc, wr = labels_np.cal_density(x.numpy(), radius, 16, 2)
    assert cls.shape == (B, N, 16) and row.shape == (B, N)
    np.testing.assert_array_equal(row, np.clip(raw, 0, 30))
    np.testing.assert_array_equal(row[sure], wr[sure])
    np.testing.assert_array_equal(cls[sure], wc[sure])
    np.testing.assert_allclose(cls.sum(-1), 1.0)
    # point 0 of every cloud is never counted (mlsp.py:254) -> its own count excludes itself
    for b in range(B):
        full = int((torch.cdist(x[b, :1].double(), x[b].double()) ** 2 < float(np.float32(radius) ** 2)).sum())
        assert not sure[b, 0] or row[b, 0] == min(min(full, 100) - 1, 30)


@pytest.mark.parametrize("name", ["dense", "far0", "copies0", "ld6", "small_K"])
def test_radius_count_clamp_point0_and_stride(dev, name):
    """The max_nn clamp against the point-0 subtraction (min(c, K) - [point 0 in range]) with every count saturated and with K in the
    middle of the counts, point 0 out of everybody's range, copies of point 0, and rows of 6 floats whose last 3 must be ignored."""
    from mlsp_amd import labels
    x, radius, K = cases.density_special_clouds()[name]
    got = labels.radius_count(torch.from_numpy(x).to(dev), radius, K).cpu().numpy()
    _check_counts(got, x, radius, K)
    if name == "dense":
        assert (got == K - 1).all()
    if name == "far0":
        assert (got[:, 0] == 0).all()


def test_label_kernels_reject_bad_arguments(dev):
    from mlsp_amd import labels, _lib
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):          # 12801 points: one more than 150 KB of LDS holds; host-side
        labels.radius_count(torch.zeros(1, 12801, 3, device=dev), 0.1)
    lib = _lib.load()
    x = torch.zeros(1, 8, 3, device=dev)
    idx = torch.zeros(8, 3, dtype=torch.int32, device=dev)
    out = torch.zeros(1, 8, 3, device=dev)
    for args in ((0, 3, idx.data_ptr(), 1, 8, 3, out.data_ptr()), (x.data_ptr(), 3, 0, 1, 8, 3, out.data_ptr()),
                 (x.data_ptr(), 3, idx.data_ptr(), 1, 8, 3, 0), (x.data_ptr(), 3, idx.data_ptr(), 1, 8, 0, out.data_ptr()),
                 (x.data_ptr(), 2, idx.data_ptr(), 1, 8, 3, out.data_ptr()), (x.data_ptr(), 3, idx.data_ptr(), 0, 8, 3, out.data_ptr())):
        with pytest.raises(_lib.MlspLibraryError, match="bad argument"):
            _lib.check(lib.mlsp_knn_normals_f32(*args, _lib.stream()), "mlsp_knn_normals_f32")
    assert (out == 0).all()


def _kernel_normals(dev, x, idx):
    """mlsp_knn_normals_f32 alone: x [B,N,ld] float32, idx [B*N,k] int32 (indices inside each cloud) -> [B,N,3]"""
    from mlsp_amd import _lib
    lib = _lib.load()
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    B, N, ld = xd.shape
    idd = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    out = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    _lib.check(lib.mlsp_knn_normals_f32(xd.data_ptr(), ld, idd.data_ptr(), B, N, idd.shape[1], out.data_ptr(), _lib.stream()),
               "mlsp_knn_normals_f32")
    return out.cpu().numpy()


def _check_normals(got, pts, idx, sel=None):
    """got [N,3] against the float64 eigh of the same neighbourhoods: for EVERY (selected) point sin(angle) <= 6 u w2 / (w1 - w0) + 4 u
    (labels_np.normal_sin_bar: what rounding the covariance to fp32 can cost, plus the output rounding), and the same orientation
    wherever the point is not within rounding of its own tangent plane."""
    want, w = labels_np.knn_normals(pts, idx)
    sel = np.ones(len(pts), bool) if sel is None else sel
    g, t = got.astype(np.float64), want.astype(np.float64)
    sin = np.linalg.norm(np.cross(g, t), axis=1)
    bar = labels_np.normal_sin_bar(w)
    print("normals: max sin / bar = %.3f over %d points" % ((sin / bar)[sel].max(), sel.sum()))
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(g, axis=1) - 1).max() <= 4 * 2.0 ** -24
    assert (sin <= bar)[sel].all(), (sin / bar)[sel].max()
    p = pts[:, :3].astype(np.float64)
    clear = np.abs((t * p).sum(1)) > 1e-6 * np.linalg.norm(p, axis=1)
    assert ((g * t).sum(1) > 0)[sel & clear].all()
    assert ((got * -pts[:, :3]).sum(1) >= -1e-6).all()           # oriented towards the origin


@pytest.mark.parametrize("name", ["ball_k7", "ball_k20", "ball_k40", "plane", "slab", "ld6"])
def test_knn_normals_kernel_vs_float64_eigh(dev, name):
    """The kernel alone, on float64 stable-sort neighbour lists computed on the host, so that kNN tie-breaking cannot enter."""
    x, k = cases.normals_clouds()[name]
    idx = [labels_np.knn_f64(x[b], k)[0] for b in range(len(x))]
    got = _kernel_normals(dev, x, np.concatenate(idx))
    for b in range(len(x)):
        _check_normals(got[b], x[b][:, :3], idx[b])


def test_knn_normals_rank_deficient_neighbourhoods(dev):
    """k points on a line (along z, x and the diagonal) and k copies of one point: a finite unit vector, orthogonal to the line."""
    x, idx, dirs = cases.degenerate_neighbourhoods()
    k = idx.shape[1]
    got = _kernel_normals(dev, x, idx)[0].astype(np.float64)
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 4 * 2.0 ** -24
    for g, d in enumerate(dirs):
        if d is not None:
            assert np.abs(got[g * k:(g + 1) * k] @ d).max() <= 1e-6, (g, got[g * k])


def test_normals_vs_numpy_and_closed_forms(dev):
    from mlsp_amd import labels
    x = _cloud(2, 2, 1024)
    n = labels.estimate_normals(x.to(dev), near=20).cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(n, axis=-1), 1.0, atol=1e-5)
    for b in range(2):
        # every point whose 20th and 21st float64 distances are clearly apart: the neighbour SET is then unambiguous
        idx, gap = labels_np.knn_f64(x[b].numpy(), 20)
        sel = gap > 1e-6
        assert sel.mean() >= 0.99
        _check_normals(n[b], x[b].numpy(), idx, sel)
        # and all points, against the canonical fp32 neighbour lists the device search reproduces
        _check_normals(n[b], x[b].numpy(), knn_canon.knn_point_major(x[b:b + 1], 20)[0])
    # plane z = 0.3: normal = (0,0,-1) (towards the origin from above)
    g = torch.Generator().manual_seed(3)
    pl = torch.rand(1, 600, 3, generator=g) * 2 - 1
    pl[..., 2] = 0.3
    npl = labels.estimate_normals(pl.to(dev), near=20).cpu().numpy()[0]
    np.testing.assert_allclose(npl, np.tile([0, 0, -1.0], (600, 1)), atol=1e-4)
    # sphere of radius 1: normal = -p (radial, towards the centre)
    sp = torch.randn(1, 4096, 3, generator=g)
    sp = sp / sp.norm(dim=-1, keepdim=True)
    nsp = labels.estimate_normals(sp.to(dev), near=20).cpu().numpy()[0]
    assert ((nsp * -sp[0].numpy()).sum(-1) > 0.97).mean() > 0.99
