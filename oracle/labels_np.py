"""ORACLE -- test infrastructure, NOT the product.  PARITY UNPINNED.

numpy restatement of the two python-pcl calls behind the reference's label generators (MLSP/mlsp.py:240-272,
PointDA/trainer.py:173-188).  python-pcl (conda `sirokujira`, unpinned, README.md:24-25) is not in the reference tree
and not installable here, so nothing from the reference pins these functions; they restate the published algorithms:
  * FLANN/PCL radius search: neighbours with squared L2 distance < radius^2 (the query itself included), at most K,
    nearest first; the reference then counts `(ind != 0).sum(1)`, i.e. every returned index except 0.
  * PCL NormalEstimation with KSearch(k): covariance of the k nearest points (self included), eigenvector of the
    smallest eigenvalue, flipped so that n . (viewpoint - p) >= 0 with viewpoint (0,0,0).
"""
import numpy as np


ROW_CHUNK = 512       # rows of an N x N pair matrix held at a time


def radius_count(pts, radius, K=100):
    """pts [N,>=3] float32 -> int64 [N]"""
    p = pts[:, :3].astype(np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    cnt = np.empty(len(p), np.int64)
    for lo in range(0, len(p), ROW_CHUNK):
        d = p[lo:lo + ROW_CHUNK, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        within = d2 < r2
        cnt[lo:lo + ROW_CHUNK] = np.minimum(within.sum(1), K) - within[:, 0].astype(np.int64)
    return np.maximum(cnt, 0)


def radius_count_bounds(pts, radius, K=100, ulps=8.0):
    """float64 bracket of radius_count: (lo, hi) int64 [N].  A pair is ambiguous when |d^2 - r^2| <= ulps * 2^-24 * (d^2 + r^2) (an fp32
    evaluation of d^2 may land on either side of r^2); lo counts the pairs with d^2 < r^2 that are not ambiguous, hi those and the ambiguous
    ones, and each is then combined like radius_count: min(count, K) - [point 0 in range], floored at 0."""
    p = pts[:, :3].astype(np.float32).astype(np.float64)
    r2 = float(np.float32(radius) * np.float32(radius))
    lo_c, hi_c = np.empty(len(p), np.int64), np.empty(len(p), np.int64)
    for s in range(0, len(p), ROW_CHUNK):
        d = p[s:s + ROW_CHUNK, None, :] - p[None, :, :]
        d2 = (d * d).sum(-1)
        amb = np.abs(d2 - r2) <= ulps * 2.0 ** -24 * (d2 + r2)
        for dst, within in ((lo_c, (d2 < r2) & ~amb), (hi_c, (d2 < r2) | amb)):
            dst[s:s + ROW_CHUNK] = np.minimum(within.sum(1), K) - within[:, 0].astype(np.int64)
    return np.maximum(lo_c, 0), np.maximum(hi_c, 0)


def knn_f64(pts, k):
    """float64 k nearest neighbours (self included; stable sort: ties to the lowest index).  pts [N,>=3] -> (idx int32 [N,k],
    gap [N]: the relative difference between the k-th and the (k+1)-th squared distance, inf when k == N)."""
    p = pts[:, :3].astype(np.float64)
    idx = np.empty((len(p), k), np.int32)
    gap = np.full(len(p), np.inf)
    for s in range(0, len(p), ROW_CHUNK):
        d = p[s:s + ROW_CHUNK, None, :] - p[None, :, :]
        d2 = (d * d).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")
        idx[s:s + ROW_CHUNK] = order[:, :k]
        if k < len(p):
            srt = np.take_along_axis(d2, order[:, k - 1:k + 1], 1)
            gap[s:s + ROW_CHUNK] = (srt[:, 1] - srt[:, 0]) / np.maximum(srt[:, 1], 1e-300)
    return idx, gap


def normal_sin_bar(w):
    """Per-point bound on sin(angle) between the float64 normal and one computed from the fp32-rounded covariance, for eigenvalues
    w [N,3] ascending: Davis-Kahan for an entrywise relative error u = 2^-24 of a symmetric 3x3 (6 u w2 / (w1 - w0)) plus the fp32
    rounding of the three output components (4 u).  inf where w1 == w0 (no unique normal)."""
    u = 2.0 ** -24
    gap = w[:, 1] - w[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gap > 0, 6 * u * w[:, 2] / gap, np.inf) + 4 * u


def cal_density(batch_pts, radius, num_cls, pergroup=2, shift=0, K=100):
    """MLSP/mlsp.py:240-272 with radius_count in place of the pcl call."""
    cls_all, row_all = [], []
    for pts in batch_pts:
        row = radius_count(np.asarray(pts), radius, K) - shift
        row[row < 0] = 0
        row[row > (num_cls - 1) * pergroup] = (num_cls - 1) * pergroup
        c1 = np.floor(row / pergroup).astype(np.int32)
        c2 = np.ceil(row / pergroup).astype(np.int32)
        eye = np.identity(num_cls)
        cls_all.append((eye[c1] + eye[c2]) / 2.0)
        row_all.append(row)
    return np.array(cls_all), np.array(row_all)


def knn_normals(pts, idx):
    """pts [N,3], idx [N,k] (self included) -> unit normals [N,3] oriented towards the origin."""
    p = pts.astype(np.float64)
    nb = p[idx]                                       # [N,k,3]
    c = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c) / idx.shape[1]
    w, v = np.linalg.eigh(cov)
    n = v[:, :, 0]
    flip = (n * (-p)).sum(1) < 0
    n[flip] = -n[flip]
    return n.astype(np.float32), w
