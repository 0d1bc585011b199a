"""oracle/ref_corrupt_np.py against the reference's own outputs (tests/golden/deform_*.npz, pcm_*.npz).  CPU only.

The second half builds the inputs of the edge-case tests in tests/test_gpu_corrupt.py and tests/test_gpu_labels.py and checks, without a
GPU, every condition those tests rely on (region populations, absence of ambiguous pairs, ...)."""
import os

import numpy as np
import pytest

from oracle import labels_np
from oracle import ref_corrupt_np as oc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_deform_against_reference(X_in, X_out, mask, g, groups):
    """Everything deterministic must be identical: the mask, the untouched coordinates; the replaced points are Gaussian
    around the chosen voxel centres (numpy's RNG stream cannot be reproduced): checked statistically."""
    ref_mask, ref_out = g["mask_g%d" % groups], g["X_out_g%d" % groups]
    assert np.array_equal(mask, ref_mask)
    keep = ref_mask[:, 0] == 0
    for b in range(X_in.shape[0]):
        assert np.array_equal(X_out[b][:, keep[b]], ref_out[b][:, keep[b]])
        hit = ~keep[b]
        assert hit.sum() >= 40
        regs = np.unique(g["regions"][b][hit])
        assert len(regs) <= groups
        for r in regs:
            sel = hit & (g["regions"][b] == r)
            d = X_out[b][:, sel] - g["lookup"][r][:, None]
            assert np.abs(d.mean(1)).max() < 4 * np.sqrt(0.001 / sel.sum()) + 1e-3
            assert abs(d.std() - np.sqrt(0.001)) < 0.3 * np.sqrt(0.001)


def test_region_assignment_bit_exact():
    g = dict(np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz")))
    assert np.array_equal(oc.assign_region(g["X"]), g["regions"])


def test_deform_oracle_vs_reference():
    g = dict(np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz")))
    rs = np.random.RandomState(0)
    for groups in (1, 3):
        noise = rs.randn(*g["X"].shape).astype(np.float32)
        X_out, mask = oc.deform(g["X"], g["lookup"], g["perm_g%d" % groups], noise, groups)
        check_deform_against_reference(g["X"], X_out, mask, g, groups)


def test_pcm_oracle_vs_reference():
    g = dict(np.load(os.path.join(GOLD, "pcm_s3_B5_N256.npz")))
    mixed = oc.mix_shapes(g["X"], g["index"], float(g["lam"]), g["start_a"], g["start_b"], g["points_perm"])
    assert np.array_equal(mixed, g["mixed"])


def test_scan_oracle_vs_reference():
    g = dict(np.load(os.path.join(GOLD, "scan_s21_B5_N512.npz")))
    out, mask = oc.scan(g["X"], float(g["pixel_size"]), g["angles"])
    assert np.array_equal(mask, g["mask"]) and np.array_equal(out, g["X_out"])


def test_collapse_to_point_oracle_vs_reference():
    """deform_input(..., 'volume_based_radius'): oracle/ref_corrupt_np.collapse_to_point with the reference's recorded draws reproduces
    the reference's mask exactly and its deformed cloud to fp32 rounding (tests/golden/collapse_*.npz, tools/make_golden.py radius)."""
    g = dict(np.load(os.path.join(GOLD, "collapse_s9_B5_N512.npz")))
    X, mask, cand = oc.collapse_to_point(g["X"], g["choice"], g["noise"])
    assert np.array_equal(mask, g["mask"])
    np.testing.assert_allclose(X, g["X_out"], rtol=0, atol=2e-7)
    assert all(cand[b, g["choice"][b]] for b in range(len(g["choice"])))       # the reference only picks candidates
    keep = g["mask"] == 0
    assert np.array_equal(X[keep], g["X"][keep])


def test_segmentation_mix_oracle_vs_reference():
    """mix_shapes_segmentation restates mix_shapes for the points (the reference's recorded mix) and carries every label with its point."""
    g = dict(np.load(os.path.join(GOLD, "pcm_s3_B5_N256.npz")))
    B, _, N = g["X"].shape
    Y = np.arange(B * N, dtype=np.int64).reshape(B, N)               # a label that names its point
    draws = (g["index"], float(g["lam"]), g["start_a"], g["start_b"], g["points_perm"])
    mixed, mixed_Y = oc.mix_shapes_segmentation(g["X"], Y, *draws)
    assert np.array_equal(mixed, g["mixed"]) and np.array_equal(mixed, oc.mix_shapes(g["X"], *draws))
    assert np.array_equal(g["X"][mixed_Y // N, :, mixed_Y % N].transpose(0, 2, 1), mixed)
    na = round(float(g["lam"]) * N)                                  # the first parent gives na points, the shuffled one the rest
    assert ((mixed_Y // N == np.arange(B)[:, None]).sum(1) >= na).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# Inputs of the GPU edge-case tests.  Each builder is deterministic; the test next to it proves what the GPU test assumes.

def ball_cloud(seed, B, N):
    """torch [B,N,3]: uniform in the unit ball"""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, N, 3, generator=g) * 2 - 1
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-6) * torch.rand(B, N, 1, generator=g) ** (1 / 3)


THR = np.array([-1 + i * (2 / 3) for i in range(4)], dtype=np.float64).astype(np.float32)      # voxel faces, as torch rounds them
CLIP = np.float32(0.99999999)
REGION_SHAPES = [(1, 3, 1), (2, 3, 257), (3, 6, 300)]


def region_points(B, C, N):
    """X [B,C,N]: random points (some beyond +-1) with constructed ones in the leading columns: coordinates exactly on every fp32
    face, at +-1, +-1.5 (clamped) and +-fp32(0.99999999), on one, two and three axes at once; the other axes strictly inside a voxel."""
    rs = np.random.RandomState(100 + N)
    X = (rs.rand(B, C, N) * 2.4 - 1.2).astype(np.float32)
    special = np.concatenate([THR, [1.5, -1.5, CLIP, -CLIP, np.nextafter(THR[1], np.float32(1)), np.nextafter(THR[2], np.float32(-1))]])
    pts = []
    for axes in [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:
        for i, v in enumerate(special):
            p = np.array([0.5, -0.5, 0.0], np.float32)
            for a in axes:
                p[a] = special[(i + a) % len(special)] if len(axes) > 1 else v
            pts.append(p)
    pts = np.array(pts, np.float32)
    for b in range(B):
        n = min(N, len(pts))
        X[b, :3, :n] = np.roll(pts, b, axis=0)[:n].T
    return X


def region_points_nonfinite(B, C, N):
    """region_points with NaN, +inf and -inf in one axis of a few points whose other two coordinates lie strictly inside voxels."""
    X = region_points(B, C, N)
    for j, (a, v) in enumerate([(0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (1, -np.inf), (2, np.inf)]):
        if j < N:
            X[:, :3, j] = 0.5
            X[:, a, j] = v
    return X


@pytest.mark.parametrize("B,C,N", REGION_SHAPES)
def test_region_inputs_hit_faces_and_clamp(B, C, N):
    X = region_points(B, C, N)
    onface = np.isin(X[:, :3], THR).sum(1)                                    # how many axes of each point sit on a face
    assert np.isin(THR, X[:, :3]).all() if N > 1 else onface.max() == 1
    if N > 1:
        assert {1, 2, 3} <= set(np.unique(onface)) and (np.abs(X[:, :3]) > 1).any() and (X[:, :3] == CLIP).any()
        Y = oc.assign_region(X)
        assert (Y[onface > 0] == 0).all() and len(np.unique(Y)) == 27
        nf = region_points_nonfinite(B, C, N)
        Yn = oc.assign_region(nf)
        assert np.isnan(nf[:, :3, :3]).any() and (Yn[:, :6] == 0).all()       # NaN fails every comparison; +-inf is clamped onto the outer face
        # the kernel's fminf(fmaxf()) turns a NaN into -clip instead; fp32(0.99999999) is 1, the outer face, so that point has no box either.
        # With a clip strictly inside the cube it would have one (here voxel 0 along the NaN axis): what the GPU test guards against
        assert CLIP == 1 and (oc.assign_region(np.where(np.isnan(nf), -CLIP, nf))[:, :3] == 0).all()
        assert (oc.assign_region(np.where(np.isnan(nf), np.float32(-0.999), nf))[:, :3] != 0).all()


DEFORM_ORDER = np.random.RandomState(7).permutation(27)
# (B,C,N) -> per cloud the number of points in the 1st, 2nd, ... voxel of the visiting order; None: spread over all 27 voxels (<= 12 each)
DEFORM_CASES = {
    (2, 3, 257): [[39, 40, 60, 45, 38, 35], None],
    (2, 6, 300): [[39, 40, 41, 100, 39, 41], None],
    (1, 3, 100): [[39, 40, 21]],
}


def deform_cloud(B, C, N):
    """X [B,C,N] whose points lie strictly inside chosen voxels (DEFORM_CASES), in shuffled order, and their voxel ids [B,N]."""
    rs = np.random.RandomState(200 + N)
    X = rs.randn(B, C, N).astype(np.float32)
    regions = np.zeros((B, N), np.int64)
    for b, counts in enumerate(DEFORM_CASES[(B, C, N)]):
        r = np.arange(N) % 27 if counts is None else np.repeat(DEFORM_ORDER[:len(counts)], counts)
        r = r[rs.permutation(N)]
        centre = np.stack([r // 9, (r // 3) % 3, r % 3]).astype(np.float64) * (2 / 3) - 1 + 1 / 3
        X[b, :3] = (centre + rs.uniform(-0.3, 0.3, (3, N))).astype(np.float32)
        regions[b] = r
    return X, regions


@pytest.mark.parametrize("B,C,N", list(DEFORM_CASES))
@pytest.mark.parametrize("groups", [1, 2, 27])
def test_deform_inputs_and_oracle_on_region_populations(B, C, N, groups):
    lookup = np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz"))["lookup"]
    X, regions = deform_cloud(B, C, N)
    assert np.array_equal(oc.assign_region(X), regions)
    noise = np.random.RandomState(groups).randn(B, 3, N).astype(np.float32)
    out, mask = oc.deform(X, lookup, DEFORM_ORDER, noise, groups)
    for b, counts in enumerate(DEFORM_CASES[(B, C, N)]):
        hist = np.bincount(regions[b], minlength=27)[DEFORM_ORDER]
        if counts is None:
            assert hist.max() < 40 and mask[b].sum() == 0 and np.array_equal(out[b], X[b])
            continue
        assert hist[0] == 39 and hist[1] == 40
        eligible = np.nonzero(hist >= 40)[0]
        taken = DEFORM_ORDER[eligible[:groups]]                                # fewer than `groups` when the order runs out
        assert len(taken) == min(groups, len(eligible)) and (groups < 27 or len(taken) < groups)
        want = np.isin(regions[b], taken)
        assert np.array_equal(mask[b, :3], np.tile(want, (3, 1)).astype(np.float32)) and mask[b, 3:].sum() == 0
        assert np.array_equal(out[b][:, ~want], X[b][:, ~want]) and np.array_equal(out[b, 3:], X[b, 3:])
        assert np.abs(out[b, :3][:, want] - lookup[regions[b][want]].T).max() < 6 * np.sqrt(0.001)


SCAN_CASES = [(2, 70, 6, True), (1, 1500, 3, False), (1, 6000, 3, False)]       # B, N, C, second half a copy of the first
SCAN_PIXELS = [0.3, 0.045]


def scan_cloud(B, N, C, dup):
    """X [B,N,C] in the unit ball (+ extra channels) and rotation angles [B,3]"""
    rs = np.random.RandomState(300 + N)
    X = rs.randn(B, N, C).astype(np.float32)
    X[..., :3] = ball_cloud(300 + N, B, N).numpy()
    if dup:
        X[:, N // 2:] = X[:, :N // 2]
    return X, rs.rand(B, 3) * 2 * np.pi


@pytest.mark.parametrize("B,N,C,dup", SCAN_CASES)
def test_scan_inputs_collide_and_tie(B, N, C, dup):
    X, angles = scan_cloud(B, N, C, dup)
    for pixel_size in SCAN_PIXELS:
        out, mask = oc.scan(X, pixel_size, angles)
        kept = mask[:, :, 0] == 0
        assert np.array_equal(out[kept], X[kept]) and (out[~kept] == 0).all() and (mask[:, :, 3:] == 1).all()
        if dup:                                                          # every point has an exact twin: only the lower index may survive
            assert not kept[:, N // 2:].any() and (kept.sum(1) > 0).all()
        if pixel_size == 0.3:
            assert (kept.sum(1) <= 43).all() and (kept.sum(1) < (N // 2 if dup else N)).all()       # cell ids 0..42: points collide
    assert (N * 12 > 64 * 1024) == (N == 6000)                           # only the last case needs more than 64 KB of LDS


COLLAPSE_SHAPES = [(2, 16), (3, 300), (1, 4096)]


def collapse_cloud(B, N):
    """X [B,3,N].  N = 16: too few points for a candidate.  N = 300: unit-ball clouds, the last one blown up threefold so that it has no
    candidate.  N = 4096: a jittered 16^3 lattice of pitch 0.11 in shuffled order -- squared distances cluster around 0.0121 m, which
    keeps every pair clear of r^2 = 0.25 (a random cloud of this size always has pairs within fp32 rounding of it)."""
    rs = np.random.RandomState(400 + N)
    if N == 4096:
        g = np.stack(np.meshgrid(*[np.arange(16) - 7.5] * 3, indexing="ij"), 0).reshape(3, -1) * 0.11
        X = (g + rs.uniform(-2e-4, 2e-4, g.shape))[:, rs.permutation(N)][None].astype(np.float32)
    else:
        X = ball_cloud(400 + N, B, N).numpy().transpose(0, 2, 1).copy()
        if N == 300:
            X[-1] *= 3
    return np.ascontiguousarray(X)


def collapse_draws(B, N):
    """the `u` vectors the rank-selection test uses, and the noise"""
    rs = np.random.RandomState(500 + N)
    top = np.float32(1) - np.float32(2.0 ** -24)
    us = [np.zeros(B, np.float32), np.full(B, 0.5, np.float32), np.full(B, top, np.float32), np.ones(B, np.float32),
          rs.rand(B).astype(np.float32), rs.rand(B).astype(np.float32)]
    return us, rs.randn(B, 3, N).astype(np.float32)


@pytest.mark.parametrize("B,N", COLLAPSE_SHAPES)
def test_collapse_inputs_have_no_ambiguous_pair(B, N):
    """The kernel forms x_i.x_j with fmaf, the oracle does not: candidate flags and masks are comparable bit for bit only when no pair
    sits within fp32 rounding of the radius.  Asserted here, not masked out there."""
    X = collapse_cloud(B, N)
    assert oc.collapse_ambiguous_pairs(X) == 0
    _, mask, cand = oc.collapse_to_point(X, -np.ones(B, np.int64), np.zeros((B, 3, N), np.float32))
    assert mask.sum() == 0
    ncand = cand.sum(1)
    if N == 16:
        assert (ncand == 0).all()
    elif N == 300:
        assert (ncand[:-1] > 20).all() and (ncand[:-1] < N).all() and ncand[-1] == 0
    else:
        assert ncand[0] == N and N * 20 > 64 * 1024
    us, _ = collapse_draws(B, N)
    picks = [oc.collapse_pick(cand, u) for u in us]
    for b in range(B):
        ids = np.nonzero(cand[b])[0]
        if len(ids):
            assert picks[0][b] == ids[0] and picks[2][b] == ids[-1] and picks[3][b] == ids[-1] and picks[1][b] == ids[len(ids) // 2]
            assert int(us[3][b] * np.float32(len(ids))) == len(ids)        # u == 1: the product reaches ncand, only the clamp keeps the rank in range
        else:
            assert all(p[b] == -1 for p in picks)


def test_largest_u_below_one_never_reaches_ncand():
    """fp32(1 - 2^-24) * fp32(ncand) = ncand - ncand 2^-24 lies more than half an ulp below ncand, so it rounds to the float below ncand
    for every ncand the kernel supports: with u in [0,1) the rank is in range before the clamp.  The clamp only matters for u == 1, which
    is what a float64 draw above 1 - 2^-25 becomes in fp32; collapse_draws has that case."""
    n = np.arange(1, 7681).astype(np.float32)
    top = np.float32(1) - np.float32(2.0 ** -24)
    assert ((top * n) < n).all() and ((top * n).astype(np.int64) == np.arange(1, 7681) - 1).all()
    assert np.float32(np.float64(1) - 2.0 ** -26) == np.float32(1)


DENSITY_CASES = [(3, 512, 0.2), (2, 1024, 0.135), (1, 300, 0.5), (2, 300, 0.5), (1, 1000, 0.135), (2, 257, 0.3), (1, 6000, 0.135)]


@pytest.mark.parametrize("B,N,radius", DENSITY_CASES)
def test_density_inputs_are_rarely_ambiguous(B, N, radius):
    x = ball_cloud(1, B, N).numpy()
    amb = 0
    for b in range(B):
        lo, hi = labels_np.radius_count_bounds(x[b], radius)
        want = labels_np.radius_count(x[b], radius)
        assert (lo <= want).all() and (want <= hi).all()
        amb += (lo != hi).sum()
    assert amb <= 0.01 * B * N


def density_special_clouds():
    """name -> (x [B,N,ld], radius, K): a saturated cloud, point 0 far from the rest, copies of point 0 inside the cloud, extra columns"""
    rs = np.random.RandomState(600)
    dense = ball_cloud(5, 1, 400).numpy()
    far = ball_cloud(6, 2, 257).numpy() * 0.5
    far[:, 0] = [3.0, 3.0, 3.0]
    copies = ball_cloud(7, 2, 300).numpy()
    copies[:, 5::50] = copies[:, :1]
    wide = np.concatenate([ball_cloud(8, 2, 300).numpy(), rs.randn(2, 300, 3).astype(np.float32) * 10], -1)
    return {"dense": (dense, 2.0, 100), "far0": (far, 0.3, 100), "copies0": (copies, 0.3, 100), "ld6": (wide, 0.3, 100),
            "small_K": (ball_cloud(9, 2, 300).numpy(), 0.3, 7)}


def test_density_special_clouds_do_what_they_say():
    c = density_special_clouds()
    x, r, K = c["dense"]
    assert (labels_np.radius_count(x[0], r, K) == K - 1).all()                # every count saturates and point 0 is always in range
    x, r, K = c["far0"]
    d0 = np.linalg.norm(x[:, 1:] - x[:, :1], axis=-1)
    assert d0.min() > 1.0 and labels_np.radius_count(x[0], r, K)[0] == 0       # nobody but point 0 subtracts; alone, its count is 1 - 1
    x, r, K = c["copies0"]
    assert (x[:, 5::50] == x[:, :1]).all() and (labels_np.radius_count(x[0], r, K)[5::50] == labels_np.radius_count(x[0], r, K)[0]).all()
    x, r, K = c["small_K"]
    cnt = labels_np.radius_count(x[0], r, K)
    assert (cnt == K).any() and (cnt == K - 1).any() and (cnt < K - 1).any()   # clamped without / with the point-0 subtraction, and unclamped
    for name, (x, r, K) in c.items():
        for b in range(len(x)):
            lo, hi = labels_np.radius_count_bounds(x[b], r, K)
            assert (lo != hi).mean() <= 0.01, name


def normals_clouds():
    """name -> (x [B,N,ld] float32, k)"""
    rs = np.random.RandomState(700)
    e1, e2 = np.array([0.6, 0.48, 0.64]), np.array([-0.8, 0.36, 0.48])      # orthonormal, off the axes
    ab = rs.uniform(-1, 1, (2, 400))
    plane = (np.array([0.3, -0.2, 0.5])[:, None] + e1[:, None] * ab[0] + e2[:, None] * ab[1]).T[None]
    slab = plane + np.cross(e1, e2)[None, None, :] * rs.uniform(-1e-3, 1e-3, (1, 400, 1))
    wide = np.concatenate([ball_cloud(13, 1, 300).numpy(), rs.randn(1, 300, 3) * 10], -1)
    return {"ball_k7": (ball_cloud(10, 2, 200).numpy(), 7), "ball_k20": (ball_cloud(11, 1, 600).numpy(), 20),
            "ball_k40": (ball_cloud(12, 1, 300).numpy(), 40), "plane": (plane.astype(np.float32), 12), "slab": (slab.astype(np.float32), 20),
            "ld6": (wide.astype(np.float32), 20)}


def degenerate_neighbourhoods(k=9):
    """x [1,N,3] and forced indices [N,k]: point i's neighbourhood is group i // k -- k points on a line along z, along x, along
    (1,1,1)/sqrt(3) (fp32-exactly collinear), and k identical points.  -> (x, idx, line direction per group or None)"""
    t = np.linspace(-0.4, 0.5, k).astype(np.float32)
    o = np.float32(0.25)
    groups = [np.stack([o + 0 * t, -o + 0 * t, t], 1), np.stack([t, o + 0 * t, o + 0 * t], 1), np.stack([t, t, t], 1),
              np.tile(np.float32([0.3, -0.1, 0.7]), (k, 1))]
    dirs = [np.array([0, 0, 1.0]), np.array([1.0, 0, 0]), np.ones(3) / np.sqrt(3), None]
    x = np.concatenate(groups)[None].astype(np.float32)
    idx = (np.arange(len(groups) * k) // k * k)[:, None] + np.arange(k)[None, :]
    return x, idx.astype(np.int32), dirs


def test_normals_inputs():
    for name, (x, k) in normals_clouds().items():
        for b in range(len(x)):
            idx, gap = labels_np.knn_f64(x[b], k)
            assert (idx[:, 0] == np.arange(x.shape[1])).all()                  # self first
            want, w = labels_np.knn_normals(x[b][:, :3], idx)
            bar = labels_np.normal_sin_bar(w)
            assert np.isfinite(bar).all() and np.median(bar) < 1e-5, name
            # what the fp32 cast of the covariance alone costs stays inside the bar (the kernel's solver has the rest)
            nb = x[b][:, :3].astype(np.float64)[idx]
            c = nb - nb.mean(1, keepdims=True)
            cov32 = (np.einsum("nki,nkj->nij", c, c) / k).astype(np.float32).astype(np.float64)
            v = np.linalg.eigh(cov32)[1][:, :, 0]
            assert (np.linalg.norm(np.cross(v, want.astype(np.float64)), axis=1) <= bar).all(), name
    x, _ = normals_clouds()["slab"]
    w = labels_np.knn_normals(x[0], labels_np.knn_f64(x[0], 20)[0])[1]
    assert np.median(w[:, 0] / w[:, 2]) < 1e-4
    x, idx, dirs = degenerate_neighbourhoods()
    w = labels_np.knn_normals(x[0], idx)[1]
    assert (w[:, 1] <= 1e-15).all() and (w[:27, 2] > 1e-3).all() and (w[27:, 2] == 0).all()      # rank <= 1 everywhere, 0 for the copies


def test_normals_end_to_end_selection():
    """The end-to-end check of estimate_normals applies to the points whose k-th and (k+1)-th float64 distances differ by more than
    1e-6 relative: at least 99 % of the cloud, and there the canonical fp32 kNN (which the device search equals bit for bit) finds
    the float64 neighbour set."""
    from oracle import knn_canon
    x = ball_cloud(2, 2, 1024)
    for b in range(2):
        idx, gap = labels_np.knn_f64(x[b].numpy(), 20)
        sel = gap > 1e-6
        assert sel.mean() >= 0.99
        canon = knn_canon.knn_point_major(x[b:b + 1], 20)[0]
        assert np.array_equal(np.sort(canon[sel], 1), np.sort(idx[sel], 1))


PCM_LAMS = [0.0, 1.0, 0.37]


def pcm_case(B=3, N=33, C=3):
    """X [B,C,N] (the last cloud's second half repeats its first), per-point labels Y [B,N], and the draws of one mix"""
    rs = np.random.RandomState(800 + N)
    X = rs.uniform(-1, 1, (B, C, N)).astype(np.float32)
    X[-1, :, N // 2:2 * (N // 2)] = X[-1, :, :N // 2]
    Y = rs.randint(0, 8, (B, N)).astype(np.int64)
    draws = {"index": rs.permutation(B), "start_a": rs.randint(0, N, B), "start_b": rs.randint(0, N, B), "points_perm": rs.permutation(N)}
    return X, Y, draws


FPS_CASES = [(2, 3, 33, 33, False), (2, 3, 33, 1, False), (1, 6, 300, 77, False), (2, 3, 32, 32, True), (1, 3, 128, 128, True)]


def fps_cloud(B, C, N, dup):
    rs = np.random.RandomState(900 + N + dup)
    X = rs.uniform(-1, 1, (B, C, N)).astype(np.float32)
    if dup:
        X[:, :, N // 2:] = X[:, :, :N // 2]
    return X, rs.randint(0, N, B)


def test_fps_inputs_tie():
    for B, C, N, npoint, dup in FPS_CASES:
        X, start = fps_cloud(B, C, N, dup)
        idx, vals = oc.fps(X, npoint, start)
        assert np.array_equal(vals, np.take_along_axis(X, idx[:, None, :].repeat(C, 1), 2))
        if dup:         # N/2 distinct points: once they are used up every distance is 0 and the arg-max tie goes to index 0
            first = idx[:, :N // 2] % (N // 2)
            assert all(len(np.unique(f)) == N // 2 for f in first) and (idx[:, N // 2:] == 0).all()
        elif npoint == N:
            assert all(len(np.unique(i)) == N for i in idx)


@pytest.mark.parametrize("lam", PCM_LAMS)
def test_pcm_inputs(lam):
    X, Y, d = pcm_case()
    N = X.shape[2]
    mixed, mixed_Y = oc.mix_shapes_segmentation(X, Y, d["index"], lam, d["start_a"], d["start_b"], d["points_perm"])
    assert np.array_equal(mixed, oc.mix_shapes(X, d["index"], lam, d["start_a"], d["start_b"], d["points_perm"]))
    assert mixed.shape == X.shape and mixed_Y.shape == Y.shape
    assert round(lam * N) == {0.0: 0, 1.0: N, 0.37: 12}[lam]
    if lam == 1.0:            # all of the first parent: a permutation of it where its points are distinct (every cloud but the last)
        assert np.array_equal(np.sort(mixed[0], 1), np.sort(X[0], 1)) and np.array_equal(np.sort(mixed_Y[0]), np.sort(Y[0]))
    if lam == 0.0:            # all of the shuffled parent
        b = int(np.nonzero(d["index"] != len(X) - 1)[0][0])
        assert np.array_equal(np.sort(mixed[b], 1), np.sort(X[d["index"][b]], 1))
