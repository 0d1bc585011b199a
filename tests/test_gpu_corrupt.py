"""On-device input corruption and PCM mixing against the reference's golden vectors and the numpy oracle."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import ref_corrupt_np as oc
import test_corrupt_oracle_cpu as cases            # the edge-case inputs; their conditions are proven there, on the CPU
from test_corrupt_oracle_cpu import GOLD, check_deform_against_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_region_assignment_bit_exact_vs_reference(dev):
    from mlsp_amd import pc_utils
    g = dict(np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz")))
    got = pc_utils.assign_region_to_point(torch.from_numpy(g["X"]).to(dev), dev)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), g["regions"])
    assert np.allclose(pc_utils.region_mean(3), g["lookup"])


@pytest.mark.parametrize("groups", [1, 3])
def test_deform_input_vs_reference_and_oracle(dev, groups):
    from mlsp_amd import mlsp
    g = dict(np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz")))
    X = torch.from_numpy(g["X"]).to(dev)
    noise = torch.randn(X.shape, generator=torch.Generator().manual_seed(groups))
    Xd, mask = mlsp.deform_input(X, torch.from_numpy(g["lookup"]), 'volume_based_voxels', dev, groups,
                                 region_ids=g["perm_g%d" % groups], noise=noise)
    assert Xd.data_ptr() == X.data_ptr()                       # in place, like the reference
    check_deform_against_reference(g["X"], Xd.cpu().numpy(), mask.cpu().numpy(), g, groups)
    want, wmask = oc.deform(g["X"], g["lookup"], g["perm_g%d" % groups], noise.numpy(), groups)
    assert np.array_equal(mask.cpu().numpy(), wmask)
    np.testing.assert_allclose(Xd.cpu().numpy(), want, rtol=0, atol=1e-7)
    # default random draws: still a valid deformation
    X2 = torch.from_numpy(g["X"]).to(dev)
    _, m2 = mlsp.deform_input(X2, torch.from_numpy(g["lookup"]), 'volume_based_voxels', dev)
    assert (m2[:, 0].sum(1) >= 40).all() and (m2[:, :3].amax(1) == m2[:, :3].amin(1)).all()


def test_pcm_mix_shapes_vs_reference(dev):
    from mlsp_amd import PCM
    g = dict(np.load(os.path.join(GOLD, "pcm_s3_B5_N256.npz")))
    args = types.SimpleNamespace(cuda=True, mixup_params=1.0, DefRec_weight=0.5)
    rng = {"index": torch.from_numpy(g["index"]), "lam": float(g["lam"]), "start_a": torch.from_numpy(g["start_a"]),
           "start_b": torch.from_numpy(g["start_b"]), "points_perm": torch.from_numpy(g["points_perm"])}
    mixed, (Ya, Yb, lam) = PCM.mix_shapes(args, torch.from_numpy(g["X"]).to(dev), torch.from_numpy(g["Y"]).to(dev), rng=rng)
    assert np.array_equal(mixed.cpu().numpy(), g["mixed"])
    assert np.array_equal(Ya.cpu().numpy(), g["Ya"]) and np.array_equal(Yb.cpu().numpy(), g["Yb"]) and lam == float(g["lam"])
    # unseeded draws: a permutation of sampled columns of the two parents
    mixed2, (_, _, lam2) = PCM.mix_shapes(args, torch.from_numpy(g["X"]).to(dev), torch.from_numpy(g["Y"]).to(dev))
    assert mixed2.shape == mixed.shape and 0.0 <= lam2 <= 1.0


def test_pc_utils_fps_vs_oracle(dev):
    from mlsp_amd import pc_utils
    gen = torch.Generator().manual_seed(2)
    xyz = torch.rand(3, 3, 500, generator=gen) * 2 - 1
    start = torch.tensor([0, 499, 123])
    idx, vals = pc_utils.farthest_point_sample(None, xyz.to(dev), 77, start=start)
    widx, wvals = oc.fps(xyz.numpy(), 77, start.numpy())
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(vals.cpu().numpy(), wvals)


def test_scan_input_vs_reference(dev):
    """mlsp.scan_input with the reference's own random draws (pixel size, rotation angles): identical survivors and mask."""
    from mlsp_amd import mlsp
    g = dict(np.load(os.path.join(GOLD, "scan_s21_B5_N512.npz")))
    X = torch.from_numpy(g["X"]).to(dev)
    Xs, mask = mlsp.scan_input(X, dev, pixel_size=float(g["pixel_size"]), angles=g["angles"])
    assert Xs.data_ptr() == X.data_ptr()
    assert np.array_equal(mask.cpu().numpy(), g["mask"]) and np.array_equal(Xs.cpu().numpy(), g["X_out"])
    # unseeded: one survivor per occupied cell, everything else zeroed
    X2 = torch.from_numpy(g["X"]).to(dev)
    Xs2, m2 = mlsp.scan_input(X2, dev)
    kept = (m2[:, :, 0] == 0)
    assert (kept.sum(1) > 100).all() and (Xs2[~kept] == 0).all() and torch.equal(Xs2[kept], torch.from_numpy(g["X"]).to(dev)[kept])


def test_deform_input_volume_based_radius(dev):
    """mlsp.deform_input(..., 'volume_based_radius') (MLSP/mlsp.py:33-36 -> pc_utils.collapse_to_point) on device: with the reference's
    recorded picks and Gaussian draws the mask is identical and the deformed cloud equal to fp32 rounding; with its own draws the
    picked point is a candidate (>= 20 points within 0.5) and exactly the points within 0.5 of it move."""
    from mlsp_amd import mlsp
    g = dict(np.load(os.path.join(GOLD, "collapse_s9_B5_N512.npz")))
    X = torch.from_numpy(g["X"]).to(dev)
    Xd, mask = mlsp.deform_input(X.clone(), None, 'volume_based_radius', dev, choice=g["choice"], noise=torch.from_numpy(g["noise"]))
    assert np.array_equal(mask.cpu().numpy(), g["mask"])
    np.testing.assert_allclose(Xd.cpu().numpy(), g["X_out"], rtol=0, atol=3e-7)
    # the trainer's calling convention: a permuted (non-contiguous) view, default draws
    Xv = torch.from_numpy(g["X"]).to(dev).permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not Xv.is_contiguous()
    orig = Xv.clone()
    X2, m2 = mlsp.deform_input(Xv, None, 'volume_based_radius', dev)
    assert X2.data_ptr() == Xv.data_ptr()
    moved = (X2 != orig).any(1)
    assert torch.equal(moved, m2[:, 0] > 0) and (m2[:, 0].sum(1) >= 20).all()
    _, _, cand = oc.collapse_to_point(g["X"], -np.ones(5, np.int32), g["noise"])
    for b in range(5):                                   # the moved set is the 0.5-ball of ONE candidate point of the original cloud
        o = orig[b].cpu().numpy()
        d2 = ((o[:, :, None] - o[:, None, :]) ** 2).sum(0)
        sets = {tuple(np.nonzero(d2[p] <= 0.25 + 1e-6)[0]) for p in np.nonzero(cand[b])[0]} | \
               {tuple(np.nonzero(d2[p] <= 0.25 - 1e-6)[0]) for p in np.nonzero(cand[b])[0]}
        assert tuple(np.nonzero(moved[b].cpu().numpy())[0]) in sets


# ---- edge cases: inputs from test_corrupt_oracle_cpu (where their conditions are asserted), expected values from the numpy oracle ----

@pytest.mark.parametrize("B,C,N", cases.REGION_SHAPES)
def test_region_assignment_faces_clamp_and_nonfinite(dev, B, C, N):
    """Coordinates exactly on the fp32 voxel faces, at and beyond +-1, on several faces at once; then NaN / +-inf coordinates: a NaN
    fails every box test (label 0), as after the reference's torch.clamp."""
    from mlsp_amd import pc_utils
    for X in (cases.region_points(B, C, N), cases.region_points_nonfinite(B, C, N)):
        got = pc_utils.assign_region_to_point(torch.from_numpy(X).to(dev), dev)
        assert got.shape == (B, N) and np.array_equal(got.cpu().numpy(), oc.assign_region(X))


@pytest.mark.parametrize("groups", [1, 2, 27])
@pytest.mark.parametrize("B,C,N", list(cases.DEFORM_CASES))
def test_deform_input_region_populations(dev, B, C, N, groups):
    """Voxels of exactly 39 (skipped) and 40 (taken) points, fewer eligible voxels than `groups`, a cloud with none, N % 256 != 0, C = 6;
    as a dense tensor, as the trainer's permuted view and as float64 -- the result lands in the caller's tensor each time."""
    from mlsp_amd import mlsp
    lookup = torch.from_numpy(np.load(os.path.join(GOLD, "deform_s5_B6_N1024.npz"))["lookup"])
    X0, _ = cases.deform_cloud(B, C, N)
    noise = torch.randn(B, 3, N, generator=torch.Generator().manual_seed(groups))
    want, wmask = oc.deform(X0, lookup.numpy(), cases.DEFORM_ORDER, noise.numpy(), groups)
    for form in ("dense", "view", "float64"):
        X = torch.from_numpy(X0).to(dev)
        if form == "view":
            X = X.permute(0, 2, 1).contiguous().permute(0, 2, 1)
            assert not X.is_contiguous()
        elif form == "float64":
            X = X.double()
        Xd, mask = mlsp.deform_input(X, lookup, 'volume_based_voxels', dev, groups, region_ids=cases.DEFORM_ORDER, noise=noise)
        assert Xd.data_ptr() == X.data_ptr() and Xd.dtype == X.dtype
        got = X.cpu().numpy()
        assert np.array_equal(mask.cpu().numpy(), wmask), form
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-7, err_msg=form)
        keep = wmask == 0                                  # rows 3.. and the cloud without a 40-point voxel among them
        assert np.array_equal(got[keep], X0[keep]), form


@pytest.mark.parametrize("pixel_size", cases.SCAN_PIXELS)
@pytest.mark.parametrize("B,N,C,dup", cases.SCAN_CASES)
def test_scan_input_ties_channels_and_sizes(dev, B, N, C, dup, pixel_size):
    """Exact twins (lowest index survives), C = 6, more than one pass of the 1024-thread loop, and the LDS opt-in size (N = 6000)."""
    from mlsp_amd import mlsp
    X0, angles = cases.scan_cloud(B, N, C, dup)
    want, wmask = oc.scan(X0, pixel_size, angles)
    X = torch.from_numpy(X0).to(dev)
    Xs, mask = mlsp.scan_input(X, dev, pixel_size=pixel_size, angles=angles)
    assert Xs.data_ptr() == X.data_ptr()
    assert np.array_equal(mask.cpu().numpy(), wmask) and np.array_equal(Xs.cpu().numpy(), want)
    if dup:
        assert (mask[:, N // 2:, 0] == 1).all() and (mask[:, :N // 2, 0] == 0).any()


def test_scan_and_collapse_reject_unsupported_sizes(dev):
    """One point more than 150 KB of LDS holds: refused on the host, nothing is launched.  So is a `choice` outside the cloud."""
    from mlsp_amd import mlsp, _lib
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        mlsp.scan_input(torch.zeros(1, 12801, 3, device=dev), dev, pixel_size=0.07, angles=np.zeros((1, 3)))
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        mlsp.deform_input(torch.zeros(1, 3, 7681, device=dev), None, 'volume_based_radius', dev)
    X = torch.from_numpy(cases.collapse_cloud(2, 16)).to(dev)
    before = X.clone()
    for bad in ([0, 16], [3], torch.tensor([40, -1])):
        with pytest.raises(ValueError):
            mlsp.deform_input(X, None, 'volume_based_radius', dev, choice=bad)
    assert torch.equal(X, before)


@pytest.mark.parametrize("B,N", cases.COLLAPSE_SHAPES)
def test_collapse_rank_selection_vs_oracle(dev, B, N):
    """The branch training uses: no `choice`, the pick is candidate number min(int(u * ncand), ncand - 1).  With `u` injected the expected
    pick follows from the oracle's candidate flags; mask identical, cloud equal to fp32 rounding.  u = 0, 0.5, the largest float below 1,
    1 itself (the clamp) and random draws; clouds without a candidate stay untouched; N = 4096 needs the LDS opt-in."""
    from mlsp_amd import mlsp
    X0 = cases.collapse_cloud(B, N)
    us, noise = cases.collapse_draws(B, N)
    cand = oc.collapse_to_point(X0, -np.ones(B, np.int64), noise)[2]
    for u in us:
        pick = oc.collapse_pick(cand, u)
        want, wmask, _ = oc.collapse_to_point(X0, pick, noise, flags=False)
        X = torch.from_numpy(X0).to(dev)
        Xd, mask = mlsp.deform_input(X, None, 'volume_based_radius', dev, noise=torch.from_numpy(noise), u=u)
        assert Xd.data_ptr() == X.data_ptr()
        assert np.array_equal(mask.cpu().numpy(), wmask), u
        np.testing.assert_allclose(X.cpu().numpy(), want, rtol=0, atol=3e-7)
        assert np.array_equal(X.cpu().numpy()[wmask == 0], X0[wmask == 0])
        for b in np.nonzero(pick < 0)[0]:
            assert wmask[b].sum() == 0 and np.array_equal(X[b].cpu().numpy(), X0[b])


def test_collapse_choice_mixed_with_draws(dev):
    """One `choice` vector with pinned picks and -1 (drawn through `u`) side by side."""
    from mlsp_amd import mlsp
    B, N = 3, 300
    X0 = cases.collapse_cloud(B, N)
    _, noise = cases.collapse_draws(B, N)
    cand = oc.collapse_to_point(X0, -np.ones(B, np.int64), noise)[2]
    u = np.float32([0.25, 0.9, 0.6])
    choice = np.array([-1, np.nonzero(cand[1])[0][3], -1])
    pick = np.where(choice >= 0, choice, oc.collapse_pick(cand, u))
    assert pick[0] >= 0 and pick[1] == choice[1] and pick[2] == -1
    want, wmask, _ = oc.collapse_to_point(X0, pick, noise)
    X = torch.from_numpy(X0).to(dev)
    _, mask = mlsp.deform_input(X, None, 'volume_based_radius', dev, noise=torch.from_numpy(noise), choice=choice, u=u)
    assert np.array_equal(mask.cpu().numpy(), wmask)
    np.testing.assert_allclose(X.cpu().numpy(), want, rtol=0, atol=3e-7)


@pytest.mark.parametrize("B,C,N,npoint,dup", cases.FPS_CASES)
def test_pc_utils_fps_sizes_and_ties(dev, B, C, N, npoint, dup):
    """npoint = N, npoint = 1, C = 6, both FPS kernels (N below and above 64), and clouds of twins whose arg-max ties go to index 0."""
    from mlsp_amd import pc_utils
    X, start = cases.fps_cloud(B, C, N, dup)
    idx, vals = pc_utils.farthest_point_sample(None, torch.from_numpy(X).to(dev), npoint, start=torch.from_numpy(start))
    widx, wvals = oc.fps(X, npoint, start)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(vals.cpu().numpy(), wvals)


@pytest.mark.parametrize("lam", cases.PCM_LAMS)
def test_pcm_mixes_vs_oracle(dev, lam):
    """mix_shapes and mix_shapes_segmentation with injected draws at lam = 0 (nothing from the first parent), 1 (everything) and 0.37,
    N = 33, one cloud with repeated points: points and per-point labels identical to the oracle."""
    from mlsp_amd import PCM
    X, Y, d = cases.pcm_case()
    B = X.shape[0]
    args = types.SimpleNamespace(cuda=True, mixup_params=1.0, DefRec_weight=0.5)
    rng = dict({k: torch.from_numpy(v) for k, v in d.items()}, lam=lam)
    draws = (d["index"], lam, d["start_a"], d["start_b"], d["points_perm"])
    Ycls = torch.arange(B, device=dev)
    mixed, (Ya, Yb, got_lam) = PCM.mix_shapes(args, torch.from_numpy(X).to(dev), Ycls, rng=rng)
    assert np.array_equal(mixed.cpu().numpy(), oc.mix_shapes(X, *draws)) and got_lam == lam
    assert torch.equal(Ya, Ycls) and np.array_equal(Yb.cpu().numpy(), d["index"])
    mixed_X, mixed_Y = PCM.mix_shapes_segmentation(args, torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), rng=rng)
    want_X, want_Y = oc.mix_shapes_segmentation(X, Y, *draws)
    assert mixed_X.shape == X.shape and np.array_equal(mixed_X.cpu().numpy(), want_X)
    assert mixed_Y.dtype == torch.int64 and np.array_equal(mixed_Y.cpu().numpy(), want_Y)
