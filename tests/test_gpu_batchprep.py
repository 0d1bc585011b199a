"""Batch preparation on the device (mlsp_amd/data.py, csrc/batchprep.hip) against its numpy restatement (tests/batchprep_restatement.py)
and the reference's recorded results (tests/golden/batchprep_s0.npz).  Tolerances: the unit cube is one rounding (2^-25 for values in
[-1, 1]) of a float64 result whose reduction order differs from the restatement's, bounded by 2^-23; every other stage is a fixed
sequence of IEEE operations and is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import batchprep_restatement as br

pytestmark = pytest.mark.gpu

FX = br.fixture()["cases"]
RAW, PRE, POST, JIT = br.F_RAW, br.F_PRE, br.F_POST, br.F_JITTER
DEV = "cuda:0"


def _pad(clouds):
    """list of [n,3] float32 -> (device [B,Nmax,3] with the tails filled with 1e30, counts)"""
    nmax = max(c.shape[0] for c in clouds)
    raw = np.full((len(clouds), nmax, 3), 1e30, dtype=np.float32)
    for b, c in enumerate(clouds):
        raw[b, :c.shape[0]] = c
    return torch.from_numpy(raw).to(DEV), [c.shape[0] for c in clouds]


def _run(clouds, S, flags, start=None, Rpre=None, Rpost=None, noise=None, sigma=0.01, clip=0.02):
    from mlsp_amd import data
    raw, counts = _pad(clouds)
    B = len(clouds)

    def dev(a, dt):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()
    if start is None:
        start = [0] * B
    out, idx = data._run(raw, S, counts, flags, dev(start, torch.int32), dev(Rpre, torch.float64), dev(Rpost, torch.float64),
                         dev(noise, torch.float64), sigma, clip)
    torch.cuda.synchronize()
    return out.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _Rx():
    from mlsp_amd import data
    return data.axis_rotation("x", -np.pi / 2)


UNIT_CLOUDS = ["scannet_val_24", "modelnet_val_33", "modelnet_train_257", "scannet_train_2048"]


def test_unit_cube_alone():
    from mlsp_amd import pc_utils
    clouds = [FX[n]["raw"] for n in UNIT_CLOUDS]
    assert [c.shape[0] for c in clouds] == [24, 33, 257, 2048]
    # the ragged batch: the sampled points of every cloud, twice
    out, idx = _run(clouds, 24, [0] * 4, start=[0, 5, 100, 2047])
    out2, idx2 = _run(clouds, 24, [0] * 4, start=[0, 5, 100, 2047])
    assert br.same_bits(out, out2) and np.array_equal(idx, idx2)
    for b, c in enumerate(clouds):
        want = br.unit_cube64(c)[idx[b]]
        assert np.abs(out[b].astype(np.float64) - want).max() <= 2.0 ** -23
    # every point of every cloud, the off-centre one included
    for name in UNIT_CLOUDS + ["shapenet_train_off50_2048"]:
        x = torch.from_numpy(FX[name]["raw"].copy()).to(DEV)
        keep = x.clone()
        got = pc_utils.scale_to_unit_cube(x)
        assert torch.equal(x, keep)                                # the twin does not scale its argument in place
        got = got.cpu().numpy()
        d = float(np.abs(got.astype(np.float64) - br.unit_cube64(FX[name]["raw"])).max())
        print("%s: |device - float64| %.3e (reference's own error %.3e)" % (name, d, float(FX[name]["own_error"])))
        assert d <= 2.0 ** -23
        assert d <= float(FX[name]["own_error"])
        assert np.abs(got).max() <= 1.0
        assert br.same_bits(got, pc_utils.scale_to_unit_cube(x).cpu().numpy())
    # a cloud's bits do not depend on the batch it travels in (a wider kernel serves a batch with a larger cloud)
    big = np.random.RandomState(3).uniform(-1, 1, (2049, 3)).astype(np.float32)
    o1, i1 = _run([clouds[2], big], 24, [0, 0], start=[100, 0])
    assert br.same_bits(o1[0], out[2]) and np.array_equal(i1[0], idx[2])


def _with_negative_zero(n):
    x = np.random.RandomState(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    x[0, 0], x[1, 2], x[n - 1, 1] = -0.0, -0.0, 0.0
    return x


@pytest.mark.parametrize("name", ["scannet_train_2048", "shapenet_val_257", "scannet_val_24"])
def test_pre_rotation_alone(name):
    u = FX[name]["unit"]
    other = _with_negative_zero(u.shape[0])
    R = np.stack([_Rx(), _Rx()])
    out, idx = _run([u, other], u.shape[0], [RAW | PRE, RAW], Rpre=R)
    assert br.same_bits(out[0], br.rotate(u, _Rx()))
    assert br.same_bits(out[1], other) and np.signbit(out[1][0, 0]) and np.signbit(out[1][1, 2])
    assert np.array_equal(idx[0], np.arange(u.shape[0]))
    far, _ = br.ulp_apart(out[0], FX[name]["pre"])
    assert far == 0


@pytest.mark.parametrize("name", ["scannet_train_2048", "modelnet_train_257", "shapenet_plant_train_33"])
def test_z_rotation_and_jitter_alone(name):
    from mlsp_amd import data, pc_utils
    c = FX[name]
    p, S = c["sampled"], c["sampled"].shape[0]
    Rz = data.axis_rotation("z", float(c["angle"]))
    other = _with_negative_zero(S)
    out, _ = _run([p, other], S, [RAW | POST, RAW], Rpost=np.stack([Rz, Rz]))
    assert br.same_bits(out[0], br.rotate(p, Rz)) and br.same_bits(out[1], other)
    assert br.ulp_apart(out[0], c["rot"])[0] == 0
    nz = np.stack([c["randn"], c["randn"]])
    out, _ = _run([c["rot"], other], S, [RAW | JIT, RAW], noise=nz)
    assert br.same_bits(out[0], br.jitter(c["rot"], c["randn"])) and br.same_bits(out[1], other)
    assert br.ulp_apart(out[0], c["out"])[0] == 0
    # the twins are these stages
    x = torch.from_numpy(p.copy()).to(DEV)
    assert br.same_bits(pc_utils.random_rotate_one_axis(x, "z", angle=float(c["angle"])).cpu().numpy(), br.rotate(p, Rz))
    assert br.same_bits(pc_utils.rotate_shape(x, "x", -np.pi / 2).cpu().numpy(), br.rotate(p, _Rx()))
    r = torch.from_numpy(c["rot"].copy()).to(DEV)
    keep = r.clone()
    got = pc_utils.jitter_pointcloud(r, noise=torch.from_numpy(c["randn"].copy()).to(DEV))
    assert torch.equal(r, keep) and br.same_bits(got.cpu().numpy(), br.jitter(c["rot"], c["randn"]))


@pytest.mark.parametrize("name", ["modelnet_val_33", "shapenet_val_257", "scannet_train_2048", "modelnet_val_dup_64"])
def test_sampling_alone_matches_the_reference(name):
    c = FX[name]
    v, S, n = c["pre"], c["idx"].shape[0], c["pre"].shape[0]
    out, idx = _run([v, v], S, [RAW, RAW], start=[int(c["start"]), n - 1])
    assert np.array_equal(idx[0], c["idx"])
    assert br.same_bits(out[0], c["sampled"])
    assert np.array_equal(idx[1], br.fps(v, S, n - 1))
    assert br.same_bits(out[1], v[idx[1]])


def test_sampling_count_equals_s_keeps_the_order():
    v = FX["scannet_val_24"]["pre"]
    out, idx = _run([v], 24, [RAW], start=[7])
    assert np.array_equal(idx[0], np.arange(24)) and br.same_bits(out[0], v)


@pytest.mark.parametrize("n", [2049, 8192])
def test_sampling_wide_kernel(n):
    v = (np.random.RandomState(n).uniform(-1, 1, (n, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)
    small = FX["modelnet_val_33"]["pre"]
    out, idx = _run([v, small], 16, [RAW, RAW], start=[n - 1, 3])
    assert np.array_equal(idx[0], br.fps(v, 16, n - 1)) and br.same_bits(out[0], v[idx[0]])
    assert np.array_equal(idx[1], br.fps(small, 16, 3))


def test_whole_chain_is_the_composition_of_its_stages():
    from mlsp_amd import data
    names = ["scannet_train_2048", "shapenet_train_off50_2048"]
    clouds = [FX[n]["raw"] for n in names]
    start = [int(FX[n]["start"]) for n in names]
    Rz = np.stack([data.axis_rotation("z", float(FX[n]["angle"])) for n in names])
    Rx = np.stack([_Rx(), _Rx()])
    nz = np.stack([FX[n]["randn"] for n in names])
    S = 1024
    out, idx = _run(clouds, S, [PRE | POST | JIT] * 2, start=start, Rpre=Rx, Rpost=Rz, noise=nz)
    unit, _ = _run(clouds, 2048, [0, 0])
    pre, _ = _run(list(unit), 2048, [RAW | PRE] * 2, Rpre=Rx)
    samp, sidx = _run(list(pre), S, [RAW] * 2, start=start)
    rot, _ = _run(list(samp), S, [RAW | POST] * 2, Rpost=Rz)
    jit, _ = _run(list(rot), S, [RAW | JIT] * 2, noise=nz)
    assert np.array_equal(idx, sidx) and br.same_bits(out, jit)
    for b in range(2):
        assert np.array_equal(idx[b], br.fps(pre[b], S, start[b]))
        assert br.same_bits(jit[b], br.jitter(br.rotate(pre[b][idx[b]], Rz[b]), nz[b]))
    # prepare_batch is this call
    raw, _ = _pad(clouds)
    got, gidx = data.prepare_batch(raw, S, pre_rotate=_Rx(), augment=True, start=torch.tensor(start), noise=torch.from_numpy(nz).to(DEV),
                                   angles=[float(FX[n]["angle"]) for n in names], return_index=True)
    assert gidx.dtype == torch.int64 and br.same_bits(got.cpu().numpy(), out) and np.array_equal(gidx.cpu().numpy(), idx)


def test_nan_cloud_leaves_its_neighbours_alone():
    same = np.tile(np.array([[0.25, -0.5, 1.0]], dtype=np.float32), (40, 1))
    a, c = FX["modelnet_train_257"]["raw"], FX["modelnet_val_33"]["raw"]
    fl = [PRE, PRE, PRE]
    R = np.stack([_Rx()] * 3)
    out, idx = _run([a, same, c], 24, fl, start=[9, 17, 32], Rpre=R)
    assert np.isnan(out[1]).all() and idx[1].tolist() == [17] + [0] * 23
    ref, ridx = _run([a, c], 24, fl[:2], start=[9, 32], Rpre=R[:2])
    assert br.same_bits(out[0], ref[0]) and br.same_bits(out[2], ref[1])
    assert np.array_equal(idx[0], ridx[0]) and np.array_equal(idx[2], ridx[1])
    assert np.isfinite(out[0]).all() and np.isfinite(out[2]).all()


def test_refusals_leave_the_outputs_alone():
    from mlsp_amd import _lib, data
    lib = _lib.load()
    raw = torch.zeros(2, 64, 3, device=DEV)
    out = torch.full((2, 16, 3), 7.0, device=DEV)
    idx = torch.full((2, 16), 7, dtype=torch.int32, device=DEV)
    start = torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(rawp, Nmax, counts, S):
        cn = (ctypes.c_int * 2)(*counts)
        return lib.mlsp_batch_prepare_f32(rawp, 3, 2, Nmax, cn, S, None, start.data_ptr(), None, None, None, 0.01, 0.02, out.data_ptr(),
                                          idx.data_ptr(), _lib.stream())
    assert call(raw.data_ptr(), 9000, [64, 8193], 16) == -3
    assert call(raw.data_ptr(), 64, [64, 15], 16) == -1
    assert call(None, 64, [64, 64], 16) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((idx == 7).all())
    with pytest.raises(ValueError):
        data.prepare_batch(raw, npoint=32, counts=[64, 31])


def test_default_draws():
    from mlsp_amd import data
    clouds = [FX["scannet_train_2048"]["raw"], FX["shapenet_train_off50_2048"]["raw"]]
    raw, _ = _pad(clouds)
    np.random.seed(5)
    torch.manual_seed(5)
    out, idx = data.prepare_batch(raw, 1024, augment=True, return_index=True)
    out, idx = out.cpu().numpy(), idx.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < 2048                     # start indices (idx[:, 0]) in range, like every other
    np.random.seed(5)
    angles = np.random.uniform(size=2) * 2 * np.pi                 # the draw prepare_batch made
    assert angles[0] != angles[1]
    # the same call without the jitter: the rotated, unjittered points
    rot, ridx = data.prepare_batch(raw, 1024, augment=True, start=idx[:, 0].copy(), angles=angles,
                                   noise=torch.zeros(2, 1024, 3, dtype=torch.float64, device=DEV), return_index=True)
    rot = rot.cpu().numpy()
    assert np.array_equal(ridx.cpu().numpy(), idx)
    delta = out.astype(np.float64) - rot.astype(np.float64)
    assert (np.abs(delta) <= 0.02 + np.spacing(np.abs(out)).astype(np.float64)).all()
    sd = float(delta.std())
    print("std of the %d jitter values: %.7f" % (delta.size, sd))
    assert delta.size == 6144 and abs(sd - 0.0095945) <= 0.05 * 0.0095945
    unit, _ = _run(clouds, 2048, [0, 0])
    p = unit[np.arange(2)[:, None], idx].astype(np.float64)
    r64 = rot.astype(np.float64)
    assert np.abs(r64[..., 2] - p[..., 2]).max() <= 1e-6
    assert np.abs((r64[..., 0] ** 2 + r64[..., 1] ** 2) - (p[..., 0] ** 2 + p[..., 1] ** 2)).max() <= 1e-6
    for b in range(2):
        assert br.same_bits(rot[b], br.rotate(unit[b][idx[b]], data.axis_rotation("z", angles[b])))


def test_strided_input_is_not_copied_and_gives_the_same_bits():
    from mlsp_amd import data
    clouds = [FX["modelnet_train_257"]["raw"], FX["shapenet_val_257"]["raw"]]
    raw, _ = _pad(clouds)
    wide = torch.full((2, 257, 6), 3.0, device=DEV)
    wide[:, :, :3] = raw
    kw = dict(npoint=24, pre_rotate=_Rx(), pre_mask=[True, False], augment=[False, True], start=[3, 200], angles=[0.3, 1.2],
              noise=torch.from_numpy(np.random.RandomState(1).randn(2, 24, 3)).to(DEV), return_index=True)
    a, ia = data.prepare_batch(raw, **kw)
    b, ib = data.prepare_batch(wide[:, :, :3], **kw)
    assert br.same_bits(a.cpu().numpy(), b.cpu().numpy()) and torch.equal(ia, ib)
    # pre_mask and augment select per cloud
    u, _ = _run(clouds, 257, [0, 0])
    want0 = br.rotate(u[0], _Rx())[ia[0].cpu().numpy()]
    assert br.same_bits(a[0].cpu().numpy(), want0)
