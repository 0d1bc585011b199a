"""The restatement of the batch-preparation chain (tests/batchprep_restatement.py) against the reference's own results
(tests/golden/batchprep_s0.npz, written by tools/make_golden_batchprep.py), and the public surface of the feature without a GPU."""
import inspect

import numpy as np
import pytest
import torch

import batchprep_restatement as br

FX = br.fixture()
CASES = FX["names"]


def _Rx():
    from mlsp_amd import data
    return data.axis_rotation("x", -np.pi / 2)


def test_fixture_covers_the_recipes():
    assert len(CASES) == 8
    shapes = sorted((FX["cases"][n]["raw"].shape[0], FX["cases"][n]["out"].shape[0]) for n in CASES)
    assert shapes == [(24, 24), (33, 24), (33, 24), (64, 24), (257, 24), (257, 24), (2048, 1024), (2048, 1024)]
    assert sorted(int(FX["cases"][n]["flags"]) for n in CASES) == [0, 0, 1, 1, 6, 6, 7, 7]
    for n in CASES:
        for a in FX["cases"][n].values():
            assert a.dtype.kind in "fiu"


@pytest.mark.parametrize("name", CASES)
def test_unit_cube_within_the_references_own_error(name):
    c = FX["cases"][name]
    got = br.unit_cube(c["raw"])
    d = float(np.abs(got.astype(np.float64) - c["unit"].astype(np.float64)).max())
    print("%s: |restatement - reference| %.3e, reference's own error %.3e" % (name, d, float(c["own_error"])))
    assert d <= float(c["own_error"]) + 2.0 ** -23
    # the restatement itself is one rounding of the float64 result, inside the unit ball
    assert np.abs(got.astype(np.float64) - br.unit_cube64(c["raw"])).max() <= 2.0 ** -25
    assert np.abs(got).max() <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_rotations_and_jitter_within_one_ulp(name):
    from mlsp_amd import data
    c = FX["cases"][name]
    fl = int(c["flags"])
    if fl & br.F_PRE:
        far, nb = br.ulp_apart(br.rotate(c["unit"], _Rx()), c["pre"])
        print("%s: x rotation: %d of %d entries not bit-equal" % (name, nb, c["pre"].size))
        assert far == 0
    else:
        assert br.same_bits(c["unit"], c["pre"])
    if fl & br.F_POST:
        far, nb = br.ulp_apart(br.rotate(c["sampled"], data.axis_rotation("z", float(c["angle"]))), c["rot"])
        print("%s: z rotation: %d of %d entries not bit-equal" % (name, nb, c["rot"].size))
        assert far == 0
        far, nb = br.ulp_apart(br.jitter(c["rot"], c["randn"]), c["out"])
        print("%s: jitter: %d of %d entries not bit-equal" % (name, nb, c["out"].size))
        assert far == 0
    else:
        assert br.same_bits(c["sampled"], c["out"])


@pytest.mark.parametrize("name", CASES)
def test_sampling_is_exact_on_the_references_input(name):
    c = FX["cases"][name]
    S = c["out"].shape[0]
    idx = br.fps(c["pre"], S, int(c["start"]))
    assert np.array_equal(idx, c["idx"])
    assert br.same_bits(c["pre"][idx], c["sampled"])
    if c["pre"].shape[0] == S:
        assert np.array_equal(idx, np.arange(S))


def test_duplicated_points_first_index_wins():
    c = FX["cases"]["modelnet_val_dup_64"]
    pre = c["pre"]
    twins = {}
    for j, p in enumerate(map(bytes, pre)):
        twins.setdefault(p, []).append(j)
    assert all(len(v) == 2 for v in twins.values())
    first = {v[0] for v in twins.values()}
    assert set(int(i) for i in c["idx"][1:]) <= first          # (sample 0 is the drawn start, either twin)


def test_cloud_of_identical_points_is_nan_with_indices_in_range():
    raw = np.tile(np.array([[0.25, -0.5, 1.0]], dtype=np.float32), (40, 1))
    r = br.chain(raw, 24, 0, start=17)
    assert np.isnan(r["out"]).all()
    assert r["idx"].tolist() == [17] + [0] * 23


def test_chain_is_the_composition_of_its_stages():
    from mlsp_amd import data
    c = FX["cases"]["scannet_train_2048"]
    Rz = data.axis_rotation("z", float(c["angle"]))
    r = br.chain(c["raw"], 1024, 7, start=int(c["start"]), Rpre=_Rx(), Rpost=Rz, noise=c["randn"])
    assert br.same_bits(r["out"], br.jitter(br.rotate(br.rotate(br.unit_cube(c["raw"]), _Rx())[r["idx"]], Rz), c["randn"]))
    assert np.array_equal(r["idx"], br.fps(r["pre"], 1024, int(c["start"])))


def test_axis_rotation_is_rotate_shapes_matrix():
    from mlsp_amd import data
    a = -np.pi / 2
    assert np.array_equal(data.axis_rotation("x", a), np.asarray([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]))
    assert np.array_equal(data.axis_rotation("y", a), np.asarray([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]))
    for ax in ("z", "w"):
        assert np.array_equal(data.axis_rotation(ax, a), np.asarray([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]))
    assert data.axis_rotation("x", a).dtype == np.float64


def test_public_names_and_no_cpu_fallback():
    from mlsp_amd import data, pc_utils, _lib
    assert list(inspect.signature(data.prepare_batch).parameters) == [
        "raw", "npoint", "counts", "pre_rotate", "pre_mask", "augment", "start", "angles", "noise", "sigma", "clip", "return_index"]
    sig = inspect.signature(data.prepare_batch).parameters
    assert (sig["npoint"].default, sig["sigma"].default, sig["clip"].default, sig["augment"].default) == (1024, 0.01, 0.02, False)
    assert list(inspect.signature(pc_utils.jitter_pointcloud).parameters) == ["pc", "sigma", "clip", "noise"]
    assert list(inspect.signature(pc_utils.random_rotate_one_axis).parameters) == ["X", "axis", "angle"]
    assert "mlsp_batch_prepare_f32" in _lib.SIGNATURES and "precision" not in str(_lib.SIGNATURES["mlsp_batch_prepare_f32"])
    x = torch.zeros(2, 32, 3)
    with pytest.raises(_lib.MlspLibraryError):
        data.prepare_batch(x, npoint=16)
    with pytest.raises(_lib.MlspLibraryError):
        pc_utils.scale_to_unit_cube(x)
    with pytest.raises(_lib.MlspLibraryError):
        pc_utils.rotate_shape(x[0], "x", 0.5)
    with pytest.raises(_lib.MlspLibraryError):
        pc_utils.random_rotate_one_axis(x, "z")
    with pytest.raises(_lib.MlspLibraryError):
        pc_utils.jitter_pointcloud(x[0])


def test_refusals_come_before_any_launch():
    """The entry point reads its host metadata and refuses before it touches the device: these calls need no GPU."""
    import ctypes
    from mlsp_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                   # a non-null pointer that is never dereferenced

    def call(raw=one, ld=3, B=2, Nmax=64, counts=None, S=16, flags=None, start=one, Rpre=None, Rpost=None, noise=None, out=one, idx=one):
        cn = (ctypes.c_int * B)(*counts) if counts is not None else None
        fg = (ctypes.c_int * B)(*flags) if flags is not None else None
        return lib.mlsp_batch_prepare_f32(raw, ld, B, Nmax, cn, S, fg, start, Rpre, Rpost, noise, 0.01, 0.02, out, idx, None)
    assert call(raw=None) == -1 and call(out=None) == -1 and call(idx=None) == -1
    assert call(ld=2) == -1 and call(B=0) == -1 and call(S=0) == -1
    assert call(Nmax=8193, S=16) == -3 and call(Nmax=9000, counts=[64, 8193]) == -3
    assert call(counts=[64, 15]) == -1 and call(counts=[64, 65]) == -1 and call(S=65) == -1
    assert call(flags=[0, 1]) == -1 and call(flags=[2, 0]) == -1 and call(flags=[0, 4]) == -1 and call(flags=[16, 0]) == -1
    assert call(start=None) == -1
