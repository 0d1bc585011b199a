"""Generate tests/golden/batchprep_s0.npz: the UNMODIFIED reference's sample preparation (utils/pc_utils.py scale_to_unit_cube,
rotate_shape, farthest_point_sample_np, random_rotate_one_axis, jitter_pointcloud) run in the order of PointDA/data/dataloader.py
`__getitem__` (:79-95 ScanNet, :136-149 ModelNet, :185-200 ShapeNet), with every intermediate and every random draw recorded.
Build-container only (imports the reference's utils/pc_utils.py, which needs numpy and torch alone); numeric arrays only.

    python tools/make_golden_batchprep.py

Per case <name>_...:  raw [n,3] f32;  unit (after scale_to_unit_cube);  pre (after the x rotation, = unit where the recipe has none);
idx [S] i64 and sampled [S,3] f32 (S == n: 0..n-1 and pre itself);  start;  angle (f64, NaN without augmentation), rot (after the z
rotation), randn [S,3] f64, out (after the jitter; = sampled without augmentation);  flags (1 pre-rotation, 2 z rotation, 4 jitter);
own_error: max |scale_to_unit_cube(raw as float32) - scale_to_unit_cube(raw as float64)|, the reference's own distance from its function
in float64.  The draws are recorded by seeding numpy's global generator before the call and replaying the same draw after it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

sys.path.insert(0, ref_import.REF_ROOT)
from utils import pc_utils as rpc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "batchprep_s0.npz")


def getitem(raw, S, pre, aug, seed):
    """dataloader.py __getitem__ with NUM_POINTS = S; pre: ScanNet / ShapeNet (label not plant); aug: a training sample outside val_ind"""
    rec = {"raw": raw.copy(), "flags": np.int64((1 if pre else 0) | (6 if aug else 0))}
    pc = rpc.scale_to_unit_cube(raw.copy())
    assert pc.dtype == np.float32
    rec["unit"] = pc.copy()
    rec["own_error"] = np.float64(np.abs(pc.astype(np.float64) - rpc.scale_to_unit_cube(raw.astype(np.float64))).max())
    if pre:
        pc = rpc.rotate_shape(pc, "x", -np.pi / 2)
    rec["pre"] = pc.copy()
    if pc.shape[0] > S:
        pcT = np.swapaxes(np.expand_dims(pc, 0), 1, 2)
        np.random.seed(seed)
        idx, vals = rpc.farthest_point_sample_np(pcT, S)
        np.random.seed(seed)
        start = np.random.randint(0, pc.shape[0], (1,), dtype=np.int64)[0]
        assert idx[0, 0] == start
        pc = np.swapaxes(vals.squeeze(), 1, 0).astype("float32")
        rec["idx"] = idx[0].astype(np.int64)
    else:
        start = 0
        rec["idx"] = np.arange(pc.shape[0], dtype=np.int64)
    rec["start"] = np.int64(start)
    rec["sampled"] = pc.copy()
    assert np.array_equal(rec["pre"][rec["idx"]], pc)
    angle = np.float64(np.nan)
    randn = np.zeros((S, 3))
    if aug:
        np.random.seed(seed + 1000)
        pc = rpc.random_rotate_one_axis(pc, "z")
        np.random.seed(seed + 1000)
        angle = np.float64(np.random.uniform() * 2 * np.pi)
        rec["rot"] = pc.copy()
        np.random.seed(seed + 2000)
        pc = rpc.jitter_pointcloud(pc.copy())
        np.random.seed(seed + 2000)
        randn = np.random.randn(S, 3)
    else:
        rec["rot"] = pc.copy()
    rec["angle"], rec["randn"], rec["out"] = angle, randn, pc.copy()
    assert pc.dtype == np.float32 and pc.shape == (S, 3)
    return rec


def main():
    g = np.random.RandomState(0)
    box = np.array([1.0, 0.6, 0.3])

    def cloud(n, off=0.0):
        return (g.uniform(-1, 1, (n, 3)) * box + off).astype(np.float32)

    dup = cloud(32)
    dup = np.concatenate([dup, dup], 0)[g.permutation(64)]
    cases = [  # name, raw, S, pre-rotation, augmentation
        ("scannet_train_2048", cloud(2048), 1024, True, True),
        ("shapenet_train_off50_2048", cloud(2048, 50.0), 1024, True, True),
        ("modelnet_train_257", cloud(257), 24, False, True),
        ("shapenet_plant_train_33", cloud(33), 24, False, True),
        ("scannet_val_24", cloud(24), 24, True, False),
        ("modelnet_val_dup_64", np.ascontiguousarray(dup), 24, False, False),
        ("shapenet_val_257", cloud(257), 24, True, False),
        ("modelnet_val_33", cloud(33), 24, False, False),
    ]
    out = {"names": np.array([c[0] for c in cases])}
    for seed, (name, raw, S, pre, aug) in enumerate(cases):
        rec = getitem(raw, S, pre, aug, 10 + seed)
        print("%-28s n %4d S %4d flags %d start %4d own_error %.2e" % (name, raw.shape[0], S, rec["flags"], rec["start"], rec["own_error"]))
        for k, v in rec.items():
            out[name + "_" + k] = v
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print("wrote %s: %d bytes" % (OUT, size))


if __name__ == "__main__":
    main()
