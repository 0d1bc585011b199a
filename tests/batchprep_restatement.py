"""numpy restatement of the batch-preparation chain (mlsp_amd/data.py, csrc/batchprep.hip), stage by stage, on the dtype trail the kernel
states: what is float64 there is float64 here, what is fp32 there is fp32 here, every rounding in the same place.  Shared by
tests/test_batchprep_cpu.py (against the reference's own results in tests/golden/batchprep_s0.npz) and tests/test_gpu_batchprep.py
(against the device).  Test-only; nothing of the product imports it.

The one thing it does not restate is the ORDER of the float64 centroid sum (numpy adds pairwise, the kernel in 256 lanes): both are
within a few 2^-53 of the exact sum, which moves the float32 result by at most one rounding."""
import os

import numpy as np

F_PRE, F_POST, F_JITTER, F_RAW = 1, 2, 4, 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batchprep_s0.npz")


def unit_cube64(x):
    """float32 [n,3] -> the float64 result before its one rounding"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = x.sum(0) / x.shape[0]
        d = x - c
        r = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
        return d / r


def unit_cube(x):
    return unit_cube64(x).astype(np.float32)


def rotate(u, R):
    """float32 [n,3] times float64 [3,3]: (u0 R[0][k] + u1 R[1][k]) + u2 R[2][k] in float64, rounded once"""
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    R = np.asarray(R, dtype=np.float64)
    return ((u[:, 0:1] * R[0] + u[:, 1:2] * R[1]) + u[:, 2:3] * R[2]).astype(np.float32)


def fps(v, S, start):
    """fp32 farthest point sampling: d = (dx dx + dy dy) + dz dz, running minimum from 1e10, first index wins; a NaN distance never
    lowers a minimum.  S == n: nothing is sampled."""
    v = np.asarray(v, dtype=np.float32)
    n = v.shape[0]
    if S == n:
        return np.arange(n, dtype=np.int64)
    dmin = np.full(n, 1e10, dtype=np.float32)
    idx = np.zeros(S, dtype=np.int64)
    far = int(start)
    with np.errstate(invalid="ignore"):
        for i in range(S):
            idx[i] = far
            d = v - v[far]
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d.dtype == np.float32
            dmin = np.where(d < dmin, d, dmin)
            far = int(np.argmax(dmin))
    return idx


def jitter(w, noise, sigma=0.01, clip=0.02):
    """f32(f64(w) + min(max(sigma noise, -clip), clip))"""
    t = np.minimum(np.maximum(sigma * np.asarray(noise, dtype=np.float64), -clip), clip)
    return (np.asarray(w, dtype=np.float32).astype(np.float64) + t).astype(np.float32)


def chain(raw, S, flags, start=0, Rpre=None, Rpost=None, noise=None, sigma=0.01, clip=0.02):
    """one cloud through the stages its flags ask for -> dict of every intermediate"""
    x = np.asarray(raw, dtype=np.float32)[:, :3]
    u = x if flags & F_RAW else unit_cube(x)
    v = rotate(u, Rpre) if flags & F_PRE else u
    idx = fps(v, S, start)
    p = v[idx]
    w = rotate(p, Rpost) if flags & F_POST else p
    out = jitter(w, noise, sigma, clip) if flags & F_JITTER else w
    return {"unit": u, "pre": v, "idx": idx, "sampled": p, "rot": w, "out": out}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ulp_apart(a, b):
    """(entries more than one float32 ulp apart, entries that are not bit-equal)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ulp = np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b)))
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return int((diff > ulp).sum()), int((a.view(np.uint32) != b.view(np.uint32)).sum())


_fixture = None


def fixture():
    """tests/golden/batchprep_s0.npz, loaded once: {"names": [...], name: {field: array}}"""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        names = [str(s) for s in z["names"]]
        cases = {}
        for nm in names:
            cases[nm] = {k[len(nm) + 1:]: z[k] for k in z.files if k.startswith(nm + "_")}
            for v in cases[nm].values():
                v.setflags(write=False)
        _fixture = {"names": names, "cases": cases}
    return _fixture
