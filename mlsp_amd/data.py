"""Training batches prepared on the device (PointDA/data/dataloader.py:79-95, 136-149, 185-200).

The reference prepares every sample of every epoch in `Dataset.__getitem__`, in numpy: `scale_to_unit_cube`, (ScanNet, ShapeNet)
`rotate_shape(pc, 'x', -pi/2)`, `farthest_point_sample_np(pc, 1024)` for a cloud of more than 1024 points -- a Python loop of 1024
iterations -- and on training samples `jitter_pointcloud(random_rotate_one_axis(pc, "z"))`.  `prepare_batch` is that chain for a whole
batch of raw clouds kept on the device: one HIP launch (csrc/batchprep.hip), one workgroup per cloud.  No CPU fallback.

Which samples are validation samples and which ShapeNet labels are plants stays the caller's knowledge: `augment` and `pre_mask` carry it.
"""
import numpy as np
import torch

from . import _lib

F_PRE, F_POST, F_JITTER, F_RAW = 1, 2, 4, 8          # the flag bits of include/mlsp_hip.h mlsp_batch_prepare_f32
MAX_POINTS = 8192


def axis_rotation(axis, angle):
    """The float64 matrix `rotate_shape(x, axis, angle)` multiplies by (utils/pc_utils.py:199-201): 'x', 'y', anything else is z.
    `random_rotate_one_axis` builds the same three matrices from its drawn angle (:221-231)."""
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.asarray([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    if axis == "y":
        return np.asarray([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    return np.asarray([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def _host_bools(v, B, name):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    v = np.asarray(v, dtype=bool)
    if v.ndim == 0:
        v = np.full(B, bool(v))
    if v.shape != (B,):
        raise ValueError("%s: expected a bool or [%d] bools, got shape %s" % (name, B, v.shape))
    return v


def _matrices(R, B, device, name):
    """None, [3,3] or [B,3,3] float64 (numpy or tensor) -> contiguous device float64 [B,3,3]"""
    if R is None:
        return None
    t = torch.as_tensor(R)
    if t.dtype != torch.float64:
        raise ValueError("%s: float64 matrices (the reference multiplies by a float64 matrix), got %s" % (name, t.dtype))
    if t.shape == (3, 3):
        t = t.expand(B, 3, 3)
    if t.shape != (B, 3, 3):
        raise ValueError("%s: expected [3,3] or [%d,3,3], got %s" % (name, B, tuple(t.shape)))
    return t.to(device).contiguous()


def _run(raw, npoint, counts, flags, start, Rpre, Rpost, noise, sigma, clip):
    """raw [B,Nmax,C>=3] float32 on the device -> (out [B,npoint,3] float32, idx [B,npoint] int32)"""
    lib = _lib.load()
    _lib.require_gpu(raw, start, Rpre, Rpost, noise)
    if raw.dtype != torch.float32 or raw.dim() != 3 or raw.shape[2] < 3:
        raise ValueError("raw: float32 [B, N, C >= 3], got %s %s" % (raw.dtype, tuple(raw.shape)))
    B, Nmax, _ = raw.shape
    if raw.stride(2) != 1 or raw.stride(1) < 3 or raw.stride(0) != Nmax * raw.stride(1):
        raw = raw.contiguous()
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    out = torch.empty((B, npoint, 3), dtype=torch.float32, device=raw.device)
    idx = torch.empty((B, npoint), dtype=torch.int32, device=raw.device)
    _lib.check(lib.mlsp_batch_prepare_f32(raw.data_ptr(), raw.stride(1), B, Nmax, counts.ctypes.data, int(npoint), flags.ctypes.data,
                                          _lib.ptr(start), _lib.ptr(Rpre), _lib.ptr(Rpost), _lib.ptr(noise), float(sigma), float(clip),
                                          out.data_ptr(), idx.data_ptr(), _lib.stream()), "mlsp_batch_prepare_f32")
    return out, idx


def prepare_batch(raw, npoint=1024, counts=None, pre_rotate=None, pre_mask=None, augment=False, start=None, angles=None, noise=None,
                  sigma=0.01, clip=0.02, return_index=False):
    """The `__getitem__` chain of the PointDA datasets for a batch of raw clouds, in one launch.

    raw        float32 CUDA [B, Nmax, C >= 3] (the first three columns are read; a row stride other than C is passed on, not copied)
    counts     host ints [B]: the points of every cloud (None: Nmax each); a count below `npoint` raises ValueError, above 8192 too
    pre_rotate None, or float64 [3,3] / [B,3,3] applied after the unit-cube scaling (`axis_rotation('x', -np.pi / 2)` for ScanNet and
               ShapeNet); pre_mask [B] bools selects the clouds it applies to (None: all) -- ShapeNet leaves its plants unrotated
    augment    bool or [B] bools: the z rotation and the jitter of training samples that are not in the validation split
    start      [B] first sample of the farthest point sampling (default: torch.randint below every count)
    angles     [B] float64 z-rotation angles (default: np.random.uniform(size=B) * 2 * np.pi, numpy's global state as in the reference)
    noise      [B, npoint, 3] float64 standard normal draws (default: torch.randn on raw's device)
    The injected draws are the reproducible path: the reference's generator streams are not reproduced.
    -> [B, npoint, 3] float32 on the device (, idx [B, npoint] int64: the points chosen, 0 .. npoint-1 where a cloud has exactly npoint)
    """
    _lib.load()
    _lib.require_gpu(raw)
    B, Nmax = raw.shape[0], raw.shape[1]
    counts = np.full(B, Nmax, dtype=np.int64) if counts is None else np.asarray(
        counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts).astype(np.int64).reshape(-1)
    if counts.shape != (B,):
        raise ValueError("counts: expected [%d] ints" % B)
    if (counts < npoint).any():
        raise ValueError("prepare_batch: a cloud of %d points cannot give %d samples" % (int(counts.min()), npoint))
    if (counts > Nmax).any() or (counts > MAX_POINTS).any():
        raise ValueError("prepare_batch: counts up to min(Nmax, %d), got %d" % (MAX_POINTS, int(counts.max())))
    aug = _host_bools(augment, B, "augment")
    flags = np.zeros(B, dtype=np.int32)
    Rpre = _matrices(pre_rotate, B, raw.device, "pre_rotate")
    if Rpre is not None:
        pm = _host_bools(pre_mask, B, "pre_mask")
        flags |= F_PRE if pm is None else np.where(pm, F_PRE, 0).astype(np.int32)
    Rpost = None
    if aug.any():
        flags |= np.where(aug, F_POST | F_JITTER, 0).astype(np.int32)
        if angles is None:
            angles = np.random.uniform(size=B) * 2 * np.pi
        elif isinstance(angles, torch.Tensor):
            angles = angles.detach().cpu().numpy()
        angles = np.asarray(angles, dtype=np.float64).reshape(B)
        Rpost = torch.from_numpy(np.stack([axis_rotation("z", a) for a in angles])).to(raw.device)
        if noise is None:
            noise = torch.randn((B, npoint, 3), dtype=torch.float64, device=raw.device)
        if noise.dtype != torch.float64 or tuple(noise.shape) != (B, npoint, 3):
            raise ValueError("noise: float64 [%d, %d, 3]" % (B, npoint))
        noise = noise.contiguous()
    else:
        noise = None
    if (counts > npoint).any():
        if start is None:
            start = torch.randint(0, 1 << 62, (B,), device=raw.device) % torch.as_tensor(counts, device=raw.device)
        start = torch.as_tensor(start).to(device=raw.device, dtype=torch.int32).contiguous()
    else:
        start = None
    out, idx = _run(raw, npoint, counts, flags, start, Rpre, Rpost, noise, sigma, clip)
    return (out, idx.long()) if return_index else out


def single_stage(x, flag, R=None, noise=None, sigma=0.0, clip=0.0):
    """One stage of the chain on [N,3] or [B,N,3] CUDA float32, every point kept in its place: what the pc_utils twins call."""
    _lib.load()
    _lib.require_gpu(x)
    rows = x if x.dim() == 3 else x[None]
    B, N = rows.shape[0], rows.shape[1]
    if N > MAX_POINTS:
        raise ValueError("at most %d points per cloud, got %d" % (MAX_POINTS, N))
    Rd = _matrices(R, B, x.device, "rotation")
    if noise is not None:
        noise = torch.as_tensor(noise).to(device=x.device, dtype=torch.float64).reshape(B, N, 3).contiguous()
    out, _ = _run(rows.detach(), N, np.full(B, N), np.full(B, flag), None, Rd if flag & F_PRE else None, Rd if flag & F_POST else None,
                  noise, sigma, clip)
    return out if x.dim() == 3 else out[0]
