"""Device versions of the point-cloud helpers the MLSP input corruption and PCM mixing lean on.

Mirrors utils/pc_utils.py of the reference for the functions on that path: `region_mean` (:13-29),
`assign_region_to_point` (:33-73), `farthest_point_sample(args, xyz, npoint)` (:137-161); same names, argument order and
return values.  The reference implements them as Python loops of tensor ops (27 region passes; `npoint` FPS iterations);
here each is one HIP kernel (csrc/corrupt.hip, csrc/sa.hip).  No CPU fallback.

The dataloader's helpers (`scale_to_unit_cube` :263-277, `rotate_shape` :190-208, `random_rotate_one_axis` :211-232,
`jitter_pointcloud` :249-260) are single stages of the batch-preparation kernel (mlsp_amd/data.py, csrc/batchprep.hip); their
`farthest_point_sample_np` is `farthest_point_sample` below with `start=`.
"""
import numpy as np
import torch

from . import _lib

NREGIONS = 3           # utils/pc_utils.py:10
MIN_POINTS = 20
RADIUS = 0.5


def region_mean(num_regions):
    """utils/pc_utils.py:13-29: centres of the num_regions^3 voxels of [-1,1]^3 in the reference's order (host table)."""
    n = num_regions
    d = 2 / n
    ax = 1 - d * (np.arange(n - 1, -1, -1) + 0.5)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


def assign_region_to_point(X, device=None):
    """utils/pc_utils.py:33-73.  X [B,C,N] -> int64 [B,N] voxel id of every point (0 for points on a voxel face)."""
    lib = _lib.load()
    x = X.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    _lib.require_gpu(x)
    B, C, N = x.shape
    n = NREGIONS
    d = 2 / n
    thr = torch.tensor([-1 + i * d for i in range(n + 1)], dtype=torch.float64).to(torch.float32).to(x.device)   # torch rounds the scalars
    clip = float(torch.tensor(0.99999999, dtype=torch.float32))
    Y = torch.empty((B, N), dtype=torch.int32, device=x.device)
    _lib.check(lib.mlsp_region_assign_f32(x.data_ptr(), B, C, N, thr.data_ptr(), n, clip, Y.data_ptr(), _lib.stream()),
               "mlsp_region_assign_f32")
    return Y.long()


def farthest_point_sample(args, xyz, npoint, start=None):
    """utils/pc_utils.py:137-161.  xyz [B,C,N] -> (indices [B,npoint] int64, values [B,C,npoint]).  `start` [B] pins the first
    sample (the reference draws it with torch.randint, :150)."""
    from .pointnet2 import farthest_point_sample as fps_rows
    B, C, N = xyz.shape
    if npoint == 0:
        return torch.zeros(B, 0, dtype=torch.long, device=xyz.device), torch.zeros(B, C, 0, device=xyz.device)
    rows = xyz.detach().transpose(1, 2).contiguous()             # [B,N,C] point-major for the kernel
    idx = fps_rows(rows, npoint, start=start)
    vals = torch.gather(xyz, 2, idx[:, None, :].expand(-1, C, -1))
    return idx, vals


def scale_to_unit_cube(x):
    """utils/pc_utils.py:263-277 for [N,3] or [B,N,3] CUDA float32 (N <= 8192): centre on the mean, divide by the largest distance from
    it; mean and radius in float64, one rounding to float32.  The reference scales its numpy argument in place; this returns a new tensor
    and leaves `x` as it was."""
    from . import data
    return data.single_stage(x, 0)


def rotate_shape(x, axis, angle):
    """utils/pc_utils.py:190-208: x times the float64 rotation matrix about 'x', 'y' or (anything else) z, rounded once to float32."""
    from . import data
    return data.single_stage(x, data.F_RAW | data.F_PRE, R=data.axis_rotation(axis, angle))


def random_rotate_one_axis(X, axis, angle=None):
    """utils/pc_utils.py:211-232.  `angle` (one, or [B]) pins the rotation; omitted, it is drawn as the reference draws it
    (np.random.uniform() * 2 * np.pi, one per cloud)."""
    from . import data
    B = X.shape[0] if X.dim() == 3 else 1
    if angle is None:
        angle = np.random.uniform(size=B) * 2 * np.pi
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64).reshape(-1), (B,))
    return data.single_stage(X, data.F_RAW | data.F_POST, R=np.stack([data.axis_rotation(axis, a) for a in angle]))


def jitter_pointcloud(pc, sigma=0.01, clip=0.02, noise=None):
    """utils/pc_utils.py:249-260: pc + clip(sigma * noise, -clip, clip), added in float64 and rounded once to float32 as numpy's in-place
    `+=` does.  `noise` (float64, pc's shape) pins the standard normal draws; omitted, torch.randn on pc's device.  The reference adds into
    its numpy argument; this returns a new tensor and leaves `pc` as it was."""
    from . import data
    if noise is None:
        noise = torch.randn(tuple(pc.shape), dtype=torch.float64, device=pc.device)
    return data.single_stage(pc, data.F_RAW | data.F_JITTER, noise=noise, sigma=sigma, clip=clip)
