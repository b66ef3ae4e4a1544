"""Surface reconstruction: the way back from scans to a surface (DESIGN "Surface reconstruction").

``TsdfVolume`` fuses the rays of posed DepthClouds into a dense truncated-signed-distance volume (csrc/dc_tsdf.hip: one lane per ray,
integer atomics, so the same rays give the same bits in any order) and extracts a ``mesh.TriangleMesh`` from it by surface nets (count,
scan, fill; one host read).  ``reconstruct`` does both for a sequence of clouds and poses, with the depth correction applied first.  The
mesh can be held against the ground truth with ``metrics.reconstruction_accuracy`` and rendered from with ``RenderedMeshDataset``.

GPU only, like the rest of the package.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .depth_cloud import DepthCloud

__all__ = ['TsdfVolume', 'reconstruct', 'STATS_FIELDS']

STATS_FIELDS = ('rays_used', 'rays_skipped', 'samples_outside', 'visits')


def _gpu(device, who):
    device = torch.device('cuda' if device is None else device)
    if device.type != 'cuda':
        raise RuntimeError('%s needs a GPU (device %s): depth_correction_amd has no CPU path' % (who, device))
    if not torch.cuda.is_available():
        raise RuntimeError('%s needs a GPU, and torch sees none: depth_correction_amd has no CPU path' % who)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def _grid_dims(lo, hi, voxel_size):
    dims = tuple(max(2, int(math.ceil((h - l) / voxel_size))) for l, h in zip(lo, hi))
    if dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('a grid of %d x %d x %d voxels of %g m has 2^31 voxels or more: use a larger voxel size or smaller bounds'
                         % (dims + (voxel_size,)))
    return dims


class TsdfVolume(object):
    """A dense TSDF volume on a GPU: minimum corner ``origin`` [3], ``dims`` (nx, ny, nz) voxels of ``voxel_size`` metres, truncation
    ``trunc`` (None: 3 voxels).  Voxel (ix, iy, iz) has the centre origin + (i + 0.5) voxel_size; its value is sum / (count 2^20) in
    units of the truncation, negative behind the surface."""

    def __init__(self, origin, dims, voxel_size, trunc=None, device=None):
        self.device = _gpu(device, 'TsdfVolume')
        self.origin = tuple(float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3))
        self.dims = tuple(int(n) for n in dims)
        self.voxel_size = float(voxel_size)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        if not (self.voxel_size > 0.0 and math.isfinite(self.voxel_size) and self.trunc > 0.0 and math.isfinite(self.trunc)):
            raise ValueError('TsdfVolume needs a voxel size and a truncation > 0, got %r and %r' % (voxel_size, trunc))
        if len(self.dims) != 3 or min(self.dims) < 2 or self.dims[0] * self.dims[1] * self.dims[2] >= 2 ** 31:
            raise ValueError('TsdfVolume needs three dims >= 2 with fewer than 2^31 voxels, got %r' % (dims,))
        self._sum = torch.zeros(self.dims, dtype=torch.int64, device=self.device)
        self._count = torch.zeros(self.dims, dtype=torch.int32, device=self.device)
        self._stats = torch.zeros((4,), dtype=torch.int64, device=self.device)

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, trunc=None, device=None):
        """The volume that holds the box lo .. hi padded by the truncation on every side."""
        voxel_size = float(voxel_size)
        pad = 3.0 * voxel_size if trunc is None else float(trunc)
        lo = np.asarray(lo, dtype=np.float64).reshape(3) - pad
        hi = np.asarray(hi, dtype=np.float64).reshape(3) + pad
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all() and voxel_size > 0.0):
            raise ValueError('from_bounds needs finite bounds lo <= hi and a voxel size > 0')
        return cls(lo, _grid_dims(lo, hi, voxel_size), voxel_size, trunc=trunc, device=device)

    def __repr__(self):
        return 'TsdfVolume(%d x %d x %d voxels of %g m at %s, truncation %g m)' % (self.dims + (self.voxel_size, self.origin, self.trunc))

    def reset(self):
        self._sum.zero_()
        self._count.zero_()
        self._stats.zero_()

    def integrate(self, cloud, pose=None, mask=None, min_depth=0.0, max_range=None, carve_from=None):
        """Adds one scan: a DepthCloud (or a structured array, through DepthCloud.from_structured_array) in the sensor frame, moved by
        ``pose`` [4,4] (world from sensor; array or tensor, None: identity).  ``mask`` [n] (None: the cloud's own mask, when it has one)
        selects rays.  Returns this call's stats as a dict of ints (STATS_FIELDS): the one host read."""
        if isinstance(cloud, np.ndarray):
            cloud = DepthCloud.from_structured_array(cloud, dtype=np.float64, device=self.device)
        if not isinstance(cloud, DepthCloud):
            raise TypeError('integrate takes a DepthCloud or a structured array, got %s' % type(cloud).__name__)
        if not cloud.dirs.is_cuda:
            raise RuntimeError('integrate needs the cloud on a GPU (depth_correction_amd has no CPU path)')
        if mask is None:
            mask = cloud.mask
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(-1).contiguous()
        if pose is not None:
            pose = torch.as_tensor(np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64),
                                   device=self.device).reshape(4, 4).contiguous()
        dt = cloud.dirs.dtype
        before = self._stats.clone()
        with torch.no_grad():
            ops.tsdf_integrate(self._sum, self._count, self._stats, self.origin, self.voxel_size, self.trunc,
                               cloud.vps.detach().to(dt).contiguous(), cloud.dirs.detach().contiguous(), cloud.depth.detach().to(dt).contiguous(),
                               pose=pose, mask=mask, min_depth=min_depth, max_range=max_range, carve_from=carve_from)
        return dict(zip(STATS_FIELDS, (self._stats - before).tolist()))

    def stats(self):
        """The stats of all calls since the last reset."""
        return dict(zip(STATS_FIELDS, self._stats.tolist()))

    def sums(self):
        return self._sum

    def counts(self):
        return self._count

    def values(self, min_count=1):
        """f64 [nx, ny, nz]: sum / (count 2^20), NaN where count < min_count."""
        obs = self._count >= int(min_count)
        f = self._sum.to(torch.float64) / (self._count.to(torch.float64) * float(2 ** 20))
        return torch.where(obs, f, torch.full_like(f, float('nan')))

    def extract(self, min_count=1):
        """(vertices f64 [Nv,3], faces i32 [Nf,3]) on the device; both empty when the volume holds no surface."""
        return ops.tsdf_extract(self._sum, self._count, self.origin, self.voxel_size, min_count=min_count)

    def extract_mesh(self, min_count=1):
        """The surface as a mesh.TriangleMesh, normals to the free side.  A volume without a face has no mesh: ValueError."""
        from .mesh import TriangleMesh
        vertices, faces = self.extract(min_count)
        if faces.shape[0] == 0:
            raise ValueError('the volume holds no surface (%d vertices, no face): nothing to make a mesh of' % vertices.shape[0])
        return TriangleMesh(vertices.cpu().numpy(), faces.cpu().numpy())


def _as_cloud(cloud, device):
    if isinstance(cloud, np.ndarray):
        return DepthCloud.from_structured_array(cloud, dtype=np.float64, device=device)
    if not isinstance(cloud, DepthCloud):
        raise TypeError('reconstruct takes DepthClouds or structured arrays, got %s' % type(cloud).__name__)
    return cloud


def reconstruct(clouds, poses, voxel_size, trunc=None, bounds=None, model=None, min_count=1, min_depth=0.0, max_range=None, carve_from=None,
                device=None):
    """(mesh, volume): the scans ``clouds`` (DepthClouds or structured arrays, sensor frame) moved by ``poses`` ([4,4] each, world from
    sensor) fused at ``voxel_size`` and extracted.  With a ``model`` every cloud is corrected by ``model(cloud)`` first.  ``bounds`` (lo
    [3], hi [3]) default to the box of the posed end points (torch min / max on the device); the volume pads them by the truncation."""
    device = _gpu(device, 'reconstruct')
    clouds = [_as_cloud(c, device) for c in clouds]
    if len(clouds) != len(poses):
        raise ValueError('%d clouds and %d poses' % (len(clouds), len(poses)))
    if not clouds:
        raise ValueError('reconstruct needs at least one cloud')
    for c in clouds:
        if not c.dirs.is_cuda:
            raise RuntimeError('reconstruct needs the clouds on a GPU (depth_correction_amd has no CPU path)')
    if model is not None:
        with torch.no_grad():
            clouds = [model(c) for c in clouds]
    poses = [np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p, dtype=np.float64).reshape(4, 4) for p in poses]
    if bounds is None:
        lo, hi = [], []
        for c, T in zip(clouds, poses):
            with torch.no_grad():
                pts = c.to_points().detach().to(torch.float64)
                Tt = torch.as_tensor(T, device=pts.device)
                pts = pts @ Tt[:3, :3].t() + Tt[:3, 3]
                pts = pts[torch.isfinite(pts).all(dim=1)]
                if pts.shape[0]:
                    lo.append(pts.min(dim=0).values)
                    hi.append(pts.max(dim=0).values)
        if not lo:
            raise ValueError('reconstruct: the clouds hold no finite point to take bounds from')
        bounds = torch.stack(lo).min(dim=0).values.tolist(), torch.stack(hi).max(dim=0).values.tolist()
    volume = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel_size, trunc=trunc, device=device)
    for c, T in zip(clouds, poses):
        volume.integrate(c, pose=T, min_depth=min_depth, max_range=max_range, carve_from=carve_from)
    return volume.extract_mesh(min_count), volume
