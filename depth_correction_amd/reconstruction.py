"""Surface reconstruction: the way back from scans to a surface (DESIGN "Surface reconstruction").

``SparseTsdfVolume`` is the same fusion and extraction on an unbounded lattice with storage for the 8 x 8 x 8 blocks rays wrote to only
(csrc/dc_tsdf_sparse.hip, DESIGN "Sparse TSDF volumes"): for scenes whose box a dense volume cannot hold.

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

__all__ = ['TsdfVolume', 'SparseTsdfVolume', 'reconstruct', 'STATS_FIELDS', 'SPARSE_STATS_FIELDS']

STATS_FIELDS = ('rays_used', 'rays_skipped', 'samples_outside', 'visits')
SPARSE_STATS_FIELDS = STATS_FIELDS + ('visits_dropped', 'blocks')


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
        vps, dirs, depth, pose, mask = _scan_args(cloud, pose, mask, self.device, 'integrate')
        before = self._stats.clone()
        with torch.no_grad():
            ops.tsdf_integrate(self._sum, self._count, self._stats, self.origin, self.voxel_size, self.trunc, vps, dirs, depth, pose=pose, mask=mask,
                               min_depth=min_depth, max_range=max_range, carve_from=carve_from)
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


def _scan_args(cloud, pose, mask, device, who):
    """(vps, dirs, depth, pose, mask) of one scan as the ops take them."""
    if isinstance(cloud, np.ndarray):
        cloud = DepthCloud.from_structured_array(cloud, dtype=np.float64, device=device)
    if not isinstance(cloud, DepthCloud):
        raise TypeError('%s takes a DepthCloud or a structured array, got %s' % (who, type(cloud).__name__))
    if not cloud.dirs.is_cuda:
        raise RuntimeError('%s needs the cloud on a GPU (depth_correction_amd has no CPU path)' % who)
    if mask is None:
        mask = cloud.mask
    if mask is not None:
        mask = torch.as_tensor(mask, device=device).reshape(-1).contiguous()
    if pose is not None:
        pose = torch.as_tensor(np.asarray(pose.detach().cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64),
                               device=device).reshape(4, 4).contiguous()
    dt = cloud.dirs.dtype
    return cloud.vps.detach().to(dt).contiguous(), cloud.dirs.detach().contiguous(), cloud.depth.detach().to(dt).contiguous(), pose, mask


class SparseTsdfVolume(object):
    """A block-allocated TSDF volume on a GPU: the unbounded lattice of voxels of ``voxel_size`` metres at ``origin`` [3] (voxel i has
    the centre origin + (i + 0.5) voxel_size, any integer i), truncation ``trunc`` (None: 3 voxels), with storage for the 8 x 8 x 8
    blocks rays have written to.  On any window of the lattice it holds the bits a TsdfVolume with the same origin holds.

    ``max_blocks`` None: the pool grows as scans need it (one host read per scan).  A number: the pool is fixed, nothing is read between
    allocation and integration, and what does not fit is dropped and reported.  Carving is not supported: it would allocate the free
    space that sparsity exists to avoid."""

    INITIAL_BLOCKS = 1024

    def __init__(self, voxel_size, trunc=None, origin=(0.0, 0.0, 0.0), max_blocks=None, device=None):
        self.device = _gpu(device, 'SparseTsdfVolume')
        self.origin = tuple(float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3))
        self.voxel_size = float(voxel_size)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        if not (self.voxel_size > 0.0 and math.isfinite(self.voxel_size) and self.trunc > 0.0 and math.isfinite(self.trunc)):
            raise ValueError('SparseTsdfVolume needs a voxel size and a truncation > 0, got %r and %r' % (voxel_size, trunc))
        if not all(math.isfinite(v) for v in self.origin):
            raise ValueError('SparseTsdfVolume needs a finite origin, got %r' % (origin,))
        self.max_blocks = None if max_blocks is None else int(max_blocks)
        if self.max_blocks is not None and not 1 <= self.max_blocks <= ops.TSDF_MAX_BLOCKS:
            raise ValueError('SparseTsdfVolume needs max_blocks in 1 .. 2^22 - 1 or None, got %r' % (max_blocks,))
        self._make(self.INITIAL_BLOCKS if self.max_blocks is None else self.max_blocks)
        self._stats = torch.zeros((5,), dtype=torch.int64, device=self.device)
        self._info = torch.zeros((2,), dtype=torch.int64, device=self.device)

    def _make(self, capacity, old=None):
        """Table and pool of ``capacity`` blocks, holding what ``old`` = (keys, slots, sum, count) held."""
        kw = dict(device=self.device)
        keys, slots = torch.zeros((capacity,), dtype=torch.int64, **kw), torch.zeros((capacity,), dtype=torch.int32, **kw)
        sum_, count = torch.zeros((capacity, 512), dtype=torch.int64, **kw), torch.zeros((capacity, 512), dtype=torch.int32, **kw)
        if old is None:
            self._n_blocks = torch.zeros((1,), dtype=torch.int64, **kw)
            self._n_host = 0
        else:
            for new, was in zip((keys, slots, sum_, count), old):
                new[:was.shape[0]] = was
        self._keys, self._slots, self._sum, self._count = keys, slots, sum_, count

    def __repr__(self):
        return 'SparseTsdfVolume(%d blocks of 8 x 8 x 8 voxels of %g m at %s, truncation %g m, room for %d)' % (
            self.n_blocks, self.voxel_size, self.origin, self.trunc, self.capacity)

    @property
    def capacity(self):
        return self._keys.shape[0]

    @property
    def n_blocks(self):
        """The blocks in the table (a host read when a fixed pool has been written to since the last one)."""
        if self._n_host is None:
            self._n_host = int(self._n_blocks.item())
        return self._n_host

    @property
    def nbytes(self):
        """The bytes of the table and the pool."""
        return sum(t.numel() * t.element_size() for t in (self._keys, self._slots, self._sum, self._count))

    def reset(self):
        for t in (self._keys, self._slots, self._sum, self._count, self._n_blocks, self._stats, self._info):
            t.zero_()
        self._n_host = 0

    def integrate(self, cloud, pose=None, mask=None, min_depth=0.0, max_range=None, carve_from=None):
        """Adds one scan as TsdfVolume.integrate does; returns this call's stats as a dict of ints (SPARSE_STATS_FIELDS: the dense
        fields, the visits dropped for want of a block, and the blocks in the table afterwards)."""
        if carve_from is not None:
            raise ValueError('a sparse volume does not carve: carve_from must be None, got %r' % (carve_from,))
        vps, dirs, depth, pose, mask = _scan_args(cloud, pose, mask, self.device, 'integrate')
        rule = (self.origin, self.voxel_size, self.trunc, vps, dirs, depth)
        kw = dict(pose=pose, mask=mask, min_depth=min_depth, max_range=max_range)
        before = self._stats.clone()
        with torch.no_grad():
            ops.tsdf_sparse_allocate(self._keys, self._slots, self._n_blocks, self._info, *rule, **kw)
            if self.max_blocks is None:
                blocks, refused = self._info.tolist()
                if refused > 0:
                    capacity = min(max(2 * self.capacity, self.capacity + refused), ops.TSDF_MAX_BLOCKS)
                    if capacity < blocks + refused:
                        raise ValueError('the scan needs %d blocks, a sparse volume holds %d at the most' % (blocks + refused, ops.TSDF_MAX_BLOCKS))
                    self._make(capacity, old=(self._keys, self._slots, self._sum, self._count))
                    ops.tsdf_sparse_allocate(self._keys, self._slots, self._n_blocks, self._info, *rule, **kw)
            ops.tsdf_sparse_integrate(self._keys, self._slots, self._n_blocks, self._sum, self._count, self._stats, *rule, **kw)
        out = (self._stats - before).tolist() + [0]
        out[-1] = self._n_host = int(self._info[0].item())
        return dict(zip(SPARSE_STATS_FIELDS, out))

    def stats(self):
        """The stats of all calls since the last reset."""
        return dict(zip(SPARSE_STATS_FIELDS, self._stats.tolist() + [self.n_blocks]))

    def blocks(self):
        """(coords i32 [n, 3] in key order, slots i32 [n]) of the blocks in the table."""
        n = self.n_blocks
        keys = self._keys[:n]
        coords = torch.stack([keys >> 42, (keys >> 21) & 0x1fffff, keys & 0x1fffff], dim=1) - 2 ** 20
        return coords.to(torch.int32), self._slots[:n].clone()

    def window(self, lo, dims):
        """(sum i64, count i32) [nx, ny, nz] of the voxels lo .. lo + dims of the lattice; a voxel without a block holds 0."""
        lo, dims = tuple(int(v) for v in lo), tuple(int(v) for v in dims)
        if len(lo) != 3 or len(dims) != 3 or min(dims) < 1:
            raise ValueError('window takes lo [3] and dims [3] >= 1, got %r and %r' % (lo, dims))
        n = self.n_blocks
        ax = [torch.arange(l, l + d, dtype=torch.int64, device=self.device) for l, d in zip(lo, dims)]
        ix, iy, iz = torch.meshgrid(*ax, indexing='ij')
        key = (((ix >> 3) + 2 ** 20) << 42) | (((iy >> 3) + 2 ** 20) << 21) | ((iz >> 3) + 2 ** 20)
        in_range = torch.ones(dims, dtype=torch.bool, device=self.device)
        for i in (ix, iy, iz):
            in_range &= ((i >> 3) >= -2 ** 20) & ((i >> 3) < 2 ** 20)
        local = ((ix & 7) * 8 + (iy & 7)) * 8 + (iz & 7)
        sum_ = torch.zeros(dims, dtype=torch.int64, device=self.device)
        count = torch.zeros(dims, dtype=torch.int32, device=self.device)
        if n:
            pos = torch.searchsorted(self._keys[:n], key.reshape(-1)).reshape(dims).clamp(max=n - 1)
            have = (self._keys[:n][pos] == key) & in_range
            at = self._slots[:n][pos].to(torch.int64) * 512 + local
            sum_[have] = self._sum.reshape(-1)[at[have]]
            count[have] = self._count.reshape(-1)[at[have]]
        return sum_, count

    def tables(self):
        """The table, the pool and the lattice as ops.tsdf_loss reads them (ops.TsdfTables; the tensors are shared, not copied)."""
        return ops.TsdfTables(self._keys, self._slots, self._n_blocks, self._sum, self._count, self.origin, self.voxel_size, self.trunc)

    def sample(self, points, pose=None, min_count=1, stop=None, out=None):
        """The fused signed distance at ``points`` [M,3] (moved by ``pose`` 4 x 4 when given): dict(x f64 [M,3] the moved points, value
        [M] metres (trilinear over the eight voxels around a point), grad [M,3] its gradient, dist [M] = |value|, flag u8 [M]: 0, 1 out of
        range / not finite, 2 one of the eight voxels unobserved), all on the device.  An invalid point has value NaN, grad 0, dist +inf.
        The distance of any cloud to the fused surface without extracting a mesh; slam.TsdfMapper registers scans with it."""
        points = torch.as_tensor(points, device=self.device).to(torch.float64).reshape(-1, 3).contiguous()
        if pose is not None and not (isinstance(pose, torch.Tensor) and pose.is_cuda):
            pose = torch.as_tensor(np.asarray(pose, dtype=np.float64), device=self.device)
        if pose is not None:
            pose = pose.to(torch.float64).reshape(4, 4).contiguous()
        with torch.no_grad():
            return ops.tsdf_sparse_sample(self._keys, self._slots, self._n_blocks, self._sum, self._count, self.origin, self.voxel_size,
                                          self.trunc, points, pose=pose, min_count=min_count, stop=stop, out=out)

    def raycast(self, vps, dirs, poses=None, scan_offset=None, **kw):
        """Casts the rays (vps, dirs [N,3]; f32 or f64) against the fused surface without extracting it: dict(face, t, inc, normal, phi,
        status, samples) of ops.tsdf_sparse_cast_rays, whose keywords (t_min, t_max, step, refine, min_count, mask, own, skip, out) pass
        through.  Without ``poses`` the rays are in the volume's frame; with ``poses`` [S,4,4] and ``scan_offset`` (S + 1 offsets) ray i
        of scan s is moved by pose s first.  ``t`` is in units of |dirs[i]|; ``normal`` is the field's gradient at the hit, not a face's."""
        dirs = torch.as_tensor(dirs, device=self.device)
        if dirs.dtype not in (torch.float32, torch.float64):
            dirs = dirs.to(torch.float64)
        dirs = dirs.reshape(-1, 3).contiguous()
        n = dirs.shape[0]
        vps = torch.as_tensor(vps, device=self.device).to(dirs.dtype).reshape(-1, 3)
        if vps.shape[0] == 1 and n != 1:
            vps = vps.expand(n, 3)
        vps = vps.contiguous()
        if poses is None:
            if scan_offset is not None:
                raise ValueError('raycast takes scan_offset with poses only')
            poses, scan_offset = torch.eye(4, dtype=torch.float64, device=self.device).reshape(1, 4, 4), [0, n]
        else:
            if not (isinstance(poses, torch.Tensor) and poses.is_cuda):
                poses = torch.as_tensor(np.asarray(poses, dtype=np.float64), device=self.device)
            poses = poses.to(torch.float64).reshape(-1, 4, 4).contiguous()
            if scan_offset is None:
                if poses.shape[0] != 1:
                    raise ValueError('raycast needs scan_offset with %d poses' % poses.shape[0])
                scan_offset = [0, n]
        with torch.no_grad():
            return ops.tsdf_sparse_cast_rays(self.tables(), vps, dirs, scan_offset, poses, **kw)

    def raycast_cloud(self, cloud, pose=None, mask=None, **kw):
        """raycast for the rays of one DepthCloud (its view points and directions, its mask unless ``mask`` is given) under ``pose``
        [4,4]: what each ray would have measured on the fused surface (t in units of |dirs[i]|: metres for unit directions, to hold
        against cloud.depth) and at what incidence angle."""
        vps, dirs, _, pose, mask = _scan_args(cloud, pose, mask, self.device, 'raycast_cloud')
        return self.raycast(vps, dirs, poses=None if pose is None else pose.reshape(1, 4, 4), mask=mask, **kw)

    def extract(self, min_count=1):
        """(vertices f64 [Nv,3], faces i32 [Nf,3]) on the device; both empty when the volume holds no surface."""
        return ops.tsdf_sparse_extract(self._keys, self._slots, self.n_blocks, self._sum, self._count, self.origin, self.voxel_size,
                                       min_count=min_count)

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
                device=None, sparse=False):
    """(mesh, volume): the scans ``clouds`` (DepthClouds or structured arrays, sensor frame) moved by ``poses`` ([4,4] each, world from
    sensor) fused at ``voxel_size`` and extracted.  With a ``model`` every cloud is corrected by ``model(cloud)`` first.  ``bounds`` (lo
    [3], hi [3]) default to the box of the posed end points (torch min / max on the device); the volume pads them by the truncation.
    With ``sparse`` the volume is a SparseTsdfVolume at the origin (0, 0, 0): no bounds are computed, and ``bounds`` or ``carve_from``
    given raise ValueError."""
    device = _gpu(device, 'reconstruct')
    if sparse and (bounds is not None or carve_from is not None):
        raise ValueError('reconstruct(sparse=True) takes neither bounds nor carve_from: the sparse lattice has no box and does not carve')
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
    if sparse:
        volume = SparseTsdfVolume(voxel_size, trunc=trunc, device=device)
        for c, T in zip(clouds, poses):
            volume.integrate(c, pose=T, min_depth=min_depth, max_range=max_range)
        return volume.extract_mesh(min_count), volume
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
