"""Surveyed point clouds as ground truth (the FEE corridor's ``global_cloud``, datasets/fee_corridor.py:169-178,240-248; the board
cloud of scripts/map_bias_removal:579-737).

``SurveyCloud`` has the role ``mesh.TriangleMesh`` has for the rendered datasets: float64 points ``[M,3]`` and unit normals
``[M,3]`` kept where they were given (host or device) and, on demand, on a GPU together with the k-NN grid of one
``dc_knn_grid_build`` -- built once and searched by every ``dc_cloud_loss`` / ``metrics.point_to_cloud_distance`` call after it.
The orientation of a normal is irrelevant (the plane residual is taken by absolute value).  Rows whose normal is not finite
can never be matched by the plane form: they are dropped at construction (``n_dropped``).
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

__all__ = ['SurfelBVH', 'SurveyCloud', 'SurveyOnDevice', 'mesh_survey', 'DEFAULT_SAMPLES', 'SURVEY_SEED']

DEFAULT_SAMPLES = 200000       # Config.cloud_samples
SURVEY_SEED = 135              # the fixed seed of the surveys the mesh datasets sample


class SurfelBVH(object):
    """Device arrays of ``dc_surfel_bvh_build`` (layout: include/dc_hip.h): the survey's points as oriented disks, for
    ops.surfel_cast_rays.  ``radii`` f64 [M] are the radii it was built with (survey order), when the builder kept them."""

    def __init__(self, leaf_index, child, parent, node_box, leaf_disk, radii=None):
        self.leaf_index, self.child, self.parent, self.node_box, self.leaf_disk = leaf_index, child, parent, node_box, leaf_disk
        self.radii = radii

    @property
    def n_disks(self):
        return self.leaf_index.shape[0]

    @property
    def device(self):
        return self.leaf_index.device


class SurveyOnDevice(object):
    """Device copies of a survey and its persistent grid: points / normals f64 [M,3], ``grid`` (ops.KnnGrid, k = 1)."""

    def __init__(self, points, normals, grid):
        self.points, self.normals, self.grid = points, normals, grid
        self.device = points.device
        self._pose = None
        self._origin = None

    @property
    def n(self):
        return self.points.shape[0]

    def identity_pose(self):
        if self._pose is None:
            self._pose = torch.eye(4, dtype=torch.float64, device=self.device)
        return self._pose

    def origin(self):
        """Centre of the survey's bounds, f64 device [3] (computed on the device, once): the origin registration takes the survey's
        moments about."""
        if self._origin is None:
            self._origin = 0.5 * (self.points.amin(dim=0) + self.points.amax(dim=0))
        return self._origin

    def reserve(self, n_query):
        """The grid's query buffer holds ``n_query_max`` rows: rebuild the grid (the same grid, a larger buffer) when more are
        asked for.  A plan asks once, before training starts."""
        if n_query > self.grid.n_query_max:
            from . import ops
            self.grid = ops.knn_grid_build(self.points, int(n_query), 1)
        return self


class SurveyCloud(object):
    """float64 points [M,3] and unit normals [M,3] of a surveyed cloud."""

    MIN_QUERIES = 1 << 16          # rows of the grid's query buffer on first use (SurveyOnDevice.reserve grows it)

    def __init__(self, points, normals):
        points, normals = torch.as_tensor(points), torch.as_tensor(normals)
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise ValueError('points must be a non-empty [M,3] array, got shape %s' % (tuple(points.shape),))
        if normals.shape != points.shape:
            raise ValueError('normals must have the shape of points %s, got %s' % (tuple(points.shape), tuple(normals.shape)))
        points = points.detach().to(torch.float64)
        normals = normals.detach().to(device=points.device, dtype=torch.float64)
        if not bool(torch.isfinite(points).all()):
            raise ValueError('survey points must be finite')
        keep = torch.isfinite(normals).all(dim=1)
        self.n_dropped = int((~keep).sum())
        if self.n_dropped:
            warnings.warn('SurveyCloud: dropped %d of %d points whose normal is not finite' % (self.n_dropped, points.shape[0]))
            points, normals = points[keep], normals[keep]
            if points.shape[0] == 0:
                raise ValueError('no survey point has a finite normal')
        norm = torch.linalg.norm(normals, dim=1, keepdim=True)
        if bool((norm == 0).any()):
            raise ValueError('survey normals must not be zero')
        self.points = points.contiguous()
        self.normals = (normals / norm).contiguous()
        self._device = {}
        self._surfels = {}
        self._descriptors = {}
        self._planes = {}

    def __len__(self):
        return self.points.shape[0]

    def __repr__(self):
        return 'SurveyCloud(%d points%s)' % (len(self), ', %d dropped' % self.n_dropped if self.n_dropped else '')

    @property
    def bounds(self):
        return self.points.min(dim=0).values.cpu().numpy(), self.points.max(dim=0).values.cpu().numpy()

    # ---- constructors ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def from_points(points, normals=None, nn_k=None, nn_r=None, device='cuda'):
        """Survey of points [M,3]; without ``normals`` they are computed once by the package's feature kernels over the ``nn_k``
        nearest neighbours / the ball ``nn_r`` (as DepthCloud.update_all; default nn_k = 10) on ``device`` -- a point with too few
        neighbours for a plane gets a NaN normal and is dropped."""
        if normals is None:
            from .depth_cloud import DepthCloud
            dev = torch.device(device)
            if dev.type != 'cuda' or not torch.cuda.is_available():
                raise RuntimeError('computing survey normals needs a GPU: depth_correction_amd has no CPU path (or pass normals)')
            pts = torch.as_tensor(points).detach().to(device=dev, dtype=torch.float64).contiguous()
            cloud = DepthCloud.from_points(pts)
            if not nn_k and not nn_r:
                nn_k = 10
            cloud.update_all(k=nn_k or None, r=nn_r or None)
            points, normals = pts, cloud.normals.detach()
        return SurveyCloud(points, normals)

    @staticmethod
    def from_file(path, nn_k=None, nn_r=None, device='cuda'):
        """Survey of an ``.npz`` cloud (scan_io.read_points_npz: a plain [M,3+] array, or the structured layout of
        fee_corridor.py:35-38 with x, y, z and optionally normal_x, normal_y, normal_z)."""
        from numpy.lib.recfunctions import structured_to_unstructured
        from .scan_io import read_points_npz
        arr = read_points_npz(path)
        normals = None
        if arr.dtype.names:
            if 'normal_x' in arr.dtype.names:
                normals = structured_to_unstructured(arr[['normal_x', 'normal_y', 'normal_z']]).astype(np.float64)
            arr = structured_to_unstructured(arr[['x', 'y', 'z']])
        pts = np.ascontiguousarray(arr[:, :3], dtype=np.float64)
        return SurveyCloud.from_points(pts, normals, nn_k=nn_k, nn_r=nn_r, device=device)

    @staticmethod
    def from_mesh(mesh, n_samples, seed=135, device='cuda'):
        """``n_samples`` area-weighted samples of a mesh.TriangleMesh with the normals of the sampled faces (TriangleMesh.sample): a
        survey whose true surface is known."""
        pts, normals, _ = mesh.sample(int(n_samples), seed=seed, device=device)
        return SurveyCloud(pts, normals)

    # ---- registration (registration.py; DESIGN "Survey registration") ------------------------------------------------------------
    def register(self, points, **kw):
        """registration.register_cloud(points, self, **kw): the Registration whose ``T`` takes ``points`` into this survey's frame."""
        from .registration import register_cloud
        return register_cloud(points, self, **kw)

    def register_global(self, points, **kw):
        """registration.register_global(points, self, **kw): the GlobalRegistration of a cloud without a prior."""
        from .registration import register_global
        return register_global(points, self, **kw)

    def global_descriptors(self, device, voxel, feature_k, feature_radius):
        """(points f64 [m,3], normals f64 [m,3], feat f32 [m,33], has i32 [m]) of the survey's side of registration.register_global
        on ``device`` (a GPU): the voxel-filtered survey with its descriptors, computed once per device and argument set."""
        dev = self.on_device(device)
        key = (dev.device, float(voxel), int(feature_k), float(feature_radius))
        got = self._descriptors.get(key)
        if got is None:
            from .registration import global_descriptors
            with torch.no_grad():
                got = self._descriptors[key] = global_descriptors(dev.points, dev.normals, *key[1:])
        return got

    def register_planes(self, points, **kw):
        """registration.register_planes(points, self, **kw): the GlobalRegistration of a map of rooms or corridors without a prior."""
        from .registration import register_planes
        return register_planes(points, self, **kw)

    def planes(self, device, plane_voxel=0.1, distance_threshold=0.03, min_support=100, ransac_iters=500, cluster_eps=0.4, max_planes=32,
               seed=0):
        """(params f64 [P,4], support i64 [P]) of the survey's side of registration.register_planes on ``device`` (a GPU): its planes
        by registration.cloud_planes, computed once per device and argument set."""
        dev = self.on_device(device)
        key = (dev.device, None if plane_voxel is None else float(plane_voxel), float(distance_threshold), int(min_support),
               int(ransac_iters), None if cluster_eps is None else float(cluster_eps), int(max_planes), int(seed))
        got = self._planes.get(key)
        if got is None:
            from .registration import cloud_planes
            with torch.no_grad():
                got = self._planes[key] = cloud_planes(dev.points, *key[1:])
        return got

    def transformed(self, T):
        """A new SurveyCloud whose points are ``T`` (4 x 4 rigid) applied to these and whose normals are rotated with them; it has a
        device cache (copies and grid) of its own."""
        T = torch.as_tensor(T.detach().cpu() if isinstance(T, torch.Tensor) else np.asarray(T, dtype=np.float64), dtype=torch.float64)
        if T.shape != (4, 4):
            raise ValueError('T must be a 4 x 4 transform, got shape %s' % (tuple(T.shape),))
        T = T.to(self.points.device)
        R, t = T[:3, :3], T[:3, 3]
        return SurveyCloud(self.points @ R.T + t, self.normals @ R.T)

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def on_device(self, device):
        """SurveyOnDevice on ``device`` (a GPU): the copies and the grid are made once."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('a survey is searched on a GPU (device %s): depth_correction_amd has no CPU path' % device)
        if not torch.cuda.is_available():
            raise RuntimeError('a survey is searched on a GPU, and torch sees none: depth_correction_amd has no CPU path')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            from . import ops
            p = self.points.to(device).contiguous()
            n = self.normals.to(device).contiguous()
            got = self._device[device] = SurveyOnDevice(p, n, ops.knn_grid_build(p, self.MIN_QUERIES, 1))
        return got

    def surfels(self, device, radius=None, k=10, scale=1.0):
        """SurfelBVH of the survey on ``device`` (a GPU), built once per device and argument set: every point with its normal is a
        disk (DESIGN "Depth bias against a surveyed cloud").  A float ``radius`` is every disk's; None gives point i ``scale`` times
        the distance to its ``k``-th nearest other survey point (ops.knn on the survey itself), so that under uniform sampling about
        k disks cover every surface point."""
        if radius is not None:
            radius = float(radius)
            if not (radius > 0.0 and radius < float('inf')):
                raise ValueError('surfel radius must be finite and > 0, got %r' % (radius,))
        dev = self.on_device(device)
        if radius is not None:
            key = (dev.device, radius, None, None)
        else:
            k, scale = int(k), float(scale)
            if not 1 <= k <= 63:
                raise ValueError('surfel k must be in 1..63, got %r' % (k,))
            if not (scale > 0.0 and scale < float('inf')):
                raise ValueError('surfel scale must be finite and > 0, got %r' % (scale,))
            if len(self) <= k:
                raise ValueError('a survey of %d points has no %d-th nearest other point: give a radius' % (len(self), k))
            key = (dev.device, None, k, scale)
        got = self._surfels.get(key)
        if got is None:
            from . import ops
            if radius is not None:
                radii = torch.full((dev.n,), radius, dtype=torch.float64, device=dev.device)
            else:
                dist, _ = ops.knn(dev.points, k + 1)                    # column 0 is the point itself
                radii = (scale * dist[:, k]).contiguous()
            box = torch.cat([dev.points.amin(dim=0), dev.points.amax(dim=0)]).cpu().numpy()
            got = self._surfels[key] = ops.surfel_bvh_build(dev.points, dev.normals, radii, box)
            got.radii = radii
        return got


def mesh_survey(ds, n_samples=None, seed=SURVEY_SEED, device=None):
    """The survey a mesh dataset (one with get_mesh()) samples from its mesh: SurveyCloud.from_mesh(mesh, n_samples, seed), built at
    the first call and kept per (n_samples, seed) -- in the state the dataset's slices share, when it has one."""
    n = int(n_samples or DEFAULT_SAMPLES)
    state = getattr(ds, '_state', None)
    cache = state.setdefault('surveys', {}) if isinstance(state, dict) else ds.__dict__.setdefault('_surveys', {})
    got = cache.get((n, int(seed)))
    if got is None:
        got = cache[(n, int(seed))] = SurveyCloud.from_mesh(ds.get_mesh(), n, seed=int(seed), device=device or getattr(ds, 'device', 'cuda'))
    return got
