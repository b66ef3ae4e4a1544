"""Per-iteration glue with the reference's signatures (preproc.py:25-243): filtered / local feature clouds, the
global cloud, neighbourhood establishment, per-iteration features and the global mask -- for ball neighbourhoods and for
plane neighbourhoods (NeighborhoodType.plane: GPU RANSAC + DBSCAN segmentation and per-plane moments, segmentation.py).
"""
from __future__ import annotations

import numpy as np
import torch

from .config import Config, NeighborhoodType
from .depth_cloud import DepthCloud
from .filters import (filter_depth, filter_eigenvalue_ratios, filter_eigenvalues, filter_grid, filter_shadow_points, shadow_points_mask,
                      filter_valid_neighbors, within_bounds)
from .transform import xyz_axis_angle_to_matrix

__all__ = ['compute_neighborhood_features', 'deskew_cloud', 'establish_neighborhoods', 'filtered_cloud', 'global_cloud',
           'global_cloud_mask', 'local_feature_cloud', 'offset_cloud']


def _ball_only(cfg):
    if cfg.nn_type not in (NeighborhoodType.ball, NeighborhoodType.plane):
        raise NotImplementedError('only ball and plane neighbourhoods are implemented, got %s' % (cfg.nn_type,))


def filtered_cloud(cloud, cfg: Config):
    """Depth + voxel-grid pre-filters (preproc.py:25-32)."""
    if (cfg.min_depth is not None and cfg.min_depth > 0.0) or (cfg.max_depth is not None and cfg.max_depth < float('inf')):
        cloud = filter_depth(cloud, min=cfg.min_depth, max=cfg.max_depth, log=cfg.log_filters)
    if cfg.grid_res > 0.0:
        cloud = filter_grid(cloud, grid_res=cfg.grid_res, keep='random', log=cfg.log_filters,
                            rng=np.random.default_rng(cfg.random_seed))
    return cloud


def deskew_cloud(cloud, twist, ref=0.0, device=None):
    """A raw moving-sweep scan taken into the sensor frame at the sweep time ``ref`` (DESIGN "Moving-sweep rendering and de-skew"):
    ``cloud`` is a structured array with the field ``t`` (the sweep time of every point, render_lidar_clouds with a SweepModel), or a
    pair (points [N,3], t [N]); ``twist`` [6] = (v, w) of the sweep in the frame at its start.  D(ref)^-1 D(tau) = D(tau - ref) under
    the twist (Exp(-ref w) v, w) (sweep.shifted_twist), so the times are shifted, v is rotated and one kernel does the rest
    (ops.deskew).  Returns the same structured dtype with x, y, z, vp_* and normal_* replaced and ``t`` kept, or the points [N,3]."""
    from . import ops
    from .sweep import shifted_twist
    from numpy.lib.recfunctions import structured_to_unstructured
    tw = np.asarray(twist, dtype=np.float64)
    if tw.shape != (6,):
        raise ValueError('twist must be [6] = (v, w), got shape %s' % (tw.shape,))
    ref = float(ref)
    if not 0.0 <= ref <= 1.0:
        raise ValueError('ref must lie in [0, 1], got %r' % (ref,))
    names = getattr(getattr(cloud, 'dtype', None), 'names', None)
    if names:
        if 't' not in names:
            raise ValueError("the cloud has no field 't' (the sweep time of every point)")
        grab = lambda fields: np.ascontiguousarray(structured_to_unstructured(cloud[fields], dtype=np.float64)).reshape(-1, 3)
        pts, t = grab(['x', 'y', 'z']), np.asarray(cloud['t'], dtype=np.float64).reshape(-1)
        vps = grab(['vp_x', 'vp_y', 'vp_z']) if 'vp_x' in names else None
        nrm = grab(['normal_x', 'normal_y', 'normal_z']) if 'normal_x' in names else None
    else:
        if not isinstance(cloud, (tuple, list)) or len(cloud) != 2:
            raise ValueError("cloud must be a structured array with the field 't' or a pair (points, t)")
        pts = np.ascontiguousarray(np.asarray(cloud[0], dtype=np.float64)).reshape(-1, 3)
        t, vps, nrm = np.asarray(cloud[1], dtype=np.float64).reshape(-1), None, None
    if t.shape[0] != pts.shape[0]:
        raise ValueError('%d sweep times for %d points' % (t.shape[0], pts.shape[0]))
    dev = torch.device(device if device is not None else 'cuda')
    up = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()
    x, v, m = ops.deskew(up(pts), up(t - ref), [0, pts.shape[0]], shifted_twist(tw, ref)[None], vps=up(vps), normals=up(nrm))
    if not names:
        return x.cpu().numpy()
    out = cloud.copy()
    for fields, a in ((('x', 'y', 'z'), x), (('vp_x', 'vp_y', 'vp_z'), v), (('normal_x', 'normal_y', 'normal_z'), m)):
        if a is not None:
            a = a.cpu().numpy()
            for k, f in enumerate(fields):
                out[f] = a[:, k]
    return out


def _and_mask(cloud, mask):
    if cloud.mask is None:
        cloud.mask = torch.ones((len(cloud),), dtype=torch.bool, device=cloud.device())
    cloud.mask = cloud.mask & mask


def local_feature_cloud(cloud, cfg: Config):
    """Scan -> DepthCloud with neighbours, features and the planarity mask (preproc.py:35-64)."""
    if getattr(cfg, 'local_nn_type', 'ball') == 'image':
        return _image_feature_cloud(cloud, cfg)
    if isinstance(cloud, torch.Tensor):
        # raw rows [N, >=3] already on the device (what the node holds after the upload of a message)
        if cloud.is_cuda and cloud.dim() == 2 and cloud.dtype in (torch.float32, torch.float64) and cfg.shadow_angle_bounds:
            return _with_features(_prefiltered_cloud(cloud.detach(), cfg), cfg, points_current=True)
        return _with_features(DepthCloud.from_points(cloud[:, :3], dtype=cfg.numpy_float_type(), device=cfg.device), cfg)
    if isinstance(cloud, np.ndarray):
        make = DepthCloud.from_structured_array if cloud.dtype.names else DepthCloud.from_points
        cloud = make(cloud, dtype=cfg.numpy_float_type(), device=cfg.device)
    assert isinstance(cloud, DepthCloud)
    if cfg.shadow_angle_bounds:                      # preproc.py:44-47
        if cloud.dirs.is_cuda:
            # the direction-neighbour table would be dropped by cloud[mask] right away: the mask comes from one grid walk
            cloud = cloud[shadow_points_mask(cloud, cfg.shadow_neighborhood_angle, cfg.shadow_angle_bounds, log=cfg.log_filters)]
        else:
            cloud.update_dir_neighbors(angle=cfg.shadow_neighborhood_angle)
            cloud = filter_shadow_points(cloud, cfg.shadow_angle_bounds, log=cfg.log_filters)
    return _with_features(cloud, cfg)


_chords = {}


def _chord(angle):
    from .nearest_neighbors import ball_angle_to_distance
    if angle not in _chords:
        _chords[angle] = float(ball_angle_to_distance(torch.as_tensor(angle)))
    return _chords[angle]


def _prefiltered_cloud(raw, cfg: Config):
    """from_points + shadow filter + cloud[mask] of raw device rows in one native call (dc_scan_prefilter): the first statements of
    local_feature_cloud (preproc.py:36-47) without the host between their launches; the same kernels, the same cloud."""
    from . import ops
    from .filters import _shadow_bounds
    lo, hi, _ = _shadow_bounds(cfg.shadow_angle_bounds)
    # (the reference evaluates the chord in float32 tensor arithmetic, nearest_neighbors.py:13-19: kept, once per configuration value)
    r = _chord(float(cfg.shadow_neighborhood_angle))
    dtype = cfg.torch_float_type()
    n = raw.shape[0]
    vps, dirs, depth, points = ops.scan_prefilter(raw.contiguous(), None, dtype, r, lo, hi)
    if cfg.log_filters:
        print('%.3f = %i / %i points kept (shadow points removed).' % (len(dirs) / max(n, 1), len(dirs), n))
    return DepthCloud(vps, dirs, depth, points=points)


def _with_features(cloud, cfg: Config, points_current=False):
    """Neighbourhoods, features and the planarity mask (preproc.py:48-63).  ``points_current``: cloud.points already are
    vps + depth * dirs of its fields (dc_scan_prefilter wrote them): update_all's first statement is skipped."""
    if points_current and cloud.points is not None:
        cloud.update_neighbors(k=cfg.nn_k, r=cfg.nn_r, _weights=False)
        cloud.update_features(scale=None)
    else:
        cloud.update_all(k=cfg.nn_k, r=cfg.nn_r)
    return _bounds_mask(cloud, cfg)


def _bounds_mask(cloud, cfg: Config):
    """The eigenvalue and eigenvalue-ratio bounds ANDed into cloud.mask (preproc.py:52-63)."""
    if cloud.eigvals.is_cuda and not cfg.log_filters and (cfg.eigenvalue_bounds or cfg.eigenvalue_ratio_bounds):
        # the same masks without the ones / and passes between them: every bound in one kernel (dc_mask_bounds_multi), or one kernel per
        # bound ANDed in place (dc_mask_bounds) beyond eight
        from . import ops
        bounds = [(int(e), None, lo, hi) for e, lo, hi in (cfg.eigenvalue_bounds or [])] + \
                 [(int(i), int(j), lo, hi) for i, j, lo, hi in (cfg.eigenvalue_ratio_bounds or [])]
        if len(bounds) <= 8:
            # every bound in one pass over the eigenvalues (dc_mask_bounds_multi), written or ANDed into the mask
            cloud.mask = ops.mask_bounds_all(cloud.eigvals.detach().contiguous(), bounds,
                                             mask=None if cloud.mask is None else cloud.mask.clone())
            return cloud
        mask = torch.ones((len(cloud),), dtype=torch.bool, device=cloud.device()) if cloud.mask is None else cloud.mask.clone()
        ev = cloud.eigvals.detach().contiguous()
        for i, j, lo, hi in bounds:
            ops.mask_bounds(mask, ev, i, None if j is None else ev, 0 if j is None else j, lo, hi)
        cloud.mask = mask
        return cloud
    if cfg.eigenvalue_bounds:
        _and_mask(cloud, filter_eigenvalues(cloud, cfg.eigenvalue_bounds, only_mask=True, log=cfg.log_filters))
    if cfg.eigenvalue_ratio_bounds:
        _and_mask(cloud, filter_eigenvalue_ratios(cloud, cfg.eigenvalue_ratio_bounds, only_mask=True, log=cfg.log_filters))
    return cloud


def _image_feature_cloud(source, cfg: Config):
    """local_feature_cloud with ``local_nn_type = 'image'``: the scan is organised on the spherical grid of the configuration
    (image_size, image_fov, image_wrap; one point per pixel, the nearest), the scan-shadow mask comes from an image window, the
    neighbourhoods are the ``image_window`` around every pixel gated at ``nn_r`` (range_image.py, csrc/dc_rangeimage.hip).  The
    stages are issued back to back with the survivor count on the device; it is read ONCE, when the cloud's tensors are sized.
    Accepts raw device rows [N, >=3], a plain or structured array (an H x W one of the grid's shape is taken pixel by pixel) or a
    DepthCloud.  Results are not those of ball neighbourhoods (DESIGN "Range-image neighbourhoods")."""
    from . import ops, range_image as ri
    from .filters import _shadow_bounds
    grid = ri.SphericalGrid.from_config(cfg)
    window = ri.check_window(grid, cfg.image_window)
    with torch.no_grad():
        out = ri.organize_buffers(source, grid, dtype=cfg.torch_float_type(), device=cfg.device)
        count, pixel, index_image = out['count'], out['pixel'], out['index_image']
        vps, dirs, depth, points = out['vps'], out['dirs'], out['depth'], out['points']
        if cfg.shadow_angle_bounds:
            lo, hi, _ = _shadow_bounds(cfg.shadow_angle_bounds)
            angle = float(cfg.shadow_neighborhood_angle)
            keep = ops.image_shadow_mask(points, vps, dirs, pixel, index_image, grid, ri.shadow_window(grid, angle), _chord(angle), lo, hi,
                                         count=count)
            # (rows beyond the count carry 0 in the mask: the compaction needs no count, and dropping rows keeps the pixel order)
            (vps, dirs, depth, points, pixel), count = ops.compact_rows_device(keep, [vps, dirs, depth, points, pixel])
            index_image = ops.range_index_image(pixel, grid.rows, grid.cols, count=count)
        f = ops.image_features_fwd(points, dirs, pixel, index_image, grid, window, r=cfg.nn_r, count=count)
        m = int(count.item())                              # the one read
    if cfg.log_filters and cfg.shadow_angle_bounds:
        print('%i points kept on the %i x %i image (one per pixel, shadow points removed).' % (m, grid.rows, grid.cols))
    cloud = DepthCloud(vps[:m], dirs[:m], depth[:m], points=points[:m], mean=f['mean'][:m], cov=f['cov'][:m], eigvals=f['eigvals'][:m],
                       eigvecs=f['eigvecs'][:m], normals=f['normals'][:m], inc_angles=f['inc_angles'][:m], neighbors=f['neighbors'][:m])
    cloud.pixel, cloud.grid, cloud.index_image, cloud.nvalid = pixel[:m], grid, index_image, f['nvalid'][:m]
    return _bounds_mask(cloud, cfg)


def offset_cloud(clouds, model):
    corrected = [model(c) if model is not None else c for c in clouds]
    return DepthCloud.concatenate(corrected, fields=DepthCloud.source_fields + ['eigvals'])


def global_cloud(clouds=None, model=None, poses=None, pose_corrections=None, dataset=None):
    """Corrected scans moved to the world frame and concatenated (preproc.py:80-119)."""
    if dataset is not None:
        assert clouds is None and poses is None
        clouds, poses = zip(*dataset)
        clouds = [DepthCloud.from_structured_array(c, dtype=np.float64) for c in clouds]
        poses = torch.as_tensor(np.array(poses))
    assert clouds is not None and poses is not None
    if pose_corrections is not None:
        if pose_corrections.shape[-1] == 6:
            pose_corrections = xyz_axis_angle_to_matrix(pose_corrections)
        poses = poses @ pose_corrections
    moved = []
    for cloud, pose in zip(clouds, poses):
        if model is not None:
            cloud = model(cloud)
        moved.append(cloud.transform(pose))
    return DepthCloud.concatenate(moved, dependent=True)


def global_cloud_mask(cloud: DepthCloud, mask, cfg: Config):
    """AND of the global-cloud filters into ``mask`` (modified in place like the reference, preproc.py:122-164)."""
    if mask is None:
        mask = torch.ones((len(cloud),), dtype=torch.bool, device=cloud.device())
    else:
        print('%.3f = %i / %i points kept (previous filters).' % (mask.double().mean(), mask.sum(), mask.numel()))
    log = cfg.log_filters
    if cfg.min_valid_neighbors:
        mask &= filter_valid_neighbors(cloud, min=cfg.min_valid_neighbors, only_mask=True, log=log)
    if cfg.eigenvalue_bounds:
        mask &= filter_eigenvalues(cloud, bounds=cfg.eigenvalue_bounds, only_mask=True, log=log)
    if cfg.eigenvalue_ratio_bounds:
        mask &= filter_eigenvalue_ratios(cloud, bounds=cfg.eigenvalue_ratio_bounds, only_mask=True, log=log)
    if cfg.dir_dispersion_bounds:
        mask &= within_bounds(cloud.dir_dispersion(), bounds=cfg.dir_dispersion_bounds,
                              log_variable='dir dispersion' if log else None)
    if cfg.vp_dispersion_bounds:
        mask &= within_bounds(cloud.vp_dispersion(), bounds=cfg.vp_dispersion_bounds,
                              log_variable='vp dispersion' if log else None)
    if cfg.vp_dispersion_to_depth2_bounds:
        mask &= within_bounds(cloud.vp_dispersion_to_depth2(), bounds=cfg.vp_dispersion_to_depth2_bounds,
                              log_variable='vp dispersion to depth2' if log else None)
    return mask


def establish_neighborhoods(dataset=None, clouds=None, poses=None, cloud=None, cfg: Config = None):
    """(neighbors, weights) of the global cloud, found once before the optimisation (preproc.py:168-185)."""
    _ball_only(cfg)
    if cloud is None:
        cloud = global_cloud(clouds=clouds, poses=poses, dataset=dataset)
    if cfg.nn_type == NeighborhoodType.plane:        # preproc.py:186-191
        from .segmentation import Planes
        if not cloud.dirs.is_cuda:
            raise RuntimeError('plane neighbourhoods need a GPU: the cloud is on %s (depth_correction_amd has no CPU path)'
                               % cloud.dirs.device)
        return Planes.fit(cloud.to_points().detach(), cfg.ransac_dist_thresh, min_support=cfg.min_valid_neighbors,
                          max_iterations=cfg.num_ransac_iters, max_models=cfg.max_neighborhoods,
                          eps=2.0 * np.sqrt(3) * cfg.grid_res, seed=cfg.random_seed)
    cloud.update_all(k=cfg.nn_k, r=cfg.nn_r, scale=cfg.nn_scale, keep_neighbors=False)
    return cloud.neighbors, cloud.weights


def compute_neighborhood_features(dataset=None, clouds=None, poses=None, model=None, pose_corrections=None, cloud=None,
                                  neighborhoods=None, cfg: Config = None):
    """Features of the (re-corrected) global cloud on fixed neighbourhoods (preproc.py:195-217)."""
    _ball_only(cfg)
    if neighborhoods is None:
        neighborhoods = establish_neighborhoods(dataset=dataset, cloud=cloud, cfg=cfg)
    plane = cfg.nn_type == NeighborhoodType.plane
    if cloud is None:
        # plane neighbourhoods: the model is applied with the plane normals below (preproc.py:205-210)
        cloud = global_cloud(clouds=clouds, model=None if plane else model, poses=poses, pose_corrections=pose_corrections,
                             dataset=dataset)
    if plane:
        return _plane_features(cloud, neighborhoods, model)
    cloud.neighbors, cloud.weights = neighborhoods
    cloud.update_all(scale=cfg.nn_scale, keep_neighbors=True)
    return cloud


def _plane_features(cloud, planes, model):
    """Per-plane covariances and eigenvalues of the global cloud (preproc.py:218-243): the incidence angles against the plane
    normal, the model and the moments in one kernel (dc_plane_moments_fwd), eigh on the [P,3,3] result."""
    from .segmentation import plane_moments
    out = planes.copy()
    cov = plane_moments(cloud, planes, model)
    out.cov = cov
    out.eigvals = torch.linalg.eigh(cov)[0]

    def plane_clouds():
        clouds = []
        with torch.no_grad():
            for i in range(len(planes)):
                c = cloud[planes.indices[i].to(cloud.dirs.device)]
                c.mask = None
                c.normals = planes.params[i:i + 1, :-1].to(device=c.dirs.device, dtype=c.dirs.dtype).expand((len(c), -1))
                c.update_incidence_angles()
                clouds.append(model(c) if model is not None else c)
        return clouds
    out._plane_cloud_fn = plane_clouds
    return out
