"""Organised scans: a cloud on a spherical H x W range image, and neighbourhoods taken from an image window.

The reference's sensor delivers H x W organised clouds; its scripts flatten them (``if cloud.ndim == 2: cloud =
cloud.reshape((-1,))``) and project them back onto the sphere where they need an image (scripts/depth_denoising:44-116
``range_projection`` / ``depth_to_points``, scripts/compare_to_ddd).  Here the image is kept: in a range image the neighbours
of a pixel are the pixels around it, so neighbourhoods need no grid, no sort and no search (csrc/dc_rangeimage.hip, DESIGN
"Range-image neighbourhoods").

An organised cloud is a plain ``DepthCloud`` of the pixels' winners in ascending pixel order that carries three plain
attributes: ``cloud.pixel`` (int32 [M], r * W + c), ``cloud.grid`` (the ``SphericalGrid``) and ``cloud.index_image`` (int32
[H,W], the row of every pixel or -1; ``None`` until ``index_image(cloud)`` builds it).  ``DepthCloud``'s field lists do not know
them: slicing a cloud loses them, ``select(cloud, mask)`` slices and re-attaches them.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .depth_cloud import DepthCloud

__all__ = ['SphericalGrid', 'depth_to_points', 'image_features', 'image_shadow_mask', 'index_image', 'is_organized', 'organize',
           'project', 'select', 'shadow_window']

MAX_WINDOW = 121        # DC_IMAGE_MAX_WINDOW: slots of the largest window


class SphericalGrid(object):
    """rows x cols pixels over the full turn and the vertical field of view [fov_down, fov_up] (degrees, the reference's
    ``proj_fov_up`` / ``proj_fov_down``); ``wrap``: windows wrap over the column seam (rows never wrap)."""

    def __init__(self, rows, cols, fov_up, fov_down, wrap=True):
        self.rows, self.cols = int(rows), int(cols)
        self.fov_up, self.fov_down = float(fov_up), float(fov_down)
        self.wrap = bool(wrap)
        if self.rows < 1 or self.cols < 1 or not (0.0 < self.fov < float('inf')):
            raise ValueError('a grid needs rows, cols >= 1 and a field of view')

    @property
    def fov(self):
        """Vertical field of view in radians, as the pixel rule evaluates it."""
        return abs(self.fov_down / 180.0 * math.pi) + abs(self.fov_up / 180.0 * math.pi)

    @property
    def pitch_step(self):
        return self.fov / self.rows

    @property
    def yaw_step(self):
        return 2.0 * math.pi / self.cols

    @property
    def pitch_max(self):
        return max(abs(self.fov_up), abs(self.fov_down)) / 180.0 * math.pi

    def __eq__(self, other):
        return isinstance(other, SphericalGrid) and vars(self) == vars(other)

    def __hash__(self):
        return hash(tuple(sorted(vars(self).items())))

    def __repr__(self):
        return 'SphericalGrid(%d, %d, %g, %g, wrap=%s)' % (self.rows, self.cols, self.fov_up, self.fov_down, self.wrap)

    @staticmethod
    def from_config(cfg):
        return SphericalGrid(cfg.image_size[0], cfg.image_size[1], cfg.image_fov[0], cfg.image_fov[1], wrap=cfg.image_wrap)


def check_window(grid, window):
    ah, aw = int(window[0]), int(window[1])
    if ah < 0 or aw < 0 or 2 * ah + 1 > grid.rows or 2 * aw + 1 > grid.cols or (2 * ah + 1) * (2 * aw + 1) > MAX_WINDOW:
        raise ValueError('window (%d, %d) does not fit: 2 ah + 1 <= %d, 2 aw + 1 <= %d and at most %d slots'
                         % (ah, aw, grid.rows, grid.cols, MAX_WINDOW))
    return ah, aw


def shadow_window(grid, angle):
    """Half extents of the window that holds every direction within ``angle`` (radians) of a pixel's own: floor(angle / pitch
    step) + 1 rows, floor(angle / (yaw step * cos(pitch_max))) + 1 columns (a column is narrowest at the rim of the field of
    view); raises when it passes the cap of 121 slots."""
    ah = int(math.floor(angle / grid.pitch_step)) + 1
    aw = int(math.floor(angle / (grid.yaw_step * math.cos(grid.pitch_max)))) + 1
    ah, aw = min(ah, (grid.rows - 1) // 2), min(aw, (grid.cols - 1) // 2)      # (the whole image is as far as a window goes)
    if (2 * ah + 1) * (2 * aw + 1) > MAX_WINDOW:
        raise ValueError('a shadow neighbourhood of %g rad needs a window of (%d, %d) on %r: more than %d slots'
                         % (angle, ah, aw, grid, MAX_WINDOW))
    return ah, aw


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _rows_of(source, dtype, device):
    """(points [N, >=3] device tensor, vps [N,3] | None, (H, W) | None) of a DepthCloud, a tensor, a plain or a structured array."""
    shape = None
    if isinstance(source, DepthCloud):
        pts = source.to_points().detach()
        vps = source.vps.detach().to(pts.dtype)
        vps = None if vps.shape[0] == 1 and not bool((vps != 0).any()) else vps.expand_as(pts).contiguous()
        return pts.contiguous(), vps, None
    vps = None
    if isinstance(source, np.ndarray) and source.dtype.names:
        from numpy.lib.recfunctions import structured_to_unstructured
        if source.ndim == 2:
            shape = source.shape
        flat = source.reshape(-1)
        pts = structured_to_unstructured(flat[['x', 'y', 'z']])
        if 'vp_x' in source.dtype.names:
            vps = torch.as_tensor(np.ascontiguousarray(structured_to_unstructured(flat[['vp_x', 'vp_y', 'vp_z']], dtype=pts.dtype)), device=device)
        source = np.ascontiguousarray(pts)
    pts = torch.as_tensor(source, device=device) if not isinstance(source, torch.Tensor) else source.detach()
    if device is not None and pts.device != torch.device(device):
        pts = pts.to(device)
    if pts.dim() == 3:
        shape = tuple(pts.shape[:2])
        pts = pts.reshape(-1, pts.shape[-1])
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError('points need shape [N, >=3] or [H, W, >=3]')
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.to(dtype or torch.float64)
    return pts.contiguous(), vps, shape


def _torch_dtype(dtype):
    if dtype is None or isinstance(dtype, torch.dtype):
        return dtype
    return getattr(torch, np.dtype(dtype).name)


def project(points, grid, vps=None, clamp=True, min_depth=0.):
    """(pixel int32 [N], index_image int32 [H,W], range_image [H,W]) of a cloud or of sensor-frame points: the reference's
    ``range_projection`` with the winner of every pixel (the nearest point, ties to the lower index) kept as an index; -1 marks
    rejected points and empty pixels (the range image holds -1 there as the reference's does)."""
    pts, own_vps, _ = _rows_of(points, None, None)
    if vps is None:
        vps = own_vps
    elif not isinstance(vps, torch.Tensor):
        vps = torch.as_tensor(np.asarray(vps), device=pts.device)
    if vps is not None:
        vps = vps.to(device=pts.device, dtype=pts.dtype).reshape(-1, 3).contiguous()
    return ops.range_project(pts, grid, vps=vps, clamp=clamp, min_depth=min_depth)


def _attach(cloud, pixel, grid, index_image_):
    cloud.pixel, cloud.grid, cloud.index_image = pixel, grid, index_image_
    return cloud


def is_organized(cloud):
    return getattr(cloud, 'pixel', None) is not None and getattr(cloud, 'grid', None) is not None


def organize_buffers(source, grid, vps=None, clamp=True, min_depth=0., dtype=None, device=None, want_index=False):
    """The native call behind ``organize`` without the read-back: full-size buffers and the survivor count on the device
    (``ops.range_organize`` / ``ops.range_from_grid``).  An H x W array whose shape is the grid's takes the no-projection entry."""
    dtype = _torch_dtype(dtype)
    pts, own_vps, shape = _rows_of(source, dtype, device)
    if vps is None:
        vps = own_vps
    elif not isinstance(vps, torch.Tensor):
        vps = torch.as_tensor(np.asarray(vps))
    if vps is not None:
        vps = vps.to(device=pts.device, dtype=pts.dtype).reshape(-1, 3).contiguous()
    if not pts.is_cuda:
        raise RuntimeError('organize needs GPU tensors (depth_correction_amd has no CPU path)')
    if shape is not None:
        if shape != (grid.rows, grid.cols):
            raise ValueError('an H x W array must have the grid\'s shape %s, got %s' % ((grid.rows, grid.cols), shape))
        return ops.range_from_grid(pts, grid.rows, grid.cols, vps=vps, min_depth=min_depth, dtype=dtype, want_index=want_index)
    return ops.range_organize(pts, grid, vps=vps, clamp=clamp, min_depth=min_depth, dtype=dtype, want_index=want_index)


def organize(source, grid, vps=None, clamp=True, min_depth=0., dtype=None, device=None, want_index=False):
    """DepthCloud of the survivors of a cloud / of points [N, >=3] / of an H x W (structured) array in ascending pixel order, with
    ``cloud.pixel``, ``cloud.grid`` and ``cloud.index_image``.  One point per pixel: the nearest, ties to the lower input row.
    ``want_index``: also ``cloud.source_index`` (int32 [M]), the input row of every survivor."""
    out = organize_buffers(source, grid, vps=vps, clamp=clamp, min_depth=min_depth, dtype=dtype, device=device, want_index=want_index)
    m = int(out['count'].item())
    cloud = DepthCloud(out['vps'][:m], out['dirs'][:m], out['depth'][:m], points=out['points'][:m])
    _attach(cloud, out['pixel'][:m], grid, out['index_image'])
    if want_index:
        cloud.source_index = out['index'][:m]
    return cloud


def index_image(cloud):
    """``cloud.index_image``, built from ``cloud.pixel`` when it is not there yet."""
    if not is_organized(cloud):
        raise ValueError('not an organised cloud: use range_image.organize')
    if getattr(cloud, 'index_image', None) is None:
        cloud.index_image = ops.range_index_image(cloud.pixel.contiguous(), cloud.grid.rows, cloud.grid.cols)
    return cloud.index_image


def select(cloud, mask):
    """``cloud[mask]`` of an organised cloud that stays organised: dropping rows keeps the pixel order, so the kept pixels are
    ``pixel[mask]`` and the index image is rebuilt from them on first use."""
    if not is_organized(cloud):
        raise ValueError('not an organised cloud: use range_image.organize')
    out = cloud[mask]
    return _attach(out, cloud.pixel[mask].contiguous(), cloud.grid, None)


def depth_to_points(range_image, grid):
    """Points [M,3] of the occupied pixels (range > 0) of a range image, in pixel order: the reference's ``depth_to_points``
    (scripts/depth_denoising:94-116) evaluated at the pixel CENTRES of ``project``'s rule, of which it is the inverse."""
    as_numpy = isinstance(range_image, np.ndarray)
    d = torch.as_tensor(range_image)
    if d.shape != (grid.rows, grid.cols):
        raise ValueError('range image has shape %s, the grid %s' % (tuple(d.shape), (grid.rows, grid.cols)))
    d64 = d.double()
    c = (torch.arange(grid.cols, dtype=torch.float64, device=d.device) + 0.5) / grid.cols
    r = (torch.arange(grid.rows, dtype=torch.float64, device=d.device) + 0.5) / grid.rows
    yaw = ((2.0 * c - 1.0) * math.pi)[None, :]                                    # -atan2(y, x)
    pitch = ((1.0 - r) * grid.fov - abs(grid.fov_down / 180.0 * math.pi))[:, None]
    pts = torch.stack([d64 * torch.cos(pitch) * torch.cos(yaw), -d64 * torch.cos(pitch) * torch.sin(yaw),
                       d64 * torch.sin(pitch).expand_as(d64)], dim=-1).reshape(-1, 3)
    pts = pts[d64.reshape(-1) > 0.0].to(d.dtype if d.dtype.is_floating_point else torch.float64)
    return pts.cpu().numpy() if as_numpy else pts


# ---- neighbourhoods ----------------------------------------------------------------------------------------------------------------
def image_features(cloud, window, r=None, count=None):
    """Fill the neighbourhood features of an organised cloud (mean, cov, eigvals, eigvecs, normals, inc_angles) and
    ``cloud.neighbors`` (the membership table, int32 [M, (2 ah + 1)(2 aw + 1)], -1 padded in place) from the image window of half
    extents ``window`` with the 3-D radius gate ``r``, in one launch (dc_image_features_fwd).  No gradient."""
    if not is_organized(cloud):
        raise ValueError('not an organised cloud: use range_image.organize')
    window = check_window(cloud.grid, window)
    with torch.no_grad():
        x = cloud.get_points().detach().contiguous()
        dirs = cloud.dirs.detach().to(x.dtype).contiguous()
        f = ops.image_features_fwd(x, dirs, cloud.pixel, index_image(cloud), cloud.grid, window, r=r, count=count)
    cloud.mean, cloud.cov, cloud.eigvals, cloud.eigvecs = f['mean'], f['cov'], f['eigvals'], f['eigvecs']
    cloud.normals, cloud.inc_angles = f['normals'], f['inc_angles']
    cloud.neighbors, cloud.weights = f['neighbors'], None
    cloud._distances, cloud.neighbor_points, cloud._feat = None, None, None
    cloud.nvalid = f['nvalid']
    return cloud


def image_shadow_mask(cloud, angle, bounds, window=None, count=None):
    """bool [M]: the scan-shadow mask of ``filters.shadow_points_mask`` (direction neighbourhoods of ``angle`` radians, angle
    bounds ``bounds``) with the candidates taken from the image window (dc_image_shadow_mask).  ``window`` defaults to
    ``shadow_window(cloud.grid, angle)``, which holds every direction neighbour of a scan that fills its grid."""
    from .filters import _shadow_bounds
    from .nearest_neighbors import ball_angle_to_distance
    if not is_organized(cloud):
        raise ValueError('not an organised cloud: use range_image.organize')
    window = shadow_window(cloud.grid, angle) if window is None else check_window(cloud.grid, window)
    lo, hi, _ = _shadow_bounds(bounds)
    r = float(ball_angle_to_distance(torch.as_tensor(angle)))
    with torch.no_grad():
        x = cloud.get_points().detach().contiguous()
        return ops.image_shadow_mask(x, cloud.vps.detach().to(x.dtype).contiguous(), cloud.dirs.detach().to(x.dtype).contiguous(),
                                     cloud.pixel, index_image(cloud), cloud.grid, window, r, lo, hi, count=count)
