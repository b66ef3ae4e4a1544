"""Map-accuracy metrics.

``chamfer_distance``: the reference's metric (metrics.py:55-125, used by scripts/model_poses_learning:142-146), the
one-directional chamfer distance = mean distance from every point of ``x`` to its nearest neighbour in ``y``.
The nearest-neighbour search is the GPU grid search (dc_knn_build with k = 1, fp64 distances, bit-exact ordering)
instead of pytorch3d's ``knn_points``; batches are lists / a leading dimension of clouds.

``point_to_mesh_distance`` / ``map_accuracy``: a map against the ground-truth MESH (what scripts/mapping_accuracy:82-118 does
against a surveyed cloud): the exact distance from every map point to the nearest triangle (dc_mesh_closest) and its
statistics; DESIGN "Map accuracy"."""
from __future__ import annotations

import torch

from . import ops

__all__ = ['chamfer_distance', 'map_accuracy', 'map_statistics', 'point_to_mesh_distance']


def _as_batch(x):
    if isinstance(x, (list, tuple)):
        return list(x)
    assert isinstance(x, torch.Tensor)
    return [x] if x.dim() == 2 else list(x)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, apply_point_reduction=True, batch_reduction='mean',
                     point_reduction='mean'):
    """Distances from the points of ``x`` to the cloud ``y`` ([P,3] / [N,P,3] tensors or lists of [P_i,3])."""
    xs, ys = _as_batch(x), _as_batch(y)
    if len(xs) != len(ys):
        raise ValueError('y does not have the correct shape.')
    per_cloud = []
    for b, (a, c) in enumerate(zip(xs, ys)):
        if x_lengths is not None:
            a = a[:int(x_lengths[b])]
        if y_lengths is not None:
            c = c[:int(y_lengths[b])]
        dist, _ = ops.knn(c.detach().contiguous(), 1, query=a.detach().to(c.dtype).contiguous())
        per_cloud.append(dist[:, 0].to(a.dtype))
    if not apply_point_reduction:
        return per_cloud[0] if isinstance(x, torch.Tensor) and x.dim() == 2 else per_cloud
    red = torch.stack([d.sum() / (len(d) if point_reduction == 'mean' else 1) for d in per_cloud])
    if batch_reduction is None:
        return red
    return red.sum() / (len(red) if batch_reduction == 'mean' else 1)


def _map_points(points):
    from .depth_cloud import DepthCloud
    if isinstance(points, DepthCloud):
        points = points.get_points()
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError('points must be a DepthCloud or an [N,3] tensor')
    if not points.is_cuda:
        raise RuntimeError('point_to_mesh_distance needs points on a GPU (depth_correction_amd has no CPU path)')
    return points.detach().contiguous()


def point_to_mesh_distance(points, mesh, max_dist=None, return_closest=False):
    """Distance from every point (tensor [N,3] on a GPU, or a DepthCloud's points) to the nearest triangle of ``mesh``
    (mesh.TriangleMesh) -> [N] in the dtype of the points (computed in fp64); with ``return_closest`` also the faces i32 [N]
    and the closest points f64 [N,3].  ``max_dist``: farther points get inf (face -1, closest NaN)."""
    pts = _map_points(points)
    bvh = mesh.on_device(pts.device)[3]
    face, dist, closest = ops.mesh_closest(bvh, pts, max_dist=max_dist, want_closest=return_closest)
    dist = dist.to(pts.dtype)
    return (dist, face, closest) if return_closest else dist


def _np_quantile(v, ratio):
    return torch.quantile(v, ratio) if v.numel() else v.new_tensor(float('nan'))


def map_statistics(dist, signed=None, inlier_ratio=0.8, quantile=None):
    """The statistics map_accuracy reports, of a vector of point-to-surface distances (tensor [N], any device; non-finite
    entries are dropped) and, optionally, their signed counterparts: dict of floats n, mean, rms, median, trimmed_mean (the
    mean of the distances <= their ``inlier_ratio`` quantile), signed_mean and max.  ``quantile(v, ratio)`` must follow numpy's rule
    (linear interpolation); the default is torch.quantile, map_accuracy passes ops.quantile."""
    quantile = quantile or _np_quantile
    dist = dist.reshape(-1).to(torch.float64)
    keep = torch.isfinite(dist)
    d = dist[keep]
    n = d.numel()
    nan = float('nan')
    if n == 0:
        return dict(n=0.0, mean=nan, rms=nan, median=nan, trimmed_mean=nan, signed_mean=nan, max=nan)
    thr = quantile(d, float(inlier_ratio)).reshape(())
    out = dict(n=float(n), mean=float(d.mean()), rms=float(d.square().mean().sqrt()), median=float(quantile(d, 0.5).reshape(())),
               trimmed_mean=float(d[d <= thr].mean()))
    out['signed_mean'] = float(signed.reshape(-1).to(torch.float64)[keep].mean()) if signed is not None else nan
    out['max'] = float(d.max())
    return out


def map_accuracy(points, mesh, inlier_ratio=0.8, n_samples=None, seed=135):
    """Accuracy of a map (points [N,3] on a GPU or a DepthCloud, world frame) against the ground-truth ``mesh``: dict of floats
    n, mean, rms, median, max, trimmed_mean (what point_to_point_dist with icp_inlier_ratio = 0.8 reports in
    scripts/mapping_accuracy:112-115) and signed_mean, the mean of n_face . (p - closest): which side of the surface the map
    sits on (at edges and vertices the sign is that of the winning face).  With ``n_samples`` also completeness_mean: the
    chamfer distance from mesh.sample(n_samples, seed) to the map -- surface the map does not cover."""
    pts = _map_points(points)
    dist, face, closest = point_to_mesh_distance(pts, mesh, return_closest=True)
    normals = mesh.on_device(pts.device)[2]
    signed = ((pts.to(torch.float64) - closest) * normals[face.clamp(min=0).long()]).sum(dim=1)
    out = map_statistics(dist, signed, inlier_ratio, quantile=lambda v, r: ops.quantile(v.contiguous(), r))
    if n_samples:
        surface = mesh.sample(int(n_samples), seed=seed, device=pts.device)[0]
        finite = pts[torch.isfinite(dist)].to(torch.float64).contiguous()
        out['completeness_mean'] = float(chamfer_distance(surface, finite)) if finite.shape[0] else float('nan')
    return out
