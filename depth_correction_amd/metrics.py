"""Map-accuracy metrics.

``chamfer_distance``: the reference's metric (metrics.py:55-125, used by scripts/model_poses_learning:142-146), the
one-directional chamfer distance = mean distance from every point of ``x`` to its nearest neighbour in ``y``.
The nearest-neighbour search is the GPU grid search (dc_knn_build with k = 1, fp64 distances, bit-exact ordering)
instead of pytorch3d's ``knn_points``; batches are lists / a leading dimension of clouds.

``point_to_mesh_distance`` / ``map_accuracy``: a map against the ground-truth MESH (what scripts/mapping_accuracy:82-118 does
against a surveyed cloud): the exact distance from every map point to the nearest triangle (dc_mesh_closest) and its
statistics; DESIGN "Map accuracy".

``depth_bias`` / ``fit_bias``: the direct measurement behind the reference's scripts/bias_estimation and depth_bias.py: the rays of
measured clouds are cast against the ground-truth mesh (dc_raycast_rays), the depth error is binned over the TRUE incidence angle,
the estimated angles are compared with the true ones, and the weights a supervised fit to ground truth would have found come from
the normal equations dc_bias_accumulate sums; DESIGN "Depth bias against the mesh"."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

__all__ = ['bias_statistics', 'chamfer_distance', 'depth_bias', 'fit_bias', 'fitted_model', 'map_accuracy', 'map_statistics',
           'point_to_cloud_distance', 'point_to_mesh_distance', 'reconstruction_accuracy']

BIAS_TOTALS, BIAS_BIN_COLS = 5, 9                    # include/dc_hip.h: DC_BIAS_TOTALS, DC_BIAS_BIN_COLS
BIAS_TOTAL_NAMES = ('rays', 'masked', 'hits', 'used', 'beyond_gate')
BIAS_BIN_FIELDS = ('count', 'mean', 'rms', 'mean_abs', 'rel_mean', 'rel_rms', 'angle_err_mean', 'angle_err_rms')
BIAS_OVERALL_FIELDS = ('mean_abs', 'rms', 'rel_rms', 'angle_err_rms')


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


def point_to_cloud_distance(points, survey, max_dist=None, return_closest=False):
    """Distance from every point (tensor [N,3] on a GPU, or a DepthCloud's points) to the nearest point of ``survey``
    (survey.SurveyCloud) -> [N] in the dtype of the points (computed in fp64) through the survey's cached grid (built once; what
    chamfer_distance rebuilds at every call); with ``return_closest`` also the survey indices i32 [N] and the nearest points f64
    [N,3].  ``max_dist``: farther points get inf (index -1, nearest point NaN), as does a row holding a NaN or an infinity."""
    pts = _map_points(points)
    sd = survey.on_device(pts.device).reserve(pts.shape[0])
    n = pts.shape[0]
    if n == 0:
        dist, idx = pts.new_zeros((0,), dtype=torch.float64), torch.zeros((0,), dtype=torch.int32, device=pts.device)
    else:
        dist, idx = ops.knn_grid_query(sd.grid, pts.to(torch.float64).contiguous(), sd.identity_pose(), 1, r=max_dist)
        dist, idx = dist[:, 0], idx[:, 0]
        dist = torch.where(idx >= 0, dist, torch.full_like(dist, float('inf')))
    if not return_closest:
        return dist.to(pts.dtype)
    closest = sd.points[idx.clamp(min=0).long()]
    closest = torch.where((idx >= 0)[:, None], closest, torch.full_like(closest, float('nan')))
    return dist.to(pts.dtype), idx, closest


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
    """Accuracy of a map (points [N,3] on a GPU or a DepthCloud, world frame) against the ground-truth ``mesh`` (or a
    survey.SurveyCloud: nearest-point distances, signed_mean NaN, no completeness_mean): dict of floats
    n, mean, rms, median, max, trimmed_mean (what point_to_point_dist with icp_inlier_ratio = 0.8 reports in
    scripts/mapping_accuracy:112-115) and signed_mean, the mean of n_face . (p - closest): which side of the surface the map
    sits on (at edges and vertices the sign is that of the winning face).  With ``n_samples`` also completeness_mean: the
    chamfer distance from mesh.sample(n_samples, seed) to the map -- surface the map does not cover."""
    pts = _map_points(points)
    if hasattr(mesh, 'normals') and not hasattr(mesh, 'faces'):
        # a survey.SurveyCloud in place of the mesh (scripts/mapping_accuracy:82-118 as it stands): the same statistics of the
        # nearest-point distances; no surface, hence no side (signed_mean NaN) and no completeness
        dist = point_to_cloud_distance(pts, mesh)
        return map_statistics(dist, None, inlier_ratio, quantile=lambda v, r: ops.quantile(v.contiguous(), r))
    dist, face, closest = point_to_mesh_distance(pts, mesh, return_closest=True)
    normals = mesh.on_device(pts.device)[2]
    signed = ((pts.to(torch.float64) - closest) * normals[face.clamp(min=0).long()]).sum(dim=1)
    out = map_statistics(dist, signed, inlier_ratio, quantile=lambda v, r: ops.quantile(v.contiguous(), r))
    if n_samples:
        surface = mesh.sample(int(n_samples), seed=seed, device=pts.device)[0]
        finite = pts[torch.isfinite(dist)].to(torch.float64).contiguous()
        out['completeness_mean'] = float(chamfer_distance(surface, finite)) if finite.shape[0] else float('nan')
    return out


# ---- depth bias against the mesh -------------------------------------------------------------------------------------------------
def reconstruction_accuracy(mesh, gt_mesh, n_samples=100000, seed=135, inlier_ratio=0.8, max_dist=None):
    """Quality of a reconstructed ``mesh`` against the ground-truth ``gt_mesh`` (both mesh.TriangleMesh; what the reference's
    scripts/reconstruction_eval is named after): dict(accuracy=map_statistics of the distances from mesh.sample(n_samples, seed) to
    gt_mesh -- how far the reconstruction is from the truth --, completeness=map_statistics of the distances from
    gt_mesh.sample(n_samples, seed) to mesh -- how far the truth is from the reconstruction --, coverage=the share of the
    ground-truth samples within ``max_dist`` of the reconstruction (None: NaN)).  Every distance is point_to_mesh_distance's, without
    a cut-off, so that a far sample weighs on the mean instead of leaving it."""
    quantile = lambda v, r: ops.quantile(v.contiguous(), r)
    ours = mesh.sample(int(n_samples), seed=seed)[0]                 # (on the current GPU; without one: "no CPU path")
    truth = gt_mesh.sample(int(n_samples), seed=seed)[0]
    to_truth = point_to_mesh_distance(ours, gt_mesh)
    to_ours = point_to_mesh_distance(truth, mesh)
    out = dict(accuracy=map_statistics(to_truth, None, inlier_ratio, quantile=quantile),
               completeness=map_statistics(to_ours, None, inlier_ratio, quantile=quantile))
    out['coverage'] = float((to_ours <= float(max_dist)).to(torch.float64).mean()) if max_dist is not None else float('nan')
    return out


def _bias_system_len(p):
    return 2 + p + p * (p + 1) // 2


def _bias_shape(count, n_terms=None):
    """(n_bins, n_terms) of an ``out`` of dc_bias_accumulate with ``count`` entries."""
    for p in ([int(n_terms)] if n_terms else range(1, 5)):
        rest = count - BIAS_TOTALS - 2 * _bias_system_len(p)
        if rest > 0 and rest % BIAS_BIN_COLS == 0:
            return rest // BIAS_BIN_COLS, p
    raise ValueError('%d values are not an out of dc_bias_accumulate%s' % (count, ' with %d terms' % n_terms if n_terms else ''))


def bias_statistics(out, n_bins):
    """The finishing arithmetic of depth_bias on the sums of dc_bias_accumulate (``out`` f64 tensor, any device; layout in
    include/dc_hip.h): dict of ``totals`` (rays, masked, hits, used, beyond_gate: floats), the per-bin f64 tensors count, mean, rms,
    mean_abs (of r = d - t, metres), rel_mean, rel_rms (of r / d), angle_err_mean, angle_err_rms (of the estimated minus the true
    incidence angle, over the rays that have an estimate) -- NaN in an empty bin -- and the same over all used rays as floats
    (mean, rms, mean_abs, rel_mean, rel_rms, angle_err_mean, angle_err_rms).  rms is sqrt(sum x^2 / count): about zero, not about
    the mean."""
    out = out.detach().reshape(-1).to(torch.float64)
    b = int(n_bins)
    if out.numel() < BIAS_TOTALS + BIAS_BIN_COLS * b:
        raise ValueError('out holds %d values, %d bins need at least %d' % (out.numel(), b, BIAS_TOTALS + BIAS_BIN_COLS * b))
    rows = out[BIAS_TOTALS:BIAS_TOTALS + BIAS_BIN_COLS * b].reshape(b, BIAS_BIN_COLS)

    def finish(r):
        nan = torch.full_like(r[..., 0], float('nan'))
        n, na = r[..., 0], r[..., 8]
        div = lambda num, den: torch.where(den > 0, num / den.clamp(min=1.0), nan)
        return dict(count=n, mean=div(r[..., 1], n), rms=div(r[..., 2], n).sqrt(), mean_abs=div(r[..., 3], n), rel_mean=div(r[..., 4], n),
                    rel_rms=div(r[..., 5], n).sqrt(), angle_err_mean=div(r[..., 6], na), angle_err_rms=div(r[..., 7], na).sqrt())

    res = finish(rows)
    res['totals'] = {k: float(v) for k, v in zip(BIAS_TOTAL_NAMES, out[:BIAS_TOTALS].tolist())}
    # the overall figures: the bins added in bin order (one fixed order)
    res['overall'] = {k: float(v) for k, v in finish(rows.sum(dim=0)).items()}
    return res


def _cat_field(clouds, name, n_cols):
    parts = [getattr(c, name) for c in clouds]
    if any(p is None for p in parts):
        return None
    parts = [p.detach().reshape(-1, n_cols) if n_cols else p.detach().reshape(-1) for p in parts]
    return torch.cat(parts).contiguous()


def _fit_basis(model, fit_class, fit_exponent):
    kind = getattr(model, 'kernel_kind', None)
    if fit_class is None:
        fit_class = kind if kind in ('Polynomial', 'ScaledPolynomial') else 'ScaledPolynomial'
    fit_class = fit_class if isinstance(fit_class, str) else fit_class.__name__
    if fit_exponent is None:
        fit_exponent = model.exponent.detach().reshape(-1).tolist() if kind in ('Polynomial', 'ScaledPolynomial') else [2.0, 4.0]
    return fit_class, [float(e) for e in fit_exponent]


def _is_tsdf_truth(truth):
    from .loss import TsdfTarget
    from .reconstruction import SparseTsdfVolume
    return isinstance(truth, (SparseTsdfVolume, TsdfTarget))


def _tsdf_truth_cast(truth, clouds, vps, dirs, offsets, T, step, max_range):
    """cast(model) -> the outputs of ops.tsdf_sparse_cast_rays for the rays of depth_bias against ``truth``: a SparseTsdfVolume as it
    is, or a loss.TsdfTarget -- as fused (fused here from ``clouds`` at the poses ``T`` when it has not been), every scan against the
    volume of the others when it leaves one out; cast(model) with a model casts against a copy of the target re-fused from model(cloud)."""
    from .loss import TsdfTarget
    dev = dirs.device
    off = torch.as_tensor(offsets, dtype=torch.int64, device=dev)

    def fused(model):
        if not isinstance(truth, TsdfTarget):
            return truth.tables(), None, 1
        target = truth
        if model is not None:
            target = TsdfTarget(truth.voxel_size, trunc=truth.trunc, leave_one_out=truth.leave_one_out, refresh_every=0,
                                min_count=truth.min_count, max_blocks=truth.max_blocks, min_depth=truth.min_depth, max_range=truth.max_range)
        if model is not None or target.total is None:
            target.refresh(clouds, T.cpu(), model)
        return target.tables, target.own, target.min_count

    t_max = max_range
    if t_max is None:                            # a ray is marched as far as the sequence measured, and through the band behind that
        depth = torch.cat([c.depth.detach().reshape(-1) for c in clouds]).to(torch.float64)
        depth = depth[torch.isfinite(depth)]
        trunc = truth.trunc
        t_max = (float(depth.max()) if depth.numel() else 0.0) + trunc

    def cast(model):
        tables, own, min_count = fused(model)
        return ops.tsdf_sparse_cast_rays(tables, vps, dirs, off, T, t_min=0.0, t_max=max(float(t_max), tables.voxel), step=step,
                                         min_count=min_count, own=own)
    return cast


def depth_bias(clouds, poses, truth, model=None, bins=18, max_residual=None, cull=True, fit_class=None, fit_exponent=None,
               surfel_radius=None, surfel_k=10, surfel_scale=1.0, surfel_window=0.1, surfel_max_normal_angle=math.pi / 4, tsdf_step=None,
               tsdf_max_range=None):
    """Depth error of every ray of the DepthClouds ``clouds`` (one sequence, on a GPU, sensor frame) against ``truth``
    (mesh.TriangleMesh or survey.SurveyCloud, the frame of ``poses`` [S,4,4]: world from sensor; only ground-truth poses give a
    meaningful answer), as a
    function of the TRUE incidence angle.  The rays (vps, dirs) are cast once (ops.raycast_rays: true depth t and true angle per
    ray); the clouds' ``mask`` and ``inc_angles`` are used when present.  Statistics (bias_statistics) are taken of the depths as
    given -> ``before`` and, with a ``model``, of the depths of ``model(cloud)`` -> ``after`` (else None), in ``bins`` equal bins of
    [0, pi/2] (``bin_edges`` f64 [bins+1]); rays with |d - t| > ``max_residual`` (the ray hit something the mesh does not hold, or
    missed what it holds) are counted and left out.  ``before['out']`` / ``after['out']`` keep the raw sums with the normal equations
    of fit_bias for ``fit_class`` / ``fit_exponent`` (default: the model's class and exponents when it is a polynomial, else
    ScaledPolynomial with [2, 4]).  ``face`` / ``t`` / ``inc`` are the cast's per-ray outputs, ``inc_est`` / ``mask`` and
    ``before['depth']`` / ``after['depth']`` the per-ray inputs of the sums, all scan-major in the order of ``clouds``.

    Against a SurveyCloud the rays are cast on its surfels (SurveyCloud.surfels(radius=``surfel_radius``, k=``surfel_k``,
    scale=``surfel_scale``); ops.surfel_cast_rays): ``t`` / ``inc`` are the blend of the disks within ``surfel_window`` metres
    behind the first one whose normals lie within ``surfel_max_normal_angle`` of its normal -- the first disk alone is biased
    towards the sensor by the survey's noise, growing with the incidence angle (DESIGN "Depth bias against a surveyed cloud") --,
    ``face`` holds the survey index of the first disk, and the result gains ``t_first`` (its depth) and ``count`` (disks blended per
    ray).  Disks are two-sided: ``cull`` is ignored.

    Without any ground truth, ``truth`` may be a fused volume (DESIGN "Ray casting the fused volume"): a
    reconstruction.SparseTsdfVolume, cast as it is (ops.tsdf_sparse_cast_rays in steps of ``tsdf_step``, None: half a voxel, up to
    ``tsdf_max_range``, None: the farthest finite depth plus the truncation), or a loss.TsdfTarget, fused here from ``clouds`` at
    ``poses`` when it has not been; with its leave_one_out every scan is cast against the volume of the OTHER scans.  ``inc`` is then
    the angle to the field's gradient at the hit, and the result gains ``status`` (ops.TSDF_CAST_* per ray).  Against a TsdfTarget
    the truth is made of the measurements, so ``after`` is taken against a copy of the target re-fused from model(cloud) and the rays
    are cast a second time: the result gains ``face_after`` / ``t_after`` / ``inc_after`` / ``status_after``.  The residual against the
    own sequence's volume is a ray's bias MINUS the mean bias of the other views of that surface: fit_bias' weights come out
    attenuated (by how much: DESIGN)."""
    clouds = list(clouds)
    if not clouds:
        raise ValueError('depth_bias needs at least one cloud')
    dev = clouds[0].depth.device
    if dev.type != 'cuda':
        raise RuntimeError('depth_bias needs clouds on a GPU (depth_correction_amd has no CPU path)')
    fit_class, fit_exponent = _fit_basis(model, fit_class, fit_exponent)
    dirs = _cat_field(clouds, 'dirs', 3)
    vps = torch.cat([c.vps.detach().reshape(-1, 3).expand(len(c), 3) for c in clouds]).to(dirs.dtype).contiguous()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    T = torch.as_tensor(np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64).reshape(-1, 4, 4),
                        device=dev).contiguous()
    if T.shape[0] != len(clouds):
        raise ValueError('%d clouds but %d poses' % (len(clouds), T.shape[0]))
    extra = {}
    recast = None                                # against a fused TsdfTarget: the cast of ``after``, against the re-fused target
    if _is_tsdf_truth(truth):
        cast = _tsdf_truth_cast(truth, clouds, vps, dirs, offsets, T, tsdf_step, tsdf_max_range)
        hit = cast(None)
        face, t, inc = hit['face'], hit['t'], hit['inc']
        extra = dict(status=hit['status'])
        if model is not None and hasattr(truth, 'refresh'):
            recast = cast
    elif hasattr(truth, 'surfels'):
        angle = float(surfel_max_normal_angle)
        if not 0.0 < angle <= math.pi / 2:
            raise ValueError('surfel_max_normal_angle must lie in (0, pi/2], got %r' % (surfel_max_normal_angle,))
        bvh = truth.surfels(dev, radius=surfel_radius, k=surfel_k, scale=surfel_scale)
        face, t_first, t, inc, count = ops.surfel_cast_rays(bvh, vps, dirs, offsets, T, t_min=0.0, window=surfel_window,
                                                            min_cos=max(math.cos(angle), 0.0))
        extra = dict(t_first=t_first, count=count)
    else:
        bvh = truth.on_device(dev)[3]
        face, t, inc = ops.raycast_rays(bvh, vps, dirs, offsets, T, t_min=0.0, cull=cull)
    inc_est = _cat_field(clouds, 'inc_angles', 0)
    mask = None
    if any(c.mask is not None for c in clouds):
        mask = torch.cat([c.mask.detach().reshape(-1).bool() if c.mask is not None else torch.ones((len(c),), dtype=torch.bool, device=dev)
                          for c in clouds]).contiguous()
    n_terms = len(fit_exponent)
    ws = ops.bias_workspace(bins, n_terms, dev)

    def stats(cs, face=face, t=t, inc=inc):
        depth = _cat_field(cs, 'depth', 0)
        est = None if inc_est is None else inc_est.to(depth.dtype)
        out = ops.bias_accumulate(depth, est, mask, face, t, inc, fit_class, fit_exponent, n_bins=bins, max_residual=max_residual, ws=ws)
        res = bias_statistics(out, bins)
        res['out'], res['depth'] = out, depth
        return res

    res = dict(bins=int(bins), bin_edges=torch.linspace(0.0, math.pi / 2, int(bins) + 1, dtype=torch.float64), fit_class=fit_class,
               fit_exponent=fit_exponent, face=face, t=t, inc=inc, inc_est=inc_est, mask=mask, before=stats(clouds), after=None)
    res.update(extra)
    if model is not None:
        with torch.no_grad():
            if recast is None:
                res['after'] = stats([model(c) for c in clouds])
            else:
                # the truth is made of the measurements: the corrected depths are held against the volume the corrected scans fuse into
                hit = recast(model)
                res['after'] = stats([model(c) for c in clouds], hit['face'], hit['t'], hit['inc'])
                res.update(face_after=hit['face'], t_after=hit['t'], inc_after=hit['inc'], status_after=hit['status'])
    return res


def _solve_normal(sys_, p):
    """(w [p], residual rms, cond(A), n, message or None) of one system of dc_bias_accumulate: count, upper triangle, b, sum y^2."""
    n = float(sys_[0])
    A = np.zeros((p, p))
    iu = np.triu_indices(p)
    A[iu] = sys_[1:1 + len(iu[0])]
    A = A + np.triu(A, 1).T
    b = sys_[1 + len(iu[0]):1 + len(iu[0]) + p]
    yy = float(sys_[1 + len(iu[0]) + p])
    nan_w = np.full(p, np.nan)
    if n < p:
        return nan_w, float('nan'), float('nan'), n, '%d rays for %d weights' % (n, p)
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return nan_w, float('nan'), float('nan'), n, 'the sums are not finite'
    # scale to a unit diagonal before judging the rank: the columns gamma^e differ by orders of magnitude by construction
    dg = np.sqrt(np.diag(A))
    if not (dg > 0).all():
        return nan_w, float('nan'), float('inf'), n, 'a basis column is zero on every ray'
    As = A / np.outer(dg, dg)
    cond = float(np.linalg.cond(As))
    if not np.isfinite(cond) or cond > 1e13:
        return nan_w, float('nan'), cond, n, 'the system is singular (condition number %.3g after diagonal scaling)' % cond
    w = np.linalg.solve(As, b / dg) / dg
    sse = yy - 2.0 * float(w @ b) + float(w @ A @ w)
    return w, math.sqrt(max(sse, 0.0) / n), cond, n, None


def fit_bias(stats_or_out, model_class, exponent):
    """The supervised fit to ground truth: the weights of ``model_class`` ('Polynomial': d - t = sum_k w_k gamma^e_k, or
    'ScaledPolynomial': (d - t) / d = sum_k w_k gamma^e_k; a name or a class of model.py) with the exponents ``exponent`` that
    minimise the squared residual over the used rays, once with the basis at the TRUE incidence angles (``w_true_angles``: the
    upper bound self-supervised training is compared with) and once at the ESTIMATED ones (``w_est_angles``).  ``stats_or_out``: a
    result of depth_bias (its ``before`` sums), one of its ``before`` / ``after`` dicts, or the raw ``out`` of ops.bias_accumulate
    taken for this class and these exponents.  Both models are linear in w: the P x P normal equations are solved in fp64 on the
    host.  Returns numpy weights, ``rms_true_angles`` / ``rms_est_angles`` (the residual rms, from the sums sum y^2 - 2 w.b + w.A w: an exact
    fit leaves the rounding of those sums, up to sqrt(3 n 2^-53) of the target's rms), ``cond_true_angles`` / ``cond_est_angles`` (condition number of A scaled to a unit diagonal),
    ``n_true_angles`` / ``n_est_angles`` and ``message``: a singular system (too few rays, every angle zero, ...) gives NaN weights
    and says why; it does not raise."""
    name = model_class if isinstance(model_class, str) else model_class.__name__
    if name not in ('Polynomial', 'ScaledPolynomial'):
        raise ValueError("fit_bias fits 'Polynomial' or 'ScaledPolynomial', got %r" % (name,))
    e = [float(x) for x in (exponent.detach().reshape(-1).tolist() if isinstance(exponent, torch.Tensor) else np.asarray(exponent).reshape(-1))]
    p = len(e)
    src = stats_or_out
    if isinstance(src, dict):
        if 'fit_class' in src and (src['fit_class'] != name or list(src['fit_exponent']) != e):
            raise ValueError('these statistics hold the systems of %s %s, not of %s %s'
                             % (src['fit_class'], src['fit_exponent'], name, e))
        src = src['before'] if 'before' in src else src
        src = src['out']
    out = (src.detach().cpu().numpy() if isinstance(src, torch.Tensor) else np.asarray(src)).astype(np.float64).reshape(-1)
    n_bins, _ = _bias_shape(out.size, p)
    base, ln = BIAS_TOTALS + BIAS_BIN_COLS * n_bins, _bias_system_len(p)
    res, messages = dict(model_class=name, exponent=e), []
    for s, key in enumerate(('true_angles', 'est_angles')):
        w, rms, cond, n, msg = _solve_normal(out[base + s * ln:base + (s + 1) * ln], p)
        res['w_' + key], res['rms_' + key], res['cond_' + key], res['n_' + key] = w, rms, cond, n
        if msg:
            messages.append('%s: %s' % (key, msg))
    res['message'] = '; '.join(messages) if messages else None
    return res


def fitted_model(fit, which='true_angles', device=None):
    """A model of the fitted class carrying the weights of a fit_bias result (``which``: 'true_angles' or 'est_angles')."""
    from .model import model_by_name
    if which not in ('true_angles', 'est_angles'):
        raise ValueError("which must be 'true_angles' or 'est_angles', got %r" % (which,))
    kw = {} if device is None else {'device': torch.device(device)}
    return model_by_name(fit['model_class'])(w=[float(x) for x in fit['w_' + which]], exponent=list(fit['exponent']), **kw)
