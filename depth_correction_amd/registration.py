"""Registration: putting a cloud, or a path, into the frame of a survey (DESIGN "Survey registration").

``cloud_loss``, ``metrics.point_to_cloud_distance`` and ``eval_map`` against a ``survey.SurveyCloud`` assume that the survey and the
scans' poses share one frame.  This module gets them there:

``absolute_orientation``  the closed-form rigid fit of paired points (utils.py:253-304 of the reference), on the host;
``align_paths``           the same for two paths, with the residual statistics scripts/paths_alignment prints;
``register_cloud``        trimmed ICP of a cloud against a survey, what scripts/map_bias_removal:167-185 icp_alignment does on the
                          host with a cKDTree -- here one queue of device work (ops.survey_align) and ONE host read, at the end;
``register_global``       the coarse stage for a cloud that is an ARBITRARY rigid motion away from the survey (DESIGN "Global
                          registration"): folded pair-feature histograms, descriptor matching and RANSAC over the matches on
                          the device, then ``register_cloud`` from the winner.
``register_planes``       the coarse stage for maps of rooms and corridors (DESIGN "Plane registration"): planes on both sides, every
                          pairing of a triple of cloud planes with a triple of survey planes fitted in closed form on the device,
                          ranked by plane agreement and then by point fitness.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import _native as nv

__all__ = ['absolute_orientation', 'align_paths', 'register_cloud', 'Registration', 'register_global', 'GlobalRegistration',
           'register_planes']


def absolute_orientation(x, y, fix_reflection=False):
    """T = [R t; 0 1] from SE(D), (D+1) x (D+1), that minimises sum |R x[:, i] + t - y[:, i]|^2 for the D x M arrays ``x`` (the points to
    align) and ``y`` (the points to align to).  Where the least-squares orthogonal matrix is a reflection (mirrored or degenerate
    data) a ``ValueError`` is raised, as the reference does for D = 3; with ``fix_reflection`` the best PROPER rotation is returned
    instead (the smallest singular direction flipped, Kabsch / Umeyama)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError('x and y must be D x M arrays of one shape, got %s and %s' % (x.shape, y.shape))
    d, m = x.shape
    if m < 1:
        raise ValueError('absolute_orientation needs at least one pair')
    xm, ym = x.mean(axis=1, keepdims=True), y.mean(axis=1, keepdims=True)
    U, _, Vt = np.linalg.svd((y - ym) @ (x - xm).T)
    R = U @ Vt
    if np.linalg.det(R) < 0.0:
        if not fix_reflection:
            raise ValueError('the least-squares orthogonal fit is a reflection (det R = -1): no rotation R, det R = 1, fits these '
                             'pairs best without flipping an axis; pass fix_reflection=True for the best proper rotation')
        flip = np.ones(d)
        flip[-1] = -1.0
        R = (U * flip) @ Vt
    T = np.eye(d + 1)
    T[:d, :d] = R
    T[:d, d:] = ym - R @ xm
    return T


def _positions(a, name):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if a.ndim == 3 and a.shape[1:] == (4, 4):
        return a[:, :3, 3]
    if a.ndim == 2 and a.shape[1] == 3:
        return a
    raise ValueError('%s must be poses [N,4,4] or positions [N,3], got shape %s' % (name, a.shape))


def align_paths(src, dst, fix_reflection=False):
    """Rigid alignment of the path ``src`` to the path ``dst`` (poses [N,4,4] or positions [N,3], paired row by row):
    dict(T [4,4] with T src ~ dst, errors [N] = |T src_i - dst_i|, mean, rmse)."""
    a, b = _positions(src, 'src'), _positions(dst, 'dst')
    if a.shape != b.shape:
        raise ValueError('the paths have %d and %d positions' % (len(a), len(b)))
    T = absolute_orientation(a.T, b.T, fix_reflection=fix_reflection)
    err = np.linalg.norm(a @ T[:3, :3].T + T[:3, 3] - b, axis=1)
    return dict(T=T, errors=err, mean=float(err.mean()), rmse=float(np.sqrt(np.mean(err ** 2))))


class Registration(object):
    """Result of ``register_cloud``: ``T`` (numpy [4,4], survey frame from the cloud's frame), ``status`` ('converged',
    'max_iterations', 'too_few_pairs', 'degenerate', 'not_finite' or 'empty'), ``ok``, ``iterations``, and of the last iteration
    ``pairs`` (kept pairs), ``rms`` (rms distance of the kept pairs before its fit) and ``threshold`` (the trimming distance);
    ``history`` [n_iters, 5] = (pairs, rms, threshold, d_rot, d_trans) per iteration, NaN in the rows never reached.  ``coarse``: the
    GlobalRegistration the prior came from (``init='global'``), else None."""

    coarse = None

    def __init__(self, T, status, iterations, pairs, rms, threshold, history):
        self.T, self.status, self.iterations = T, status, int(iterations)
        self.pairs, self.rms, self.threshold, self.history = pairs, rms, threshold, history

    @property
    def ok(self):
        return self.status in ('converged', 'max_iterations')

    def __repr__(self):
        return 'Registration(%s after %d iterations, %d pairs, rms %.6g)' % (self.status, self.iterations, self.pairs, self.rms)

    def as_dict(self):
        return dict(T=self.T.tolist(), status=self.status, ok=self.ok, iterations=self.iterations, pairs=self.pairs, rms=self.rms,
                    threshold=self.threshold)


def register_cloud(points, survey, init=None, inlier_ratio=1.0, max_dist=None, n_iters=100, min_rot=0.0, min_trans=0.0, min_pairs=3,
                   mask=None, device=None, global_kwargs=None):
    """Trimmed ICP of ``points`` [N,3] (tensor or array, frame A) against ``survey`` (survey.SurveyCloud): the T with T points ~ survey.
    Every iteration matches T_k p to its nearest survey point within ``max_dist`` (required, finite, > 0), keeps the pairs whose
    distance is at most the ``inlier_ratio`` quantile of the matched distances, and fits T_{k+1} in closed form from the ORIGINAL
    points; it stops when the rotation and the translation increments fall below ``min_rot`` (rad) and ``min_trans`` (strictly: 0
    disables the check), after ``n_iters`` iterations, or on a failure, which leaves the estimate as it was.  ``init`` [4,4]: the
    prior (default identity), or 'global' / 'planes': the prior is ``register_global`` / ``register_planes(points, survey,
    refine=False, **global_kwargs)``, which the result carries as ``coarse``.  Rows outside ``mask`` (bool [N]) are left out.  Defaults as icp_alignment of the reference.

    All iterations are queued on the device by one call (ops.survey_align); the host reads the result once, at the end."""
    if max_dist is None:
        raise ValueError('register_cloud needs max_dist (finite, > 0)')
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else 'cuda'
    coarse = None
    if isinstance(init, str):
        if init not in ('global', 'planes'):
            raise ValueError("init must be a 4 x 4 transform, None, 'global' or 'planes', got %r" % (init,))
        coarse = (register_global if init == 'global' else register_planes)(points, survey, refine=False, mask=mask, device=device,
                                                                            **dict(global_kwargs or {}))
        if coarse.status != 'ok':
            warnings.warn('register_cloud: the global prior is not reliable (%r); the refinement starts from it all the same' % (coarse,))
        init = coarse.T
    elif global_kwargs is not None:
        raise ValueError("global_kwargs goes with init='global' or init='planes'")
    reg = _register_cloud(points, survey, init, inlier_ratio, max_dist, n_iters, min_rot, min_trans, min_pairs, mask, device)
    reg.coarse = coarse
    return reg


def _register_cloud(points, survey, init, inlier_ratio, max_dist, n_iters, min_rot, min_trans, min_pairs, mask, device):
    from . import ops
    sd = survey.on_device(device)
    dev = sd.device
    pts = torch.as_tensor(points).detach().to(device=dev, dtype=torch.float64).reshape(-1, 3)
    if mask is not None:
        keep = torch.as_tensor(mask).to(device=dev).reshape(-1)
        if keep.dtype != torch.bool or keep.shape[0] != pts.shape[0]:
            raise ValueError('mask must be bool [%d]' % pts.shape[0])
        pts = pts[keep]
    pts = pts.contiguous()
    T0 = np.eye(4) if init is None else np.array(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
    if T0.shape != (4, 4):
        raise ValueError('init must be a 4 x 4 transform')
    n = pts.shape[0]
    if n == 0:
        return Registration(T0, 'empty', 0, 0, float('nan'), float('nan'), np.zeros((0, nv.DC_ALIGN_HISTORY_COLS)))
    # the fixed origins the moments are taken about, on the device: the centre of the query's bounding box (non-finite rows aside)
    # and the centre of the survey's bounds
    lo = torch.nan_to_num(pts, nan=float('inf'), posinf=float('inf'), neginf=float('inf')).amin(dim=0)
    hi = torch.nan_to_num(pts, nan=float('-inf'), posinf=float('-inf'), neginf=float('-inf')).amax(dim=0)
    o_p = torch.nan_to_num(0.5 * (lo + hi), nan=0.0, posinf=0.0, neginf=0.0)
    origins = torch.cat([o_p, sd.origin()]).contiguous()
    prior = None if init is None else torch.as_tensor(T0).to(dev).contiguous()
    state, status, history = ops.survey_align(sd, pts, origins, prior=prior, inlier_ratio=inlier_ratio, max_dist=max_dist, n_iters=n_iters,
                                              min_rot=min_rot, min_trans=min_trans, min_pairs=min_pairs)
    packed = torch.cat([state, status.to(torch.float64), history.reshape(-1)]).cpu().numpy()          # the one host read
    st, code, hist = packed[:nv.DC_ALIGN_STATE_COUNT], packed[nv.DC_ALIGN_STATE_COUNT:nv.DC_ALIGN_STATE_COUNT + 4], \
        packed[nv.DC_ALIGN_STATE_COUNT + 4:].reshape(-1, nv.DC_ALIGN_HISTORY_COLS)
    iters = int(code[1])
    return Registration(st[nv.DC_ALIGN_STATE_POSE:nv.DC_ALIGN_STATE_POSE + 16].reshape(4, 4).copy(), nv.ALIGN_STATUS[int(code[0])], iters,
                        int(st[nv.DC_ALIGN_STATE_PAIRS]) if np.isfinite(st[nv.DC_ALIGN_STATE_PAIRS]) else 0,
                        float(st[nv.DC_ALIGN_STATE_RMS]), float(st[nv.DC_ALIGN_STATE_THRESHOLD]), hist.copy())


class GlobalRegistration(object):
    """Result of ``register_global``: ``T`` (numpy [4,4], survey frame from the cloud's frame; the refined one with ``refine``),
    ``T_coarse`` (the winning hypothesis's), ``status`` ('ok', 'low_fitness', 'no_correspondences', 'no_hypothesis' or 'empty'), ``ok``,
    ``hypothesis`` (the winner's number, -1 without one), its ``score`` (matches within eps) and ``fitness`` (voxel-filtered cloud
    points with a survey point within eps), ``n_points`` (cloud points after the voxel filter), ``n_correspondences``, ``n_valid``
    (valid hypotheses), ``candidates`` int64 [M,3] = (h, score, fitness) in the order they were tried, and with ``refine`` ``refined``,
    the Registration of register_cloud from the coarse T.

    ``register_planes`` returns the same class with ``method`` 'planes' (else 'descriptors'): ``status`` may also be 'too_few_planes',
    ``score`` is the summed support of the agreeing cloud planes, ``n_planes`` = (Pc, Ps), ``n_triples`` the independent cloud
    triples, ``n_enumerated`` the hypotheses walked, ``hypothesis`` and the first column of ``candidates`` are 64-bit hypothesis
    numbers, and ``runner_up`` is the best fitness among the OTHER candidates (an ambiguous room shows there); ``n_correspondences``
    stays 0."""

    method = 'descriptors'
    n_planes = None
    n_triples = 0
    n_enumerated = 0
    runner_up = None

    def __init__(self, T, status, hypothesis=-1, score=0, fitness=0, n_points=0, n_correspondences=0, n_valid=0, candidates=None):
        self.T, self.T_coarse, self.status = T, T.copy(), status
        self.hypothesis, self.score, self.fitness = int(hypothesis), int(score), int(fitness)
        self.n_points, self.n_correspondences, self.n_valid = int(n_points), int(n_correspondences), int(n_valid)
        self.candidates = np.zeros((0, 3), dtype=np.int64) if candidates is None else candidates
        self.refined = None

    @property
    def ok(self):
        return self.status == 'ok' and (self.refined is None or self.refined.ok)

    def __repr__(self):
        if self.method == 'planes':
            return 'GlobalRegistration(planes: %s, %s planes, hypothesis %d of %d valid, score %d, fitness %d of %d points, runner-up %s)' % (
                self.status, self.n_planes, self.hypothesis, self.n_valid, self.score, self.fitness, self.n_points, self.runner_up)
        return 'GlobalRegistration(%s, hypothesis %d, score %d of %d matches, fitness %d of %d points)' % (
            self.status, self.hypothesis, self.score, self.n_correspondences, self.fitness, self.n_points)

    def as_dict(self):
        out = dict(T=self.T.tolist(), T_coarse=self.T_coarse.tolist(), status=self.status, ok=self.ok, hypothesis=self.hypothesis,
                   score=self.score, fitness=self.fitness, n_points=self.n_points, n_correspondences=self.n_correspondences,
                   n_valid=self.n_valid, candidates=self.candidates.tolist())
        if self.method == 'planes':
            out.update(method=self.method, n_planes=self.n_planes, n_triples=self.n_triples, n_enumerated=self.n_enumerated,
                       runner_up=self.runner_up)
        return out


def global_descriptors(points, normals, voxel, feature_k, feature_radius):
    """The descriptor side of ``register_global`` for one cloud on the device (points f64 [N,3] finite, normals f64 [N,3] or None):
    (points, normals, feat f32 [n,33], has i32 [n]) of the n survivors of ops.voxel_filter(preserve_order=True).  The neighbour table
    is ops.knn of the filtered cloud in itself with min(feature_k + 1, 64) columns within ``feature_radius``, the point's own row
    taken out: the feature_k nearest OTHER points (63 of them at feature_k = 64, the most ops.knn's table holds beside the point
    itself).  ``normals=None`` estimates them on the filtered cloud with the package's feature kernels (k = 10, as
    SurveyCloud.from_points does); a point without one has no descriptor."""
    from . import ops
    keep = ops.voxel_filter(points, float(voxel), preserve_order=True)
    if keep is None:
        raise ValueError('the cloud spans too many voxels of %g m for the voxel filter: use a larger voxel' % voxel)
    fp = points[keep].contiguous()
    if normals is None:
        from .depth_cloud import DepthCloud
        cloud = DepthCloud.from_points(fp)
        cloud.update_all(k=10, r=None)
        fn = cloud.normals.detach().to(torch.float64).contiguous()
    else:
        fn = normals[keep].contiguous()
    n = fp.shape[0]
    k_tab = min(int(feature_k) + 1, 64)
    dist, idx = ops.knn(fp, k_tab, r=float(feature_radius))
    idx = torch.where(idx == torch.arange(n, dtype=torch.int32, device=fp.device)[:, None], torch.full_like(idx, -1), idx).contiguous()
    feat, has = ops.pair_histograms(fp, fn, idx, dist)
    return fp, fn, feat, has


def register_global(points, survey, normals=None, voxel=0.25, feature_k=64, feature_radius=None, n_hypotheses=2 ** 20, eps=None,
                    edge_ratio=0.9, min_edge=None, n_candidates=16, seed=135, min_fitness=0.5, refine=True, refine_kwargs=None, mask=None,
                    device=None):
    """Registration of ``points`` [N,3] against ``survey`` (survey.SurveyCloud) WITHOUT a prior (DESIGN "Global registration"): both
    clouds are voxel-filtered at ``voxel``, every point gets a 33-bin descriptor of the folded pair features of its ``feature_k``
    nearest other points within ``feature_radius`` (default 6 voxel; ``normals`` [N,3] of any sign, estimated when None), every cloud
    descriptor is matched to its nearest survey descriptor, ``n_hypotheses`` triples of matches are drawn (seeded: ``seed``), those
    whose edges are at least ``min_edge`` (default 4 voxel) long and within ``edge_ratio`` of their images are fitted in closed form
    and scored by the matches they bring within ``eps`` (default 0.6 voxel); the ``n_candidates`` best are ranked by their fitness,
    the filtered cloud points they bring within eps of the survey.  status 'low_fitness': the winner's fitness is below
    ``min_fitness`` x the filtered points (T is still returned).  With ``refine`` the coarse T is the prior of
    register_cloud(points, survey, **refine_kwargs) (max_dist defaults to 2 voxel), and T is the refined one.  Rows outside ``mask``
    and rows that are not finite are left out.  The survey's side is computed once per device and argument set.  The default
    ``n_hypotheses`` is too few where only 1 to 2 % of the matches are right: on the test room it leaves three of five placements
    without an all-inlier triple, and 2^22 is what all five need (DESIGN "Global registration"); a 'low_fitness' status says that the
    pose found does not explain the cloud -- raise n_hypotheses or the voxel -- and the refinement then runs with a warning.  All of it runs on
    the device; the host reads two counts on the way (the matches, the valid hypotheses) and the candidates once, at the end."""
    from . import ops
    voxel = float(voxel)
    if not (voxel > 0.0 and voxel < float('inf')):
        raise ValueError('voxel must be finite and > 0, got %r' % (voxel,))
    feature_radius = 6.0 * voxel if feature_radius is None else float(feature_radius)
    eps = 0.6 * voxel if eps is None else float(eps)
    min_edge = 4.0 * voxel if min_edge is None else float(min_edge)
    feature_k, n_hyp, n_cand = int(feature_k), int(n_hypotheses), int(n_candidates)
    if not 1 <= feature_k <= 64:
        raise ValueError('feature_k must lie in 1..64, got %r' % (feature_k,))
    if not (feature_radius > 0.0 and eps > 0.0 and min_edge >= 0.0 and 0.0 < float(edge_ratio) <= 1.0):
        raise ValueError('register_global needs feature_radius, eps > 0, min_edge >= 0 and 0 < edge_ratio <= 1')
    if n_hyp < 1 or n_cand < 1:
        raise ValueError('register_global needs n_hypotheses >= 1 and n_candidates >= 1')
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else 'cuda'
    sd = survey.on_device(device)
    dev = sd.device
    pts = torch.as_tensor(points).detach().to(device=dev, dtype=torch.float64).reshape(-1, 3)
    nrm = None if normals is None else torch.as_tensor(normals).detach().to(device=dev, dtype=torch.float64).reshape(-1, 3)
    if nrm is not None and nrm.shape[0] != pts.shape[0]:
        raise ValueError('normals must be [%d,3]' % pts.shape[0])
    keep = torch.isfinite(pts).all(dim=1)
    if mask is not None:
        m = torch.as_tensor(mask).to(device=dev).reshape(-1)
        if m.dtype != torch.bool or m.shape[0] != pts.shape[0]:
            raise ValueError('mask must be bool [%d]' % pts.shape[0])
        keep = keep & m
    pts = pts[keep].contiguous()
    nrm = None if nrm is None else nrm[keep].contiguous()
    if pts.shape[0] == 0:
        return GlobalRegistration(np.eye(4), 'empty')
    with torch.no_grad():
        fp, _, feat, has = global_descriptors(pts, nrm, voxel, feature_k, feature_radius)
        sp, _, sfeat, shas = survey.global_descriptors(dev, voxel, feature_k, feature_radius)
        n = fp.shape[0]
        midx, _ = ops.feature_nn(feat, has, sfeat, shas)
        rows = torch.nonzero(midx >= 0).reshape(-1)                 # ascending; a host read: the number of matches
        c = rows.shape[0]
        if c == 0:
            return GlobalRegistration(np.eye(4), 'no_correspondences', n_points=n)
        p = fp[rows].contiguous()
        y = sp[midx[rows].long()].contiguous()
        # the two fixed origins of register_cloud: the centre of the cloud's bounding box and the centre of the survey's bounds
        origins = torch.cat([0.5 * (pts.amin(dim=0) + pts.amax(dim=0)), sd.origin()]).contiguous()
        valid, T = ops.greg_fit(p, y, origins, n_hyp, seed, min_edge, edge_ratio)
        score, vlist = ops.greg_score(valid, T, p, y, eps, want_list=True)   # a host read: the number of valid hypotheses
        n_valid = vlist.shape[0]
        if n_valid == 0:
            return GlobalRegistration(np.eye(4), 'no_hypothesis', n_points=n, n_correspondences=c)
        # the candidates: the largest (score, then lower h) by one int64 key, sorted on the device
        h_all = torch.arange(n_hyp, dtype=torch.int64, device=dev)
        key = score.to(torch.int64) * (1 << 32) + ((1 << 32) - 1 - h_all)
        cand = (1 << 32) - 1 - (torch.topk(key, min(n_cand, n_valid), sorted=True).values & ((1 << 32) - 1))
        sd.reserve(n)
        idx1 = torch.empty((n, 1), dtype=torch.int32, device=dev)
        dist1 = torch.empty((n, 1), dtype=torch.float64, device=dev)
        Tc = T[cand].contiguous()
        fitness = torch.empty((cand.shape[0],), dtype=torch.int64, device=dev)
        for q in range(cand.shape[0]):
            ops.knn_grid_query(sd.grid, fp, Tc[q], 1, r=eps, idx=idx1, dist=dist1)
            fitness[q] = (idx1 >= 0).sum()
        packed = torch.cat([cand.to(torch.float64), score[cand].to(torch.float64), fitness.to(torch.float64), Tc.reshape(-1)]).cpu().numpy()
    m_c = cand.shape[0]                                              # the one read of the result
    table = np.stack([packed[:m_c], packed[m_c:2 * m_c], packed[2 * m_c:3 * m_c]], axis=1).astype(np.int64)
    best = int(np.argmax(table[:, 2]))                              # the first of the largest: ties go to the earlier candidate
    T_best = packed[3 * m_c:].reshape(m_c, 4, 4)[best].copy()
    status = 'ok' if table[best, 2] >= float(min_fitness) * n else 'low_fitness'
    res = GlobalRegistration(T_best, status, table[best, 0], table[best, 1], table[best, 2], n, c, n_valid, table)
    if refine:
        if status != 'ok':
            warnings.warn('register_global: refining from a prior of low fitness (%d of %d points): the result is not reliable'
                          % (res.fitness, n))
        kw = dict(refine_kwargs or {})
        kw.setdefault('max_dist', 2.0 * voxel)
        res.refined = register_cloud(pts, survey, init=T_best, device=dev, **kw)
        res.T = res.refined.T
    return res


def _planes_result(status, n_planes=None, **kw):
    res = GlobalRegistration(np.eye(4), status, **kw)
    res.method, res.n_planes = 'planes', n_planes
    return res


def cloud_planes(points, plane_voxel, distance_threshold, min_support, ransac_iters, cluster_eps, max_planes, seed):
    """(params f64 device [P,4], support i64 device [P]) of one side of ``register_planes``: segmentation.fit_planes on the rows
    ops.voxel_filter(preserve_order=True) keeps at ``plane_voxel`` (all rows when None); a plane's support is its point count."""
    from . import ops
    from .segmentation import fit_planes
    x = points
    if plane_voxel is not None:
        keep = ops.voxel_filter(points, float(plane_voxel), preserve_order=True)
        if keep is None:
            raise ValueError('the cloud spans too many voxels of %g m for the voxel filter: use a larger plane_voxel' % plane_voxel)
        x = points[keep].contiguous()
    planes = fit_planes(x, float(distance_threshold), min_support=int(min_support), max_iterations=int(ransac_iters),
                        max_models=int(max_planes), eps=cluster_eps, seed=int(seed))
    params = planes.params.to(device=points.device, dtype=torch.float64).reshape(-1, 4).contiguous()
    support = torch.tensor([int(i.shape[0]) for i in planes.indices], dtype=torch.int64, device=points.device)
    return params, support


def register_planes(points, survey, plane_voxel=0.1, distance_threshold=0.03, min_support=40, survey_min_support=100, ransac_iters=500,
                    cluster_eps=0.4, max_planes=32, min_det=0.5, tol_dot=0.05, angle_tol=math.radians(3.0), offset_tol=0.05, voxel=0.25,
                    eps=None, n_candidates=64, dedupe_rot=math.radians(5.0), dedupe_trans=0.25, seed=0, min_fitness=0.5, refine=True,
                    refine_kwargs=None, mask=None, device=None):
    """Registration of ``points`` [N,3] against ``survey`` (survey.SurveyCloud) WITHOUT a prior, from plane correspondences (DESIGN
    "Plane registration"): for maps of rooms and corridors, where ``register_global``'s descriptors are those of a plane almost
    everywhere.  Planes are fitted on both sides (segmentation.fit_planes on the rows the voxel filter keeps at ``plane_voxel``, all
    rows when None; threshold ``distance_threshold``, ``ransac_iters`` hypotheses a round, clusters of ``cluster_eps``, at most
    ``max_planes`` <= 64 planes of at least ``min_support`` / ``survey_min_support`` points; the survey's once per device and argument
    set).  Every pairing of an independent triple of cloud planes (|det| >= ``min_det``) with three survey planes under the eight sign
    patterns is enumerated on the device: those whose normals' dot products agree within ``tol_dot`` and whose handedness agrees are
    fitted in closed form and scored by the summed support of the cloud planes that land on a survey plane within ``angle_tol``
    (radians) and ``offset_tol``.  The best by (score, then lower number) are walked with suppression of poses within ``dedupe_rot``
    AND ``dedupe_trans`` (at the cloud's bounding-box centre) of one already kept, until ``n_candidates`` distinct poses are kept;
    they are ranked by fitness exactly as in ``register_global`` (the cloud voxel-filtered at ``voxel``, a survey point within
    ``eps``, default 0.6 voxel).  The infinite planes of a box room agree under many wrong poses, and only the fitness tells them
    apart: the true pose must be AMONG the candidates, which is why there are 64 of them and why they are distinct.
    status 'too_few_planes': fewer than 3 planes on a side, or no independent triple (``register_global`` remains the fallback);
    'no_hypothesis', 'low_fitness', 'empty' and ``refine`` / ``refine_kwargs`` / ``mask`` as in register_global.  The host reads the
    per-round results of the plane fits, the number of valid hypotheses, the kept rows and the candidates, once each."""
    from . import ops
    voxel = float(voxel)
    if not (voxel > 0.0 and voxel < float('inf')):
        raise ValueError('voxel must be finite and > 0, got %r' % (voxel,))
    eps = 0.6 * voxel if eps is None else float(eps)
    n_cand, max_planes = int(n_candidates), int(max_planes)
    if not (eps > 0.0 and n_cand >= 1 and 3 <= max_planes <= nv.DC_PLANEREG_MAX_PLANES):
        raise ValueError('register_planes needs eps > 0, n_candidates >= 1 and 3 <= max_planes <= %d' % nv.DC_PLANEREG_MAX_PLANES)
    tol = (float(min_det), float(tol_dot), math.cos(float(angle_tol)), float(offset_tol))
    if not all(math.isfinite(v) for v in tol + (float(dedupe_rot), float(dedupe_trans))) or min(tol[0], tol[1], tol[3]) < 0.0:
        raise ValueError('register_planes needs finite tolerances, min_det, tol_dot and offset_tol >= 0')
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else 'cuda'
    sd = survey.on_device(device)
    dev = sd.device
    pts = torch.as_tensor(points).detach().to(device=dev, dtype=torch.float64).reshape(-1, 3)
    keep = torch.isfinite(pts).all(dim=1)
    if mask is not None:
        m = torch.as_tensor(mask).to(device=dev).reshape(-1)
        if m.dtype != torch.bool or m.shape[0] != pts.shape[0]:
            raise ValueError('mask must be bool [%d]' % pts.shape[0])
        keep = keep & m
    pts = pts[keep].contiguous()
    if pts.shape[0] == 0:
        return _planes_result('empty')
    with torch.no_grad():
        cp, cs = cloud_planes(pts, plane_voxel, distance_threshold, min_support, ransac_iters, cluster_eps, max_planes, seed)
        sp, _ = survey.planes(dev, plane_voxel, distance_threshold, survey_min_support, ransac_iters, cluster_eps, max_planes, seed)
        n_planes = (int(cp.shape[0]), int(sp.shape[0]))
        fkeep = ops.voxel_filter(pts, voxel, preserve_order=True)
        if fkeep is None:
            raise ValueError('the cloud spans too many voxels of %g m for the voxel filter: use a larger voxel' % voxel)
        fp = pts[fkeep].contiguous()
        n = fp.shape[0]
        if min(n_planes) < nv.DC_PLANEREG_MIN_PLANES:
            return _planes_result('too_few_planes', n_planes, n_points=n)
        tri = ops.planereg_triples(cp, tol[0])
        n_tri = tri.shape[0]
        if n_tri == 0:
            return _planes_result('too_few_planes', n_planes, n_points=n)
        n_enum = n_tri * n_planes[1] ** 3 * 8
        h, T, score = ops.planereg_hypotheses(cp, cs, sp, tri, *tol)          # a host read: the number of valid hypotheses
        n_valid = h.shape[0]
        if n_valid == 0:
            res = _planes_result('no_hypothesis', n_planes, n_points=n)
            res.n_triples, res.n_enumerated = n_tri, n_enum
            return res
        centre = 0.5 * (pts.amin(dim=0) + pts.amax(dim=0))
        rows = ops.planereg_select(score, T, centre, n_cand, float(dedupe_rot), float(dedupe_trans))
        rows = rows[rows >= 0]                                              # a host read: the distinct poses kept
        sd.reserve(n)
        idx1 = torch.empty((n, 1), dtype=torch.int32, device=dev)
        dist1 = torch.empty((n, 1), dtype=torch.float64, device=dev)
        Tc = T[rows].contiguous()
        fitness = torch.empty((rows.shape[0],), dtype=torch.int64, device=dev)
        for q in range(rows.shape[0]):
            ops.knn_grid_query(sd.grid, fp, Tc[q], 1, r=eps, idx=idx1, dist=dist1)
            fitness[q] = (idx1 >= 0).sum()
        table = torch.stack([h[rows], score[rows], fitness], dim=1).cpu().numpy()      # the read of the result (int64: h passes 2^53)
        Tc = Tc.cpu().numpy()
    best = int(np.argmax(table[:, 2]))                              # the first of the largest: ties go to the earlier candidate
    others = np.delete(table[:, 2], best)
    status = 'ok' if table[best, 2] >= float(min_fitness) * n else 'low_fitness'
    res = GlobalRegistration(Tc[best].copy(), status, table[best, 0], table[best, 1], table[best, 2], n, 0, n_valid, table)
    res.method, res.n_planes, res.n_triples, res.n_enumerated = 'planes', n_planes, n_tri, n_enum
    res.runner_up = int(others.max()) if len(others) else 0
    if refine:
        if status != 'ok':
            warnings.warn('register_planes: refining from a prior of low fitness (%d of %d points): the result is not reliable'
                          % (res.fitness, n))
        kw = dict(refine_kwargs or {})
        kw.setdefault('max_dist', 2.0 * voxel)
        res.refined = register_cloud(pts, survey, init=Tc[best], device=dev, **kw)
        res.T = res.refined.T
    return res
