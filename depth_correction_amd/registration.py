"""Registration: putting a cloud, or a path, into the frame of a survey (DESIGN "Survey registration").

``cloud_loss``, ``metrics.point_to_cloud_distance`` and ``eval_map`` against a ``survey.SurveyCloud`` assume that the survey and the
scans' poses share one frame.  This module gets them there:

``absolute_orientation``  the closed-form rigid fit of paired points (utils.py:253-304 of the reference), on the host;
``align_paths``           the same for two paths, with the residual statistics scripts/paths_alignment prints;
``register_cloud``        trimmed ICP of a cloud against a survey, what scripts/map_bias_removal:167-185 icp_alignment does on the
                          host with a cKDTree -- here one queue of device work (ops.survey_align) and ONE host read, at the end.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nv

__all__ = ['absolute_orientation', 'align_paths', 'register_cloud', 'Registration']


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
    ``history`` [n_iters, 5] = (pairs, rms, threshold, d_rot, d_trans) per iteration, NaN in the rows never reached."""

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
                   mask=None, device=None):
    """Trimmed ICP of ``points`` [N,3] (tensor or array, frame A) against ``survey`` (survey.SurveyCloud): the T with T points ~ survey.
    Every iteration matches T_k p to its nearest survey point within ``max_dist`` (required, finite, > 0), keeps the pairs whose
    distance is at most the ``inlier_ratio`` quantile of the matched distances, and fits T_{k+1} in closed form from the ORIGINAL
    points; it stops when the rotation and the translation increments fall below ``min_rot`` (rad) and ``min_trans`` (strictly: 0
    disables the check), after ``n_iters`` iterations, or on a failure, which leaves the estimate as it was.  ``init`` [4,4]: the
    prior (default identity).  Rows outside ``mask`` (bool [N]) are left out.  Defaults as icp_alignment of the reference.

    All iterations are queued on the device by one call (ops.survey_align); the host reads the result once, at the end."""
    from . import ops
    if max_dist is None:
        raise ValueError('register_cloud needs max_dist (finite, > 0)')
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else 'cuda'
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
