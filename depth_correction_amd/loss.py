"""Map-consistency losses with the reference's signatures (loss.py:125-579).

Two execution paths produce the same numbers:
  * fused (eval.eval_loss_clouds, plan.SequencePlan): covariance -> eigen -> pointwise loss -> backward record in
    the HIP kernels, never materialising per-point features;
  * un-fused (this module on a DepthCloud whose features came from ``update_all``): the pointwise post-processing
    of loss.py:250-289 on ``cloud.eigvals`` / ``cloud.cov`` (small ``[M]`` tensors), differentiable down to the
    points through dc_features_bwd.  All of the reference's options are available here (mask, offset, sqrt,
    normalisation, quantile inliers, reductions).
``mesh_loss`` is the supervised counterpart: the mean distance of the corrected, posed points to a ground-truth mesh, forward
and backward (weights, exponents, poses) out of one dc_mesh_loss call per sequence.
``cloud_loss`` is the same against a surveyed point cloud (survey.SurveyCloud): point-to-plane or point-to-point distances to the
nearest survey points, gated and trimmed, out of one dc_cloud_loss call per sequence.
``tsdf_loss`` is the self-supervised counterpart of the two: the target is the sparse TSDF volume the sequence's own corrected scans
fuse into (``TsdfTarget``, re-fused as training goes), each scan scored against the volume of the other scans, out of one dc_tsdf_loss
call per sequence.
``icp_loss`` with precomputed correspondences runs as one kernel per scan pair (dc_p2plane_sequence for
point-to-plane, dc_p2point_sequence for point-to-point distances) including its backward to the model weights and
poses; ``point_to_point_dist`` as a metric on GPU clouds (scripts/model_poses_learning:142-146) uses the same kernel.
"""
from __future__ import annotations

import warnings
from enum import Enum

import torch

from . import ops
from .depth_cloud import DepthCloud
from .plan import PlanRegistry
from .segmentation import Planes
from .utils import trace

__all__ = ['batch_loss', 'cloud_loss', 'create_loss', 'icp_loss', 'loss_by_name', 'mesh_loss', 'min_eigval_loss', 'point_to_plane_dist',
           'point_to_point_dist', 'reduce', 'Reduction', 'trace_loss', 'icp_correspondences', 'tsdf_loss', 'TsdfTarget']


class Reduction(Enum):
    NONE = 'none'
    MEAN = 'mean'
    SUM = 'sum'


def reduce(x, reduction=Reduction.MEAN, weights=None, only_finite=False, skip_nans=False):
    assert reduction in Reduction
    keep = x.isfinite() if only_finite else (~x.isnan() if skip_nans else None)
    if keep is not None:
        weights = weights[keep] if weights is not None else None
        x = x[keep]
    if reduction == Reduction.MEAN:
        return x.mean() if weights is None else (weights * x).sum() / weights.sum()
    if reduction == Reduction.SUM:
        return x.sum() if weights is None else (weights * x).sum()
    return x


def batch_loss(loss_fun, clouds, masks=None, offsets=None, reduction=Reduction.MEAN, only_finite=False,
               skip_nans=False, **kwargs):
    """Pointwise losses of several sequences, concatenated, then reduced once (loss.py:181-213)."""
    assert callable(loss_fun) and isinstance(clouds, (list, tuple))
    masks = len(clouds) * [None] if masks is None else masks
    offsets = len(clouds) * [None] if offsets is None else offsets
    assert len(masks) == len(clouds) == len(offsets)
    parts, loss_clouds = [], []
    for cloud, mask, offset in zip(clouds, masks, offsets):
        part, loss_cloud = loss_fun(cloud, mask=mask, offset=offset, reduction=Reduction.NONE, **kwargs)
        parts.append(part)
        loss_clouds.append(loss_cloud)
    return reduce(torch.cat(parts), reduction=reduction, only_finite=only_finite, skip_nans=skip_nans), loss_clouds


def _pointwise(raw_fun, cloud, mask, offset, sqrt, reduction, inlier_max_loss, inlier_ratio, inlier_loss_mult,
               only_finite, skip_nans):
    """Shared tail of min_eigval_loss / trace_loss (loss.py:244-294, 324-370)."""
    assert offset is None or isinstance(offset, (DepthCloud, torch.Tensor))
    # (plane neighbourhoods: every plane is one entry, loss.py:216-294 on Planes.eigvals / Planes.cov)
    if mask is not None:
        print('Using %.3f valid entries from input cloud.' % mask.float().mean())
        cloud, mask = cloud[mask], None
    loss = raw_fun(cloud)
    if inlier_ratio < 1.0:
        assert offset is None
        q = torch.quantile(loss, inlier_ratio, dim=0)
        if inlier_loss_mult != 1.0:
            q = inlier_loss_mult * q
        inlier_max_loss = q if inlier_max_loss is None else torch.min(torch.as_tensor(inlier_max_loss, dtype=q.dtype,
                                                                                       device=q.device), q)
    if inlier_max_loss is not None:
        assert offset is None
        mask = loss <= inlier_max_loss
        print('Using %i (%.3g) inliers with loss <= %.3g.' % (mask.sum().item(), mask.float().mean().item(),
                                                              float(torch.as_tensor(inlier_max_loss).detach())))
        cloud, loss = cloud[mask], loss[mask]
    if offset is not None:
        loss = loss - (offset.loss if isinstance(offset, DepthCloud) else offset)
    loss = torch.relu(loss)
    if sqrt:
        loss = torch.sqrt(loss)
    cloud = cloud.copy()
    cloud.loss = loss
    return reduce(loss, reduction=reduction, only_finite=only_finite, skip_nans=skip_nans), cloud


def min_eigval_loss(cloud, mask=None, offset=None, sqrt=False, normalization=False, reduction=Reduction.MEAN,
                    inlier_max_loss=None, inlier_ratio=1.0, inlier_loss_mult=1.0, only_finite=False, skip_nans=False,
                    **kwargs):
    """Smallest neighbourhood eigenvalue (optionally over the total variance) averaged over the masked points."""
    if isinstance(cloud, (list, tuple)):
        return batch_loss(min_eigval_loss, cloud, masks=mask, offsets=offset, sqrt=sqrt, normalization=normalization,
                          reduction=reduction, inlier_max_loss=inlier_max_loss, inlier_ratio=inlier_ratio,
                          inlier_loss_mult=inlier_loss_mult, only_finite=only_finite, skip_nans=skip_nans)
    assert isinstance(cloud, (DepthCloud, Planes)) and cloud.eigvals is not None

    def raw(c):
        lam = c.eigvals
        return lam[:, 0] / lam.sum(dim=-1).clamp(min=1e-6) if normalization else lam[:, 0]
    return _pointwise(raw, cloud, mask, offset, sqrt, reduction, inlier_max_loss, inlier_ratio, inlier_loss_mult,
                      only_finite, skip_nans)


def trace_loss(cloud, mask=None, offset=None, sqrt=None, reduction=Reduction.MEAN, inlier_max_loss=None,
               inlier_ratio=1.0, inlier_loss_mult=1.0, only_finite=False, skip_nans=False, **kwargs):
    """Trace of the neighbourhood covariance averaged over the masked points."""
    if isinstance(cloud, (list, tuple)):
        return batch_loss(trace_loss, cloud, masks=mask, offsets=offset, sqrt=sqrt, reduction=reduction,
                          inlier_max_loss=inlier_max_loss, inlier_ratio=inlier_ratio, inlier_loss_mult=inlier_loss_mult,
                          only_finite=only_finite, skip_nans=skip_nans)
    assert isinstance(cloud, (DepthCloud, Planes)) and cloud.cov is not None
    return _pointwise(lambda c: trace(c.cov), cloud, mask, offset, sqrt, reduction, inlier_max_loss, inlier_ratio,
                      inlier_loss_mult, only_finite, skip_nans)


# ---- ICP-style losses ---------------------------------------------------------------------------------------------
def icp_correspondences(points1, points2, ratio):
    """(mask1 bool [N1], idx2 int64 [M]): 1-NN of scan 1 in scan 2 on the GPU, inliers = dist <= quantile(dist, ratio)
    (train.py:186-193, loss.py:440-452)."""
    dist, idx = ops.knn(points2.detach().contiguous(), 1, query=points1.detach().to(points2.dtype).contiguous())
    dist, idx = dist[:, 0].contiguous(), idx[:, 0].contiguous()
    mask1, idx2, _ = ops.nn1_corr(dist, idx, ratio)                  # quantile select + compaction on the device (dc_nn1_corr)
    return mask1, idx2.long(), dist


def _pair_points(cloud):
    pts = cloud.to_points() if cloud.points is None else cloud.points
    assert not torch.all(torch.isnan(pts))
    return torch.as_tensor(pts, dtype=torch.float)


def _pair_matches(points1, points2, masks, i, ratio):
    if masks is not None:
        m1, m2 = masks[i]
        return torch.as_tensor(m1, device=points1.device), torch.as_tensor(m2, device=points1.device), torch.tensor(-1.0)
    mask1, idx2, dist = icp_correspondences(points1, points2, ratio)
    return mask1, idx2, dist[mask1].mean()


def point_to_plane_dist(clouds: list, icp_inlier_ratio=0.5, masks=None, differentiable=True, verbose=False, **kwargs):
    """Mean symmetric point-to-plane distance over consecutive scan pairs (loss.py:406-488), un-fused form."""
    assert 0.0 <= icp_inlier_ratio <= 1.0
    assert masks is None or len(clouds) == len(masks) + 1
    total, n_pairs = 0.0, len(clouds) - 1
    for i in range(n_pairs):
        c1, c2 = clouds[i], clouds[i + 1]
        assert c1.normals is not None, 'Cloud must have normals computed to estimate point to plane distance'
        p1, p2 = _pair_points(c1), _pair_points(c2)
        mask1, mask2, inl_err = _pair_matches(p1, p2, masks, i, icp_inlier_ratio)
        a, b = p1[mask1], p2[mask2]
        assert len(a) > 0, 'Point clouds do not intersect. Try to sample lidar scans more frequently'
        n1, n2 = c1.normals[mask1], c2.normals[mask2]
        d12 = torch.linalg.norm((n1 * (b - a)).sum(dim=-1, keepdims=True) * n1, dim=-1).mean()
        d21 = torch.linalg.norm((n2 * (a - b)).sum(dim=-1, keepdims=True) * n2, dim=-1).mean()
        total = total + 0.5 * (d12 + d21)
        if inl_err > 0.3:
            warnings.warn('ICP inliers error is too big: %.3f (> 0.3) [m] for pairs (%i, %i)' % (inl_err, i, i + 1))
        if verbose:
            print('Mean point to plane distance: %.3f [m] for scans: (%i, %i), inliers error: %.6f'
                  % (float(total), i, i + 1, float(inl_err)))
    return torch.as_tensor(total / n_pairs)


def _as_cloud(c):
    return c if isinstance(c, DepthCloud) else DepthCloud.from_points(torch.as_tensor(c))


def point_to_point_dist(clouds: list, icp_inlier_ratio=0.5, masks=None, differentiable=True, verbose=False, **kwargs):
    """Mean point-to-point distance over consecutive scan pairs (loss.py:491-565).

    On GPU clouds that carry no autograd graph (the map-accuracy metric of scripts/model_poses_learning:142-146) the
    distances of all pairs come from one dc_p2point_sequence call; correspondences not given are found by the GPU 1-NN
    builder.  Clouds inside an autograd graph take the reference's tensor expressions (icp_loss routes training through
    the fused kernel with its hand-derived backward instead)."""
    assert 0.0 <= icp_inlier_ratio <= 1.0
    assert masks is None or len(clouds) == len(masks) + 1
    n_pairs = len(clouds) - 1
    pts = [_pair_points(c) if isinstance(c, DepthCloud) else torch.as_tensor(c, dtype=torch.float) for c in clouds]
    if n_pairs > 0 and all(p.is_cuda and not p.requires_grad for p in pts):
        pairs, errs = [], []
        for i in range(n_pairs):
            mask1, mask2, inl_err = _pair_matches(pts[i], pts[i + 1], masks, i, icp_inlier_ratio)
            ia = (torch.nonzero(mask1).reshape(-1) if mask1.dtype == torch.bool else mask1).to(torch.int32).contiguous()
            ib = mask2.to(torch.int32).contiguous()
            assert len(ia) > 0 and len(ib) > 0, 'Point clouds do not intersect. Try to sample lidar scans more frequently'
            pairs.append((i, i + 1, ia, ib))
            errs.append(inl_err)
        # the points as they are (already corrected and posed by the caller): unit "directions" x, depth 1, identity poses
        scans = [(ops.PointSet(None, p.contiguous(), torch.ones((len(p),), dtype=p.dtype, device=p.device)), None) for p in pts]
        seq = ops.IcpSequence(scans, pairs, with_model=False, plane=False)
        eye = torch.eye(4, dtype=torch.float64, device=pts[0].device)[:3].reshape(1, 12).repeat(len(pts), 1).contiguous()
        out = seq.eval(eye)
        for i, inl_err in enumerate(errs):
            if inl_err > 0.3:
                warnings.warn('ICP inliers error is too big: %.3f (> 0.3) [m] for pairs (%i, %i)' % (inl_err, i, i + 1))
        return out[0].to(torch.float32)
    total = 0.0
    for i in range(n_pairs):
        p1, p2 = pts[i], pts[i + 1]
        mask1, mask2, inl_err = _pair_matches(p1, p2, masks, i, icp_inlier_ratio)
        a, b = p1[mask1], p2[mask2]
        assert len(a) > 0 and len(b) > 0, 'Point clouds do not intersect. Try to sample lidar scans more frequently'
        total = total + torch.linalg.norm(b - a, dim=1).mean()
        if inl_err > 0.3:
            warnings.warn('ICP inliers error is too big: %.3f (> 0.3) [m] for pairs (%i, %i)' % (inl_err, i, i + 1))
        if verbose:
            print('Mean point to point distance: %.3f [m] for scans: (%i, %i), inliers error: %.6f'
                  % (float(total), i, i + 1, float(inl_err)))
    return torch.as_tensor(total / n_pairs)


class _P2PlaneSequence(torch.autograd.Function):
    """icp_loss of one sequence (all consecutive pairs) through dc_p2plane_sequence: forward and backward come out
    of the same host call."""

    @staticmethod
    def forward(ctx, w, exponent, poses, plan, kind):
        P12 = poses.detach().to(torch.float64)[:, :3, :].reshape(-1, 12).contiguous()
        wv = None if w is None else w.detach().reshape(-1).to(torch.float64).contiguous()
        ev = None if exponent is None else exponent.detach().reshape(-1).to(torch.float64).contiguous()
        out = plan.eval(P12, kind, wv, ev)
        ctx.save_for_backward(out)
        ctx.meta = (None if w is None else (w.shape, w.dtype), poses.dtype, poses.shape[0],
                    exponent.shape if isinstance(exponent, torch.Tensor) else None)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        wmeta, pdt, ns, eshape = ctx.meta
        nt = (out.numel() - 1 - 12 * ns) // 2
        gw = ge = gT = None
        if wmeta is not None and ctx.needs_input_grad[0]:
            gw = (g * out[1:1 + nt]).reshape(wmeta[0]).to(wmeta[1])
        if eshape is not None and ctx.needs_input_grad[1]:
            ge = (g * out[1 + nt:1 + 2 * nt]).reshape(eshape)
        if ctx.needs_input_grad[2]:
            gT = torch.zeros((ns, 4, 4), dtype=torch.float64, device=out.device)
            gT[:, :3, :] = (g * out[1 + 2 * nt:]).reshape(ns, 3, 4)
            gT = gT.to(pdt)
        return gw, ge, gT, None, None


_icp_plans = PlanRegistry()


def _icp_sequence_plan(seq_clouds, seq_masks, with_model, plane):
    fields = [t for c in seq_clouds for t in (c.vps, c.dirs, c.depth, c.inc_angles, c.normals if plane else None, c.mask)]
    fields += [m for pair in seq_masks for m in pair]

    def build():
        scans = []
        for c in seq_clouds:
            n = len(c)
            cont = lambda t: t.detach().expand(n, t.shape[-1]).contiguous() if t.dim() == 2 else t.detach().contiguous()
            vps = None if not bool(c.vps.any()) else cont(c.vps)
            inc = cont(c.inc_angles) if (with_model and c.inc_angles is not None) else None
            scans.append((ops.PointSet(vps, cont(c.dirs), cont(c.depth), inc, c.mask if with_model else None),
                          cont(c.normals.to(c.dirs.dtype)) if plane else None))
        dev = scans[0][0].device
        pairs = []
        for i, (m1, m2) in enumerate(seq_masks):
            m1 = torch.as_tensor(m1, device=dev)
            ia = (torch.nonzero(m1).reshape(-1) if m1.dtype == torch.bool else m1).to(torch.int32).contiguous()
            ib = torch.as_tensor(m2, device=dev).to(torch.int32).contiguous()
            assert len(ia) > 0, 'Point clouds do not intersect. Try to sample lidar scans more frequently'
            pairs.append((i, i + 1, ia, ib))
        return ops.IcpSequence(scans, pairs, with_model=with_model, plane=plane)
    return _icp_plans.get(fields, (bool(with_model), bool(plane)), build)


def _fused_icp_sequence(seq_clouds, seq_poses, model, seq_masks, plane=True):
    """ICP loss of one sequence through dc_p2plane_sequence / dc_p2point_sequence (clouds in the sensor frame + poses + model)."""
    kind = getattr(model, 'kernel_kind', None) if model is not None else None
    w, e = model.kernel_params() if kind else (None, None)
    plan = _icp_sequence_plan(seq_clouds, seq_masks, bool(kind), plane)
    poses = seq_poses if isinstance(seq_poses, torch.Tensor) else torch.stack(list(seq_poses))
    return _P2PlaneSequence.apply(w, e, poses, plan, kind)


class _MovedClouds(object):
    """The corrected, posed scans of a sequence (what the reference's icp_loss concatenates into its loss cloud,
    loss.py:381-386,396-398), produced only when a caller looks at the returned cloud."""

    def __init__(self, seq, poses, model, loss):
        self._args, self._cloud, self.loss = (seq, poses, model), None, loss

    def _materialize(self):
        if self._cloud is None:
            seq, poses, model = self._args
            with torch.no_grad():
                moved = [model(c) for c in seq] if model is not None else list(seq)
                if poses is not None:
                    moved = [c.transform(p) for c, p in zip(moved, poses)]
                self._cloud = DepthCloud.concatenate(moved)
                self._cloud.loss = self.loss
        return self._cloud

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self._materialize(), name)

    def __len__(self):
        return sum(len(c) for c in self._args[0])


def icp_loss(clouds, poses=None, model=None, masks=None, **kwargs):
    """ICP-like loss over lists of sequences of scans (loss.py:373-403)."""
    p2plane = kwargs['icp_point_to_plane']
    fused = (masks is not None and poses is not None and clouds and clouds[0][0].dirs.is_cuda
             and (not p2plane or all(c.normals is not None for seq in clouds for c in seq))
             and (model is None or getattr(model, 'kernel_kind', None)))
    loss, loss_cloud = 0., []
    for i, seq in enumerate(clouds):
        if fused:
            loss_seq = _fused_icp_sequence(seq, poses[i], model, masks[i], plane=bool(p2plane))
            loss = loss + loss_seq
            loss_cloud.append(_MovedClouds(seq, poses[i], model, loss))
            continue
        moved = [model(c) for c in seq] if model is not None else seq
        if poses is not None:
            moved = [c.transform(p) for c, p in zip(moved, poses[i])]
        fun = point_to_plane_dist if p2plane else point_to_point_dist
        loss_seq = fun(moved, masks=None if masks is None else masks[i], **kwargs)
        loss = loss + loss_seq
        cloud = DepthCloud.concatenate(moved)
        cloud.loss = loss
        loss_cloud.append(cloud)
    return loss / len(clouds), loss_cloud


# ---- supervised losses against a ground-truth mesh and against a surveyed point cloud ------------------------------------------
class _ScanLossSequence(torch.autograd.Function):
    """mesh_loss / cloud_loss of one sequence through dc_mesh_loss / dc_cloud_loss: forward and backward come out of the same host
    call.  ``opts``: the plan's options as sorted (name, value) pairs."""

    @staticmethod
    def forward(ctx, w, exponent, poses, plan, kind, opts):
        P12 = poses.detach().to(torch.float64)[:, :3, :].reshape(-1, 12).contiguous()
        wv = None if w is None else w.detach().reshape(-1).to(torch.float64).contiguous()
        ev = None if exponent is None else exponent.detach().reshape(-1).to(torch.float64).contiguous()
        want_e = isinstance(exponent, torch.Tensor) and bool(ctx.needs_input_grad[1])
        out = plan.eval(P12, kind, wv, ev, want_exponent=want_e, **dict(opts))
        ctx.save_for_backward(out)
        ctx.meta = (None if w is None else (w.shape, w.dtype), poses.dtype, poses.shape[0],
                    exponent.shape if isinstance(exponent, torch.Tensor) else None, plan.header)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        wmeta, pdt, ns, eshape, h = ctx.meta
        nt = (out.numel() - h - 12 * ns) // 2
        gw = ge = gT = None
        if wmeta is not None and ctx.needs_input_grad[0]:
            gw = (g * out[h:h + nt]).reshape(wmeta[0]).to(wmeta[1])
        if eshape is not None and ctx.needs_input_grad[1]:
            ge = (g * out[h + nt:h + 2 * nt]).reshape(eshape)
        if ctx.needs_input_grad[2]:
            gT = torch.zeros((ns, 4, 4), dtype=torch.float64, device=out.device)
            gT[:, :3, :] = (g * out[h + 2 * nt:]).reshape(ns, 3, 4)
            gT = gT.to(pdt)
        return gw, ge, gT, None, None, None


class _ScanLossPlan(object):
    """What is constant over the optimisation of one sequence against its target: the scans' fields concatenated scan-major, the
    scan offsets, the loss mask, the workspace per term count.  A subclass adds the target, ``header`` (the entries of ``out`` in
    front of the gradients), ``_workspace`` and ``_call``, its one ops call."""

    def __init__(self, seq_clouds, point_mask, with_model):
        dev = seq_clouds[0].dirs.device
        sizes = [len(c) for c in seq_clouds]

        def rows(field, width):
            parts = [getattr(c, field).detach().expand(n, width) for c, n in zip(seq_clouds, sizes)]
            return torch.cat(parts).contiguous()
        vps = rows('vps', 3) if any(bool(c.vps.any()) for c in seq_clouds) else None
        inc = lmask = None
        if with_model:
            if any(c.inc_angles is None for c in seq_clouds):
                raise ValueError('the model needs incidence angles')
            inc = rows('inc_angles', 1)
            if any(c.mask is not None for c in seq_clouds):
                lmask = torch.cat([c.mask if c.mask is not None else torch.ones((n,), dtype=torch.bool, device=dev)
                                   for c, n in zip(seq_clouds, sizes)]).contiguous()
        self.ps = ops.PointSet(vps, rows('dirs', 3), rows('depth', 1), inc, lmask)
        self.n, self.n_scans, self.device = self.ps.n, len(sizes), dev
        ptr_host = [0]
        for n in sizes:
            ptr_host.append(ptr_host[-1] + n)
        self.scan_ptr = torch.tensor(ptr_host, dtype=torch.int64, device=dev)
        self.mask = None if point_mask is None else torch.as_tensor(point_mask, device=dev).to(torch.bool).contiguous()
        self._ws = {}

    def eval(self, poses12, kind=None, w=None, e=None, **opts):
        nt = 0 if not kind else w.numel()
        ws = self._ws.get(nt)
        if ws is None:
            ws = self._ws[nt] = self._workspace(self.n, self.n_scans, nt, self.device)
        return self._call(poses12, kind, w, e, ws=ws, **opts)


class _MeshLossPlan(_ScanLossPlan):
    """The mesh's tree, and the leaf hint, which starts at -1 and is carried from one evaluation to the next (a point's nearest face
    changes little between two optimiser steps)."""
    header, _workspace = 4, staticmethod(ops.mesh_loss_workspace)

    def __init__(self, seq_clouds, mesh, point_mask, with_model):
        super().__init__(seq_clouds, point_mask, with_model)
        self.mesh = mesh
        self.bvh = mesh.on_device(self.device)[3]
        self.leaf_hint = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)

    def _call(self, poses12, kind, w, e, **opts):
        return ops.mesh_loss(self.bvh, self.ps, self.scan_ptr, poses12, kind, w, e, mask=self.mask, leaf_hint=self.leaf_hint, **opts)


class _CloudLossPlan(_ScanLossPlan):
    """The survey's device copies with their grid (built once, its query buffer sized here)."""
    header, _workspace = 6, staticmethod(ops.cloud_loss_workspace)

    def __init__(self, seq_clouds, survey, point_mask, with_model):
        super().__init__(seq_clouds, point_mask, with_model)
        self.survey = survey
        self.survey_dev = survey.on_device(self.device).reserve(self.n)

    def _call(self, poses12, kind, w, e, **opts):
        return ops.cloud_loss(self.survey_dev, self.ps, self.scan_ptr, poses12, kind, w, e, mask=self.mask, **opts)


_mesh_plans = PlanRegistry()
_cloud_plans = PlanRegistry()


def _scan_loss_plan(registry, plan_type, seq_clouds, target, point_mask, with_model):
    fields = [t for c in seq_clouds for t in (c.vps, c.dirs, c.depth, c.inc_angles, c.mask)] + [point_mask, target]
    return registry.get(fields, (bool(with_model),), lambda: plan_type(seq_clouds, target, point_mask, with_model))


def _posed_points64(seq_clouds, seq_poses, model, keep=None):
    """x in fp64 through the model and the poses, scan-major (torch autograd); ``keep`` [N] bool: only these rows are formed (a row
    with a NaN input would otherwise put 0 x NaN into the pose gradient)."""
    parts, off = [], 0
    for i, c in enumerate(seq_clouds):
        n = len(c)
        c64 = DepthCloud(vps=c.vps.double().expand(n, 3), dirs=c.dirs.double(), depth=c.depth.double(),
                         inc_angles=None if c.inc_angles is None else c.inc_angles.double(), mask=c.mask)
        if keep is not None and not bool(keep[off:off + n].all()):
            c64 = c64[keep[off:off + n]]
        off += n
        if model is not None:
            c64 = model(c64)
        if seq_poses is not None:
            c64 = c64.transform(seq_poses[i].double())
        parts.append(c64.vps + c64.depth * c64.dirs)
    return torch.cat(parts)


def _unfused_mesh_sequence(seq_clouds, seq_poses, model, mesh, point_mask, squared, max_dist):
    """The same loss from tensor operations: x in fp64 through the model and the poses, the closest points (detached) from
    ops.mesh_closest, l = |x - c|, torch autograd.  For models without a kernel kind, and what the fused form is tested against."""
    dev = seq_clouds[0].dirs.device
    x = _posed_points64(seq_clouds, seq_poses, model)
    bvh = mesh.on_device(dev)[3]
    face, _, closest = ops.mesh_closest(bvh, x.detach().contiguous(), max_dist=max_dist)
    used = face >= 0
    if point_mask is not None:
        used = used & torch.as_tensor(point_mask, device=dev).to(torch.bool)
    d = x[used] - closest[used]
    sq = (d * d).sum(dim=-1)
    if squared:
        return sq.mean()
    # r = 0 has no direction: zero gradient there (sqrt'(0) is infinite), as in the kernel
    pos = sq > 0
    return (torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))) * pos).mean()


def _unfused_cloud_sequence(seq_clouds, seq_poses, model, survey, point_mask, plane, squared, max_dist, inlier_ratio):
    """The same loss from tensor operations: x in fp64 through the model and the poses, the nearest survey points (detached) from
    ops.knn, the inlier threshold from ops.quantile, torch autograd.  For models without a kernel kind, and what the fused form is
    tested against."""
    dev = seq_clouds[0].dirs.device
    with torch.no_grad():
        keep = torch.cat([torch.isfinite(c.vps.expand(len(c), 3)).all(dim=1) & torch.isfinite(c.dirs).all(dim=1)
                          & torch.isfinite(c.depth).reshape(-1) for c in seq_clouds])
    x = _posed_points64(seq_clouds, seq_poses, model, keep)
    sd = survey.on_device(dev)
    in_mask = torch.ones((x.shape[0],), dtype=torch.bool, device=dev) if point_mask is None \
        else torch.as_tensor(point_mask, device=dev).to(torch.bool)[keep]
    query = torch.where(in_mask[:, None], x.detach(), torch.full_like(x, float('nan'))).contiguous()
    dist, idx = ops.knn(sd.points, 1, r=float(max_dist), query=query)
    dist, idx = dist[:, 0].contiguous(), idx[:, 0]
    used = (idx >= 0) & in_mask & torch.isfinite(x.detach()).all(dim=1)
    if inlier_ratio < 1.0 and bool(used.any()):
        used = used & (dist <= ops.quantile(dist, inlier_ratio))
    j = idx[used].long()
    d = x[used] - sd.points[j]
    if plane:
        r = (sd.normals[j] * d).sum(dim=-1)
        return (r * r).mean() if squared else r.abs().mean()          # (abs: zero gradient at r = 0, as in the kernel)
    sq = (d * d).sum(dim=-1)
    if squared:
        return sq.mean()
    pos = sq > 0
    return (torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))) * pos).mean()


def _scan_loss(name, target, registry, plan_type, unfused, options, clouds, poses, model, masks, kwargs):
    """The driver of mesh_loss and cloud_loss.  ``target`` = (its name in masks[i], what it is, the attributes it must have);
    ``options(kwargs)`` -> the options of the plan's ops call and of ``unfused``, read once the operands have been checked."""
    short, long, attrs = target
    if not clouds or not clouds[0]:
        raise ValueError('%s needs at least one sequence with one scan' % name)
    if not clouds[0][0].dirs.is_cuda:
        raise RuntimeError('%s: the clouds must live on the GPU (depth_correction_amd has no CPU path)' % name)
    if masks is None or len(masks) != len(clouds):
        raise ValueError('%s needs masks[i] = (%s, point mask or None) for every sequence' % (name, short))
    opts = options(kwargs)
    kind = getattr(model, 'kernel_kind', None) if model is not None else None
    fused = kwargs.get('fused', True) and poses is not None and (model is None or kind)
    loss, loss_cloud = 0., []
    for i, seq in enumerate(clouds):
        tgt, point_mask = masks[i] if isinstance(masks[i], (tuple, list)) else (masks[i], None)
        if tgt is None or not all(hasattr(tgt, a) for a in attrs):
            raise ValueError('%s: sequence %d has no %s (masks[%d] = (%s, point mask))' % (name, i, long, i, short))
        if fused:
            w, e = model.kernel_params() if kind else (None, None)
            plan = _scan_loss_plan(registry, plan_type, seq, tgt, point_mask, bool(kind))
            seq_poses = poses[i] if isinstance(poses[i], torch.Tensor) else torch.stack(list(poses[i]))
            loss_seq = _ScanLossSequence.apply(w, e, seq_poses, plan, kind, tuple(sorted(opts.items())))
        else:
            loss_seq = unfused(seq, None if poses is None else poses[i], model, tgt, point_mask, **opts)
        loss = loss + loss_seq
        loss_cloud.append(_MovedClouds(seq, None if poses is None else poses[i], model, loss))
    return loss / len(clouds), loss_cloud


def mesh_loss(clouds, poses=None, model=None, masks=None, **kwargs):
    """Supervised loss against ground-truth meshes over lists of sequences of scans: the mean distance of the corrected, posed
    points of a sequence to its mesh (``mesh_squared``: the mean squared distance; ``mesh_max_dist``: points farther away are left
    out), averaged over the sequences like icp_loss.  ``masks[i]`` = (mesh.TriangleMesh, bool point mask [N_i] or None) of sequence
    ``i``.  Differentiable to the model's weights and exponents and to the poses; GPU clouds with a kernel model (or none) and
    poses take one dc_mesh_loss call per sequence (``fused=False`` forces the tensor form)."""
    options = lambda kw: dict(squared=bool(kw.get('mesh_squared', False)), max_dist=kw.get('mesh_max_dist'))
    return _scan_loss('mesh_loss', ('mesh', 'ground-truth mesh', ('on_device',)), _mesh_plans, _MeshLossPlan, _unfused_mesh_sequence,
                      options, clouds, poses, model, masks, kwargs)


def _cloud_options(kwargs):
    max_dist = kwargs.get('cloud_max_dist')
    if max_dist is None:
        raise ValueError("cloud_loss needs loss_kwargs['cloud_max_dist'] (metres, finite, > 0)")
    return dict(plane=bool(kwargs.get('cloud_point_to_plane', True)), squared=bool(kwargs.get('cloud_squared', False)),
                max_dist=float(max_dist), inlier_ratio=float(kwargs.get('cloud_inlier_ratio', 1.0)))


def cloud_loss(clouds, poses=None, model=None, masks=None, **kwargs):
    """Supervised loss against surveyed clouds over lists of sequences of scans: the mean distance of the corrected, posed points of
    a sequence to their nearest survey points -- to the planes through them (``cloud_point_to_plane``, default True) or to the points
    themselves; ``cloud_squared`` (False): the mean squared distance; ``cloud_max_dist`` (required): points without a survey point
    within it are left out; ``cloud_inlier_ratio`` (1.0): below 1, points whose nearest-neighbour distance exceeds that quantile of the
    matched distances are left out (the reference's inlier rule, loss.py:440-452) -- averaged over the sequences like icp_loss.
    ``masks[i]`` = (survey.SurveyCloud, bool point mask [N_i] or None) of sequence ``i``.  Differentiable to the model's weights and
    exponents and to the poses, the correspondences held constant; GPU clouds with a kernel model (or none) and poses take one
    dc_cloud_loss call per sequence (``fused=False`` forces the tensor form)."""
    return _scan_loss('cloud_loss', ('survey', 'surveyed cloud', ('on_device', 'normals')), _cloud_plans, _CloudLossPlan,
                      _unfused_cloud_sequence, _cloud_options, clouds, poses, model, masks, kwargs)


# ---- self-supervised loss against the volume the sequence's own scans fuse into ---------------------------------------------------
class TsdfTarget(object):
    """The per-sequence target of tsdf_loss: the sparse TSDF volume (reconstruction.SparseTsdfVolume, voxels of ``voxel_size`` metres,
    truncation ``trunc``, None: three voxels) that the corrected, posed scans of the sequence fuse into, re-fused as the model and the
    poses move.  ``leave_one_out``: every scan is scored against the volume of the OTHER scans, so that it does not pull the map
    towards itself; the volume's sums are integers, so that volume is bit for bit the total minus the volume of the scan alone, and
    S + 1 volumes are fused instead of S volumes of S - 1 scans.  The target counts the evaluations tsdf_loss makes with it and
    re-fuses before evaluation 0 and then before every ``refresh_every``-th (0: never again).  ``min_count``, ``max_blocks``,
    ``min_depth``, ``max_range`` as for SparseTsdfVolume and its integrate.

    A re-fusion reads the host (the pools grow as the scans need them), so an evaluation cannot be captured into a graph: asked to
    evaluate during a stream capture, the target raises unless ``refresh_every`` is 0, and train()'s loop then runs eagerly."""

    def __init__(self, voxel_size, trunc=None, leave_one_out=True, refresh_every=1, min_count=1, max_blocks=None, min_depth=0.,
                 max_range=None):
        self.voxel_size = float(voxel_size)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        if not (self.voxel_size > 0.0 and self.trunc > 0.0 and self.trunc < float('inf') and self.voxel_size < float('inf')):
            raise ValueError('TsdfTarget needs a voxel size and a truncation > 0, got %r and %r' % (voxel_size, trunc))
        self.leave_one_out, self.refresh_every, self.min_count = bool(leave_one_out), int(refresh_every), int(min_count)
        if self.refresh_every < 0 or self.min_count < 1:
            raise ValueError('TsdfTarget needs refresh_every >= 0 and min_count >= 1, got %r and %r' % (refresh_every, min_count))
        self.max_blocks, self.min_depth, self.max_range = max_blocks, float(min_depth), max_range
        self.evaluations = self.refreshes = 0
        self.total = self.tables = self.own = None
        self._scans, self._loo = None, None

    def _volume(self, device):
        from .reconstruction import SparseTsdfVolume
        return SparseTsdfVolume(self.voxel_size, trunc=self.trunc, max_blocks=self.max_blocks, device=device)

    def _fuse(self, scans, device):
        volume = self._volume(device)
        for cloud, pose in scans:
            volume.integrate(cloud, pose=pose, min_depth=self.min_depth, max_range=self.max_range)
        return volume

    def refresh(self, seq_clouds, seq_poses=None, model=None):
        """Re-fuses the target from the scans ``seq_clouds`` (sensor frame) corrected by ``model(cloud)`` as reconstruct does and moved
        by ``seq_poses`` ([4,4] each, None: identity): the total volume and, with leave_one_out, one volume per scan, concatenated
        into one table with one pool.  Nothing of it enters an autograd graph."""
        device = seq_clouds[0].dirs.device
        with torch.no_grad():
            clouds = [model(c) for c in seq_clouds] if model is not None else list(seq_clouds)
            eye = torch.eye(4, dtype=torch.float64)
            poses = [eye if seq_poses is None else seq_poses[i].detach().to(torch.float64).cpu() for i in range(len(clouds))]
            self._scans, self._loo = list(zip(clouds, poses)), None
            self.total = self._fuse(self._scans, device)
            self.tables = self.total.tables()
            self.own = None
            if self.leave_one_out:
                keys, slots, sums, counts, ptr_host = [], [], [], [], [0]
                for scan in self._scans:
                    v = self._fuse([scan], device)
                    nb = v.n_blocks
                    keys.append(v._keys[:nb])
                    slots.append(v._slots[:nb] + ptr_host[-1])        # a volume hands out the slots 0 .. nb - 1: its pool is [:nb]
                    sums.append(v._sum[:nb])
                    counts.append(v._count[:nb])
                    ptr_host.append(ptr_host[-1] + nb)
                if ptr_host[-1] == 0:                                 # no scan wrote a block: a pool of one empty block
                    sums.append(torch.zeros((1, 512), dtype=torch.int64, device=device))
                    counts.append(torch.zeros((1, 512), dtype=torch.int32, device=device))
                self.own = ops.TsdfOwnTables(torch.cat(keys).contiguous(), torch.cat(slots).to(torch.int32).contiguous(),
                                             torch.tensor(ptr_host, dtype=torch.int64, device=device), torch.cat(sums).contiguous(),
                                             torch.cat(counts).contiguous())
        self.refreshes += 1
        return self

    def before_evaluation(self, seq_clouds, seq_poses=None, model=None):
        """Counts one evaluation of tsdf_loss with this target and re-fuses first when it is due.  A stream capture runs nothing and is
        not counted (nor are the replays of the graph it makes, which the host does not see: with refresh_every = 0, the one setting
        that can be captured, the count decides nothing any more)."""
        due = self.total is None or (self.refresh_every > 0 and self.evaluations % self.refresh_every == 0)
        if torch.cuda.is_current_stream_capturing():
            if due or self.refresh_every > 0:
                raise RuntimeError('a TsdfTarget with refresh_every = %d re-fuses between evaluations and cannot be captured into a graph'
                                   % self.refresh_every)
            return
        if due:
            self.refresh(seq_clouds, seq_poses, model)
        self.evaluations += 1

    def leave_one_out_volumes(self):
        """The S volumes of S - 1 scans each, fused explicitly from the scans of the last refresh: what the subtraction stands for,
        and what the tensor form of the loss samples (built on first use after a refresh)."""
        if self._scans is None:
            raise RuntimeError('the target has not been fused yet: call refresh first')
        if self._loo is None:
            device = self.total.device
            self._loo = [self._fuse([sc for j, sc in enumerate(self._scans) if j != s], device) for s in range(len(self._scans))]
        return self._loo


class _TsdfLossPlan(_ScanLossPlan):
    """The target, whose tables are read anew at every call: a refresh replaces them."""
    header, _workspace = 5, staticmethod(ops.tsdf_loss_workspace)

    def __init__(self, seq_clouds, target, point_mask, with_model):
        super().__init__(seq_clouds, point_mask, with_model)
        self.target = target

    def _call(self, poses12, kind, w, e, **opts):
        t = self.target
        return ops.tsdf_loss(t.tables, self.ps, self.scan_ptr, poses12, kind, w, e, mask=self.mask, own=t.own, min_count=t.min_count,
                             **opts)


_tsdf_plans = PlanRegistry()


def _unfused_tsdf_sequence(seq_clouds, seq_poses, model, target, point_mask, squared, max_residual, return_used=False):
    """The same loss from tensor operations: x in fp64 through the model and the poses, the sample (detached) from
    SparseTsdfVolume.sample -- with leave-one-out, of S explicitly fused volumes of the other scans, which checks the subtraction
    independently -- l from phi(x0) + grad . (x - x0), torch autograd.  For models without a kernel kind, and what the fused form is
    tested against."""
    dev = seq_clouds[0].dirs.device
    with torch.no_grad():
        keep = torch.cat([torch.isfinite(c.vps.expand(len(c), 3)).all(dim=1) & torch.isfinite(c.dirs).all(dim=1)
                          & torch.isfinite(c.depth).reshape(-1) for c in seq_clouds])
        scan_of = torch.cat([torch.full((len(c),), s, dtype=torch.int64, device=dev) for s, c in enumerate(seq_clouds)])[keep]
    x = _posed_points64(seq_clouds, seq_poses, model, keep)
    x0 = x.detach().contiguous()
    in_mask = torch.ones((x.shape[0],), dtype=torch.bool, device=dev) if point_mask is None \
        else torch.as_tensor(point_mask, device=dev).to(torch.bool)[keep]
    if target.leave_one_out:
        phi0 = torch.full((x.shape[0],), float('nan'), dtype=torch.float64, device=dev)
        grad = torch.zeros((x.shape[0], 3), dtype=torch.float64, device=dev)
        flag = torch.full((x.shape[0],), 255, dtype=torch.uint8, device=dev)
        for s, volume in enumerate(target.leave_one_out_volumes()):
            rows = torch.nonzero(scan_of == s).reshape(-1)
            if rows.numel():
                smp = volume.sample(x0[rows], min_count=target.min_count)
                phi0[rows], grad[rows], flag[rows] = smp['value'], smp['grad'], smp['flag']
    else:
        smp = target.total.sample(x0, min_count=target.min_count)
        phi0, grad, flag = smp['value'], smp['grad'], smp['flag']
    gate = target.trunc if max_residual is None else float(max_residual)
    used = in_mask & (flag == 0) & (phi0.abs() < gate)
    phi = phi0[used] + (grad[used] * (x[used] - x0[used])).sum(dim=-1)
    loss = (phi * phi).mean() if squared else phi.abs().mean()     # (abs: zero gradient at phi = 0, as in the kernel)
    if return_used:
        full = torch.zeros((keep.shape[0],), dtype=torch.bool, device=dev)
        full[keep] = used
        return loss, full
    return loss


def _tsdf_options(kwargs):
    max_residual = kwargs.get('tsdf_max_residual')
    return dict(squared=bool(kwargs.get('tsdf_squared', True)), max_residual=None if max_residual is None else float(max_residual))


def tsdf_loss(clouds, poses=None, model=None, masks=None, **kwargs):
    """Self-supervised loss against the volume the scans themselves fuse into, over lists of sequences of scans: the mean squared
    (``tsdf_squared``, default True: the sum of phi^2 is what the scan-to-TSDF tracker minimises) or absolute trilinear distance phi
    of the corrected, posed points of a sequence to the surface of its TsdfTarget; ``tsdf_max_residual`` (None: the truncation):
    points with |phi| >= it are left out -- averaged over the sequences like icp_loss.  ``masks[i]`` = (TsdfTarget, bool point mask
    [N_i] or None) of sequence ``i``; the target re-fuses itself inside this call when it is due (TsdfTarget.refresh_every), from
    the clouds, the poses and the model of the call.  Differentiable to the model's weights and exponents and to the poses, the
    volume held constant; GPU clouds with a kernel model (or none) and poses take one dc_tsdf_loss call per sequence
    (``fused=False`` forces the tensor form)."""
    if clouds and clouds[0] and clouds[0][0].dirs.is_cuda and masks is not None and len(masks) == len(clouds):
        for i, seq in enumerate(clouds):
            tgt = masks[i][0] if isinstance(masks[i], (tuple, list)) else masks[i]
            if isinstance(tgt, TsdfTarget):
                tgt.before_evaluation(seq, None if poses is None else poses[i], model)
    return _scan_loss('tsdf_loss', ('TsdfTarget', 'TSDF target', ('before_evaluation', 'tables')), _tsdf_plans, _TsdfLossPlan,
                      _unfused_tsdf_sequence, _tsdf_options, clouds, poses, model, masks, kwargs)


def loss_by_name(name):
    assert name in ('min_eigval_loss', 'trace_loss', 'icp_loss', 'mesh_loss', 'cloud_loss', 'tsdf_loss')
    return globals()[name]


def create_loss(cfg):
    loss = loss_by_name(cfg.loss)

    def loss_fun(*args, **kwargs):
        return loss(*args, **kwargs, **cfg.loss_kwargs)
    loss_fun.name = cfg.loss
    loss_fun.kwargs = cfg.loss_kwargs
    return loss_fun
