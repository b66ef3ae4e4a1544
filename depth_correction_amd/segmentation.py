"""Plane neighbourhoods (segmentation.py:28-276 of the reference): deterministic GPU RANSAC + DBSCAN segmentation and the
per-iteration plane moments with their hand-derived backward (csrc/dc_planes.hip; its header comment is the specification).

The reference gets its planes from PCL (RANSAC with a least-squares refit) and open3d (DBSCAN); both draw random samples, so
this module restates them deterministically: the same seed gives bit-identical planes.  Deviations: every one of the
``max_iterations`` hypotheses is scored (PCL stops early once its confidence is reached), and a border point of DBSCAN joins
the smallest-labelled core cluster next to it (open3d: whichever cluster's breadth-first search reaches it first).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._native import MODEL_KINDS, check, dtype_code, lib, need, on_device, ptr, stream_ptr

__all__ = ['Planes', 'fit_planes', 'plane_landscape', 'plane_moments', 'ransac_sample', 'splitmix64', 'DBSCAN_MIN_POINTS']

DBSCAN_MIN_POINTS = 10          # cluster_open3d ignores its min_points argument (segmentation.py:166-177)
_M64 = (1 << 64) - 1


def splitmix64(x):
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def ransac_sample(seed, m, h, n_remaining):
    """(j0, j1, j2): positions in the remaining-point list that hypothesis ``h`` of RANSAC round ``m`` draws (dc_planes.hip)."""
    s = int(seed) & _M64
    return tuple(splitmix64(s ^ ((int(m) << 40) & _M64) ^ (int(h) << 2) ^ t) % int(n_remaining) for t in range(3))


class Planes(object):
    """Plane neighbourhoods of a global cloud (segmentation.py:100-123): ``params`` [P,4] (n, d with n.x + d = 0), ``indices``
    (P int64 tensors of ascending point indices), ``cloud`` (P references to the segmented points); after
    compute_neighborhood_features also ``cov`` [P,3,3] and ``eigvals`` [P,3].  ``plane_cloud`` (the per-plane corrected clouds)
    is built on first access."""

    def __init__(self, params, cloud=None, indices=None, cov=None, eigvals=None):
        self.params = torch.as_tensor(params).reshape((-1, 4))
        self.cloud = list(cloud) if cloud is not None else len(self.params) * [None]
        self.indices = list(indices) if indices is not None else []
        assert len(self.indices) == len(self.params)
        self.cov, self.eigvals, self.loss, self.mask = cov, eigvals, None, None
        self._plane_cloud, self._plane_cloud_fn = None, None
        self._csr = None

    def __len__(self):
        return len(self.params)

    def size(self):
        return len(self)

    def copy(self):
        out = Planes(self.params, cloud=self.cloud, indices=self.indices, cov=self.cov, eigvals=self.eigvals)
        out._csr = self._csr
        return out

    def __getitem__(self, item):
        """A subset of the planes (boolean mask or indices), as the loss's inlier gating takes it."""
        sel = torch.as_tensor(item, device=self.params.device)
        sel = torch.nonzero(sel).reshape(-1) if sel.dtype == torch.bool else sel.reshape(-1).long()
        keep = sel.tolist()
        out = Planes(self.params[sel], cloud=[self.cloud[i] for i in keep], indices=[self.indices[i] for i in keep],
                     cov=None if self.cov is None else self.cov[sel], eigvals=None if self.eigvals is None else self.eigvals[sel])
        return out

    def distance(self, x):
        """Signed distances [N,P] of points [N,3] (or a DepthCloud's points) to every plane."""
        from .depth_cloud import DepthCloud
        if isinstance(x, DepthCloud):
            x = x.get_points()
        x = torch.as_tensor(x)
        p = self.params.to(device=x.device, dtype=x.dtype)
        return (x @ p[:, :3].t() + p[:, 3]).squeeze()

    def orient(self, x):
        """The planes flipped when the viewpoints ``x`` lie on their negative side on average (segmentation.py:115-122)."""
        from .depth_cloud import DepthCloud
        if isinstance(x, DepthCloud):
            x = x.vps
        flip = torch.sign(self.distance(x)).mean() < 0.0
        return Planes(-self.params if flip else self.params, cloud=self.cloud, indices=self.indices)

    @property
    def plane_cloud(self):
        if self._plane_cloud is None and self._plane_cloud_fn is not None:
            self._plane_cloud = self._plane_cloud_fn()
        return self._plane_cloud

    @plane_cloud.setter
    def plane_cloud(self, value):
        self._plane_cloud = value

    def csr(self, device):
        """(plane_ptr int32 [P+1], idx int32 [M], work split) on ``device``; built once per Planes object."""
        if self._csr is None or self._csr.ptr.device != torch.device(device):
            self._csr = _PlaneCSR(self.indices, device)
        return self._csr

    def eval_landscape(self, cloud, model_kind, weights, exponent, out, loss='min_eigval_loss', normalization=False, sqrt=False,
                       mask=None):
        """The plane loss for every weight row in one pass over the plane points (plane_landscape)."""
        return plane_landscape(cloud, self, model_kind, weights, exponent, out, loss=loss, normalization=normalization, sqrt=sqrt,
                               mask=mask)

    @staticmethod
    def fit(x, distance_threshold, min_support=3, max_iterations=1000, max_models=10, eps=None, seed=0, **kwargs):
        return fit_planes(x, distance_threshold, min_support=min_support, max_iterations=max_iterations,
                          max_models=max_models, eps=eps, seed=seed)


def _signed64(v):
    v = int(v) & _M64
    return v - (1 << 64) if v >= (1 << 63) else v


# ---- segmentation ---------------------------------------------------------------------------------------------------
@on_device
def _ransac_round(x, rem, seed, m, H, thresh, bufs):
    """(best h, its count) of one RANSAC round over the remaining rows ``rem``; the hypotheses stay in ``bufs``."""
    n = rem.shape[0]
    check(lib().dc_ransac_score(ptr(x), dtype_code(x), ptr(rem), n, _signed64(seed),
                                int(m), int(H), float(thresh), ptr(bufs['hyp']), ptr(bufs['anchor']), ptr(bufs['valid']),
                                ptr(bufs['counts']), ptr(bufs['best']), stream_ptr()), 'dc_ransac_score')
    h, c = bufs['best'].tolist()
    return h, c


@on_device
def _refit(x, rem, thresh, bufs):
    """(refined params double [4], support mask uint8 [n_rem]) of the round's winner."""
    n = rem.shape[0]
    npart = lib().dc_ransac_refit_partial_count(n)
    partials = torch.empty((npart, 10), dtype=torch.float64, device=x.device)
    params = torch.empty((4,), dtype=torch.float64, device=x.device)
    mask = torch.empty((n,), dtype=torch.uint8, device=x.device)
    check(lib().dc_ransac_refit(ptr(x), dtype_code(x), ptr(rem), n, ptr(bufs['hyp']), ptr(bufs['anchor']), ptr(bufs['best']),
                                float(thresh), ptr(partials), npart, ptr(params), ptr(mask), stream_ptr()), 'dc_ransac_refit')
    return params, mask


@on_device
def dbscan(points, eps, min_points=DBSCAN_MIN_POINTS):
    """(labels int32 [m], best label, its size) of DBSCAN on ``points`` [m,3] with the radius grid's neighbourhoods."""
    m = points.shape[0]
    if m == 0:
        return torch.empty((0,), dtype=torch.int32, device=points.device), -1, 0
    nbr = ops.radius_neighbors(points.contiguous(), float(eps))
    dev = points.device
    core = torch.empty((m,), dtype=torch.uint8, device=dev)
    lab = torch.empty((m,), dtype=torch.int32, device=dev)
    labels = torch.empty((m,), dtype=torch.int32, device=dev)
    sizes = torch.empty((m,), dtype=torch.int32, device=dev)
    flag = torch.empty((1,), dtype=torch.int32, device=dev)
    best = torch.empty((2,), dtype=torch.int32, device=dev)
    check(lib().dc_dbscan(ptr(nbr), m, nbr.shape[1], int(min_points), ptr(core), ptr(lab), ptr(labels), ptr(sizes), ptr(flag),
                          ptr(best), stream_ptr()), 'dc_dbscan')
    lbl, size = best.tolist()
    return labels, lbl, size


def _compact(mask, fields, want_index=False):
    return ops.compact_rows(mask.to(torch.bool).contiguous(), fields, want_index=want_index)


def fit_planes(x, distance_threshold, min_support=3, max_iterations=1000, max_models=10, eps=None, seed=0, verbose=0):
    """Planes of the points ``x`` ([N,3] device tensor or DepthCloud): the loop of segmentation.py:194-276 on the host, each
    round's RANSAC, refit and DBSCAN on the GPU.  Rounds are numbered from 0 and every RANSAC call counts as one."""
    from .depth_cloud import DepthCloud
    src = x
    if isinstance(x, DepthCloud):
        x = x.to_points()
    x = torch.as_tensor(x)
    if not x.is_cuda:
        raise RuntimeError('plane segmentation needs a GPU: the points are on %s (depth_correction_amd has no CPU path)' % x.device)
    x = need(x.detach().contiguous(), (None, 3), name='points')
    assert distance_threshold >= 0.0 and max_iterations > 0
    if max_iterations > 1024:
        raise ValueError('at most 1024 RANSAC hypotheses per round, got %d' % max_iterations)
    dev = x.device
    H = int(max_iterations)
    bufs = dict(hyp=torch.empty((H, 4), dtype=torch.float64, device=dev), anchor=torch.empty((H, 3), dtype=torch.float64, device=dev),
                valid=torch.empty((H,), dtype=torch.int32, device=dev), counts=torch.empty((H,), dtype=torch.int32, device=dev),
                best=torch.empty((2,), dtype=torch.int32, device=dev))
    rem = torch.arange(x.shape[0], dtype=torch.int32, device=dev)
    params, indices = [], []
    m = 0
    while rem.shape[0] >= 3:
        h, count = _ransac_round(x, rem, seed, m, H, distance_threshold, bufs)
        m += 1
        if count < min_support:
            if verbose:
                print('Halt due to insufficient plane support.')
            break
        plane, mask = _refit(x, rem, distance_threshold, bufs)
        (support,), support_pos = _compact(mask, [rem], want_index=True)
        if len(support) < min_support:
            break
        keep = support
        keep_pos = support_pos
        if eps:
            labels, lbl, size = dbscan(ops.gather_rows(x, support.long()), eps)
            if size < min_support:
                # no cluster with enough support: the whole support leaves the remaining points (segmentation.py:222-235)
                (rem,) = _compact(mask == 0, [rem])
                if rem.shape[0] < min_support:
                    break
                continue
            (keep, keep_pos) = _compact(labels == lbl, [support, support_pos])
        params.append(plane)
        indices.append(keep.long())
        if max_models is not None and len(params) == max_models:
            break
        left = torch.ones((rem.shape[0],), dtype=torch.bool, device=dev)
        left[keep_pos.long()] = False
        (rem,) = _compact(left, [rem])
        if rem.shape[0] < min_support:
            break
    if verbose:
        print('%i planes with minimum support of %i points were found.' % (len(params), min_support))
    P = torch.stack(params) if params else torch.empty((0, 4), dtype=torch.float64, device=dev)
    return Planes(P, cloud=len(params) * [src], indices=indices)


# ---- per-iteration plane moments ---------------------------------------------------------------------------------------
class _PlaneCSR(object):
    """Concatenated plane indices and the work split of dc_plane_moments_fwd / _bwd (blocks of CHUNK entries of one plane)."""
    CHUNK = 2048

    def __init__(self, indices, device):
        device = torch.device(device)
        sizes = [int(len(i)) for i in indices]
        self.n_planes = len(sizes)
        if min(sizes, default=1) < 1:
            # the kernels anchor a plane's moments at its first point: idx[ptr[p]] must exist
            raise ValueError('plane %d has no indices' % sizes.index(0))
        self.ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=device)
        self.idx = (torch.cat([torch.as_tensor(i, device=device) for i in indices]) if sizes else
                    torch.empty((0,), dtype=torch.int64, device=device)).to(torch.int32).contiguous()
        if len(self.idx) and int(torch.bincount(self.idx.long()).max()) > 1:
            raise ValueError('plane neighbourhoods must not share points')
        blk_plane, blk_begin, plane_blk = [], [], [0]
        start = 0
        for p, s in enumerate(sizes):
            nb = max(1, (s + self.CHUNK - 1) // self.CHUNK)
            blk_plane += nb * [p]
            blk_begin += [start + b * self.CHUNK for b in range(nb)]
            plane_blk.append(plane_blk[-1] + nb)
            start += s
        self.n_blocks = len(blk_plane)
        self.blk_plane = torch.tensor(blk_plane, dtype=torch.int32, device=device)
        self.blk_begin = torch.tensor(blk_begin, dtype=torch.int32, device=device)
        self.plane_blk = torch.tensor(plane_blk, dtype=torch.int32, device=device)
        self.sizes = sizes
        self.device = device


def _model_args(kind, w, e, device):
    code = MODEL_KINDS[kind]
    if code == 0:
        return 0, 0, None, None
    wv = w.detach().reshape(-1).to(device=device, dtype=torch.float64).contiguous()
    ev = (torch.zeros_like(wv) if e is None else e.detach().reshape(-1).to(device=device, dtype=torch.float64)).contiguous()
    return code, wv.numel(), wv, ev


class _PlaneMoments(torch.autograd.Function):
    """(vps [N,3], dirs [N,3], depth [N,1], w [1,P] | None) -> cov double [P,3,3] of the corrected points of every plane."""

    @staticmethod
    @on_device
    def forward(ctx, vps, dirs, depth, w, e, normals, csr, kind):
        dev = dirs.device
        vps, dirs, depth = (t.detach().contiguous() for t in (vps, dirs, depth))
        code, nt, wv, ev = _model_args(kind, w, e, dev)
        P = csr.n_planes
        nrm = normals.detach().to(device=dev, dtype=torch.float64).contiguous()
        partials = torch.empty((max(csr.n_blocks, 1), 9), dtype=torch.float64, device=dev)
        cov = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
        mean = torch.empty((P, 3), dtype=torch.float64, device=dev)
        check(lib().dc_plane_moments_fwd(ptr(vps), ptr(dirs), ptr(depth), dtype_code(dirs), ptr(csr.idx), ptr(csr.ptr), ptr(nrm), P,
                                         ptr(csr.blk_plane), ptr(csr.blk_begin), ptr(csr.plane_blk), csr.n_blocks, csr.CHUNK, code, nt,
                                         ptr(wv), ptr(ev), ptr(partials), ptr(cov), ptr(mean), stream_ptr()), 'dc_plane_moments_fwd')
        ctx.save_for_backward(vps, dirs, depth, nrm, mean)
        ctx.meta = (csr, code, nt, wv, ev, None if w is None else (w.shape, w.dtype))
        return cov

    @staticmethod
    @on_device
    def backward(ctx, g):
        vps, dirs, depth, nrm, mean = ctx.saved_tensors
        csr, code, nt, wv, ev, wmeta = ctx.meta
        dev = dirs.device
        gcov = g.detach().to(torch.float64).contiguous()
        g_vps, g_dirs, g_depth = torch.zeros_like(vps), torch.zeros_like(dirs), torch.zeros_like(depth)
        wpart = torch.empty((max(csr.n_blocks * nt, 1),), dtype=torch.float64, device=dev)
        gw = torch.empty((max(nt, 1),), dtype=torch.float64, device=dev)
        check(lib().dc_plane_moments_bwd(ptr(vps), ptr(dirs), ptr(depth), dtype_code(dirs), ptr(csr.idx), ptr(csr.ptr), ptr(nrm),
                                         csr.n_planes, ptr(csr.blk_plane), ptr(csr.blk_begin), csr.n_blocks, csr.CHUNK, code, nt,
                                         ptr(wv), ptr(ev), ptr(mean), ptr(gcov), ptr(g_vps), ptr(g_dirs), ptr(g_depth),
                                         ptr(wpart) if nt else None, ptr(gw) if nt else None, stream_ptr()), 'dc_plane_moments_bwd')
        g_w = gw[:nt].reshape(wmeta[0]).to(wmeta[1]) if (wmeta is not None and ctx.needs_input_grad[3]) else None
        return g_vps, g_dirs, g_depth, g_w, None, None, None, None


def plane_moments(cloud, planes, model=None):
    """cov [P,3,3] of every plane of ``planes`` in the global ``cloud`` (not corrected yet) after ``model``
    (preproc.py:218-243), differentiable to the cloud's vps / dirs / depth and the model's weights.  Models with a
    ``kernel_kind`` run inside the kernel; any other model is applied by its tensor expression to the plane points first."""
    n = len(cloud)
    dirs = cloud.dirs
    if not dirs.is_cuda:
        raise RuntimeError('plane features need a GPU: the cloud is on %s (depth_correction_amd has no CPU path)' % dirs.device)
    vps = cloud.vps.expand(n, 3) if cloud.vps.dim() == 2 else cloud.vps
    depth = cloud.depth.reshape(n, 1)
    csr = planes.csr(dirs.device)
    normals = planes.params[:, :3].to(dirs.device)
    kind = getattr(model, 'kernel_kind', None) if model is not None else None
    if model is not None and kind is not None:
        w, e = model.kernel_params()
        if isinstance(e, torch.Tensor) and e.requires_grad:
            kind = None                              # learnable exponents: the tensor path carries their gradient
    if model is None or kind is not None:
        w, e = (model.kernel_params() if model is not None else (None, None))
        cov = _PlaneMoments.apply(vps, dirs, depth, w, e, normals, csr, kind)
        return cov if model is not None else cov.to(dirs.dtype)     # the reference's dtype: float64 weights promote the points
    # tensor path: the plane points with their incidence angles, the model's own expression, then the moments (no model)
    from .depth_cloud import DepthCloud
    idx = csr.idx.long()
    plane_of = torch.repeat_interleave(torch.arange(csr.n_planes, device=dirs.device),
                                       torch.as_tensor(csr.sizes, device=dirs.device))
    sub = DepthCloud(vps[idx], dirs[idx], depth[idx])
    sub.normals = normals.to(dirs.dtype)[plane_of]
    sub.update_incidence_angles()
    sub = model(sub)
    dt = torch.promote_types(dirs.dtype, sub.depth.dtype)
    local = Planes(planes.params, indices=[torch.arange(a, b, device=dirs.device) for a, b in
                                           zip(csr.ptr[:-1].tolist(), csr.ptr[1:].tolist())])
    cov = _PlaneMoments.apply(sub.vps.to(dt).contiguous(), sub.dirs.to(dt).contiguous(), sub.depth.reshape(-1, 1).to(dt).contiguous(),
                              None, None, normals, local.csr(dirs.device), None)
    return cov.to(dt)


PLANE_LANDSCAPE_KINDS = ('Polynomial', 'ScaledPolynomial')


@on_device
def plane_landscape(cloud, planes, model_kind, weights, exponent, out, loss='min_eigval_loss', normalization=False, sqrt=False,
                    mask=None):
    """Plane loss of the global ``cloud`` (not corrected yet) for every row of ``weights`` fp64 device [W, P] (P in {1, 2}) of a
    Polynomial / ScaledPolynomial model with ``exponent`` fp64 [P] (dc_plane_landscape): the plane features of
    compute_neighborhood_features and min_eigval_loss / trace_loss over the planes (every plane one entry; ``mask`` bool [planes]:
    the planes that count).  out fp64 device [W, 2] <- (sum of the loss over the planes, their number)."""
    n = len(cloud)
    dirs = cloud.dirs
    if not dirs.is_cuda:
        raise RuntimeError('plane features need a GPU: the cloud is on %s (depth_correction_amd has no CPU path)' % dirs.device)
    if model_kind not in PLANE_LANDSCAPE_KINDS:
        raise ValueError('the plane landscape takes %s models, not %s' % (' / '.join(PLANE_LANDSCAPE_KINDS), model_kind))
    dev = dirs.device
    nw, nt = weights.shape
    need(weights, (nw, nt), dtype=torch.float64, name='weights', device=dev)
    need(out, (nw, 2), dtype=torch.float64, name='out', device=dev)
    ev = exponent.detach().reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    need(ev, (nt,), dtype=torch.float64, name='exponent', device=dev)
    vps = (cloud.vps.expand(n, 3) if cloud.vps.dim() == 2 else cloud.vps).detach().contiguous()
    dirs = dirs.detach().contiguous()
    depth = cloud.depth.reshape(n).detach().contiguous()
    csr = planes.csr(dev)
    nrm = planes.params[:, :3].detach().to(device=dev, dtype=torch.float64).contiguous()
    m8 = None
    if mask is not None:
        m8 = torch.as_tensor(mask, device=dev).to(torch.bool).contiguous()
        need(m8, (csr.n_planes,), dtype=torch.bool, name='mask', device=dev)
        m8 = m8.view(torch.uint8)
    count = lib().dc_plane_landscape_partials_count(csr.n_blocks, nt)
    if count < 0:
        raise ValueError('the plane landscape takes 1 or 2 weights, not %d' % nt)
    partials = torch.empty((count,), dtype=torch.float64, device=dev)
    pm = torch.empty((max(csr.n_planes, 1) * (count // max(csr.n_blocks, 1)),), dtype=torch.float64, device=dev)
    check(lib().dc_plane_landscape(ptr(vps), ptr(dirs), ptr(depth), dtype_code(dirs), ptr(csr.idx), ptr(csr.ptr), ptr(nrm), csr.n_planes,
                                   ptr(csr.blk_plane), ptr(csr.blk_begin), ptr(csr.plane_blk), csr.n_blocks, csr.CHUNK,
                                   MODEL_KINDS[model_kind], nt, ptr(ev), ptr(m8), ptr(weights), nw,
                                   {'min_eigval_loss': 0, 'trace_loss': 1}[loss], int(normalization), int(sqrt), ptr(partials),
                                   partials.numel(), ptr(pm), ptr(out), stream_ptr()), 'dc_plane_landscape')
    return out
