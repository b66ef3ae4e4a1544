"""Operator layer: one Python function per C-ABI entry point (include/dc_hip.h), torch tensors in and out.

No autograd here (see ``autograd.py``) and no CPU implementation: every function requires GPU tensors
and the HIP library.  Shapes follow the reference's tensors (``[N,3]`` points, ``[N,K]`` neighbours ...).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native as nv
from ._native import lib, check, need, ptr, stream_ptr, dtype_code, on_device

__all__ = [
    'knn', 'radius_neighbors', 'knn_transpose', 'BlockTable', 'block_table', 'table_to_csr', 'spatial_order', 'points_fwd', 'points_bwd', 'features_fwd',
    'features_bwd', 'consistency_fwd', 'consistency_bwd', 'mask_bounds', 'valid_count', 'dispersion', 'p2plane_pair', 'p2point_pair',
    'IcpSequence', 'shadow_mask', 'shadow_filter', 'correct_depth', 'cloud_from_points', 'mask_bounds_all', 'compact_rows', 'to_points', 'valid_weights', 'scan_prefilter',
    'as_index32', 'scan_ids', 'points_extent', 'gather_rows', 'cat_rows', 'bvh_build', 'raycast', 'raycast_rays', 'beam_subrays', 'raycast_beams', 'bias_accumulate', 'bias_out_count', 'mesh_closest', 'mesh_sample', 'mesh_loss', 'mesh_loss_workspace', 'cloud_loss', 'cloud_loss_workspace',
    'KnnGrid', 'knn_grid_build', 'knn_grid_query', 'quantile', 'icp_blocks', 'icp_init', 'icp_accumulate', 'icp_finish', 'map_select',
    'dyn_directions', 'dyn_update', 'align_blocks', 'align_init', 'align_accumulate', 'align_finish', 'survey_align',
    'survey_align_workspace', 'pair_histograms', 'feature_nn', 'feature_nn_tile', 'greg_fit', 'greg_score', 'planereg_triples', 'planereg_count', 'planereg_fill',
    'planereg_hypotheses', 'planereg_select', 'tsdf_k_steps', 'tsdf_integrate', 'tsdf_extract',
    'tsdf_sparse_allocate', 'tsdf_sparse_integrate', 'tsdf_sparse_extract', 'tsdf_sparse_sample', 'tsdf_icp_accumulate',
    'TsdfTables', 'TsdfOwnTables', 'tsdf_loss', 'tsdf_loss_workspace', 'tsdf_sparse_cast_rays',
    'compact_rows_device', 'range_project', 'range_organize', 'range_from_grid', 'range_index_image', 'image_features_fwd', 'image_shadow_mask',
]


def _ws(nbytes, device):
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def _out_arg(out, count, device):
    """``out`` f64 [count]: the caller's, checked, or a new one."""
    if out is None:
        return torch.empty((count,), dtype=torch.float64, device=device)
    return need(out, (count,), dtype=torch.float64, name='out', device=device)


def _ws_arg(ws, nbytes, device):
    """``ws`` uint8 of at least nbytes: the caller's, checked, or a new one."""
    if ws is None:
        return _ws(nbytes, device)
    need(ws, (None,), dtype=torch.uint8, name='ws', device=device)
    if ws.shape[0] < nbytes:
        raise ValueError('workspace of %d bytes, %d needed' % (ws.shape[0], nbytes))
    return ws


def as_index32(neighbors):
    """Reference neighbour tensors are int64 (nearest_neighbors.py:78); the kernels take int32."""
    if neighbors.dtype == torch.int32:
        return neighbors.contiguous()
    assert neighbors.dtype == torch.int64
    return neighbors.to(torch.int32).contiguous()


# ------------------------------------------------------------------------------------------------
# neighbourhood builder
# ------------------------------------------------------------------------------------------------
@on_device
def knn(points, k, r=None, query=None, cell_hint=0.0, want_dist=True, want_index64=False):
    """k-NN of ``query`` (default: ``points`` itself) in ``points``: (dist f64 [M,k] | None, idx i32 [M,k]); with
    ``want_index64`` a third result, the same table as int64 written by the same kernels (dc_knn_build_i64)."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    if not (1 <= k <= 64):
        raise ValueError('k must be in 1..64, got %r' % (k,))
    if query is not None:
        need(query, (None, 3), dtype=points.dtype, name='query', device=points.device)
    m = n if query is None else query.shape[0]
    idx = torch.empty((m, k), dtype=torch.int32, device=points.device)
    # (the kernels write every entry of both tables -- inf beside a missing neighbour --; only the empty cloud needs the fill)
    dist = (torch.empty if n else torch.full)((m, k), *(() if n else (float('inf'),)), dtype=torch.float64, device=points.device) if want_dist else None
    if n == 0:
        idx.fill_(-1)
        return (dist, idx, idx.long()) if want_index64 else (dist, idx)
    idx64 = torch.empty((m, k), dtype=torch.int64, device=points.device) if want_index64 else None
    nbytes = lib().dc_knn_workspace_bytes(n, 0 if query is None else m)
    ws = _ws(nbytes, points.device)
    check(lib().dc_knn_build_i64(ptr(points), 3, dtype_code(points), n, ptr(query), 3, 0 if query is None else m, k,
                                 float(r) if r else 0.0, float(cell_hint), ptr(idx), ptr(idx64), ptr(dist), ptr(ws), nbytes,
                                 stream_ptr()), 'dc_knn_build_i64')
    return (dist, idx, idx64) if want_index64 else (dist, idx)


@on_device
def nn1_corr(dist, idx, ratio):
    """(mask bool [n], idx[mask] int32 [m], threshold fp64 0-dim): the inlier correspondences of a scan pair from the 1-NN distances
    (dc_nn1_corr: np.quantile by a radix select on the device, train.py:186-193).  One synchronisation: the survivors' count."""
    need(dist, (None,), dtype=torch.float64, name='dist')
    n = dist.shape[0]
    need(idx, (n,), dtype=torch.int32, name='idx', device=dist.device)
    mask = torch.empty((n,), dtype=torch.uint8, device=dist.device)
    out = torch.empty((max(n, 1),), dtype=torch.int32, device=dist.device)
    count = torch.zeros((1,), dtype=torch.int64, device=dist.device)
    th = torch.empty((1,), dtype=torch.float64, device=dist.device)
    nbytes = lib().dc_nn1_corr_workspace_bytes(n)
    ws = _ws(nbytes, dist.device)
    check(lib().dc_nn1_corr(ptr(dist), ptr(idx), n, float(ratio), ptr(mask), ptr(out), ptr(count), ptr(th), ptr(ws), nbytes, stream_ptr()),
          'dc_nn1_corr')
    return mask.view(torch.bool), out[:int(count.item())], th[0]


@on_device
def gather_rows(src, order):
    """src[order] for a contiguous per-point array [n, ...] and an int64 permutation (dc_gather_rows: one kernel family for every
    dtype and row shape)."""
    row_bytes = src.element_size() * (src[0].numel() if src.shape[0] else 1)
    if not (src.is_contiguous() and order.dtype == torch.int64 and order.is_contiguous() and (row_bytes == 1 or row_bytes % 4 == 0)):
        return src[order].contiguous()
    out = torch.empty((order.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(lib().dc_gather_rows(ptr(src), row_bytes, ptr(order), order.shape[0], ptr(out), stream_ptr()), 'dc_gather_rows')
    return out


def cat_rows(parts):
    """torch.cat(parts) -- without a copy when the parts are consecutive row ranges of ONE contiguous allocation (the clouds of
    pipeline.local_features_batch are slices of the arrays it built for all scans at once): a view over all of them."""
    parts = list(parts)
    first = parts[0]
    if len(parts) > 1 and first.dim() >= 1 and all(p.is_contiguous() and p.dtype == first.dtype and p.device == first.device
                                                   and p.shape[1:] == first.shape[1:] for p in parts):
        row = first.element_size() * (first[0].numel() if first.shape[0] else 0)
        store = first.untyped_storage().data_ptr()
        at, ok = first.data_ptr(), row > 0
        for p_ in parts:
            ok = ok and p_.untyped_storage().data_ptr() == store and p_.data_ptr() == at
            at += p_.shape[0] * row
        if ok:
            n = sum(p_.shape[0] for p_ in parts)
            return torch.as_strided(first, (n,) + tuple(first.shape[1:]), first.stride())
    return torch.cat(parts).contiguous()


def scan_ids(sizes, device):
    """int32 [sum(sizes)]: the scan of every row of scans concatenated in order (torch.repeat_interleave(arange(S), sizes) in one
    small launch: dc_scan_ids)."""
    import numpy as _np
    n = int(sum(sizes))
    out = torch.empty((n,), dtype=torch.int32, device=device)
    if n == 0:
        return out
    scan_ptr = torch.as_tensor(_np.concatenate([[0], _np.cumsum(sizes)]).astype(_np.int64), device=device)
    with torch.cuda.device(out.device):
        check(lib().dc_scan_ids(ptr(scan_ptr), len(sizes), n, ptr(out), stream_ptr()), 'dc_scan_ids')
    return out


@on_device
def points_extent(points):
    """(lo, hi): per-axis minimum and maximum of a cloud [n, 3 | 4] (float32 / float64) as Python lists -- ONE synchronisation
    (dc_points_extent; the extent the q32 point format is sized for)."""
    need(points, (None, None), name='points')
    n, stride = points.shape
    if n == 0:
        return [float('inf')] * 3, [float('-inf')] * 3
    out = torch.empty((6,), dtype=torch.float64, device=points.device)
    nbytes = lib().dc_points_extent_workspace_bytes()
    check(lib().dc_points_extent(ptr(points), stride, dtype_code(points), n, ptr(out), ptr(_ws(nbytes, points.device)), nbytes,
                                 stream_ptr()), 'dc_points_extent')
    v = out.tolist()
    return v[:3], v[3:]


@on_device
def radius_neighbors(points, r, query=None):
    """All neighbours within ``r`` (inclusive) of every point -- or of every row of ``query``, another cloud -- ascending
    index, padded with -1: idx i32 [N | M, Kmax]."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    if query is not None:
        need(query, (None, 3), dtype=points.dtype, name='query', device=points.device)
        m = query.shape[0]
        if m == 0:
            return torch.empty((0, 0), dtype=torch.int32, device=points.device)
        nbytes = lib().dc_knn_workspace_bytes(n, m)
        ws = _ws(nbytes, points.device)
        count = torch.empty((m,), dtype=torch.int32, device=points.device)
        kmax = torch.zeros((1,), dtype=torch.int32, device=points.device)
        check(lib().dc_radius_count_query(ptr(points), 3, dtype_code(points), n, ptr(query), 3, m, float(r), ptr(count), ptr(kmax),
                                          ptr(ws), nbytes, stream_ptr()), 'dc_radius_count_query')
        km = max(int(kmax.item()), 1)
        if m * km * 4 > (16 << 30):
            raise MemoryError('radius neighbourhoods too dense for a padded [M, Kmax] table (%d x %d)' % (m, km))
        idx = torch.empty((m, km), dtype=torch.int32, device=points.device)
        check(lib().dc_radius_fill_query(n, m, float(r), km, ptr(idx), ptr(ws), nbytes, stream_ptr()), 'dc_radius_fill_query')
        return idx
    if n == 0:
        return torch.empty((0, 0), dtype=torch.int32, device=points.device)
    nbytes = lib().dc_knn_workspace_bytes(n, 0)
    ws = _ws(nbytes, points.device)
    count = torch.empty((n,), dtype=torch.int32, device=points.device)
    kmax = torch.zeros((1,), dtype=torch.int32, device=points.device)
    check(lib().dc_radius_count(ptr(points), 3, dtype_code(points), n, float(r), ptr(count), ptr(kmax), ptr(ws), nbytes,
                                stream_ptr()), 'dc_radius_count')
    km = int(kmax.item())            # set-up phase: the padded width is needed on the host
    if n * max(km, 1) * 4 > (16 << 30):
        raise MemoryError('radius neighbourhoods too dense: %d points x %d neighbours do not fit a padded [N, Kmax] table; '
                          'voxel-filter the cloud first (cfg.grid_res) as the reference pipeline does' % (n, km))
    idx = torch.empty((n, max(km, 1)), dtype=torch.int32, device=points.device)
    check(lib().dc_radius_fill(n, float(r), max(km, 1), ptr(idx), ptr(ws), nbytes, stream_ptr()), 'dc_radius_fill')
    return idx


@on_device
def knn_transpose(nbr, n_dst=None):
    """(csr_ptr i32 [n_dst+1], csr_src i32 [rows*K]) -- for every point the rows whose neighbourhood contains it.
    ``n_dst`` (default: the number of rows) is the number of points the indices refer to."""
    need(nbr, (None, None), dtype=torch.int32, name='neighbors')
    n, k = nbr.shape
    n_dst = n if n_dst is None else int(n_dst)
    csr_ptr = torch.empty((n_dst + 1,), dtype=torch.int32, device=nbr.device)
    csr_src = torch.empty((max(n * k, 1),), dtype=torch.int32, device=nbr.device)
    nbytes = lib().dc_knn_transpose_workspace_bytes(n, k)
    ws = _ws(nbytes, nbr.device)
    check(lib().dc_knn_transpose(ptr(nbr), n, k, n_dst, ptr(csr_ptr), ptr(csr_src), ptr(ws), nbytes, stream_ptr()),
          'dc_knn_transpose')
    return csr_ptr, csr_src


class BlockTable:
    """Block table of a reference list (dcBlockTable): per block of 256 rows the distinct rows it references and the
    16-bit LDS positions (16 x index in that list) of every reference -- slot-major (``slot_ptr``; the forward's
    [rows, K] table) or as per-row runs padded to four (``run_ptr``; the backward's incoming-edge lists).  Lets the
    fused kernels gather from LDS."""

    def __init__(self, blk_ptr, blk_ids, slot_ptr, loc, max_rows, n_rows, run_ptr=None, own_base=None, packed=0, row_ptr=None):
        self.blk_ptr, self.blk_ids, self.slot_ptr, self.loc, self.run_ptr = blk_ptr, blk_ids, slot_ptr, loc, run_ptr
        self.own_base, self.packed, self.row_ptr = own_base, int(packed), row_ptr
        self.max_rows, self.n_rows = int(max_rows), int(n_rows)
        self.layout = nv.DC_TABLE_SLOTS if run_ptr is None else nv.DC_TABLE_RUNS
        self.device = blk_ptr.device
        self.desc = nv.BlockTableDesc(ptr(blk_ptr), ptr(blk_ids), ptr(slot_ptr), ptr(loc), self.max_rows, self.layout, ptr(run_ptr),
                                      ptr(own_base), self.packed, 0, ptr(row_ptr))

    def ref(self):
        return ctypes.cast(ctypes.pointer(self.desc), ctypes.c_void_p)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.blk_ptr, self.blk_ids, self.slot_ptr, self.loc, self.run_ptr)
                   if t is not None)


def _table_ref(table, n_rows):
    if table is None:
        return None
    assert isinstance(table, BlockTable) and table.n_rows == n_rows, 'block table built for another row count'
    return table.ref()


@on_device
def block_table(nbr=None, csr=None, layout=None, own_rows=True):
    """BlockTable of a neighbour table ``nbr`` int32 [rows, K] (forward; slot-major) or of CSR lists ``csr`` = (ptr, ids)
    (backward: knn_transpose's output; ``layout`` 'runs' (default) or 'slots').  ``own_rows``: the table's rows and ids
    are the same points (not a compact centre list), so the position of each block's own rows in its list is recorded.
    Returns None when a block references 4095 or more distinct rows."""
    if nbr is not None:
        need(nbr, (None, None), dtype=torch.int32, name='neighbors')
        n_rows, k = nbr.shape
        row_ptr, ids, n_refs, dev = None, nbr, n_rows * k, nbr.device
        layout = layout or 'slots'
        if layout != 'slots':
            raise ValueError('a neighbour table [rows, K] is stored slot-major')
    else:
        row_ptr, ids = csr
        need(row_ptr, (None,), dtype=torch.int32, name='csr_ptr')
        need(ids, (None,), dtype=torch.int32, name='csr_src', device=row_ptr.device)
        n_rows, k, n_refs, dev = row_ptr.shape[0] - 1, 0, ids.shape[0], row_ptr.device
        layout = layout or 'runs'
    assert layout in ('slots', 'runs')
    nb = (n_rows + 255) // 256
    blk_ptr = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
    blk_ids = torch.empty((max(n_refs, 1),), dtype=torch.int32, device=dev)
    info = torch.empty((4,), dtype=torch.int32, device=dev)
    if nbr is not None:
        nbytes = lib().dc_block_table_slots_workspace_bytes(n_rows, k)      # (the LDS build: a tenth of the radix build's)
    else:
        nbytes = lib().dc_block_table_workspace_bytes(max(n_refs, n_rows + 1))
    ws = _ws(nbytes, dev)
    slot_ptr = run_ptr = None
    if layout == 'runs':
        run_ptr = torch.empty((n_rows + 1,), dtype=torch.int32, device=dev)
        loc = torch.empty((lib().dc_block_table_run_capacity(n_rows, n_refs) * 4,), dtype=torch.uint16, device=dev)
        check(lib().dc_block_table_build_runs(ptr(row_ptr), ptr(ids), n_rows, n_refs, ptr(run_ptr), ptr(blk_ptr), ptr(blk_ids),
                                              ptr(loc), ptr(info), ptr(ws), nbytes, stream_ptr()), 'dc_block_table_build_runs')
    else:
        slot_ptr = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
        if row_ptr is None:
            # a table [rows, K]: every block has K slots, known without asking the device
            import numpy as _np
            slot_ptr = torch.as_tensor(_np.arange(nb + 1, dtype=_np.int32) * _np.int32(k), device=dev)      # (a copy from the host: no kernel)
            n_slot_rows = nb * k
        else:
            cnt = torch.empty((max(nb, 1),), dtype=torch.int32, device=dev)
            check(lib().dc_block_table_slots(ptr(row_ptr), n_rows, k, ptr(cnt), ptr(slot_ptr), stream_ptr()), 'dc_block_table_slots')
            n_slot_rows = int(slot_ptr[-1])                          # one synchronisation, at set-up time
        # (eight slot rows of slack: the ragged kernels request the next trip's positions before they know it is the last one)
        loc = torch.empty(((max(n_slot_rows, 1) + 8) * 256,), dtype=torch.uint16, device=dev)
        check(lib().dc_block_table_build(ptr(row_ptr), ptr(ids), n_rows, k, n_refs, ptr(slot_ptr), n_slot_rows, ptr(blk_ptr),
                                         ptr(blk_ids), ptr(loc), ptr(info), ptr(ws), nbytes, stream_ptr()), 'dc_block_table_build')
    total, max_rows, overflow, _ = info.tolist()
    if overflow:
        return None
    own_base = None
    if layout == 'slots' and own_rows and (row_ptr is None or own_rows == 'csr'):
        # rows and ids of a k-NN table share one index space: where does every block find its own rows in its list?
        own_base = torch.empty((max(nb, 1),), dtype=torch.int32, device=dev)
        check(lib().dc_block_table_own_base(ptr(blk_ptr), ptr(blk_ids), n_rows, ptr(own_base), stream_ptr()),
              'dc_block_table_own_base')
    packed = 1 if (row_ptr is not None and layout == 'slots') else 0
    # (forward tables from CSR lists keep the offsets: the ragged one-pass kernel takes the rows' lengths from them; it needs every
    # block's own rows in its list -- own_base >= 0 throughout -- because its padding slots read the lane's own row)
    own_all = packed and own_base is not None and nb > 0 and bool((own_base >= 0).all())
    return BlockTable(blk_ptr, blk_ids[:max(total, 1)].clone(), slot_ptr, loc, max_rows, n_rows, run_ptr=run_ptr,
                      own_base=own_base, packed=packed, row_ptr=row_ptr if own_all else None)


def table_to_csr(nbr):
    """(ptr int32 [rows + 1], ids int32 [E]) of a padded neighbour table [rows, Kmax] with -1 for missing entries (radius
    neighbourhoods, nearest_neighbors.py:69-73): its valid entries row by row, in their order."""
    need(nbr, (None, None), dtype=torch.int32, name='neighbors')
    valid = nbr >= 0
    ptr_ = torch.zeros((nbr.shape[0] + 1,), dtype=torch.int32, device=nbr.device)
    ptr_[1:] = valid.sum(dim=1).cumsum(dim=0).to(torch.int32)
    return ptr_, nbr[valid].contiguous()


@on_device
def spatial_order(points):
    need(points, (None, 3), name='points')
    n = points.shape[0]
    order = torch.empty((n,), dtype=torch.int32, device=points.device)
    nbytes = lib().dc_spatial_order_workspace_bytes(n)
    ws = _ws(nbytes, points.device)
    check(lib().dc_spatial_order(ptr(points), 3, dtype_code(points), n, ptr(order), ptr(ws), nbytes, stream_ptr()),
          'dc_spatial_order')
    return order


# ------------------------------------------------------------------------------------------------
# points (model + pose + ray end point)
# ------------------------------------------------------------------------------------------------
class PointSet:
    """Validated per-point inputs of one sequence (local scans concatenated)."""

    def __init__(self, vps, dirs, depth, inc=None, lmask=None, scan_id=None):
        need(dirs, (None, 3), name='dirs')
        n = dirs.shape[0]
        dev, dt = dirs.device, dirs.dtype
        if vps is not None:                  # None: every viewpoint is the sensor origin
            need(vps, (n, 3), dtype=dt, name='vps', device=dev)
        depth = depth.reshape(-1)
        need(depth, (n,), dtype=dt, name='depth', device=dev)
        if inc is not None:
            inc = inc.reshape(-1)
            need(inc, (n,), dtype=dt, name='inc_angles', device=dev)
        if lmask is not None:
            need(lmask, (n,), dtype=torch.bool, name='mask', device=dev)
        if scan_id is not None:
            need(scan_id, (n,), dtype=torch.int32, name='scan_id', device=dev)
        self.vps, self.dirs, self.depth, self.inc, self.lmask, self.scan_id = vps, dirs, depth, inc, lmask, scan_id
        self.n, self.device, self.dtype = n, dev, dt


def _model_args(model_kind, w, e, ps):
    kind = nv.MODEL_KINDS[model_kind] if not isinstance(model_kind, int) else model_kind
    if kind == 0:
        return 0, 0, None, None
    need(w, (None,), dtype=torch.float64, name='w', device=ps.device)
    need(e, (w.shape[0],), dtype=torch.float64, name='exponent', device=ps.device)
    if not (1 <= w.shape[0] <= nv.MAX_MODEL_TERMS):
        raise ValueError('model must have 1..%d terms' % nv.MAX_MODEL_TERMS)
    if ps.inc is None:
        raise ValueError('the model needs incidence angles')
    return kind, w.shape[0], w, e


def _pose_args(poses, ps):
    if poses is None:
        if ps.scan_id is not None:
            raise ValueError('scan_id given without poses')
        return None, 0
    need(poses, (None, 12), dtype=torch.float64, name='poses[S,12]', device=ps.device)
    return poses, poses.shape[0]


class QFormat:
    """Fixed-point parameters of the DC_Q32 point format: x = origin + q * scale (q int32)."""

    def __init__(self, origin, scale):
        self.origin = [float(v) for v in origin]
        self.scale = float(scale)
        self._c = (ctypes.c_double * 4)(*self.origin, self.scale)

    # Resolution up to which 32-bit fixed point keeps neighbourhood eigenvalues within 1e-5 of the fp64 result when the
    # surfaces are as smooth as a millimetre-noise lidar sees them (lambda0 ~ 1e-6 m^2): the rounding of K = 10 points
    # perturbs lambda0 by about 0.2 * sqrt(lambda0) * scale, i.e. 1e-5 * lambda0 at scale = 5e-8 m (a map of ~50 m with
    # the 4x pose margin).  Larger maps keep their points in fp64 instead (SequencePlan, point_format='auto').
    MAX_AUTO_SCALE = 2.0 ** -24

    @staticmethod
    def for_extent(lo, hi, margin=4.0):
        """Power-of-two resolution covering `margin` x the half extent of the box [lo, hi] about its centre."""
        import math
        origin = [(a + b) / 2 for a, b in zip(lo, hi)]
        half = max(max((b - a) / 2 for a, b in zip(lo, hi)), 1e-3)
        return QFormat(origin, 2.0 ** (math.ceil(math.log2(half * margin)) - 31))


def _fmt_args(points_dtype, qfmt):
    """(point_fmt code, qparams pointer) for a points / rec buffer."""
    if qfmt is not None:
        return nv.DC_Q32, qfmt._c
    return (nv.DC_F32 if points_dtype == torch.float32 else nv.DC_F64), None


def _check_points(points, qfmt, name='points'):
    need(points, (None, None), name=name)
    if qfmt is not None:
        need(points, (None, 4), dtype=torch.int32, name=name + ' (q32)')
    elif points.shape[1] not in (3, 4) or not points.dtype.is_floating_point:
        raise ValueError('%s must be float [N,3] or [N,4]' % name)


@on_device
def points_fwd(ps, poses=None, model_kind=None, w=None, e=None, stride=3, want_parts=False, qfmt=None, out=None, status=None):
    """x = pose(vps) + model(depth) * pose(dirs); optionally also (vps', dirs', depth').
    With ``qfmt`` the points are written as int32 fixed-point rows [N,4] (DC_Q32); ``status`` (int32 [1], optional)
    then gets bit 0 set when a coordinate does not fit the format's extent or is NaN."""
    kind, nt, w, e = _model_args(model_kind, w, e, ps)
    poses, ns = _pose_args(poses, ps)
    if qfmt is not None:
        stride = 4
        if ps.dtype != torch.float32:
            raise TypeError('the q32 point format goes with float32 inputs')
    x = out if out is not None else torch.empty((ps.n, stride), dtype=torch.int32 if qfmt is not None else ps.dtype,
                                                device=ps.device)
    _check_points(x, qfmt, 'points_out')
    assert x.shape == (ps.n, stride) and x.device == ps.device
    fmt, qptr = _fmt_args(ps.dtype, qfmt)
    parts = (torch.empty_like(ps.dirs), torch.empty_like(ps.dirs), torch.empty_like(ps.depth)) if want_parts \
        else (None, None, None)
    check(lib().dc_points_fwd(ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth), ptr(ps.inc), ptr(ps.lmask), ptr(ps.scan_id),
                              ptr(poses), ns, kind, nt, ptr(w), ptr(e), ps.n, dtype_code(ps.dirs), fmt, qptr, stride,
                              ptr(x), ptr(parts[0]), ptr(parts[1]), ptr(parts[2]), ptr(status), stream_ptr()), 'dc_points_fwd')
    return (x,) + parts if want_parts else x


def _grads_split(g, nt, ns):
    return g[:nt], g[nt:2 * nt], g[2 * nt:].reshape(ns, 3, 4)


@on_device
def points_bwd(grad_points, ps, poses=None, model_kind=None, w=None, e=None, want_exponent=False, want_pose=False,
               perm=None, out=None):
    """(dL/dw [P], dL/dexponent [P], dL/d[R|t] [S,3,4]) for a given dL/dpoints; ``perm`` int32 [N]: point i uses
    row perm[i] of ``grad_points``."""
    kind, nt, w, e = _model_args(model_kind, w, e, ps)
    poses, ns = _pose_args(poses, ps)
    need(grad_points, (ps.n, None), dtype=ps.dtype, name='grad_points', device=ps.device)
    if perm is not None:
        need(perm, (ps.n,), dtype=torch.int32, name='perm', device=ps.device)
    stride = grad_points.shape[1]
    nacc = 2 * nt + 12 * ns
    if out is None:
        out = torch.zeros((max(nacc, 1),), dtype=torch.float64, device=ps.device)
    else:
        need(out, (nacc,), dtype=torch.float64, name='grads_out', device=ps.device)
    if nacc == 0:
        return _grads_split(out[:0], 0, 0)
    rows = lib().dc_partial_rows(ps.n)
    part = torch.empty((rows * nacc,), dtype=torch.float64, device=ps.device)
    check(lib().dc_points_bwd(ptr(grad_points), ptr(perm), stride, dtype_code(grad_points), ps.n, ptr(ps.vps), ptr(ps.dirs),
                              ptr(ps.depth), ptr(ps.inc), ptr(ps.lmask), ptr(ps.scan_id), ptr(poses), ns, kind, nt,
                              ptr(w), ptr(e), int(want_exponent), int(want_pose), ptr(part), ptr(out), stream_ptr()),
          'dc_points_bwd')
    return _grads_split(out, nt, ns)


# ------------------------------------------------------------------------------------------------
# neighbourhood features
# ------------------------------------------------------------------------------------------------
@on_device
def features_fwd(points, nbr, dirs=None, mean_weights=None, scale=None, want=('mean', 'cov', 'eigvals', 'eigvecs',
                                                                             'normals', 'inc_angles'),
                 want_saved=False, want_weights=False):
    need(points, (None, None), name='points')
    n, stride = points.shape
    assert stride in (3, 4)
    dev, dt = points.device, points.dtype
    need(nbr, (n, None), dtype=torch.int32, name='neighbors', device=dev)
    k = nbr.shape[1]
    if dirs is not None:
        need(dirs, (n, 3), dtype=dt, name='dirs', device=dev)
    if mean_weights is not None:
        mean_weights = mean_weights.reshape(n, k)
        need(mean_weights, (n, k), dtype=dt, name='weights', device=dev)
    shapes = dict(mean=(n, 3), cov=(n, 3, 3), eigvals=(n, 3), eigvecs=(n, 3, 3), normals=(n, 3), inc_angles=(n, 1))
    out = {f: (torch.empty(shapes[f], dtype=dt, device=dev) if f in want else None) for f in shapes}
    if (out['normals'] is not None or out['inc_angles'] is not None) and dirs is None:
        raise ValueError('normals / incidence angles need dirs')
    nvalid = torch.empty((n,), dtype=torch.int32, device=dev) if want_saved else None
    cmean = torch.empty((n, 3), dtype=dt, device=dev) if want_saved else None
    invd = torch.empty((n,), dtype=dt, device=dev) if want_saved else None
    wout = torch.empty((n, k), dtype=dt, device=dev) if want_weights else None
    check(lib().dc_features_fwd(ptr(points), stride, dtype_code(points), ptr(nbr), n, k, ptr(mean_weights),
                                float(scale) if scale else 0.0, ptr(dirs), ptr(out['mean']), ptr(out['cov']),
                                ptr(out['eigvals']), ptr(out['eigvecs']), ptr(out['normals']), ptr(out['inc_angles']),
                                ptr(nvalid), ptr(wout), ptr(cmean), ptr(invd), stream_ptr()), 'dc_features_fwd')
    out.update(nvalid=nvalid, cmean=cmean, invd=invd, weights=wout)
    return out


@on_device
def features_bwd(points, csr_ptr, csr_src, cmean, invd, nvalid, eigvecs=None, grad_mean=None, grad_cov=None,
                 grad_eigvals=None):
    need(points, (None, None), name='points')
    n, stride = points.shape
    dev, dt = points.device, points.dtype
    need(csr_ptr, (n + 1,), dtype=torch.int32, name='csr_ptr', device=dev)
    need(csr_src, (None,), dtype=torch.int32, name='csr_src', device=dev)
    need(cmean, (n, 3), dtype=dt, name='cmean', device=dev)
    need(invd, (n,), dtype=dt, name='invd', device=dev)
    need(nvalid, (n,), dtype=torch.int32, name='nvalid', device=dev)
    for t, shp, nm in ((eigvecs, (n, 3, 3), 'eigvecs'), (grad_mean, (n, 3), 'grad_mean'), (grad_cov, (n, 3, 3), 'grad_cov'),
                       (grad_eigvals, (n, 3), 'grad_eigvals')):
        if t is not None:
            need(t, shp, dtype=dt, name=nm, device=dev)
    grec = torch.empty((n, 12), dtype=dt, device=dev)
    gp = torch.empty((n, stride), dtype=dt, device=dev)
    check(lib().dc_features_bwd(ptr(points), stride, dtype_code(points), ptr(csr_ptr), ptr(csr_src), n, ptr(cmean),
                                ptr(invd), ptr(nvalid), ptr(eigvecs), ptr(grad_mean), ptr(grad_cov), ptr(grad_eigvals),
                                ptr(grec), ptr(gp), stream_ptr()), 'dc_features_bwd')
    return gp


# ------------------------------------------------------------------------------------------------
# fused consistency loss
# ------------------------------------------------------------------------------------------------
@on_device
def consistency_fwd(points, nbr, mask=None, offset=None, loss='min_eigval_loss', normalization=True, sqrt=False,
                    rec=None, want_pointwise=False, want_eigvals=False, partials=None, sums=None, qfmt=None,
                    centre_idx=None, table=None, raw_pointwise=False):
    """raw_pointwise: the pointwise output holds the loss before relu / sqrt (what the quantile-inlier gating of
    loss.py:256-277 compares; see consistency_gate)."""
    _check_points(points, qfmt)
    n_points, stride = points.shape
    dev = points.device
    dt = torch.float32 if qfmt is not None else points.dtype
    if centre_idx is not None:               # compact centre list: rows of nbr / rec / outputs follow it
        need(centre_idx, (None,), dtype=torch.int32, name='centre_idx', device=dev)
        n = centre_idx.shape[0]
        assert n == 0 or (int(centre_idx.min()) >= 0 and int(centre_idx.max()) < n_points)
    else:
        n = n_points
    need(nbr, (n, None), dtype=torch.int32, name='neighbors', device=dev)
    k = nbr.shape[1]
    if mask is not None:
        need(mask, (n,), dtype=torch.bool, name='mask', device=dev)
    if offset is not None:
        need(offset, (n,), dtype=dt, name='offset', device=dev)
    if rec is None:
        rec = torch.empty((n, 8), dtype=points.dtype, device=dev)
    else:
        need(rec, (n, 8), dtype=points.dtype, name='rec', device=dev)
    fmt, qptr = _fmt_args(dt, qfmt)
    pw = torch.empty((n,), dtype=dt, device=dev) if want_pointwise else None
    ev = torch.empty((n, 3), dtype=dt, device=dev) if want_eigvals else None
    rows = lib().dc_partial_rows(n)
    if partials is None:
        partials = torch.empty((rows * 2,), dtype=torch.float64, device=dev)
    else:
        need(partials, (None,), dtype=torch.float64, name='partials', device=dev)
        assert partials.numel() >= rows * 2
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=dev)
    check(lib().dc_consistency_fwd(ptr(points), stride, fmt if qfmt is None else nv.DC_F32, fmt, qptr, ptr(nbr),
                                   ptr(centre_idx), _table_ref(table, n), n, k,
                                   ptr(mask), ptr(offset), nv.LOSS_KINDS[loss] | (nv.LOSS_RAW_POINTWISE if raw_pointwise else 0),
                                   int(bool(normalization)), int(bool(sqrt)), ptr(rec), ptr(pw),
                                   ptr(ev), ptr(partials), ptr(sums), stream_ptr()), 'dc_consistency_fwd')
    return dict(sums=sums, rec=rec, pointwise=pw, eigvals=ev)


@on_device
def consistency_gate(raw, rec, threshold, mask=None, sqrt=False, partials=None, sums=None, qfmt=None):
    """Quantile-inlier gating of a fused forward (loss.py:256-277): masked centres whose raw loss exceeds the device scalar
    ``threshold`` stop contributing -- their records' coefficients are zeroed in place -- and ``sums`` becomes
    {sum of the inliers' loss, number of inliers}."""
    n = raw.shape[0]
    dev = raw.device
    need(rec, (n, 8), name='rec', device=dev)
    need(threshold, (), dtype=torch.float64, name='threshold', device=dev)
    if mask is not None:
        need(mask, (n,), dtype=torch.bool, name='mask', device=dev)
    fmt, _ = _fmt_args(raw.dtype, qfmt)
    rows = lib().dc_partial_rows(n)
    if partials is None:
        partials = torch.empty((rows * 2,), dtype=torch.float64, device=dev)
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=dev)
    check(lib().dc_consistency_gate(ptr(raw), nv.DC_F32 if raw.dtype == torch.float32 else nv.DC_F64, fmt, ptr(mask), n,
                                    ptr(threshold), int(bool(sqrt)), ptr(rec), ptr(partials), ptr(sums), stream_ptr()),
          'dc_consistency_gate')
    return sums


def degree_lane_perm(csr_ptr, block=256):
    """u8 [block * ceil(n / block)]: per block of consecutive points the lane -> point map by ascending in-degree."""
    n = csr_ptr.shape[0] - 1
    nb = (n + block - 1) // block
    deg = torch.full((nb * block,), 2 ** 30, dtype=torch.int32, device=csr_ptr.device)
    deg[:n] = csr_ptr[1:] - csr_ptr[:-1]
    return torch.argsort(deg.reshape(nb, block), dim=1, stable=True).to(torch.uint8).reshape(-1).contiguous()


@on_device
def consistency_bwd(points, rec, csr_ptr, csr_src, ps=None, poses=None, model_kind=None, w=None, e=None,
                    want_exponent=False, want_pose=False, want_grad_points=False, partials=None, grads=None, qfmt=None,
                    lane_perm=None, table=None):
    _check_points(points, qfmt)
    n, stride = points.shape
    dev = points.device
    dt = torch.float32 if qfmt is not None else points.dtype
    fmt, qptr = _fmt_args(dt, qfmt)
    dcode = nv.DC_F32 if qfmt is not None else fmt
    need(rec, (None, 8), dtype=points.dtype, name='rec', device=dev)        # one row per centre (<= n with a centre list)
    need(csr_ptr, (n + 1,), dtype=torch.int32, name='csr_ptr', device=dev)
    need(csr_src, (None,), dtype=torch.int32, name='csr_src', device=dev)
    gp = torch.empty((n, stride), dtype=dt, device=dev) if want_grad_points else None
    if lane_perm is not None:
        need(lane_perm, (((n + 255) // 256) * 256,), dtype=torch.uint8, name='lane_perm', device=dev)
    if ps is None:
        assert want_grad_points
        check(lib().dc_consistency_bwd(ptr(points), stride, dcode, fmt, qptr, ptr(rec), ptr(csr_ptr), ptr(csr_src),
                                       ptr(lane_perm), _table_ref(table, n), n, None, None, None, None, None, None, None, 0, 0, 0,
                                       None, None, 0, 0, ptr(gp), None,
                                       None, stream_ptr()), 'dc_consistency_bwd')
        return gp, None
    assert ps.n == n and ps.dtype == dt and ps.device == dev
    kind, nt, w, e = _model_args(model_kind, w, e, ps)
    poses, ns = _pose_args(poses, ps)
    nacc = 2 * nt + 12 * ns
    rows = lib().dc_partial_rows(n)
    if partials is None:
        partials = torch.empty((max(rows * nacc, 1),), dtype=torch.float64, device=dev)
    else:
        assert partials.numel() >= rows * nacc
    if grads is None:
        grads = torch.zeros((max(nacc, 1),), dtype=torch.float64, device=dev)
    check(lib().dc_consistency_bwd(ptr(points), stride, dcode, fmt, qptr, ptr(rec), ptr(csr_ptr), ptr(csr_src),
                                   ptr(lane_perm), _table_ref(table, n), n, ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth), ptr(ps.inc), ptr(ps.lmask), ptr(ps.scan_id),
                                   ptr(poses), ns, kind, nt, ptr(w), ptr(e), int(want_exponent), int(want_pose), ptr(gp),
                                   ptr(partials), ptr(grads), stream_ptr()), 'dc_consistency_bwd')
    return gp, _grads_split(grads, nt, ns)


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
def _bound(v, default):
    if v is None:
        return default
    v = float(v)
    if v != v:                             # config files encode "unbounded" as nan (config.py:41-43)
        return default
    # the reference compares with torch.tensor(bound), a float32 scalar whatever the values' dtype (filters.py:97-104):
    # the kernels get its widened value (infinities stay what they are)
    return v if v in (float('-inf'), float('inf')) else torch.tensor(v, dtype=torch.float32).item()


@on_device
def mask_bounds(mask, num, num_index=0, den=None, den_index=0, lo=None, hi=None):
    """mask &= lo <= num[:, num_index] (/ den[:, den_index]) <= hi   (in place, returns mask)."""
    n = mask.shape[0]
    need(mask, (n,), dtype=torch.bool, name='mask')
    num2 = num.reshape(n, -1)
    need(num2, (n, None), name='values', device=mask.device)
    den2 = None
    if den is not None:
        den2 = den.reshape(n, -1)
        need(den2, (n, None), dtype=num2.dtype, name='denominator', device=mask.device)
    check(lib().dc_mask_bounds(ptr(num2), num2.shape[1], num_index, ptr(den2), den2.shape[1] if den2 is not None else 0,
                               den_index, dtype_code(num2), n, _bound(lo, float('-inf')), _bound(hi, float('inf')),
                               ptr(mask), stream_ptr()), 'dc_mask_bounds')
    return mask


@on_device
def mask_bounds_all(values, bounds, mask=None):
    """bool [N]: every ``(num_index, den_index | None, lo, hi)`` of ``bounds`` on the columns of ``values`` [N, C] in ONE pass
    (dc_mask_bounds_multi), ANDed into ``mask`` when given (in place), else into a new mask."""
    n = values.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.bool, device=values.device) if mask is None else mask
    v2 = values.reshape(n, -1)
    need(v2, (n, None), name='values')
    init = mask is None
    if init:
        mask = torch.empty((n,), dtype=torch.bool, device=v2.device)
    need(mask, (n,), dtype=torch.bool, name='mask', device=v2.device)
    nb = len(bounds)
    if nb > 8:
        raise ValueError('at most 8 bounds per pass')
    num = (ctypes.c_int32 * max(nb, 1))(*[int(b[0]) for b in bounds])
    den = (ctypes.c_int32 * max(nb, 1))(*[-1 if b[1] is None else int(b[1]) for b in bounds])
    lo = (ctypes.c_double * max(nb, 1))(*[_bound(b[2], float('-inf')) for b in bounds])
    hi = (ctypes.c_double * max(nb, 1))(*[_bound(b[3], float('inf')) for b in bounds])
    check(lib().dc_mask_bounds_multi(ptr(v2), v2.shape[1], dtype_code(v2), n, nb, num, den, lo, hi, 1 if init else 0, ptr(mask),
                                     stream_ptr()), 'dc_mask_bounds_multi')
    return mask


@on_device
def compact_rows(mask, fields, want_index=False):
    """``[f[mask] for f in fields]`` (and the kept row numbers, int32) for up to 8 contiguous arrays of N rows on the device: two
    launches and ONE synchronisation (the number of kept rows) for all of them (dc_compact_rows; depth_cloud.py:126-134)."""
    n = mask.shape[0]
    need(mask, (n,), dtype=torch.bool, name='mask')
    dev = mask.device
    if len(fields) > 8:
        raise ValueError('at most 8 fields per call')
    srcs, outs, rb = [], [], []
    for f in fields:
        if f.shape[0] != n or f.device != dev:
            raise ValueError('every field needs %d rows on %s' % (n, dev))
        f = f.contiguous()
        srcs.append(f)
        outs.append(torch.empty_like(f))
        rb.append(f.element_size() * (f.numel() // n if n else 1))
    index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    nf = len(srcs)
    a_src = (ctypes.c_void_p * max(nf, 1))(*[ptr(f) for f in srcs])
    a_dst = (ctypes.c_void_p * max(nf, 1))(*[ptr(f) for f in outs])
    a_rb = (ctypes.c_int32 * max(nf, 1))(*rb)
    nbytes = lib().dc_compact_rows_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib().dc_compact_rows(ptr(mask), n, nf, a_src, a_dst, a_rb, ptr(index), ptr(count), ptr(ws), nbytes, stream_ptr()),
          'dc_compact_rows')
    m = int(count.item())
    outs = [o[:m] for o in outs]
    return (outs, index[:m]) if want_index else outs


@on_device
def compact_rows_device(mask, fields):
    """``compact_rows`` without the read-back: (full-size outputs whose first ``count`` rows are the kept ones, ``count`` device
    int64 [1]) -- for callers that keep issuing work and size their tensors later."""
    n = mask.shape[0]
    need(mask, (n,), dtype=torch.bool, name='mask')
    dev = mask.device
    if len(fields) > 8:
        raise ValueError('at most 8 fields per call')
    srcs, outs, rb = [], [], []
    for f in fields:
        if f.shape[0] != n or f.device != dev:
            raise ValueError('every field needs %d rows on %s' % (n, dev))
        f = f.contiguous()
        srcs.append(f)
        outs.append(torch.empty_like(f))
        rb.append(f.element_size() * (f.numel() // n if n else 1))
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    nf = len(srcs)
    a_src = (ctypes.c_void_p * max(nf, 1))(*[ptr(f) for f in srcs])
    a_dst = (ctypes.c_void_p * max(nf, 1))(*[ptr(f) for f in outs])
    a_rb = (ctypes.c_int32 * max(nf, 1))(*rb)
    nbytes = lib().dc_compact_rows_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib().dc_compact_rows(ptr(mask), n, nf, a_src, a_dst, a_rb, None, ptr(count), ptr(ws), nbytes, stream_ptr()), 'dc_compact_rows')
    return outs, count


@on_device
def scan_prefilter(points, vps, dtype, r, lo, hi):
    """Raw rows [N, >=3] (and viewpoints [N,3] | None) on the device -> (vps, dirs, depth [M,1], points) of the rays the scan-shadow
    filter keeps: from_points, to_points, dc_shadow_filter and cloud[mask] launched by ONE call (dc_scan_prefilter), one
    synchronisation (M)."""
    need(points, (None, None), name='points')
    n, stride = points.shape
    if stride < 3:
        raise ValueError('points need at least 3 columns')
    dev = points.device
    dtype = points.dtype if dtype is None else dtype
    if vps is not None:
        need(vps, (n, 3), dtype=points.dtype, name='vps', device=dev)
    outs = [torch.empty((n, c), dtype=dtype, device=dev) for c in (3, 3, 1, 3)]
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    nbytes = lib().dc_scan_prefilter_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib().dc_scan_prefilter(ptr(points), stride, dtype_code(points), ptr(vps), n, nv.DC_F32 if dtype == torch.float32 else nv.DC_F64,
                                  float(r), float(lo), float(hi), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(count),
                                  ptr(ws), nbytes, stream_ptr()), 'dc_scan_prefilter')
    m = int(count.item())
    return tuple(o[:m] for o in outs)


@on_device
def to_points(vps, dirs, depth):
    """``vps + depth * dirs`` in one kernel, bit-equal to the two tensor operations (dc_to_points; no autograd)."""
    n = dirs.shape[0]
    need(dirs, (n, 3), name='dirs')
    need(depth, (n, 1), dtype=dirs.dtype, name='depth', device=dirs.device)
    vps = vps.reshape(-1, 3)
    need(vps, (None, 3), dtype=dirs.dtype, name='vps', device=dirs.device)
    if vps.shape[0] not in (1, n):
        raise ValueError('vps must have 1 or %d rows' % n)
    out = torch.empty_like(dirs)
    check(lib().dc_to_points(ptr(vps), vps.shape[0], ptr(dirs), ptr(depth), dtype_code(dirs), n, ptr(out), stream_ptr()), 'dc_to_points')
    return out


@on_device
def valid_weights(nbr):
    """float32 [N, K, 1]: 1 where the table holds a neighbour (``valid_neighbor_mask().float()[..., None]``)."""
    need(nbr, (None, None), dtype=torch.int32, name='neighbors')
    out = torch.empty(tuple(nbr.shape) + (1,), dtype=torch.float32, device=nbr.device)
    check(lib().dc_valid_weights(ptr(nbr), nbr.numel(), ptr(out), stream_ptr()), 'dc_valid_weights')
    return out


@on_device
def valid_count(nbr):
    need(nbr, (None, None), dtype=torch.int32, name='neighbors')
    cnt = torch.empty((nbr.shape[0],), dtype=torch.int32, device=nbr.device)
    check(lib().dc_valid_count(ptr(nbr), nbr.shape[0], nbr.shape[1], ptr(cnt), stream_ptr()), 'dc_valid_count')
    return cnt


@on_device
def dispersion(vec, nbr, weights=None):
    need(vec, (None, 3), name='vectors')
    n = vec.shape[0]
    need(nbr, (n, None), dtype=torch.int32, name='neighbors', device=vec.device)
    k = nbr.shape[1]
    if weights is not None:
        weights = weights.reshape(n, k)
        need(weights, (n, k), dtype=vec.dtype, name='weights', device=vec.device)
    out = torch.empty((n,), dtype=vec.dtype, device=vec.device)
    check(lib().dc_dispersion(ptr(vec), dtype_code(vec), ptr(nbr), ptr(weights), n, k, ptr(out), stream_ptr()),
          'dc_dispersion')
    return out


@on_device
def cloud_from_points(points, vps=None, dtype=None, ego_box=None, min_depth=None, max_depth=None, want_index=False, want_zero_vps=False):
    """Raw rows [N, >=3] on the device -> (vps [M,3] | None, dirs [M,3], depth [M,1], index int64 [M] | None) of the rows
    that survive the ego-box crop and the depth bounds, in their original order (dc_cloud_from_points: kitti360.py:101-105,
    filters.py:116-141, depth_cloud.py:592-638).  One synchronisation (the number of kept rows) when a filter is active."""
    need(points, (None, None), name='points')
    n, stride = points.shape
    if stride < 3:
        raise ValueError('points need at least 3 columns')
    dev = points.device
    dtype = points.dtype if dtype is None else dtype
    if vps is not None:
        need(vps, (n, 3), dtype=points.dtype, name='vps', device=dev)
    dirs = torch.empty((n, 3), dtype=dtype, device=dev)
    depth = torch.empty((n, 1), dtype=dtype, device=dev)
    filtered = bool(ego_box and ego_box > 0) or min_depth is not None or max_depth is not None
    # (want_zero_vps: the kernel that writes the fields also writes the zero viewpoints of a cloud without any)
    vps_out = torch.empty((n, 3), dtype=dtype, device=dev) if (vps is not None or want_zero_vps) else None
    index = torch.empty((n,), dtype=torch.int32, device=dev) if want_index else None
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    nbytes = lib().dc_cloud_from_points_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    nan = float('nan')
    # (the depth bounds go through the reference's within_bounds too, filters.py:137: float32-rounded on fp64 rows as well)
    check(lib().dc_cloud_from_points(ptr(points), stride, dtype_code(points), ptr(vps), n, float(ego_box or 0.0),
                                     _bound(min_depth, nan), _bound(max_depth, nan),
                                     nv.DC_F32 if dtype == torch.float32 else nv.DC_F64, ptr(dirs), ptr(depth), ptr(vps_out),
                                     ptr(index), ptr(count), ptr(ws), nbytes, stream_ptr()), 'dc_cloud_from_points')
    m = int(count.item()) if filtered else n
    return (None if vps_out is None else vps_out[:m], dirs[:m], depth[:m], None if index is None else index[:m].long())


@on_device
def correct_depth(depth, gamma, mask, w, exponent, op):
    """depth' [N,1]: the polynomial models outside the training loop (dc_correct_depth; op 0 d-b, 1 d+b, 2 d(1-b), 3 d/(1-b));
    ``mask`` bool [N] or None; ``w`` / ``exponent`` fp64 [1,P] on the device.  No autograd."""
    n = depth.shape[0]
    dev = depth.device
    need(depth, (n, 1), name='depth')
    need(gamma, (n, 1), dtype=depth.dtype, name='inc_angles', device=dev)
    w1, e1 = w.detach().reshape(-1).contiguous(), exponent.detach().reshape(-1).contiguous()
    need(w1, (None,), dtype=torch.float64, name='w', device=dev)
    need(e1, (w1.shape[0],), dtype=torch.float64, name='exponent', device=dev)
    if mask is not None:
        need(mask, (n,), dtype=torch.bool, name='mask', device=dev)
    out = torch.empty_like(depth)
    check(lib().dc_correct_depth(ptr(depth), ptr(gamma), ptr(mask), ptr(w1), ptr(e1), w1.shape[0], int(op), dtype_code(depth), n,
                                 ptr(out), stream_ptr()), 'dc_correct_depth')
    return out


@on_device
def shadow_filter(points, vps, dirs, r, lo, hi):
    """bool [N]: ``shadow_mask`` over the direction neighbourhoods of radius ``r`` (chord length) WITHOUT building their table
    (dc_shadow_filter: grid over ``dirs`` + one walk); the same mask as radius_neighbors(dirs, r) -> shadow_mask."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    dev, dt = points.device, points.dtype
    vps = vps.reshape(-1, 3)
    need(vps, (None, 3), dtype=dt, name='vps', device=dev)
    need(dirs, (n, 3), dtype=dt, name='dirs', device=dev)
    if vps.shape[0] not in (1, n):
        raise ValueError('vps must have 1 or %d rows' % n)
    mask = torch.empty((n,), dtype=torch.bool, device=dev)
    if n:
        nbytes = lib().dc_knn_workspace_bytes(n, 0)
        ws = _ws(nbytes, dev)
        check(lib().dc_shadow_filter(ptr(points), ptr(vps), vps.shape[0], ptr(dirs), dtype_code(points), n, float(r), float(lo), float(hi),
                                     ptr(mask), ptr(ws), nbytes, stream_ptr()), 'dc_shadow_filter')
    return mask


@on_device
def shadow_mask(points, vps, dir_nbr, lo, hi, fill):
    """bool [N]: every angle between (vps - x) and (x_j - x), j in dir_nbr[i], within [lo, hi] (filters.py:257-309)."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    dev, dt = points.device, points.dtype
    vps = vps.reshape(-1, 3)
    need(vps, (None, 3), dtype=dt, name='vps', device=dev)
    if vps.shape[0] not in (1, n):
        raise ValueError('vps must have 1 or %d rows' % n)
    need(dir_nbr, (n, None), dtype=torch.int32, name='dir_neighbors', device=dev)
    mask = torch.empty((n,), dtype=torch.bool, device=dev)
    if n and dir_nbr.shape[1]:
        check(lib().dc_shadow_mask(ptr(points), ptr(vps), vps.shape[0], dtype_code(points), ptr(dir_nbr), n, dir_nbr.shape[1],
                                   float(lo), float(hi), float(fill), ptr(mask), stream_ptr()), 'dc_shadow_mask')
    else:
        mask.fill_(True)
    return mask


@on_device
def voxel_filter(points, grid_res, seq=None, preserve_order=False):
    """Indices (int64, device) of one survivor per voxel with filter_grid's dict semantics; None if the voxel range
    does not fit the 63-bit key (caller falls back to the host algorithm)."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    dev = points.device
    if seq is not None:
        need(seq, (n,), dtype=torch.int32, name='seq', device=dev)
    out = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    meta = torch.zeros((2,), dtype=torch.int32, device=dev)
    nbytes = lib().dc_voxel_filter_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib().dc_voxel_filter(ptr(points), 3, dtype_code(points), n, float(grid_res), ptr(seq), int(bool(preserve_order)),
                                ptr(out), ctypes.c_void_p(meta.data_ptr()), ctypes.c_void_p(meta.data_ptr() + 4), ptr(ws),
                                nbytes, stream_ptr()), 'dc_voxel_filter')
    count, status = meta.tolist()
    return None if status else out[:count].long()


# ------------------------------------------------------------------------------------------------
# point-to-plane ICP pair
# ------------------------------------------------------------------------------------------------
@on_device
def p2plane_pair(psa, normals_a, psb, normals_b, pose_a, pose_b, idx_a, idx_b, model_kind=None, w=None, e=None):
    """Sums of point-to-plane distances over the correspondences of one scan pair and their gradients:
    returns (sums f64 [2], dw [P], de [P], dTa [3,4], dTb [3,4]) for d(sum12 + sum21)."""
    dev, dt = psa.device, psa.dtype
    assert psb.device == dev and psb.dtype == dt
    need(normals_a, (psa.n, 3), dtype=dt, name='normals_a', device=dev)
    need(normals_b, (psb.n, 3), dtype=dt, name='normals_b', device=dev)
    need(pose_a, (12,), dtype=torch.float64, name='pose_a', device=dev)
    need(pose_b, (12,), dtype=torch.float64, name='pose_b', device=dev)
    need(idx_a, (None,), dtype=torch.int32, name='idx_a', device=dev)
    m = idx_a.shape[0]
    need(idx_b, (m,), dtype=torch.int32, name='idx_b', device=dev)
    kind, nt, w, e = _model_args(model_kind, w, e, psa)
    if kind != 0 and psb.inc is None:
        raise ValueError('the model needs incidence angles')
    part = torch.empty((lib().dc_p2plane_partial_count(m),), dtype=torch.float64, device=dev)
    out = torch.empty((2 + 2 * nt + 24,), dtype=torch.float64, device=dev)
    check(lib().dc_p2plane_pair(ptr(psa.vps), ptr(psa.dirs), ptr(psa.depth), ptr(psa.inc), ptr(psa.lmask),
                                ptr(normals_a), ptr(psb.vps), ptr(psb.dirs), ptr(psb.depth), ptr(psb.inc),
                                ptr(psb.lmask), ptr(normals_b), dtype_code(psa.dirs), ptr(pose_a), ptr(pose_b), kind, nt,
                                ptr(w), ptr(e), ptr(idx_a), ptr(idx_b), m, 1, 1, ptr(part), ptr(out), stream_ptr()),
          'dc_p2plane_pair')
    return out[:2], out[2:2 + nt], out[2 + nt:2 + 2 * nt], out[2 + 2 * nt:14 + 2 * nt].reshape(3, 4), \
        out[14 + 2 * nt:].reshape(3, 4)


@on_device
def p2point_pair(psa, psb, pose_a, pose_b, idx_a, idx_b, model_kind=None, w=None, e=None):
    """Sum of point-to-point distances over the correspondences of one scan pair and its gradients:
    returns (sums f64 [2] = {sum |xb - xa|, 0}, dw [P], de [P], dTa [3,4], dTb [3,4])."""
    dev, dt = psa.device, psa.dtype
    assert psb.device == dev and psb.dtype == dt
    need(pose_a, (12,), dtype=torch.float64, name='pose_a', device=dev)
    need(pose_b, (12,), dtype=torch.float64, name='pose_b', device=dev)
    need(idx_a, (None,), dtype=torch.int32, name='idx_a', device=dev)
    m = idx_a.shape[0]
    need(idx_b, (m,), dtype=torch.int32, name='idx_b', device=dev)
    kind, nt, w, e = _model_args(model_kind, w, e, psa)
    if kind != 0 and psb.inc is None:
        raise ValueError('the model needs incidence angles')
    part = torch.empty((lib().dc_p2plane_partial_count(m),), dtype=torch.float64, device=dev)
    out = torch.empty((2 + 2 * nt + 24,), dtype=torch.float64, device=dev)
    check(lib().dc_p2point_pair(ptr(psa.vps), ptr(psa.dirs), ptr(psa.depth), ptr(psa.inc), ptr(psa.lmask), ptr(psb.vps),
                                ptr(psb.dirs), ptr(psb.depth), ptr(psb.inc), ptr(psb.lmask), dtype_code(psa.dirs), ptr(pose_a),
                                ptr(pose_b), kind, nt, ptr(w), ptr(e), ptr(idx_a), ptr(idx_b), m, ptr(part), ptr(out),
                                stream_ptr()), 'dc_p2point_pair')
    return out[:2], out[2:2 + nt], out[2 + nt:2 + 2 * nt], out[2 + 2 * nt:14 + 2 * nt].reshape(3, 4), \
        out[14 + 2 * nt:].reshape(3, 4)


class IcpSequence:
    """Descriptors of one sequence of scans and its pair correspondences for dc_p2plane_sequence / dc_p2point_sequence,
    filled once; ``eval`` is then one host call per evaluation.  ``scans``: list of (PointSet, normals [n,3] | None);
    ``pairs``: list of (scan_a, scan_b, idx_a int32 [m], idx_b int32 [m]); pair weights follow icp_loss
    (loss.py:391-403): 0.5 / (m * n_pairs) for point to plane (two directed sums), 1 / (m * n_pairs) for point to
    point (``plane=False``, loss.py:553,563)."""

    @on_device
    def __init__(self, scans, pairs, with_model=True, plane=True):
        ps0 = scans[0][0]
        self.device, self.dtype, self.n_scans = ps0.device, ps0.dtype, len(scans)
        self.with_model, self.plane = bool(with_model), bool(plane)
        self._keep = []
        self.scan_desc = (nv.IcpScan * max(len(scans), 1))()
        for d, (ps, normals) in zip(self.scan_desc, scans):
            assert ps.device == self.device and ps.dtype == self.dtype
            if plane:
                need(normals, (ps.n, 3), dtype=self.dtype, name='normals', device=self.device)
            else:
                normals = None
            if with_model and ps.inc is None:
                raise ValueError('the model needs incidence angles')
            self._keep.append((ps, normals))
            d.vps, d.dirs, d.depth, d.inc = ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth), ptr(ps.inc)
            d.lmask, d.normals = ptr(ps.lmask), ptr(normals)
        self.pair_desc = (nv.IcpPair * max(len(pairs), 1))()
        self.n_pairs, max_m = len(pairs), 0
        for d, (a, b, idx_a, idx_b) in zip(self.pair_desc, pairs):
            need(idx_a, (None,), dtype=torch.int32, name='idx_a', device=self.device)
            m = idx_a.shape[0]
            need(idx_b, (m,), dtype=torch.int32, name='idx_b', device=self.device)
            if not (0 <= a < self.n_scans and 0 <= b < self.n_scans and a != b):
                raise ValueError('pair (%d, %d) outside the sequence' % (a, b))
            self._keep.append((idx_a, idx_b))
            d.scan_a, d.scan_b, d.idx_a, d.idx_b, d.m = int(a), int(b), ptr(idx_a), ptr(idx_b), m
            d.weight = (0.5 if plane else 1.0) / (max(m, 1) * len(pairs))
            max_m = max(max_m, m)
        self.part = torch.empty((lib().dc_p2plane_sequence_partial_count(ctypes.cast(self.pair_desc, ctypes.c_void_p), self.n_pairs),),
                                dtype=torch.float64, device=self.device)
        self.ticket = torch.zeros((32,), dtype=torch.int32, device=self.device)      # dc_icp_sequence_step's (left zero by every launch)

    @on_device
    def eval(self, poses12, model_kind=None, w=None, e=None, out=None):
        """out fp64 [1 + 2P + 12 S] = {loss, dloss/dw, dloss/dexponent, dloss/d[R|t]}."""
        kind, nt, w, e = _model_args(model_kind, w, e, self._keep[0][0]) if self.n_scans else (0, 0, None, None)
        if kind != 0 and not self.with_model:
            raise ValueError('sequence was built without incidence angles')
        need(poses12, (self.n_scans, 12), dtype=torch.float64, name='poses[S,12]', device=self.device)
        n_out = 1 + 2 * nt + 12 * self.n_scans
        out = _out_arg(out, n_out, self.device)
        fn = lib().dc_p2plane_sequence if self.plane else lib().dc_p2point_sequence
        check(fn(ctypes.cast(self.scan_desc, ctypes.c_void_p), self.n_scans, ctypes.cast(self.pair_desc, ctypes.c_void_p),
                 self.n_pairs, 0 if self.dtype == torch.float32 else 1, ptr(poses12), kind, nt, ptr(w), ptr(e),
                 ptr(self.part), ptr(out), stream_ptr()), 'dc_p2plane_sequence' if self.plane else 'dc_p2point_sequence')
        return out

    @on_device
    def step(self, poses12, model_kind, w, e, out, fin=None):
        """``eval`` as ONE launch (dc_icp_sequence_step: the sums are finished by the block that takes the last ticket) and, with
        ``fin`` (a _native.PoseTrainStepDesc), the finishing step of a training iteration -- dc_pose_train_finish's work -- by
        that same block.  Returns False when the sequence cannot take it (more than sixteen pairs, no correspondence at all)."""
        kind, nt, w, e = _model_args(model_kind, w, e, self._keep[0][0]) if self.n_scans else (0, 0, None, None)
        if kind != 0 and not self.with_model:
            raise ValueError('sequence was built without incidence angles')
        need(poses12, (self.n_scans, 12), dtype=torch.float64, name='poses[S,12]', device=self.device)
        need(out, (1 + 2 * nt + 12 * self.n_scans,), dtype=torch.float64, name='out', device=self.device)
        rc = lib().dc_icp_sequence_step(1 if self.plane else 0, ctypes.cast(self.scan_desc, ctypes.c_void_p), self.n_scans,
                                        ctypes.cast(self.pair_desc, ctypes.c_void_p), self.n_pairs, 0 if self.dtype == torch.float32 else 1,
                                        ptr(poses12), kind, nt, ptr(w), ptr(e), ptr(self.part), ptr(out), ptr(self.ticket),
                                        None if fin is None else ctypes.byref(fin), stream_ptr())
        if rc == nv.DC_ERR_UNSUPPORTED:
            return False
        check(rc, 'dc_icp_sequence_step')
        return True


# ------------------------------------------------------------------------------------------------
# triangle-mesh ray casting (dc_raycast.hip)
# ------------------------------------------------------------------------------------------------
def _scene_box_arg(scene_box):
    """``scene_box`` (6 floats: lo xyz, hi xyz) as the host float64 array the tree builds take."""
    import numpy as np
    box = np.ascontiguousarray(np.asarray(scene_box, dtype=np.float64).reshape(6))
    if not (np.isfinite(box).all() and (box[3:] >= box[:3]).all()):
        raise ValueError('scene_box must be finite with hi >= lo, got %s' % box)
    return box


def _tree_arrays(n, dev):                    # -> leaf index i32 [n], child i32 [n-1,2], parent i32 [2n-1], node_box f32 [2n-1,6]
    return (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=dev),
            torch.empty((2 * n - 1,), dtype=torch.int32, device=dev), torch.empty((2 * n - 1, 6), dtype=torch.float32, device=dev))


def _scan_offset_arg(scan_offset, s, n, dev):
    """s + 1 scan offsets from 0 to n.  An int64 device tensor is taken as it is, not read back (the kernels clamp the scan index: wrong
    offsets give wrong poses, never a read outside a per-scan array; ``dev`` None: only its shape is checked).  A host sequence is checked."""
    if isinstance(scan_offset, torch.Tensor) and scan_offset.is_cuda:
        if dev is not None:
            return need(scan_offset, (s + 1,), dtype=torch.int64, name='scan_offset', device=dev)
        if tuple(scan_offset.shape) != (s + 1,):
            raise ValueError('scan_offset has shape %s, expected %s' % (tuple(scan_offset.shape), (s + 1,)))
        return scan_offset
    off = torch.as_tensor(scan_offset, dtype=torch.int64).reshape(-1)
    if off.numel() != s + 1 or int(off[0]) != 0 or int(off[-1]) != n or bool((off[1:] < off[:-1]).any()):
        raise ValueError('scan_offset must hold %d non-decreasing offsets from 0 to %d, got %s' % (s + 1, n, off.tolist()))
    return off


def _measured_rays_arg(dev, vps, dirs, scan_offset, poses, what='rays'):
    """The checks raycast_rays, surfel_cast_rays and raycast_beams share -> (n, dtype code, s, scan offsets)."""
    need(dirs, (None, 3), name='dirs', device=dev)
    n = dirs.shape[0]
    need(vps, (n, 3), dtype=dirs.dtype, name='vps', device=dev)
    code = dtype_code(dirs)
    need(poses, (None, 4, 4), dtype=torch.float64, name='poses', device=dev)
    s = poses.shape[0]
    off = _scan_offset_arg(scan_offset, s, n, dev)
    if n and s < 1:
        raise ValueError('%s need at least one pose' % what)
    return n, code, s, off


def _t_min_arg(t_min, n=None, dev=None):
    """``t_min`` -> (per-ray device tensor f64 [n] or None, float): a tensor is taken per ray where ``n`` is given."""
    if n is not None and isinstance(t_min, torch.Tensor):
        return need(t_min, (n,), dtype=torch.float64, name='t_min', device=dev), 0.0
    tm = float(t_min)
    if tm != tm:
        raise ValueError('t_min must not be NaN')
    return None, tm


@on_device
def bvh_build(verts, faces, scene_box):
    """LBVH of verts f64 [V,3] / faces i32 [F,3] (indices checked here) in the box ``scene_box`` (6 floats: lo xyz, hi xyz) ->
    mesh.MeshBVH (leaf_face i32 [F], child i32 [F-1,2], parent i32 [2F-1], node_box f32 [2F-1,6], leaf_tri f64 [F,9])."""
    from .mesh import MeshBVH
    need(verts, (None, 3), dtype=torch.float64, name='verts')
    need(faces, (None, 3), dtype=torch.int32, name='faces', device=verts.device)
    nv_, nf = verts.shape[0], faces.shape[0]
    if nv_ == 0 or nf == 0:
        raise ValueError('bvh_build needs at least one vertex and one face')
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= nv_:
        raise ValueError('face indices must lie in [0, %d), got [%d, %d]' % (nv_, lo, hi))
    box = _scene_box_arg(scene_box)
    dev = verts.device
    leaf_face, child, parent, node_box = _tree_arrays(nf, dev)
    leaf_tri = torch.empty((nf, 9), dtype=torch.float64, device=dev)
    nbytes = lib().dc_bvh_workspace_bytes(nf)
    ws = _ws(nbytes, dev)
    check(lib().dc_bvh_build(ptr(verts), nv_, ptr(faces), nf, box.ctypes.data_as(ctypes.c_void_p), ptr(leaf_face),
                             ptr(child) if nf > 1 else None, ptr(parent), ptr(node_box), ptr(leaf_tri), ptr(ws), nbytes, stream_ptr()),
          'dc_bvh_build')
    return MeshBVH(leaf_face, child, parent, node_box, leaf_tri)


@on_device
def raycast(bvh, dirs, poses, t_min, cull=True):
    """Closest hits of the rays dirs f64 [R,3] (sensor frame) of every pose of poses f64 [P,4,4] (world from sensor), hits
    beyond t_min f64 [R] (and facing the ray with ``cull``) -> (face i32 [P,R] (-1 = miss), t f64 [P,R] (inf on a miss),
    bary f64 [P,R,2]): the hit is v0 + u (v1 - v0) + v (v2 - v0).  One launch (dc_raycast)."""
    dev = bvh.leaf_face.device
    need(dirs, (None, 3), dtype=torch.float64, name='dirs', device=dev)
    r = dirs.shape[0]
    need(t_min, (r,), dtype=torch.float64, name='t_min', device=dev)
    need(poses, (None, 4, 4), dtype=torch.float64, name='poses', device=dev)
    p = poses.shape[0]
    if p * r >= 2 ** 62:
        raise ValueError('too many rays')
    face = torch.empty((p, r), dtype=torch.int32, device=dev)
    t = torch.empty((p, r), dtype=torch.float64, device=dev)
    bary = torch.empty((p, r, 2), dtype=torch.float64, device=dev)
    nf = bvh.n_faces
    check(lib().dc_raycast(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                           ptr(dirs), ptr(t_min), r, ptr(poses), p, 1 if cull else 0, ptr(face), ptr(t), ptr(bary), stream_ptr()),
          'dc_raycast')
    return face, t, bary


@on_device
def raycast_rays(bvh, vps, dirs, scan_offset, poses, t_min=0.0, cull=True):
    """Closest hits of the rays of measured clouds: ray i (view point vps[i], direction dirs[i], f32 | f64 [N,3], sensor frame,
    scan-major) of the scan s with scan_offset[s] <= i < scan_offset[s+1] (S+1 integers from 0 to N: a sequence, checked here, or an int64
    device tensor, taken as it is) is cast
    from R_s vps[i] + t_s along R_s dirs[i] (poses f64 [S,4,4], world from sensor) -> (face i32 [N] (-1 = miss), t f64 [N] in units
    of |dirs[i]| (inf on a miss), inc f64 [N] the incidence angle on the face that was hit (NaN on a miss)).  Hits count beyond
    ``t_min`` (and facing the ray with ``cull``); traversal and tie rule are raycast's.  One launch (dc_raycast_rays)."""
    dev = bvh.leaf_face.device
    n, code, s, off = _measured_rays_arg(dev, vps, dirs, scan_offset, poses)
    tm = _t_min_arg(t_min)[1]
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    t = torch.empty((n,), dtype=torch.float64, device=dev)
    inc = torch.empty((n,), dtype=torch.float64, device=dev)
    if n == 0:
        return face, t, inc
    off = off.to(dev)
    nf = bvh.n_faces
    check(lib().dc_raycast_rays(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                                ptr(vps), ptr(dirs), code, n, ptr(off), ptr(poses), s, tm, 1 if cull else 0, ptr(face), ptr(t),
                                ptr(inc), stream_ptr()), 'dc_raycast_rays')
    return face, t, inc


@on_device
def surfel_bvh_build(points, normals, radii, scene_box):
    """LBVH over the surfels of a surveyed cloud: the two-sided disks (points[i], normals[i], radii[i]), f64 [M,3] / [M,3] / [M]
    (radii finite and > 0 and normals finite and non-zero, checked here), in the box ``scene_box`` (6 floats: lo xyz, hi xyz) ->
    survey.SurfelBVH (leaf_index i32 [M], child i32 [M-1,2], parent i32 [2M-1], node_box f32 [2M-1,6], leaf_disk f64 [M,8])."""
    from .survey import SurfelBVH
    need(points, (None, 3), dtype=torch.float64, name='points')
    dev = points.device
    m = points.shape[0]
    need(normals, (m, 3), dtype=torch.float64, name='normals', device=dev)
    need(radii, (m,), dtype=torch.float64, name='radii', device=dev)
    if m == 0:
        raise ValueError('surfel_bvh_build needs at least one point')
    if not bool((torch.isfinite(radii) & (radii > 0)).all()):
        raise ValueError('surfel radii must be finite and > 0')
    if not bool(torch.isfinite(points).all()):
        raise ValueError('surfel points must be finite')
    if not bool((torch.isfinite(normals).all(dim=1) & (normals != 0).any(dim=1)).all()):
        raise ValueError('surfel normals must be finite and not zero')
    box = _scene_box_arg(scene_box)
    leaf_index, child, parent, node_box = _tree_arrays(m, dev)
    leaf_disk = torch.empty((m, 8), dtype=torch.float64, device=dev)
    nbytes = lib().dc_surfel_bvh_workspace_bytes(m)
    ws = _ws(nbytes, dev)
    check(lib().dc_surfel_bvh_build(ptr(points), ptr(normals), ptr(radii), m, box.ctypes.data_as(ctypes.c_void_p), ptr(leaf_index),
                                    ptr(child) if m > 1 else None, ptr(parent), ptr(node_box), ptr(leaf_disk), ptr(ws), nbytes,
                                    stream_ptr()), 'dc_surfel_bvh_build')
    return SurfelBVH(leaf_index, child, parent, node_box, leaf_disk)


SURFEL_MIN_COS = 0.7071067811865476          # cos(pi / 4): the default normal gate of the surfel blend


@on_device
def surfel_cast_rays(bvh, vps, dirs, scan_offset, poses, t_min=0.0, window=0.0, min_cos=SURFEL_MIN_COS):
    """The rays of raycast_rays (same arguments, same checks) against a survey.SurfelBVH -> (index i32 [N] the survey index of the
    closest disk (-1 = miss), t_first f64 [N] its t (inf), t f64 [N] the blended depth, inc f64 [N] the incidence angle on the
    blended normal (NaN on a miss), count i32 [N] the number of blended disks (0 on a miss)).  The blend takes the disks the ray hits
    within ``window`` (>= 0, along the ray in units of |dirs[i]|) behind the first hit whose normal lies within acos(``min_cos``)
    (0 <= min_cos < 1) of the first hit's, weighted 1 - r^2 / rho^2; window = 0: t = t_first, inc on the first disk, count 1.
    One launch (dc_surfel_cast_rays)."""
    dev = bvh.leaf_index.device
    n, code, s, off = _measured_rays_arg(dev, vps, dirs, scan_offset, poses)
    tm, win, mc = _t_min_arg(t_min)[1], float(window), float(min_cos)
    if not win >= 0.0:
        raise ValueError('window must be >= 0, got %r' % (window,))
    if not 0.0 <= mc < 1.0:
        raise ValueError('min_cos must lie in [0, 1), got %r' % (min_cos,))
    index = torch.empty((n,), dtype=torch.int32, device=dev)
    t_first = torch.empty((n,), dtype=torch.float64, device=dev)
    t = torch.empty((n,), dtype=torch.float64, device=dev)
    inc = torch.empty((n,), dtype=torch.float64, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return index, t_first, t, inc, count
    off = off.to(dev)
    m = bvh.n_disks
    check(lib().dc_surfel_cast_rays(ptr(bvh.child) if m > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_disk), ptr(bvh.leaf_index), m,
                                    ptr(vps), ptr(dirs), code, n, ptr(off), ptr(poses), s, tm, win, mc, ptr(index), ptr(t_first), ptr(t),
                                    ptr(inc), ptr(count), stream_ptr()), 'dc_surfel_cast_rays')
    return index, t_first, t, inc, count


def _beam_pattern_arg(pattern, r0, spread, power_of_two):
    """The footprint pattern as a host float64 [S,3] array, checked the way the library checks it."""
    import numpy as np
    pat = np.ascontiguousarray(np.asarray(pattern.detach().cpu() if isinstance(pattern, torch.Tensor) else pattern, dtype=np.float64))
    if pat.ndim != 2 or pat.shape[1] != 3 or not 1 <= pat.shape[0] <= nv.DC_BEAM_MAX_SAMPLES:
        raise ValueError('pattern must be [S,3] rows (px, py, weight) with 1 <= S <= %d, got shape %s' % (nv.DC_BEAM_MAX_SAMPLES, pat.shape))
    s = pat.shape[0]
    if power_of_two and s & (s - 1):
        raise ValueError('the number of samples per beam must be a power of two, got %d' % s)
    if not np.isfinite(pat).all() or (pat[:, 2] < 0).any():
        raise ValueError('pattern entries must be finite and the weights non-negative')
    r0, spread = float(r0), float(spread)
    if not (0.0 <= r0 < float('inf')) or not (0.0 <= spread < float('inf')):
        raise ValueError('r0 and spread must be finite and >= 0, got %r, %r' % (r0, spread))
    return pat, r0, spread


@on_device
def beam_subrays(vps, dirs, pattern, r0, spread):
    """Sub-rays of finite beams (dc_beam_subrays): beam i (view point vps[i], direction dirs[i], f32 | f64 [N,3], sensor frame) and the
    pattern rows (px, py, weight) [S,3] (host array, units of the 1/e^2 radius) -> (origins f64 [N,S,3], directions f64 [N,S,3]) in
    the sensor frame: origin v + r0 q and direction d + spread q, q = px e1 + py e2 in the beam's frame (include/dc_hip.h).  The
    directions are not normalised: a cast's t along them is the axial depth."""
    need(dirs, (None, 3), name='dirs')
    dev = dirs.device
    n = dirs.shape[0]
    need(vps, (n, 3), dtype=dirs.dtype, name='vps', device=dev)
    code = dtype_code(dirs)
    pat, r0, spread = _beam_pattern_arg(pattern, r0, spread, False)
    s = pat.shape[0]
    origins = torch.empty((n, s, 3), dtype=torch.float64, device=dev)
    out = torch.empty((n, s, 3), dtype=torch.float64, device=dev)
    if n == 0:
        return origins, out
    check(lib().dc_beam_subrays(ptr(vps), ptr(dirs), code, n, pat.ctypes.data_as(ctypes.c_void_p), s, r0, spread, ptr(origins), ptr(out),
                                stream_ptr()), 'dc_beam_subrays')
    return origins, out


@on_device
def raycast_beams(bvh, vps, dirs, scan_offset, poses, pattern, r0, spread, t_min=0.0, cull=True, weight='uniform', detection='quantile',
                  tau=None, min_hits=1, want_samples=False):
    """One return per finite beam (dc_raycast_beams): the S sub-rays of beam_subrays are cast like raycast_rays' rays (scan_offset
    counts beams: S+1 integers from 0 to N as a sequence, checked here, or an int64 device tensor, taken as it is; poses f64 [S,4,4])
    and reduced in the same launch -> (face i32 [N] (-1 = miss), depth f64 [N] axial depth in metres (inf on a miss), n_hits i32 [N]).
    ``weight``: 'uniform' | 'lambert' (the pattern weight times the cosine of incidence); ``detection``: 'quantile' (the t of the
    first hit, ordered by depth, at which the running weight reaches ``tau`` of the total: tau = 1/S (the default) the first return,
    0.5 the weighted median, 1 the last return) | 'mean' (weighted mean depth).  A beam with fewer than ``min_hits`` hits is a miss.
    ``t_min``: a float, or a device tensor f64 [N] of per-beam near clips.  ``want_samples`` adds (sub_face i32 [N,S], sub_t f64
    [N,S], sub_w f64 [N,S]) of every sub-ray (-1 / inf / 0 for one that is not a hit)."""
    dev = bvh.leaf_face.device
    n, code, s, off = _measured_rays_arg(dev, vps, dirs, scan_offset, poses, what='beams')
    pat, r0, spread = _beam_pattern_arg(pattern, r0, spread, True)
    ns = pat.shape[0]
    if weight not in nv.BEAM_WEIGHTS:
        raise ValueError('weight must be one of %s, got %r' % (sorted(nv.BEAM_WEIGHTS), weight))
    if detection not in nv.BEAM_DETECTIONS:
        raise ValueError('detection must be one of %s, got %r' % (sorted(nv.BEAM_DETECTIONS), detection))
    tau = 1.0 / ns if tau is None else float(tau)
    if not 0.0 < tau <= 1.0:
        raise ValueError('tau must lie in (0, 1], got %r' % (tau,))
    if isinstance(min_hits, bool) or int(min_hits) != min_hits or not 1 <= int(min_hits) <= ns:
        raise ValueError('min_hits must be an int in 1 .. %d, got %r' % (ns, min_hits))
    tm_beam, tm = _t_min_arg(t_min, n, dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    depth = torch.empty((n,), dtype=torch.float64, device=dev)
    n_hits = torch.empty((n,), dtype=torch.int32, device=dev)
    sub = ()
    if want_samples:
        sub = (torch.empty((n, ns), dtype=torch.int32, device=dev), torch.empty((n, ns), dtype=torch.float64, device=dev),
               torch.empty((n, ns), dtype=torch.float64, device=dev))
    if n:
        off = off.to(dev)
        nf = bvh.n_faces
        check(lib().dc_raycast_beams(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                                     ptr(vps), ptr(dirs), code, n, ptr(off), ptr(poses), s, pat.ctypes.data_as(ctypes.c_void_p), ns, r0,
                                     spread, ptr(tm_beam), tm, 1 if cull else 0, nv.BEAM_WEIGHTS[weight], nv.BEAM_DETECTIONS[detection], tau,
                                     int(min_hits), ptr(face), ptr(depth), ptr(n_hits), ptr(sub[0]) if sub else None,
                                     ptr(sub[1]) if sub else None, ptr(sub[2]) if sub else None, stream_ptr()), 'dc_raycast_beams')
    return (face, depth, n_hits) + sub


# ------------------------------------------------------------------------------------------------
# moving-sweep rendering and de-skew (dc_raycast.hip, dc_sweep.hip; the model: include/dc_hip.h)
# ------------------------------------------------------------------------------------------------
def _sweep_args(rows, tau, scan_offset, twists, poses=None):
    """The checks sweep_rays, raycast_sweep and deskew share, all ValueError and all made before anything is uploaded or launched:
    ``rows`` ((name, tensor [N,3] or None) pairs, the first one present), tau [N], twists [S,6] finite with |w| <= pi (checked on the
    host copy), poses [S,4,4] where given, and raycast_rays' check of scan_offset.  -> (n, s, offsets on the device, twists f64 on the
    device).  The twists are checked and uploaded at every call (S x 48 bytes); twists given as a device tensor are read back for the
    check first, which synchronises: keep them on the host."""
    import math
    import numpy as np
    first = rows[0][1]
    if not isinstance(first, torch.Tensor) or first.dim() != 2 or first.shape[1] != 3:
        raise ValueError('%s must be a tensor [N,3]' % rows[0][0])
    n = first.shape[0]
    for name, a in rows[1:]:
        if a is not None and (not isinstance(a, torch.Tensor) or tuple(a.shape) != (n, 3)):
            raise ValueError('%s must be a tensor [%d,3] like %s' % (name, n, rows[0][0]))
    if not isinstance(tau, torch.Tensor) or tuple(tau.shape) != (n,):
        raise ValueError('tau must be a tensor of %d sweep times, got %s' % (n, tuple(tau.shape) if isinstance(tau, torch.Tensor) else type(tau)))
    tw = np.asarray(twists.detach().cpu() if isinstance(twists, torch.Tensor) else twists, dtype=np.float64)
    if tw.ndim != 2 or tw.shape[1] != 6:
        raise ValueError('twists must be [S,6] rows (v, w), got shape %s' % (tw.shape,))
    if not np.isfinite(tw).all():
        raise ValueError('twists must be finite')
    if tw.shape[0] and float(np.linalg.norm(tw[:, 3:], axis=1).max()) > math.pi:
        raise ValueError('the rotation of a twist must not exceed pi, got %r' % float(np.linalg.norm(tw[:, 3:], axis=1).max()))
    s = tw.shape[0]
    if poses is not None and (not isinstance(poses, torch.Tensor) or tuple(poses.shape) != (s, 4, 4)):
        raise ValueError('poses must be a tensor [%d,4,4], one per twist' % s)
    off = _scan_offset_arg(scan_offset, s, n, None)         # the device, and with it the rest of a device tensor's checks, come below
    if n and s < 1:
        raise ValueError('rays need at least one scan')
    dev = need(first, name=rows[0][0]).device
    for name, a in rows[1:]:
        if a is not None:
            need(a, dtype=first.dtype, name=name, device=dev)
    need(tau, dtype=torch.float64, name='tau', device=dev)
    if poses is not None:
        need(poses, dtype=torch.float64, name='poses', device=dev)
    off = need(off, dtype=torch.int64, name='scan_offset', device=dev) if off.is_cuda else off.to(dev)
    return n, s, off, torch.as_tensor(np.ascontiguousarray(tw), device=dev)


@on_device
def sweep_rays(vps, dirs, tau, scan_offset, twists):
    """Rays of a moving sweep in the start frame of their scan (dc_sweep_rays): ray i (vps[i], dirs[i], f32 | f64 [N,3], instantaneous
    sensor frame) taken at the sweep time tau[i] (f64 [N]) of the scan s with scan_offset[s] <= i < scan_offset[s+1] under twists[s]
    ([S,6]: v, w; a host array, or a device tensor at the price of a synchronising read-back; checked on the host: finite, |w| <= pi) -> (origins f64 [N,3] = D(tau) vp, directions f64 [N,3] =
    Exp(tau w) dir), D(tau) = [Exp(tau w) | tau v]."""
    n, s, off, tw = _sweep_args((('dirs', dirs), ('vps', vps)), tau, scan_offset, twists)
    dev = dirs.device
    code = dtype_code(dirs)
    origins = torch.empty((n, 3), dtype=torch.float64, device=dev)
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    if n == 0:
        return origins, out
    check(lib().dc_sweep_rays(ptr(vps), ptr(dirs), code, ptr(tau), n, ptr(off), ptr(tw), s, ptr(origins), ptr(out), stream_ptr()),
          'dc_sweep_rays')
    return origins, out


@on_device
def raycast_sweep(bvh, vps, dirs, tau, scan_offset, poses, twists, t_min=0.0, cull=True):
    """The cast of a moving sweep (dc_raycast_sweep): sweep_rays' ray i, posed by poses[s] (f64 [S,4,4], world from sensor at sweep
    time 0), through raycast_rays' traversal -> (face i32 [N], t f64 [N], inc f64 [N]), bit-equal to raycast_rays on sweep_rays'
    output.  ``t_min``: a float, or a device tensor f64 [N] of per-ray near clips.  A ray whose tau is not finite is a miss.  One
    launch."""
    n, s, off, tw = _sweep_args((('dirs', dirs), ('vps', vps)), tau, scan_offset, twists, poses=poses)
    dev = bvh.leaf_face.device
    need(dirs, name='dirs', device=dev)
    code = dtype_code(dirs)
    tm_ray, tm = _t_min_arg(t_min, n, dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    t = torch.empty((n,), dtype=torch.float64, device=dev)
    inc = torch.empty((n,), dtype=torch.float64, device=dev)
    if n == 0:
        return face, t, inc
    nf = bvh.n_faces
    check(lib().dc_raycast_sweep(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                                 ptr(vps), ptr(dirs), code, ptr(tau), n, ptr(off), ptr(poses), ptr(tw), s, ptr(tm_ray), tm,
                                 1 if cull else 0, ptr(face), ptr(t), ptr(inc), stream_ptr()), 'dc_raycast_sweep')
    return face, t, inc


@on_device
def deskew(points, tau, scan_offset, twists, vps=None, normals=None):
    """De-skew (dc_deskew): point i measured at the sweep time tau[i] (f64 [N]) in the instantaneous sensor frame, under the twist of
    its scan (``scan_offset`` / ``twists`` as in sweep_rays) -> (points', vps', normals') f64 [N,3] in the scan's start frame:
    x' = D(tau) x, vp' = D(tau) vp, n' = Exp(tau w) n; None for an input that is None.  Rigid per point: depth and incidence angle
    are kept."""
    n, s, off, tw = _sweep_args((('points', points), ('vps', vps), ('normals', normals)), tau, scan_offset, twists)
    dev = points.device
    code = dtype_code(points)
    outs = [torch.empty((n, 3), dtype=torch.float64, device=dev) if a is not None else None for a in (points, vps, normals)]
    if n:
        check(lib().dc_deskew(ptr(points), ptr(vps), ptr(normals), code, ptr(tau), n, ptr(off), ptr(tw), s, ptr(outs[0]), ptr(outs[1]),
                              ptr(outs[2]), stream_ptr()), 'dc_deskew')
    return tuple(outs)


# ------------------------------------------------------------------------------------------------
# depth bias against the mesh (dc_bias.hip)
# ------------------------------------------------------------------------------------------------
def bias_out_count(n_bins, n_terms):
    """Length of bias_accumulate's ``out`` (DC_BIAS_OUT_COUNT of include/dc_hip.h)."""
    return nv.DC_BIAS_TOTALS + nv.DC_BIAS_BIN_COLS * n_bins + 2 * (2 + n_terms + n_terms * (n_terms + 1) // 2)


@on_device
def bias_accumulate(depth, inc_est, mask, face, t_true, inc_true, model_kind, exponent, n_bins=18, max_residual=None, out=None, ws=None):
    """Binned statistics of r = depth - t_true over the true incidence angle and the normal equations of the supervised fit
    (dc_bias_accumulate; definitions and the layout of the returned f64 [bias_out_count(n_bins, P)] in include/dc_hip.h).  depth /
    inc_est f32 | f64 [N] or [N,1] (inc_est optional), mask bool | uint8 [N] (optional), face i32 / t_true f64 / inc_true f64 [N] of
    raycast_rays, model_kind 'Polynomial' | 'ScaledPolynomial', exponent the P <= 4 exponents (host floats), n_bins <= 256.  ``out`` /
    ``ws`` (bias_workspace) from the caller make the call allocation-free."""
    need(face, (None,), dtype=torch.int32, name='face')
    dev, n = face.device, face.shape[0]
    depth = depth.reshape(-1) if isinstance(depth, torch.Tensor) else depth
    need(depth, (n,), name='depth', device=dev)
    code = dtype_code(depth)
    if inc_est is not None:
        inc_est = inc_est.reshape(-1) if isinstance(inc_est, torch.Tensor) else inc_est
        need(inc_est, (n,), dtype=depth.dtype, name='inc_est', device=dev)
    if mask is not None:
        need(mask, (n,), name='mask', device=dev)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        elif mask.dtype != torch.uint8:
            raise TypeError('mask must be bool or uint8, got %s' % mask.dtype)
    need(t_true, (n,), dtype=torch.float64, name='t_true', device=dev)
    need(inc_true, (n,), dtype=torch.float64, name='inc_true', device=dev)
    if model_kind not in ('Polynomial', 'ScaledPolynomial'):
        raise ValueError("model_kind must be 'Polynomial' or 'ScaledPolynomial', got %r" % (model_kind,))
    e = [float(x) for x in (exponent.detach().reshape(-1).tolist() if isinstance(exponent, torch.Tensor) else exponent)]
    p, b = len(e), int(n_bins)
    if not 1 <= p <= nv.DC_BIAS_MAX_TERMS or not 1 <= b <= nv.DC_BIAS_MAX_BINS:
        raise ValueError('bias_accumulate takes 1..%d terms and 1..%d bins, got %d and %d' % (nv.DC_BIAS_MAX_TERMS, nv.DC_BIAS_MAX_BINS, p, b))
    count = bias_out_count(b, p)
    out = _out_arg(out, count, dev)
    nbytes = lib().dc_bias_workspace_bytes(b, p)
    if ws is None:
        ws = _ws(nbytes, dev)
    need(ws, (None,), dtype=torch.uint8, name='ws', device=dev)
    e_host = (ctypes.c_double * p)(*e)
    check(lib().dc_bias_accumulate(ptr(depth), ptr(inc_est), code, ptr(mask), ptr(face), ptr(t_true), ptr(inc_true), n,
                                   nv.MODEL_KINDS[model_kind], ctypes.cast(e_host, ctypes.c_void_p), p, b,
                                   0.0 if max_residual is None else float(max_residual), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          'dc_bias_accumulate')
    return out


def bias_workspace(n_bins, n_terms, device):
    """Workspace of bias_accumulate for the given sizes (uint8 tensor)."""
    return _ws(lib().dc_bias_workspace_bytes(int(n_bins), int(n_terms)), device)


# ------------------------------------------------------------------------------------------------
# map accuracy against a mesh (dc_meshdist.hip)
# ------------------------------------------------------------------------------------------------
@on_device
def mesh_closest(bvh, points, max_dist=None, want_closest=True):
    """Nearest triangle of the mesh behind ``bvh`` (mesh.MeshBVH) for every row of points f32 | f64 [N,3] (world frame) -> (face i32
    [N], dist f64 [N], closest f64 [N,3] or None without ``want_closest``): the smallest distance wins, equal distance the lower
    face index.  With ``max_dist`` a point whose nearest triangle is farther gets -1 / inf / NaN, as does a row holding a NaN or an
    infinity.  One launch (dc_mesh_closest)."""
    dev = bvh.leaf_face.device
    need(points, (None, 3), name='points', device=dev)
    code = dtype_code(points)
    n = points.shape[0]
    md = 0.0 if max_dist is None else float(max_dist)
    if md != md:
        raise ValueError('max_dist must not be NaN')
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    dist = torch.empty((n,), dtype=torch.float64, device=dev)
    closest = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_closest else None
    nf = bvh.n_faces
    check(lib().dc_mesh_closest(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                                ptr(points), code, n, md, ptr(face), ptr(dist), ptr(closest), stream_ptr()), 'dc_mesh_closest')
    return face, dist, closest


def mesh_loss_workspace(n, n_scans, n_terms, device):
    """Workspace of mesh_loss for the given sizes (uint8 tensor)."""
    return _ws(lib().dc_mesh_loss_workspace_bytes(int(n), int(n_scans), int(n_terms)), device)


def _check_scan_ptr(ps, scan_ptr):
    """scan_ptr int64 [S+1] on the points' device, ascending from 0 to ps.n: read back once per (PointSet, tensor) -- the kernel lays
    its blocks out from it."""
    need(scan_ptr, (None,), dtype=torch.int64, name='scan_ptr', device=ps.device)
    if scan_ptr.shape[0] < 2:
        raise ValueError('scan_ptr needs at least two entries ([S+1]), got %d' % scan_ptr.shape[0])
    seen = getattr(ps, '_scan_ptr_checked', None)
    if seen is None or seen[0] is not scan_ptr or seen[1] != scan_ptr._version:
        host = scan_ptr.tolist()
        if host[0] != 0 or host[-1] != ps.n or any(b < a for a, b in zip(host, host[1:])):
            raise ValueError('scan_ptr must ascend from 0 to the number of points (%d), got %s' % (ps.n, host))
        ps._scan_ptr_checked = (scan_ptr, scan_ptr._version)
    return scan_ptr.shape[0] - 1


def _scan_loss_args(ps, scan_ptr, poses12, model_kind, w, e, mask, dev):
    """The operand checks mesh_loss and cloud_loss share -> (kind, n_terms, w, e, n_scans)."""
    kind, nt, w, e = _model_args(model_kind, w, e, ps)
    ns = _check_scan_ptr(ps, scan_ptr)
    need(poses12, (ns, 12), dtype=torch.float64, name='poses[S,12]', device=dev)
    if mask is not None:
        need(mask, (ps.n,), dtype=torch.bool, name='mask', device=dev)
    return kind, nt, w, e, ns


@on_device
def mesh_loss(bvh, ps, scan_ptr, poses12, model_kind=None, w=None, e=None, mask=None, squared=False, max_dist=None, leaf_hint=None,
              want_points=False, want_exponent=False, out=None, ws=None):
    """Mean distance of the corrected, posed points of a sequence to the mesh behind ``bvh`` (mesh.MeshBVH), with its gradient, in
    one host call (dc_mesh_loss).  ``ps``: PointSet of the scans' sensor-frame fields, scan-major (its lmask: the points the model
    corrects; its scan_id is not used); ``scan_ptr`` int64 [S+1]: scan s holds the points scan_ptr[s] .. scan_ptr[s+1]; ``poses12``
    f64 [S,12].  ``mask`` bool [N]: the points that enter the loss; ``max_dist``: points farther from the mesh are left out (gated).
    Returns out f64 [4 + 2P + 12 S] = {mean loss, used, gated, invalid, dL/dw, dL/dexponent (zero unless ``want_exponent``),
    dL/d[R|t]}; with ``want_points`` also (face i32 [N], dist f64 [N], closest f64 [N,3]) -- what mesh_closest gives for the
    points, -1 / inf / NaN where a point is not used.  ``leaf_hint`` int32 [N] is read and written: the winning leaves of the last
    call shorten the walk of this one and never change a bit of a result (start it at -1)."""
    dev = bvh.leaf_face.device
    if ps.device != dev:
        raise RuntimeError('points are on %s, the mesh on %s' % (ps.device, dev))
    kind, nt, w, e, ns = _scan_loss_args(ps, scan_ptr, poses12, model_kind, w, e, mask, dev)
    if leaf_hint is not None:
        need(leaf_hint, (ps.n,), dtype=torch.int32, name='leaf_hint', device=dev)
    md = 0.0 if max_dist is None else float(max_dist)
    if md != md:
        raise ValueError('max_dist must not be NaN')
    n_out = 4 + 2 * nt + 12 * ns
    out = _out_arg(out, n_out, dev)
    ws = _ws_arg(ws, lib().dc_mesh_loss_workspace_bytes(ps.n, ns, nt), dev)
    face = dist = closest = None
    if want_points:
        face = torch.empty((ps.n,), dtype=torch.int32, device=dev)
        dist = torch.empty((ps.n,), dtype=torch.float64, device=dev)
        closest = torch.empty((ps.n, 3), dtype=torch.float64, device=dev)
    nf = bvh.n_faces
    check(lib().dc_mesh_loss(ptr(bvh.child) if nf > 1 else None, ptr(bvh.node_box), ptr(bvh.leaf_tri), ptr(bvh.leaf_face), nf,
                             ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth), ptr(ps.inc), ptr(ps.lmask), ptr(mask), dtype_code(ps.dirs), ps.n,
                             ptr(scan_ptr), ptr(poses12), ns, kind, nt, ptr(w), ptr(e), int(bool(want_exponent)), int(bool(squared)), md,
                             ptr(leaf_hint), ptr(face), ptr(dist), ptr(closest), ptr(out), ptr(ws), ws.shape[0], stream_ptr()),
          'dc_mesh_loss')
    return (out, face, dist, closest) if want_points else out


@on_device
def mesh_sample(verts, faces, area_cdf, n_samples, seed):
    """``n_samples`` area-weighted samples of the mesh verts f64 [V,3] / faces i32 [F,3] (indices checked by the caller, as for
    bvh_build) with area_cdf f64 [F] the inclusive prefix sum of the face areas -> (face i32 [n], points f64 [n,3]); a pure function
    of (mesh, n_samples, seed) (dc_mesh_sample)."""
    need(verts, (None, 3), dtype=torch.float64, name='verts')
    dev = verts.device
    need(faces, (None, 3), dtype=torch.int32, name='faces', device=dev)
    nf = faces.shape[0]
    need(area_cdf, (nf,), dtype=torch.float64, name='area_cdf', device=dev)
    n, seed = int(n_samples), int(seed)
    if nf < 1 or n < 0:
        raise ValueError('mesh_sample needs at least one face and n_samples >= 0')
    if not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError('seed must fit a signed 64-bit integer, got %d' % seed)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    check(lib().dc_mesh_sample(ptr(verts), ptr(faces), nf, ptr(area_cdf), n, seed, ptr(face), ptr(pts), stream_ptr()), 'dc_mesh_sample')
    return face, pts


# ------------------------------------------------------------------------------------------------
# SLAM evaluation: scan-to-map point-to-plane ICP (csrc/dc_slam.hip, slam.py).  The per-iteration wrappers take every output and
# workspace from the caller, so a queue of iterations allocates nothing and copies nothing.
# ------------------------------------------------------------------------------------------------
class KnnGrid(object):
    """A k-NN grid of ``n`` points kept in ``ws`` for later queries of at most ``n_query_max`` points (dc_knn_grid_build)."""

    def __init__(self, ws, n, n_query_max, device):
        self.ws, self.n, self.n_query_max, self.device = ws, n, n_query_max, device


@on_device
def knn_grid_build(points, n_query_max, k, cell_hint=0.0, ws=None):
    """Grid of points [N,3] (N >= 1) for k-NN queries of up to ``n_query_max`` points; ``ws`` (uint8, optional) is reused when large
    enough (dc_knn_grid_build)."""
    need(points, (None, 3), name='points')
    n = points.shape[0]
    if n < 1:
        raise ValueError('knn_grid_build needs at least one point')
    nbytes = lib().dc_knn_workspace_bytes(n, n_query_max)
    if ws is None or ws.numel() < nbytes or ws.device != points.device:
        ws = _ws(nbytes, points.device)
    check(lib().dc_knn_grid_build(ptr(points), 3, dtype_code(points), n, int(n_query_max), int(k), float(cell_hint), ptr(ws), ws.numel(),
                                  stream_ptr()), 'dc_knn_grid_build')
    return KnnGrid(ws, n, int(n_query_max), points.device)


@on_device
def knn_grid_query(grid, query, pose, k, r=None, stop=None, idx=None, dist=None):
    """k-NN of ``pose @ query`` (query f64 [M,3], pose f64 device [4,4]) in ``grid`` -> (dist f64 [M,k], idx i32 [M,k]), written into
    ``idx`` / ``dist`` when given; ``stop`` (int32 device word): rows -1 / inf once it is non-zero (dc_knn_grid_query)."""
    need(query, (None, 3), dtype=torch.float64, name='query', device=grid.device)
    need(pose, (4, 4), dtype=torch.float64, name='pose', device=grid.device)
    m = query.shape[0]
    if m > grid.n_query_max:
        raise ValueError('%d queries, the grid was built for %d' % (m, grid.n_query_max))
    idx = torch.empty((m, k), dtype=torch.int32, device=grid.device) if idx is None else need(idx, (m, k), torch.int32, 'idx', grid.device)
    dist = torch.empty((m, k), dtype=torch.float64, device=grid.device) if dist is None else need(dist, (m, k), torch.float64, 'dist',
                                                                                                  grid.device)
    if stop is not None:
        need(stop, None, dtype=torch.int32, name='stop', device=grid.device)
    check(lib().dc_knn_grid_query(grid.n, grid.n_query_max, ptr(query), m, ptr(pose), ptr(stop), int(k), float(r) if r else 0.0,
                                  ptr(idx), ptr(dist), ptr(grid.ws), grid.ws.numel(), stream_ptr()), 'dc_knn_grid_query')
    return dist, idx


@on_device
def quantile(v, ratio, stop=None, out=None, ws=None):
    """np.quantile(v[isfinite(v)], ratio) of non-negative v (f64, any shape) as a device f64 [1] (``out`` when given), by dc_nn1_corr's
    radix select; NaN and +inf entries (missing neighbours) are not counted, NaN when nothing is left; ``stop`` as in knn_grid_query
    (dc_quantile)."""
    need(v, None, dtype=torch.float64, name='v')
    n = v.numel()
    nbytes = lib().dc_quantile_workspace_bytes()
    ws = _ws(nbytes, v.device) if ws is None else ws
    out = torch.empty((1,), dtype=torch.float64, device=v.device) if out is None else need(out, (1,), torch.float64, 'out', v.device)
    check(lib().dc_quantile(ptr(v), n, float(ratio), ptr(stop), ptr(out), ptr(ws), ws.numel(), stream_ptr()), 'dc_quantile')
    return out


def cloud_loss_workspace(n, n_scans, n_terms, device):
    """Workspace of cloud_loss for the given sizes (uint8 tensor)."""
    return _ws(lib().dc_cloud_loss_workspace_bytes(int(n), int(n_scans), int(n_terms)), device)


@on_device
def cloud_loss(survey_dev, ps, scan_ptr, poses12, model_kind=None, w=None, e=None, mask=None, plane=True, squared=False, max_dist=None,
               inlier_ratio=1.0, want_points=False, want_exponent=False, out=None, ws=None):
    """Mean point-to-plane (``plane``) or point-to-point distance of the corrected, posed points of a sequence to their nearest points
    of a surveyed cloud, with its gradient, in one host call (dc_cloud_loss).  ``survey_dev``: survey.SurveyOnDevice (points, unit
    normals, the persistent k-NN grid); ``ps``, ``scan_ptr``, ``poses12``, ``mask`` as for mesh_loss.  ``max_dist`` (required, finite,
    > 0): points without a survey point within it are gated; ``inlier_ratio`` < 1: points whose nearest-neighbour distance exceeds
    that quantile of the matched distances are trimmed.  Returns out f64 [6 + 2P + 12 S] = {mean loss, used, gated, trimmed, invalid,
    threshold, dL/dw, dL/dexponent (zero unless ``want_exponent``), dL/d[R|t]}; with ``want_points`` also (idx i32 [N], dist f64 [N],
    resid f64 [N]) -- the survey point, its distance and the residual r of every used point, -1 / inf / NaN elsewhere."""
    dev = survey_dev.device
    if ps.device != dev:
        raise RuntimeError('points are on %s, the survey on %s' % (ps.device, dev))
    kind, nt, w, e, ns = _scan_loss_args(ps, scan_ptr, poses12, model_kind, w, e, mask, dev)
    if max_dist is None:
        raise ValueError('cloud_loss needs max_dist (finite, > 0)')
    md, ratio = float(max_dist), float(inlier_ratio)
    if not (md > 0.0 and md < float('inf')):
        raise ValueError('max_dist must be finite and > 0, got %r' % (max_dist,))
    if not 0.0 <= ratio <= 1.0:
        raise ValueError('inlier_ratio must lie in [0, 1], got %r' % (inlier_ratio,))
    need(survey_dev.points, (None, 3), dtype=torch.float64, name='survey points', device=dev)
    need(survey_dev.normals, (survey_dev.points.shape[0], 3), dtype=torch.float64, name='survey normals', device=dev)
    survey_dev.reserve(ps.n)
    grid = survey_dev.grid
    n_out = 6 + 2 * nt + 12 * ns
    out = _out_arg(out, n_out, dev)
    ws = _ws_arg(ws, lib().dc_cloud_loss_workspace_bytes(ps.n, ns, nt), dev)
    idx = dist = resid = None
    if want_points:
        idx = torch.empty((ps.n,), dtype=torch.int32, device=dev)
        dist = torch.empty((ps.n,), dtype=torch.float64, device=dev)
        resid = torch.empty((ps.n,), dtype=torch.float64, device=dev)
    check(lib().dc_cloud_loss(ptr(grid.ws), grid.ws.numel(), grid.n_query_max, ptr(survey_dev.points), ptr(survey_dev.normals), grid.n,
                              ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth), ptr(ps.inc), ptr(ps.lmask), ptr(mask), dtype_code(ps.dirs), ps.n,
                              ptr(scan_ptr), ptr(poses12), ns, kind, nt, ptr(w), ptr(e), int(bool(want_exponent)), int(bool(plane)),
                              int(bool(squared)), md, ratio, ptr(idx), ptr(dist), ptr(resid), ptr(out), ptr(ws), ws.shape[0],
                              stream_ptr()), 'dc_cloud_loss')
    return (out, idx, dist, resid) if want_points else out


# ------------------------------------------------------------------------------------------------
# survey registration: trimmed closed-form ICP against a surveyed cloud (csrc/dc_align.hip, registration.py).  As for the SLAM
# wrappers every output and workspace is the caller's: a queue of iterations allocates nothing and copies nothing.
# ------------------------------------------------------------------------------------------------
def align_blocks(n):
    """Blocks (rows of partials) of align_accumulate for n query points (dc_align_blocks)."""
    return int(lib().dc_align_blocks(int(n)))


def _align_state_args(state, status, dev):
    need(state, (nv.DC_ALIGN_STATE_COUNT,), dtype=torch.float64, name='state', device=dev)
    need(status, (4,), dtype=torch.int32, name='status', device=dev)


@on_device
def align_init(state, status, prior=None, history=None):
    """state f64 [DC_ALIGN_STATE_COUNT] / status i32 [4] of a registration that starts from prior f64 device [4,4] (None: the
    identity); history f64 [n_iters, 5] (optional) is filled with NaN (dc_align_init)."""
    dev = state.device
    _align_state_args(state, status, dev)
    if prior is not None:
        need(prior, (4, 4), dtype=torch.float64, name='prior', device=dev)
    rows = 0
    if history is not None:
        need(history, (None, nv.DC_ALIGN_HISTORY_COLS), dtype=torch.float64, name='history', device=dev)
        rows = history.shape[0]
    check(lib().dc_align_init(ptr(prior), ptr(state), ptr(status), ptr(history) if rows else None, rows, stream_ptr()), 'dc_align_init')


@on_device
def align_accumulate(query, map_points, idx, dist, threshold, origins, partials, status=None, kept=None):
    """Moments of the kept pairs (idx >= 0 and dist <= threshold) of query f64 [N,3] and map_points[idx] about origins f64 [6] -> block
    partials f64 [align_blocks(N), DC_ALIGN_PARTIALS] (dc_align_accumulate); idx i32 / dist f64 [N] or [N,1] as knn_grid_query returns
    them; ``kept`` (uint8 [N], optional) receives the kept flags; ``status`` (i32 [4], optional): nothing is done once it is set."""
    dev = query.device
    need(query, (None, 3), dtype=torch.float64, name='query')
    n = query.shape[0]
    if n < 1:
        raise ValueError('align_accumulate needs at least one query point')
    need(map_points, (None, 3), dtype=torch.float64, name='map_points', device=dev)
    if map_points.shape[0] < 1:
        raise ValueError('align_accumulate needs at least one map point')
    if idx.dim() == 2:
        idx, dist = idx.reshape(-1), dist.reshape(-1)
    need(idx, (n,), dtype=torch.int32, name='idx', device=dev)
    need(dist, (n,), dtype=torch.float64, name='dist', device=dev)
    need(threshold, (1,), dtype=torch.float64, name='threshold', device=dev)
    need(origins, (6,), dtype=torch.float64, name='origins', device=dev)
    nb = align_blocks(n)
    need(partials, (nb, nv.DC_ALIGN_PARTIALS), dtype=torch.float64, name='partials', device=dev)
    if status is not None:
        need(status, (4,), dtype=torch.int32, name='status', device=dev)
    if kept is not None:
        need(kept, (n,), dtype=torch.uint8, name='kept', device=dev)
    check(lib().dc_align_accumulate(ptr(query), n, ptr(map_points), map_points.shape[0], ptr(idx), ptr(dist), ptr(threshold), ptr(origins),
                                    ptr(status), ptr(partials), nb, ptr(kept), stream_ptr()), 'dc_align_accumulate')


@on_device
def align_finish(partials, origins, state, status, min_rot=0.0, min_trans=0.0, min_pairs=3, max_iters=1, history=None):
    """Sum the partials, fit, update and check one registration iteration in one block (dc_align_finish); history f64 [rows, 5]
    (optional): the row of this iteration is written."""
    dev = partials.device
    need(partials, (None, nv.DC_ALIGN_PARTIALS), dtype=torch.float64, name='partials')
    need(origins, (6,), dtype=torch.float64, name='origins', device=dev)
    _align_state_args(state, status, dev)
    rows = 0
    if history is not None:
        need(history, (None, nv.DC_ALIGN_HISTORY_COLS), dtype=torch.float64, name='history', device=dev)
        rows = history.shape[0]
    check(lib().dc_align_finish(ptr(partials), partials.shape[0], ptr(origins), float(min_rot), float(min_trans), int(min_pairs),
                                int(max_iters), ptr(state), ptr(status), ptr(history) if rows else None, rows, stream_ptr()), 'dc_align_finish')


def survey_align_workspace(n, device):
    """Workspace of survey_align for n query points (uint8 tensor)."""
    return _ws(lib().dc_survey_align_workspace_bytes(int(n)), device)


@on_device
def survey_align(survey_dev, query, origins, prior=None, inlier_ratio=1.0, max_dist=None, n_iters=100, min_rot=0.0, min_trans=0.0,
                 min_pairs=3, state=None, status=None, history=None, ws=None):
    """A whole trimmed closed-form ICP of query f64 [N,3] (N >= 1) against ``survey_dev`` (survey.SurveyOnDevice) queued on the stream
    in one host call (dc_survey_align): n_iters x {knn_grid_query, quantile, align_accumulate, align_finish}, which return at once
    after the status word is set.  origins f64 device [6] = (o_p, o_y); prior f64 device [4,4] (None: the identity).  Returns (state
    f64 [DC_ALIGN_STATE_COUNT], status i32 [4], history f64 [n_iters, 5]) -- device tensors, nothing is read back."""
    dev = survey_dev.device
    need(query, (None, 3), dtype=torch.float64, name='query', device=dev)
    n = query.shape[0]
    if n < 1:
        raise ValueError('survey_align needs at least one query point')
    if max_dist is None:
        raise ValueError('survey_align needs max_dist (finite, > 0)')
    md, ratio, n_iters, min_pairs = float(max_dist), float(inlier_ratio), int(n_iters), int(min_pairs)
    if not (md > 0.0 and md < float('inf')):
        raise ValueError('max_dist must be finite and > 0, got %r' % (max_dist,))
    if not 0.0 < ratio <= 1.0:
        raise ValueError('inlier_ratio must lie in (0, 1], got %r' % (inlier_ratio,))
    if n_iters < 1 or min_pairs < 3 or not float(min_rot) >= 0.0 or not float(min_trans) >= 0.0:
        raise ValueError('survey_align needs n_iters >= 1, min_pairs >= 3 and min_rot, min_trans >= 0')
    need(origins, (6,), dtype=torch.float64, name='origins', device=dev)
    if prior is not None:
        need(prior, (4, 4), dtype=torch.float64, name='prior', device=dev)
    need(survey_dev.points, (None, 3), dtype=torch.float64, name='survey points', device=dev)
    survey_dev.reserve(n)
    grid = survey_dev.grid
    state = torch.empty((nv.DC_ALIGN_STATE_COUNT,), dtype=torch.float64, device=dev) if state is None else state
    status = torch.empty((4,), dtype=torch.int32, device=dev) if status is None else status
    _align_state_args(state, status, dev)
    if history is None:
        history = torch.empty((n_iters, nv.DC_ALIGN_HISTORY_COLS), dtype=torch.float64, device=dev)
    else:
        need(history, (n_iters, nv.DC_ALIGN_HISTORY_COLS), dtype=torch.float64, name='history', device=dev)
    ws = _ws_arg(ws, lib().dc_survey_align_workspace_bytes(n), dev)
    check(lib().dc_survey_align(ptr(grid.ws), grid.ws.numel(), grid.n_query_max, ptr(survey_dev.points), grid.n, ptr(query), n, ptr(prior),
                                ratio, md, n_iters, float(min_rot), float(min_trans), min_pairs, ptr(origins), ptr(state), ptr(status),
                                ptr(history), ptr(ws), ws.shape[0], stream_ptr()), 'dc_survey_align')
    return state, status, history


# ------------------------------------------------------------------------------------------------
# global registration, the coarse stage (csrc/dc_globalreg.hip, registration.register_global)
# ------------------------------------------------------------------------------------------------
def feature_nn_tile():
    """Survey rows per LDS tile of feature_nn (dc_feature_nn_tile)."""
    return int(lib().dc_feature_nn_tile())


@on_device
def pair_histograms(points, normals, nbr_idx, nbr_dist=None, want_spfh=False):
    """Folded pair-feature descriptors of points / normals f64 [N,3] over the neighbour table nbr_idx i32 [N,k] (k <= 64, -1 for a
    missing slot; as ops.knn returns it): (feat f32 [N,33], has i32 [N]) by dc_pair_spfh + dc_pair_fpfh; with ``want_spfh`` also (spfh
    f64 [N,33], m i32 [N]), the simplified histograms and the valid pairs per row.  ``nbr_dist`` (f64 [N,k], ops.knn's other result) is
    checked for its shape only: a pair's length is taken from the points, by the rule of the pair feature."""
    need(points, (None, 3), dtype=torch.float64, name='points')
    dev = points.device
    n = points.shape[0]
    need(normals, (n, 3), dtype=torch.float64, name='normals', device=dev)
    need(nbr_idx, (n, None), dtype=torch.int32, name='nbr_idx', device=dev)
    k = nbr_idx.shape[1]
    if not 1 <= k <= 64:
        raise ValueError('the neighbour table must have 1..64 slots per row, got %d' % k)
    if nbr_dist is not None:
        need(nbr_dist, (n, k), dtype=torch.float64, name='nbr_dist', device=dev)
    spfh = torch.empty((n, nv.DC_GREG_FEAT), dtype=torch.float64, device=dev)
    m = torch.empty((n,), dtype=torch.int32, device=dev)
    feat = torch.empty((n, nv.DC_GREG_FEAT), dtype=torch.float32, device=dev)
    has = torch.empty((n,), dtype=torch.int32, device=dev)
    check(lib().dc_pair_spfh(ptr(points), ptr(normals), n, ptr(nbr_idx), k, ptr(spfh), ptr(m), stream_ptr()), 'dc_pair_spfh')
    check(lib().dc_pair_fpfh(ptr(points), ptr(normals), n, ptr(nbr_idx), k, ptr(spfh), ptr(feat), ptr(has), stream_ptr()), 'dc_pair_fpfh')
    return (feat, has, spfh, m) if want_spfh else (feat, has)


@on_device
def feature_nn(feat_q, has_q, feat_s, has_s):
    """(idx i32 [Nq], dist f32 [Nq]): the nearest row of feat_s f32 [Ns,33] to every row of feat_q f32 [Nq,33] by the fp32 squared
    distance in bin order, the lower survey row among equal distances; rows with has == 0 (i32) take no part on either side, a cloud
    row without a match gets -1 / +inf (dc_feature_nn)."""
    need(feat_q, (None, nv.DC_GREG_FEAT), dtype=torch.float32, name='feat_q')
    dev = feat_q.device
    nq = feat_q.shape[0]
    need(has_q, (nq,), dtype=torch.int32, name='has_q', device=dev)
    need(feat_s, (None, nv.DC_GREG_FEAT), dtype=torch.float32, name='feat_s', device=dev)
    ns = feat_s.shape[0]
    need(has_s, (ns,), dtype=torch.int32, name='has_s', device=dev)
    idx = torch.empty((nq,), dtype=torch.int32, device=dev)
    dist = torch.empty((nq,), dtype=torch.float32, device=dev)
    check(lib().dc_feature_nn(ptr(feat_q), ptr(has_q), nq, ptr(feat_s), ptr(has_s), ns, ptr(idx), ptr(dist), stream_ptr()), 'dc_feature_nn')
    return idx, dist


def _greg_pairs(p, y):
    need(p, (None, 3), dtype=torch.float64, name='p')
    need(y, (p.shape[0], 3), dtype=torch.float64, name='y', device=p.device)
    return p.shape[0]


@on_device
def greg_fit(p, y, origins, n_hypotheses, seed, min_edge, edge_ratio=0.9):
    """(valid i32 [K], T f64 [K,4,4]): hypothesis h draws three of the correspondences p / y f64 [C,3] (splitmix64(seed ^ (h << 2) ^ t)
    mod C), checks that they are distinct and that every edge is at least ``min_edge`` long and within ``edge_ratio`` of its image,
    and fits them in closed form about origins f64 device [6]; NaN transforms where it is not valid (dc_greg_fit)."""
    c = _greg_pairs(p, y)
    dev = p.device
    need(origins, (6,), dtype=torch.float64, name='origins', device=dev)
    k, seed, min_edge, rho = int(n_hypotheses), int(seed), float(min_edge), float(edge_ratio)
    if k < 0 or k > 0x7fffffff:
        raise ValueError('n_hypotheses must lie in 0..2^31-1, got %r' % (n_hypotheses,))
    if not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError('seed must fit a signed 64-bit integer, got %d' % seed)
    if not min_edge >= 0.0 or not 0.0 < rho <= 1.0:
        raise ValueError('greg_fit needs min_edge >= 0 and 0 < edge_ratio <= 1, got %r and %r' % (min_edge, rho))
    valid = torch.empty((k,), dtype=torch.int32, device=dev)
    T = torch.empty((k, 4, 4), dtype=torch.float64, device=dev)
    check(lib().dc_greg_fit(ptr(p), ptr(y), c, k, seed, min_edge, rho, ptr(origins), ptr(valid), ptr(T), stream_ptr()), 'dc_greg_fit')
    return valid, T


@on_device
def greg_score(valid, T, p, y, eps, want_list=False):
    """score i32 [K]: for every valid hypothesis the number of correspondences p / y f64 [C,3] with |T_h p - y|^2 <= eps^2, -1 for the
    others (dc_greg_score over the valid hypotheses in ascending order, compacted on the device: ONE host read, of their number).
    With ``want_list`` also that list (i32)."""
    c = _greg_pairs(p, y)
    dev = p.device
    need(valid, (None,), dtype=torch.int32, name='valid', device=dev)
    k = valid.shape[0]
    need(T, (k, 4, 4), dtype=torch.float64, name='T', device=dev)
    eps = float(eps)
    if not (eps >= 0.0 and eps < float('inf')):
        raise ValueError('eps must be finite and >= 0, got %r' % (eps,))
    vlist = torch.nonzero(valid).reshape(-1).to(torch.int32)        # ascending; the read of its length
    score = torch.full((k,), -1, dtype=torch.int32, device=dev)
    check(lib().dc_greg_score(ptr(vlist), vlist.shape[0], ptr(T), k, ptr(p), ptr(y), c, eps, ptr(score), stream_ptr()), 'dc_greg_score')
    return (score, vlist) if want_list else score


# ------------------------------------------------------------------------------------------------
# plane registration, the coarse stage from plane correspondences (csrc/dc_planereg.hip, registration.register_planes)
# ------------------------------------------------------------------------------------------------
def planereg_triples(cloud_planes, min_det):
    """int32 device [U,3]: the triples a < b < c of cloud_planes f64 device [Pc,4] with |det[n_a n_b n_c]| >= min_det in lexicographic
    order, the determinant in the order of csrc/dc_planereg_math.h (a torch expression: at most 41 664 rows)."""
    need(cloud_planes, (None, 4), dtype=torch.float64, name='cloud_planes')
    pc = cloud_planes.shape[0]
    abc = torch.combinations(torch.arange(pc, device=cloud_planes.device), 3)          # lexicographic
    n = cloud_planes[:, :3]
    a, b, c = n[abc[:, 0]], n[abc[:, 1]], n[abc[:, 2]]
    m0 = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    m1 = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    m2 = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    det = (a[:, 0] * m0 + a[:, 1] * m1) + a[:, 2] * m2
    return abc[det.abs() >= float(min_det)].to(torch.int32).contiguous()


def _planereg_args(cloud_planes, support, survey_planes, triples, h_begin, h_end, min_det, tol_dot, cos_tol, tol_d, who):
    need(cloud_planes, (None, 4), dtype=torch.float64, name='cloud_planes')
    dev = cloud_planes.device
    pc = cloud_planes.shape[0]
    need(support, (pc,), dtype=torch.int64, name='support', device=dev)
    need(survey_planes, (None, 4), dtype=torch.float64, name='survey_planes', device=dev)
    ps = survey_planes.shape[0]
    need(triples, (None, 3), dtype=torch.int32, name='triples', device=dev)
    u = triples.shape[0]
    total = u * ps ** 3 * 8
    h_begin, h_end = int(h_begin), total if h_end is None else int(h_end)
    tol = tuple(float(v) for v in (min_det, tol_dot, cos_tol, tol_d))
    if not (nv.DC_PLANEREG_MIN_PLANES <= pc <= nv.DC_PLANEREG_MAX_PLANES and nv.DC_PLANEREG_MIN_PLANES <= ps <= nv.DC_PLANEREG_MAX_PLANES):
        raise ValueError('%s needs 3..64 planes a side, got %d and %d' % (who, pc, ps))
    if not 0 <= h_begin <= h_end <= total:
        raise ValueError('%s: the range %d..%d lies outside the %d hypotheses' % (who, h_begin, h_end, total))
    if not all(math.isfinite(v) for v in tol) or tol[0] < 0.0 or tol[1] < 0.0 or tol[3] < 0.0:
        raise ValueError('%s needs finite tolerances, min_det, tol_dot and tol_d >= 0, got %r' % (who, tol))
    return dev, pc, ps, u, h_begin, h_end, tol


@on_device
def planereg_count(cloud_planes, support, survey_planes, triples, min_det, tol_dot, cos_tol, tol_d, h_begin=0, h_end=None):
    """counts i32 [blocks]: the valid hypotheses of every block's range of h_begin <= h < h_end (default: the whole enumeration,
    U Ps^3 8) over the plane tables cloud_planes f64 [Pc,4] / support i64 [Pc] / survey_planes f64 [Ps,4] and the cloud triples i32
    [U,3] of planereg_triples (dc_planereg_count; the rules: csrc/dc_planereg_math.h)."""
    dev, pc, ps, u, h0, h1, tol = _planereg_args(cloud_planes, support, survey_planes, triples, h_begin, h_end, min_det, tol_dot, cos_tol,
                                                 tol_d, 'planereg_count')
    counts = torch.empty((int(lib().dc_planereg_blocks(h1 - h0)),), dtype=torch.int32, device=dev)
    check(lib().dc_planereg_count(ptr(cloud_planes), ptr(support), pc, ptr(survey_planes), ps, ptr(triples), u, h0, h1, *tol, ptr(counts),
                                  stream_ptr()), 'dc_planereg_count')
    return counts


@on_device
def planereg_fill(cloud_planes, support, survey_planes, triples, min_det, tol_dot, cos_tol, tol_d, offsets, n_valid, h_begin=0, h_end=None):
    """(h i64 [n_valid] ascending, T f64 [n_valid,4,4], score i64 [n_valid]) of the valid hypotheses, written at offsets i64 [blocks],
    the exclusive scan of planereg_count's counts for the same arguments (dc_planereg_fill)."""
    dev, pc, ps, u, h0, h1, tol = _planereg_args(cloud_planes, support, survey_planes, triples, h_begin, h_end, min_det, tol_dot, cos_tol,
                                                 tol_d, 'planereg_fill')
    need(offsets, (int(lib().dc_planereg_blocks(h1 - h0)),), dtype=torch.int64, name='offsets', device=dev)
    n_valid = int(n_valid)
    h = torch.empty((n_valid,), dtype=torch.int64, device=dev)
    T = torch.empty((n_valid, 4, 4), dtype=torch.float64, device=dev)
    score = torch.empty((n_valid,), dtype=torch.int64, device=dev)
    check(lib().dc_planereg_fill(ptr(cloud_planes), ptr(support), pc, ptr(survey_planes), ps, ptr(triples), u, h0, h1, *tol, ptr(offsets),
                                 n_valid, ptr(h), ptr(T), ptr(score), stream_ptr()), 'dc_planereg_fill')
    return h, T, score


def planereg_hypotheses(cloud_planes, support, survey_planes, triples, min_det, tol_dot, cos_tol, tol_d, h_begin=0, h_end=None):
    """(h, T, score) of planereg_fill after planereg_count and the exclusive scan of its counts; ONE host read, of the total, which
    sizes the results."""
    args = (cloud_planes, support, survey_planes, triples, min_det, tol_dot, cos_tol, tol_d)
    counts = planereg_count(*args, h_begin=h_begin, h_end=h_end)
    ends = torch.cumsum(counts, dim=0, dtype=torch.int64)
    n_valid = int(ends[-1]) if ends.shape[0] else 0
    return planereg_fill(*args, (ends - counts).contiguous(), n_valid, h_begin=h_begin, h_end=h_end)


def planereg_select(score, T, centre, n_candidates, dedupe_rot, dedupe_trans):
    """rows i64 device [n_candidates] into the valid list (ascending h), -1 where none remained: the greedy suppression of DESIGN "Plane
    registration".  Every round keeps the best remaining hypothesis by (score descending, row ascending) and drops every remaining one
    whose rotation lies within ``dedupe_rot`` of it (the angle of csrc/dc_align_math.h's rotation_angle_between) AND whose image of
    ``centre`` f64 device [3] lies within ``dedupe_trans`` of its image.  score i64 [V], T f64 [V,4,4].  Elementwise torch operations
    and device-side reductions only: nothing is read back."""
    need(score, (None,), dtype=torch.int64, name='score')
    dev = score.device
    v = score.shape[0]
    need(T, (v, 4, 4), dtype=torch.float64, name='T', device=dev)
    need(centre, (3,), dtype=torch.float64, name='centre', device=dev)
    m = int(n_candidates)
    if v == 0 or m == 0:
        return torch.full((m,), -1, dtype=torch.int64, device=dev)
    R = T[:, :3, :3].contiguous()
    img = R @ centre + T[:, :3, 3]
    pos = torch.arange(v, dtype=torch.int64, device=dev)
    alive = torch.ones((v,), dtype=torch.bool, device=dev)
    none = torch.full((), -1, dtype=torch.int64, device=dev)
    last = torch.full((), v, dtype=torch.int64, device=dev)
    rows = []
    for c in range(m):
        masked = torch.where(alive, score, none)
        smax = masked.max()
        best = torch.where(masked == smax, pos, last).amin().reshape(1)         # the first of the largest score
        rows.append(torch.where(alive.any(), best, none))
        # the kept row by index_select: indexing with a device scalar (R[best]) would read it back, a host sync per round
        D = R @ R.index_select(0, best)[0].t()
        ax = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], dim=1)
        ang = torch.atan2(torch.linalg.norm(ax, dim=1), 0.5 * (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - 1.0))
        dist = torch.linalg.norm(img - img.index_select(0, best), dim=1)
        alive = alive & ~((ang <= float(dedupe_rot)) & (dist <= float(dedupe_trans))) & (pos != best)
    return torch.cat(rows)


def icp_blocks(m):
    """Blocks (rows of partials) of icp_accumulate for m reading points (dc_icp_blocks)."""
    return int(lib().dc_icp_blocks(int(m)))


@on_device
def icp_init(prior, state, status):
    """state f64 [DC_ICP_STATE_COUNT] / status i32 [4] of a registration that starts from prior f64 device [4,4] (dc_icp_init)."""
    need(prior, (4, 4), dtype=torch.float64, name='prior')
    need(state, (nv.DC_ICP_STATE_COUNT,), dtype=torch.float64, name='state', device=prior.device)
    need(status, (4,), dtype=torch.int32, name='status', device=prior.device)
    check(lib().dc_icp_init(ptr(prior), ptr(state), ptr(status), stream_ptr()), 'dc_icp_init')


def _icp_accumulate_args(reading, per_point, map_points, map_normals, idx, dist, threshold, state, status, partials, width, kept,
                         ct_state=None):
    """The checks icp_accumulate and icp_ct_accumulate share (``per_point``: (name, tensor, trailing shape) of the caller's own
    per-point inputs; ``width`` of a row of partials) -> (M, k, blocks)."""
    dev = reading.device
    need(reading, (None, 3), dtype=torch.float64, name='reading')
    m = reading.shape[0]
    for name, t, tail in per_point:
        need(t, (m,) + tail, dtype=torch.float64, name=name, device=dev)
    need(map_points, (None, 3), dtype=torch.float64, name='map_points', device=dev)
    need(map_normals, tuple(map_points.shape), dtype=torch.float64, name='map_normals', device=dev)
    need(idx, (m, None), dtype=torch.int32, name='idx', device=dev)
    k = idx.shape[1]
    need(dist, (m, k), dtype=torch.float64, name='dist', device=dev)
    need(threshold, (1,), dtype=torch.float64, name='threshold', device=dev)
    _icp_state_args(state, status, dev, ct_state)
    nb = icp_blocks(m)
    need(partials, (nb, width), dtype=torch.float64, name='partials', device=dev)
    if kept is not None:
        need(kept, (m, k), dtype=torch.uint8, name='kept', device=dev)
    return m, k, nb


def _icp_state_args(state, status, dev, ct_state=None):
    """The state / status (and twist state) checks of the ICP calls."""
    need(state, (nv.DC_ICP_STATE_COUNT,), dtype=torch.float64, name='state', device=dev)
    if ct_state is not None:
        need(ct_state, (nv.DC_ICP_CT_STATE_COUNT,), dtype=torch.float64, name='ct_state', device=dev)
    need(status, (4,), dtype=torch.int32, name='status', device=dev)


@on_device
def icp_accumulate(reading, normals, map_points, map_normals, idx, dist, threshold, cos_min, state, status, partials, kept=None):
    """Filtered point-to-plane pairs of one ICP iteration -> block partials f64 [icp_blocks(M), DC_ICP_PARTIALS] (dc_icp_accumulate);
    ``kept`` (uint8 [M,k], optional) receives the kept flags."""
    m, k, nb = _icp_accumulate_args(reading, [('normals', normals, (3,))], map_points, map_normals, idx, dist, threshold, state, status,
                                    partials, nv.DC_ICP_PARTIALS, kept)
    check(lib().dc_icp_accumulate(ptr(reading), ptr(normals), m, ptr(map_points), ptr(map_normals), ptr(idx), ptr(dist), k, ptr(threshold),
                                  float(cos_min), ptr(state), ptr(status), ptr(partials), nb, ptr(kept), stream_ptr()), 'dc_icp_accumulate')


@on_device
def icp_finish(partials, m, state, status, min_rot, min_trans, smooth, max_iters, max_rot, max_trans, min_pairs=6):
    """Solve, update and check one ICP iteration in one block (dc_icp_finish)."""
    need(partials, (None, nv.DC_ICP_PARTIALS), dtype=torch.float64, name='partials')
    _icp_state_args(state, status, partials.device)
    check(lib().dc_icp_finish(ptr(partials), partials.shape[0], int(m), float(min_rot), float(min_trans), int(smooth), int(max_iters),
                              float(max_rot), float(max_trans), int(min_pairs), ptr(state), ptr(status), stream_ptr()), 'dc_icp_finish')


@on_device
def deskew_device_twist(points, normals, tau, twist, scan_offset, points_out, normals_out):
    """dc_deskew of one scan under a twist that lives on the device (f64 [6], the estimate of a sweep-aware registration), into
    ``points_out`` / ``normals_out`` f64 [M,3]; ``scan_offset`` the device int64 [0, M].  Nothing is read back: the host-side check of
    deskew (finite, |w| <= pi) is left out, dc_icp_ct_finish keeps the twist inside that bound."""
    dev = points.device
    need(points, (None, 3), dtype=torch.float64, name='points')
    m = points.shape[0]
    need(normals, (m, 3), dtype=torch.float64, name='normals', device=dev)
    need(tau, (m,), dtype=torch.float64, name='tau', device=dev)
    need(twist, (6,), dtype=torch.float64, name='twist', device=dev)
    need(scan_offset, (2,), dtype=torch.int64, name='scan_offset', device=dev)
    need(points_out, (m, 3), dtype=torch.float64, name='points_out', device=dev)
    need(normals_out, (m, 3), dtype=torch.float64, name='normals_out', device=dev)
    if m:
        check(lib().dc_deskew(ptr(points), None, ptr(normals), dtype_code(points), ptr(tau), m, ptr(scan_offset), ptr(twist), 1,
                              ptr(points_out), None, ptr(normals_out), stream_ptr()), 'dc_deskew')


@on_device
def icp_ct_init(twist, ct_state):
    """ct_state f64 [DC_ICP_CT_STATE_COUNT] of a sweep-aware registration whose twist starts from, and is held to, twist f64 device [6]
    (dc_icp_ct_init; icp_init sets the pose state and the status word)."""
    need(twist, (6,), dtype=torch.float64, name='twist')
    need(ct_state, (nv.DC_ICP_CT_STATE_COUNT,), dtype=torch.float64, name='ct_state', device=twist.device)
    check(lib().dc_icp_ct_init(ptr(twist), ptr(ct_state), stream_ptr()), 'dc_icp_ct_init')


@on_device
def icp_ct_accumulate(reading, q, nq, tau, map_points, map_normals, idx, dist, threshold, cos_min, state, ct_state, status, partials,
                      kept=None):
    """icp_accumulate for the sweep-aware iteration: the pairs of the de-skewed points ``q`` / normals ``nq`` (deskew_device_twist of
    ``reading`` at ``tau``) -> block partials f64 [icp_blocks(M), DC_ICP_CT_PARTIALS] (dc_icp_ct_accumulate)."""
    m, k, nb = _icp_accumulate_args(reading, [('q', q, (3,)), ('nq', nq, (3,)), ('tau', tau, ())], map_points, map_normals, idx, dist,
                                    threshold, state, status, partials, nv.DC_ICP_CT_PARTIALS, kept, ct_state)
    check(lib().dc_icp_ct_accumulate(ptr(reading), ptr(q), ptr(nq), ptr(tau), m, ptr(map_points), ptr(map_normals), ptr(idx), ptr(dist), k,
                                     ptr(threshold), float(cos_min), ptr(state), ptr(ct_state), ptr(status), ptr(partials), nb, ptr(kept),
                                     stream_ptr()), 'dc_icp_ct_accumulate')


@on_device
def icp_ct_finish(partials, m, state, ct_state, status, min_rot, min_trans, smooth, max_iters, max_rot, max_trans, beta_v, beta_w,
                  max_twist_trans, max_twist_rot, min_pairs=6):
    """Solve the 12 x 12 system with the twist prior, update pose and twist and check, in one block (dc_icp_ct_finish)."""
    need(partials, (None, nv.DC_ICP_CT_PARTIALS), dtype=torch.float64, name='partials')
    _icp_state_args(state, status, partials.device, ct_state)
    check(lib().dc_icp_ct_finish(ptr(partials), partials.shape[0], int(m), float(min_rot), float(min_trans), int(smooth), int(max_iters),
                                 float(max_rot), float(max_trans), int(min_pairs), float(beta_v), float(beta_w), float(max_twist_trans),
                                 float(max_twist_rot), ptr(state), ptr(ct_state), ptr(status), stream_ptr()), 'dc_icp_ct_finish')


@on_device
def map_select(reading, normals, depth, pose, dist1, min_dist, max_range):
    """(mask bool [M], points f64 [M,3], normals f64 [M,3]): reading points and normals moved by pose f64 device [4,4] and the mask of
    those the map takes -- nearest map point (dist1 [M]; None = empty map) beyond min_dist, depth <= max_range (dc_map_select)."""
    dev = reading.device
    need(reading, (None, 3), dtype=torch.float64, name='reading')
    m = reading.shape[0]
    need(normals, (m, 3), dtype=torch.float64, name='normals', device=dev)
    need(depth, (m,), dtype=torch.float64, name='depth', device=dev)
    need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    if dist1 is not None:
        need(dist1, (m,), dtype=torch.float64, name='dist1', device=dev)
    mask = torch.empty((m,), dtype=torch.uint8, device=dev)
    pts = torch.empty((m, 3), dtype=torch.float64, device=dev)
    nrm = torch.empty((m, 3), dtype=torch.float64, device=dev)
    check(lib().dc_map_select(ptr(reading), ptr(normals), ptr(depth), m, ptr(pose), ptr(dist1), float(min_dist), float(max_range),
                              ptr(mask), ptr(pts), ptr(nrm), stream_ptr()), 'dc_map_select')
    return mask.view(torch.bool), pts, nrm


# ------------------------------------------------------------------------------------------------
# Dynamic points in the map (csrc/dc_dynamic.hip, slam.IcpMapper.update_dynamic; DESIGN "Dynamic points in the map")
# ------------------------------------------------------------------------------------------------
@on_device
def dyn_directions(points, pose=None, max_range=0.0):
    """(dirs f64 [N,3], depth f64 [N], valid bool [N]) of points f64 [N,3] as the sensor at pose f64 device [4,4] sees them; pose None:
    the points are in the sensor frame.  valid = depth finite, > 0 and <= max_range (<= 0 or inf: no bound); invalid rows have a zero
    direction (dc_dyn_directions)."""
    need(points, (None, 3), dtype=torch.float64, name='points')
    dev = points.device
    if pose is not None:
        need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    max_range = float(max_range)
    if max_range != max_range:
        raise ValueError('max_range must not be NaN')
    n = points.shape[0]
    dirs = torch.empty((n, 3), dtype=torch.float64, device=dev)
    depth = torch.empty((n,), dtype=torch.float64, device=dev)
    valid = torch.empty((n,), dtype=torch.uint8, device=dev)
    check(lib().dc_dyn_directions(ptr(points), n, ptr(pose), max_range, ptr(dirs), ptr(depth), ptr(valid), stream_ptr()), 'dc_dyn_directions')
    return dirs, depth, valid.view(torch.bool)


@on_device
def dyn_update(map_points, map_normals, pose, reading, rows, match_idx, match_chord, chord_max, epsilon_a, epsilon_d, alpha, beta, threshold,
               max_range, prob, seen=None):
    """Visibility test and Bayesian update of prob f64 [N] (in place) for the map rows ``rows`` (int32 [R], strictly ascending --
    the caller's contract: a thread owns its row) matched to the reading rows ``match_idx`` (int32 [R], rows of reading f64 [M,3]) at
    the chords ``match_chord`` (f64 [R]); ``seen`` (uint8 [N], zeroed by the caller, optional) gets 1 occluded / 2 updated
    (dc_dyn_update)."""
    need(map_points, (None, 3), dtype=torch.float64, name='map_points')
    dev = map_points.device
    n = map_points.shape[0]
    need(map_normals, (n, 3), dtype=torch.float64, name='map_normals', device=dev)
    need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    need(reading, (None, 3), dtype=torch.float64, name='reading', device=dev)
    need(rows, (None,), dtype=torch.int32, name='rows', device=dev)
    r = rows.shape[0]
    need(match_idx, (r,), dtype=torch.int32, name='match_idx', device=dev)
    need(match_chord, (r,), dtype=torch.float64, name='match_chord', device=dev)
    need(prob, (n,), dtype=torch.float64, name='prob', device=dev)
    if seen is not None:
        need(seen, (n,), dtype=torch.uint8, name='seen', device=dev)
    check(lib().dc_dyn_update(ptr(map_points), ptr(map_normals), n, ptr(pose), ptr(reading), reading.shape[0], ptr(rows), ptr(match_idx),
                              ptr(match_chord), r, float(chord_max), float(epsilon_a), float(epsilon_d), float(alpha), float(beta),
                              float(threshold), float(max_range), ptr(prob), ptr(seen), stream_ptr()), 'dc_dyn_update')
    return prob


# ------------------------------------------------------------------------------------------------
# range-image neighbourhoods (csrc/dc_rangeimage.hip; range_image.py holds the grid and the cloud-level functions)
# ------------------------------------------------------------------------------------------------
def _grid_args(grid):
    return int(grid.rows), int(grid.cols), float(grid.fov_up), float(grid.fov_down), int(bool(grid.wrap))


def _range_vps(vps, points, n):
    if vps is None:
        return None, 0
    vps = vps.reshape(-1, 3)
    need(vps, (None, 3), dtype=points.dtype, name='vps', device=points.device)
    if vps.shape[0] not in (1, n):
        raise ValueError('vps must have 1 or %d rows' % n)
    return vps, vps.shape[0]


@on_device
def range_project(points, grid, vps=None, clamp=True, min_depth=0.0):
    """(pixel int32 [N], index_image int32 [H,W], range_image [H,W]) of sensor-frame points [N, >=3] on a spherical grid
    (dc_range_project): the reference's range_projection (scripts/depth_denoising:44-91) with the winner of every pixel -- the
    nearest point, ties to the lower index -- kept as an index."""
    need(points, (None, None), name='points')
    n, stride = points.shape
    if stride < 3:
        raise ValueError('points need at least 3 columns')
    dev = points.device
    rows, cols, up, down, wrap = _grid_args(grid)
    vps, vps_rows = _range_vps(vps, points, n)
    pixel = torch.empty((n,), dtype=torch.int32, device=dev)
    index_image = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    range_image = torch.empty((rows, cols), dtype=points.dtype, device=dev)
    nbytes = lib().dc_range_project_workspace_bytes(n, rows, cols)
    ws = _ws(nbytes, dev)
    check(lib().dc_range_project(ptr(points), stride, dtype_code(points), ptr(vps), vps_rows, n, rows, cols, up, down, wrap, int(bool(clamp)),
                                 float(min_depth), ptr(pixel), ptr(index_image), ptr(range_image), ptr(ws), nbytes, stream_ptr()),
          'dc_range_project')
    return pixel, index_image, range_image


def _organized_outputs(rows_max, hw_shape, dtype, dev, want_index, want_range):
    out = dict(vps=torch.empty((rows_max, 3), dtype=dtype, device=dev), dirs=torch.empty((rows_max, 3), dtype=dtype, device=dev),
               depth=torch.empty((rows_max, 1), dtype=dtype, device=dev), points=torch.empty((rows_max, 3), dtype=dtype, device=dev),
               pixel=torch.empty((rows_max,), dtype=torch.int32, device=dev),
               index=torch.empty((rows_max,), dtype=torch.int32, device=dev) if want_index else None,
               index_image=torch.empty(hw_shape, dtype=torch.int32, device=dev),
               range_image=torch.empty(hw_shape, dtype=dtype, device=dev) if want_range else None,
               count=torch.empty((1,), dtype=torch.int64, device=dev))
    return out


@on_device
def range_organize(points, grid, vps=None, clamp=True, min_depth=0.0, dtype=None, want_index=False, want_range=False):
    """Projection + the winners compacted in ascending pixel order (dc_range_organize).  Returns a dict of FULL-SIZE buffers
    (min(N, H W) rows: vps, dirs, depth [.,1], points, pixel, index | None), index_image [H,W] pointing at the compact rows,
    range_image | None and ``count`` (device int64 [1]): nothing is read back here -- the caller slices once it knows the count."""
    need(points, (None, None), name='points')
    n, stride = points.shape
    if stride < 3:
        raise ValueError('points need at least 3 columns')
    dev = points.device
    dtype = points.dtype if dtype is None else dtype
    rows, cols, up, down, wrap = _grid_args(grid)
    vps, vps_rows = _range_vps(vps, points, n)
    out = _organized_outputs(min(n, rows * cols), (rows, cols), dtype, dev, want_index, want_range)
    nbytes = lib().dc_range_organize_workspace_bytes(n, rows, cols)
    ws = _ws(nbytes, dev)
    check(lib().dc_range_organize(ptr(points), stride, dtype_code(points), ptr(vps), vps_rows, n, rows, cols, up, down, wrap, int(bool(clamp)),
                                  float(min_depth), nv.DC_F32 if dtype == torch.float32 else nv.DC_F64, ptr(out['vps']), ptr(out['dirs']),
                                  ptr(out['depth']), ptr(out['points']), ptr(out['pixel']), ptr(out['index']), ptr(out['index_image']),
                                  ptr(out['range_image']), ptr(out['count']), ptr(ws), nbytes, stream_ptr()), 'dc_range_organize')
    return out


@on_device
def range_from_grid(points, rows, cols, vps=None, min_depth=0.0, dtype=None, want_index=False, want_range=False):
    """The same outputs for an H x W array of points [H W, >=3] in row-major order (dc_range_from_grid): no projection, a pixel is
    occupied when its ray is finite and deeper than ``min_depth``."""
    need(points, (rows * cols, None), name='points')
    stride = points.shape[1]
    if stride < 3:
        raise ValueError('points need at least 3 columns')
    dev = points.device
    dtype = points.dtype if dtype is None else dtype
    vps, vps_rows = _range_vps(vps, points, rows * cols)
    out = _organized_outputs(rows * cols, (rows, cols), dtype, dev, want_index, want_range)
    nbytes = lib().dc_range_organize_workspace_bytes(0, rows, cols)
    ws = _ws(nbytes, dev)
    check(lib().dc_range_from_grid(ptr(points), stride, dtype_code(points), ptr(vps), vps_rows, int(rows), int(cols), float(min_depth),
                                   nv.DC_F32 if dtype == torch.float32 else nv.DC_F64, ptr(out['vps']), ptr(out['dirs']), ptr(out['depth']),
                                   ptr(out['points']), ptr(out['pixel']), ptr(out['index']), ptr(out['index_image']), ptr(out['range_image']),
                                   ptr(out['count']), ptr(ws), nbytes, stream_ptr()), 'dc_range_from_grid')
    return out


@on_device
def range_index_image(pixel, rows, cols, count=None):
    """int32 [H,W]: index_image[pixel[i]] = i, -1 elsewhere (dc_range_index_image); ``count`` (device int64 [1]) bounds the rows."""
    need(pixel, (None,), dtype=torch.int32, name='pixel')
    index_image = torch.empty((int(rows), int(cols)), dtype=torch.int32, device=pixel.device)
    check(lib().dc_range_index_image(ptr(pixel), pixel.shape[0], ptr(count), int(rows), int(cols), ptr(index_image), stream_ptr()),
          'dc_range_index_image')
    return index_image


@on_device
def image_features_fwd(points, dirs, pixel, index_image, grid, window, r=None, want=('mean', 'cov', 'eigvals', 'eigvecs', 'normals',
                                                                                     'inc_angles'),
                       want_nvalid=True, want_neighbors=True, count=None):
    """dc_features_fwd's outputs on the window neighbourhoods of an organised cloud, one launch (dc_image_features_fwd).  ``window`` =
    (ah, aw) half extents, ``r`` the 3-D radius gate (None / <= 0 / inf: none).  Returns a dict with the wanted fields, ``nvalid``
    int32 [M] and ``neighbors`` int32 [M, (2 ah + 1)(2 aw + 1)] (-1 padded in place)."""
    need(points, (None, 3), name='points')
    m = points.shape[0]
    dev, dt = points.device, points.dtype
    need(dirs, (m, 3), dtype=dt, name='dirs', device=dev)
    need(pixel, (None,), dtype=torch.int32, name='pixel', device=dev)
    if pixel.shape[0] < m:
        raise ValueError('pixel has %d rows, the cloud %d' % (pixel.shape[0], m))
    rows, cols, _, _, wrap = _grid_args(grid)
    need(index_image, (rows, cols), dtype=torch.int32, name='index_image', device=dev)
    ah, aw = int(window[0]), int(window[1])
    k = (2 * ah + 1) * (2 * aw + 1)
    shapes = dict(mean=(m, 3), cov=(m, 3, 3), eigvals=(m, 3), eigvecs=(m, 3, 3), normals=(m, 3), inc_angles=(m, 1))
    out = {f: (torch.empty(shapes[f], dtype=dt, device=dev) if f in want else None) for f in shapes}
    nvalid = torch.empty((m,), dtype=torch.int32, device=dev) if want_nvalid else None
    nbr = torch.empty((m, max(k, 1)), dtype=torch.int32, device=dev) if want_neighbors else None
    check(lib().dc_image_features_fwd(ptr(points), ptr(dirs), dtype_code(points), ptr(pixel), ptr(index_image), m, ptr(count), rows, cols, wrap,
                                      ah, aw, float(r) if r else 0.0, ptr(out['mean']), ptr(out['cov']), ptr(out['eigvals']),
                                      ptr(out['eigvecs']), ptr(out['normals']), ptr(out['inc_angles']), ptr(nvalid), ptr(nbr), stream_ptr()),
          'dc_image_features_fwd')
    out.update(nvalid=nvalid, neighbors=nbr)
    return out


@on_device
def image_shadow_mask(points, vps, dirs, pixel, index_image, grid, window, r, lo, hi, count=None):
    """bool [M]: dc_shadow_filter's mask with the candidates taken from the image window (dc_image_shadow_mask); rows at and beyond
    ``count`` (device int64 [1]) are False."""
    need(points, (None, 3), name='points')
    m = points.shape[0]
    dev, dt = points.device, points.dtype
    vps = vps.reshape(-1, 3)
    need(vps, (None, 3), dtype=dt, name='vps', device=dev)
    need(dirs, (m, 3), dtype=dt, name='dirs', device=dev)
    if vps.shape[0] not in (1, m):
        raise ValueError('vps must have 1 or %d rows' % m)
    need(pixel, (None,), dtype=torch.int32, name='pixel', device=dev)
    if pixel.shape[0] < m:
        raise ValueError('pixel has %d rows, the cloud %d' % (pixel.shape[0], m))
    rows, cols, _, _, wrap = _grid_args(grid)
    need(index_image, (rows, cols), dtype=torch.int32, name='index_image', device=dev)
    mask = torch.empty((m,), dtype=torch.bool, device=dev)
    check(lib().dc_image_shadow_mask(ptr(points), ptr(vps), vps.shape[0], ptr(dirs), dtype_code(points), ptr(pixel), ptr(index_image), m,
                                     ptr(count), rows, cols, wrap, int(window[0]), int(window[1]), float(r), float(lo), float(hi), ptr(mask),
                                     stream_ptr()), 'dc_image_shadow_mask')
    return mask


# ------------------------------------------------------------------------------------------------
# surface reconstruction: TSDF fusion and surface-nets extraction (csrc/dc_tsdf.hip, reconstruction.TsdfVolume)
# ------------------------------------------------------------------------------------------------
def tsdf_k_steps(trunc, voxel):
    """K = ceil(trunc / h) with h = voxel / 2: the samples a ray takes on either side of its end point."""
    return int(math.ceil(float(trunc) / (float(voxel) / 2.0)))


def _tsdf_volume_args(sum_, count, origin, voxel, who):
    need(sum_, (None, None, None), dtype=torch.int64, name='sum')
    dev, dims = sum_.device, tuple(sum_.shape)
    need(count, dims, dtype=torch.int32, name='count', device=dev)
    origin = tuple(float(v) for v in origin)
    voxel = float(voxel)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError('%s needs a finite origin of 3 values, got %r' % (who, origin))
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError('%s needs a voxel size > 0, got %r' % (who, voxel))
    if min(dims) < 2 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('%s needs dims >= 2 with fewer than 2^31 voxels, got %r' % (who, dims))
    return dev, dims, origin, voxel


@on_device
def tsdf_integrate(sum_, count, stats, origin, voxel, trunc, vps, dirs, depth, pose=None, mask=None, min_depth=0., max_range=None,
                   carve_from=None):
    """Adds the rays (vps [n,3] or [1,3], dirs [n,3], depth [n] or [n,1]; f32 or f64, sensor frame) of one scan to the volume sum i64 /
    count i32 [nx,ny,nz] with the minimum corner ``origin`` and the voxel size ``voxel``, truncated at ``trunc`` (dc_tsdf_integrate; the
    rule: csrc/dc_tsdf_math.h).  pose f64 device [4,4] (world from sensor) or None; mask bool / uint8 [n] or None; rays at or below
    ``min_depth`` or beyond ``max_range`` are skipped; ``carve_from`` >= 0 also samples the free space from that range on.  stats i64
    device [4] += {rays used, rays skipped, samples outside the grid, visits}.  In place; nothing is read back."""
    dev, dims, origin, voxel = _tsdf_volume_args(sum_, count, origin, voxel, 'tsdf_integrate')
    need(stats, (4,), dtype=torch.int64, name='stats', device=dev)
    trunc = float(trunc)
    if not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('tsdf_integrate needs a truncation > 0, got %r' % trunc)
    need(dirs, (None, 3), name='dirs', device=dev)
    n, dt = dirs.shape[0], dirs.dtype
    code = dtype_code(dirs)
    vps = vps.reshape(-1, 3)
    if vps.shape[0] == 1 and n != 1:
        vps = vps.expand(n, 3).contiguous()
    need(vps, (n, 3), dtype=dt, name='vps', device=dev)
    depth = depth.reshape(-1)
    need(depth, (n,), dtype=dt, name='depth', device=dev)
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError('mask must be bool or uint8, got %s' % mask.dtype)
        need(mask, (n,), name='mask', device=dev)
    if pose is not None:
        need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    min_depth = float(min_depth)
    max_range = math.inf if max_range is None else float(max_range)
    carve_from = -1.0 if carve_from is None else float(carve_from)
    if math.isnan(min_depth) or math.isnan(max_range) or math.isnan(carve_from) or (carve_from < 0.0 and carve_from != -1.0):
        raise ValueError('tsdf_integrate needs min_depth and max_range that are numbers and carve_from >= 0 or None')
    check(lib().dc_tsdf_integrate(ptr(vps), ptr(dirs), ptr(depth), code, n, ptr(mask), ptr(pose), *origin, voxel, *dims, trunc,
                                  tsdf_k_steps(trunc, voxel), min_depth, max_range, carve_from, ptr(sum_), ptr(count), ptr(stats), stream_ptr()),
          'dc_tsdf_integrate')


@on_device
def tsdf_extract(sum_, count, origin, voxel, min_count=1, ws=None):
    """(vertices f64 [Nv,3], faces i32 [Nf,3]): the surface nets of the volume sum i64 / count i32 [nx,ny,nz] on the lattice of voxel
    centres, vertices in ascending cell index and faces in ascending (lattice point, axis), normals to the free side
    (dc_tsdf_extract_count, the library's scans, dc_tsdf_extract_fill).  ONE host read: the two totals, which size the outputs."""
    dev, dims, origin, voxel = _tsdf_volume_args(sum_, count, origin, voxel, 'tsdf_extract')
    min_count = int(min_count)
    if min_count < 1:
        raise ValueError('tsdf_extract needs min_count >= 1, got %d' % min_count)
    nbytes = int(lib().dc_tsdf_extract_workspace_bytes(*dims))
    if nbytes == 0:
        raise ValueError('tsdf_extract takes volumes of fewer than 2^31 / 3 voxels, got %r' % (dims,))
    ws = _ws_arg(ws, nbytes, dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    check(lib().dc_tsdf_extract_count(ptr(sum_), ptr(count), *dims, min_count, ptr(totals), ptr(ws), ws.shape[0], stream_ptr()),
          'dc_tsdf_extract_count')
    n_vertices, n_faces = totals.tolist()
    vertices = torch.empty((n_vertices, 3), dtype=torch.float64, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    check(lib().dc_tsdf_extract_fill(ptr(sum_), ptr(count), *origin, voxel, *dims, min_count, ptr(ws), ws.shape[0], n_vertices, n_faces,
                                     ptr(vertices), ptr(faces), stream_ptr()), 'dc_tsdf_extract_fill')
    return vertices, faces


# ------------------------------------------------------------------------------------------------
# sparse TSDF volumes: block-allocated fusion and extraction (csrc/dc_tsdf_sparse.hip, reconstruction.SparseTsdfVolume)
# ------------------------------------------------------------------------------------------------
TSDF_BLOCK_VOXELS = 512
TSDF_MAX_BLOCKS = 2 ** 22 - 1


def _tsdf_sparse_table(keys, slots, n_blocks, who):
    """The device and capacity of the table keys i64 [capacity] (the 63-bit keys, never negative), slots i32 [capacity], n_blocks i64 [1]."""
    need(keys, (None,), dtype=torch.int64, name='keys')
    dev, capacity = keys.device, keys.shape[0]
    if not 1 <= capacity <= TSDF_MAX_BLOCKS:
        raise ValueError('%s needs a table of 1 .. 2^22 - 1 blocks, got %d' % (who, capacity))
    need(slots, (capacity,), dtype=torch.int32, name='slots', device=dev)
    if n_blocks is not None:
        need(n_blocks, (1,), dtype=torch.int64, name='n_blocks', device=dev)
    return dev, capacity


def _tsdf_sparse_rays(who, dev, origin, voxel, trunc, vps, dirs, depth, pose, mask, min_depth, max_range):
    """The checked ray and rule arguments of dc_tsdf_sparse_allocate / _integrate, in the order of the C calls up to max_range."""
    origin = tuple(float(v) for v in origin)
    voxel, trunc = float(voxel), float(trunc)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError('%s needs a finite origin of 3 values, got %r' % (who, origin))
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError('%s needs a voxel size > 0, got %r' % (who, voxel))
    if not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('%s needs a truncation > 0, got %r' % (who, trunc))
    need(dirs, (None, 3), name='dirs', device=dev)
    n, dt = dirs.shape[0], dirs.dtype
    code = dtype_code(dirs)
    vps = vps.reshape(-1, 3)
    if vps.shape[0] == 1 and n != 1:
        vps = vps.expand(n, 3).contiguous()
    need(vps, (n, 3), dtype=dt, name='vps', device=dev)
    depth = depth.reshape(-1)
    need(depth, (n,), dtype=dt, name='depth', device=dev)
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError('mask must be bool or uint8, got %s' % mask.dtype)
        need(mask, (n,), name='mask', device=dev)
    if pose is not None:
        need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    min_depth = float(min_depth)
    max_range = math.inf if max_range is None else float(max_range)
    if math.isnan(min_depth) or math.isnan(max_range):
        raise ValueError('%s needs min_depth and max_range that are numbers' % who)
    k = tsdf_k_steps(trunc, voxel)
    if not 1 <= k <= 2 ** 20:
        raise ValueError('%s: a truncation of %g at a voxel size of %g takes %d steps, 1 .. 2^20 are supported' % (who, trunc, voxel, k))
    keep = (vps, dirs, depth, mask, pose)
    return n, k, keep, (ptr(vps), ptr(dirs), ptr(depth), code, n, ptr(mask), ptr(pose)) + origin + (voxel, trunc, k, min_depth, max_range)


@on_device
def tsdf_sparse_allocate(keys, slots, n_blocks, info, origin, voxel, trunc, vps, dirs, depth, pose=None, mask=None, min_depth=0., max_range=None,
                         ws=None):
    """Admits the blocks the rays will add to into the table keys i64 [capacity] / slots i32 [capacity] / n_blocks i64 [1]
    (dc_tsdf_sparse_allocate; the rule: csrc/dc_tsdf_sparse_math.h): the wanted keys the table lacks, ascending, get the next slots until
    the capacity; info i64 device [2] <- {n_blocks after the call, blocks wanted but not admitted}.  In place; nothing is read back."""
    dev, capacity = _tsdf_sparse_table(keys, slots, n_blocks, 'tsdf_sparse_allocate')
    need(info, (2,), dtype=torch.int64, name='info', device=dev)
    n, k, keep, args = _tsdf_sparse_rays('tsdf_sparse_allocate', dev, origin, voxel, trunc, vps, dirs, depth, pose, mask, min_depth, max_range)
    nbytes = int(lib().dc_tsdf_sparse_workspace_bytes(n, k, capacity))
    if nbytes == 0:
        raise ValueError('tsdf_sparse_allocate takes fewer than 2^31 / (2 K + 1) rays a call, got %d rays at K = %d' % (n, k))
    ws = _ws_arg(ws, nbytes, dev)
    check(lib().dc_tsdf_sparse_allocate(*args, capacity, ptr(keys), ptr(slots), ptr(n_blocks), ptr(info), ptr(ws), ws.shape[0], stream_ptr()),
          'dc_tsdf_sparse_allocate')


@on_device
def tsdf_sparse_integrate(keys, slots, n_blocks, sum_, count, stats, origin, voxel, trunc, vps, dirs, depth, pose=None, mask=None, min_depth=0.,
                          max_range=None):
    """Adds the rays to the pool sum i64 / count i32 [capacity, 512] at the slots of the table (dc_tsdf_sparse_integrate); a visit whose
    block the table lacks is dropped.  stats i64 device [5] += {rays used, rays skipped, samples outside, visits, visits dropped}.  In
    place; nothing is read back."""
    dev, capacity = _tsdf_sparse_table(keys, slots, n_blocks, 'tsdf_sparse_integrate')
    need(sum_, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='sum', device=dev)
    need(count, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='count', device=dev)
    need(stats, (5,), dtype=torch.int64, name='stats', device=dev)
    _, _, keep, args = _tsdf_sparse_rays('tsdf_sparse_integrate', dev, origin, voxel, trunc, vps, dirs, depth, pose, mask, min_depth, max_range)
    check(lib().dc_tsdf_sparse_integrate(*args, capacity, ptr(keys), ptr(slots), ptr(n_blocks), ptr(sum_), ptr(count), ptr(stats), stream_ptr()),
          'dc_tsdf_sparse_integrate')


@on_device
def tsdf_sparse_extract(keys, slots, n_blocks, sum_, count, origin, voxel, min_count=1, ws=None):
    """(vertices f64 [Nv,3], faces i32 [Nf,3]): the surface nets of the sparse volume, vertices in ascending (block key, local cell) and
    faces in ascending (block key, local point, axis), normals to the free side (dc_tsdf_sparse_extract_count, the library's scans,
    dc_tsdf_sparse_extract_fill).  ``n_blocks`` is the host's int.  ONE host read: the two totals, which size the outputs."""
    dev, capacity = _tsdf_sparse_table(keys, slots, None, 'tsdf_sparse_extract')
    need(sum_, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='sum', device=dev)
    need(count, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='count', device=dev)
    n_blocks, min_count = int(n_blocks), int(min_count)
    origin = tuple(float(v) for v in origin)
    voxel = float(voxel)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin) or not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError('tsdf_sparse_extract needs a finite origin of 3 values and a voxel size > 0, got %r and %r' % (origin, voxel))
    if not 0 <= n_blocks <= capacity:
        raise ValueError('tsdf_sparse_extract needs 0 <= n_blocks <= the capacity %d, got %d' % (capacity, n_blocks))
    if min_count < 1:
        raise ValueError('tsdf_sparse_extract needs min_count >= 1, got %d' % min_count)
    nbytes = int(lib().dc_tsdf_sparse_extract_workspace_bytes(n_blocks))
    if nbytes == 0:
        raise ValueError('tsdf_sparse_extract takes fewer than 2^31 / 1536 blocks, got %d' % n_blocks)
    ws = _ws_arg(ws, nbytes, dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)
    check(lib().dc_tsdf_sparse_extract_count(ptr(keys), ptr(slots), n_blocks, ptr(sum_), ptr(count), min_count, ptr(totals), ptr(ws), ws.shape[0],
                                             stream_ptr()), 'dc_tsdf_sparse_extract_count')
    n_vertices, n_faces = totals.tolist()
    vertices = torch.empty((n_vertices, 3), dtype=torch.float64, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    check(lib().dc_tsdf_sparse_extract_fill(ptr(keys), ptr(slots), n_blocks, ptr(sum_), ptr(count), *origin, voxel, min_count, ptr(ws),
                                            ws.shape[0], n_vertices, n_faces, ptr(vertices), ptr(faces), stream_ptr()),
          'dc_tsdf_sparse_extract_fill')
    return vertices, faces


# ------------------------------------------------------------------------------------------------
# scan-to-TSDF registration: sampling the sparse volume and the point-to-surface row (csrc/dc_tsdf_track.hip, slam.TsdfMapper)
# ------------------------------------------------------------------------------------------------
TSDF_SAMPLE_RANGE, TSDF_SAMPLE_UNOBSERVED = 1, 2


@on_device
def tsdf_sparse_sample(keys, slots, n_blocks, sum_, count, origin, voxel, trunc, points, pose=None, min_count=1, stop=None, out=None):
    """Samples the sparse volume at ``points`` f64 [M,3] moved by ``pose`` (device f64 [4,4], None: as they are) -> dict(x [M,3] the
    moved points, value [M] the trilinear distance in metres, grad [M,3] its analytic gradient, dist [M] = |value|, flag u8 [M]: 0,
    TSDF_SAMPLE_RANGE or TSDF_SAMPLE_UNOBSERVED); an invalid point has value NaN, grad 0 and dist +inf (dc_tsdf_sparse_sample; the rule:
    csrc/dc_tsdf_track_math.h).  ``out``: such a dict to write into; ``stop`` (device i32): nonzero leaves ``out`` as it is.  Nothing is
    read back."""
    dev, capacity = _tsdf_sparse_table(keys, slots, n_blocks, 'tsdf_sparse_sample')
    need(sum_, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='sum', device=dev)
    need(count, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='count', device=dev)
    origin = tuple(float(v) for v in origin)
    voxel, trunc, min_count = float(voxel), float(trunc), int(min_count)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin) or not (voxel > 0.0 and math.isfinite(voxel)) or \
            not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('tsdf_sparse_sample needs a finite origin of 3 values, a voxel size and a truncation > 0, got %r, %r and %r'
                         % (origin, voxel, trunc))
    if min_count < 1:
        raise ValueError('tsdf_sparse_sample needs min_count >= 1, got %d' % min_count)
    need(points, (None, 3), dtype=torch.float64, name='points', device=dev)
    m = points.shape[0]
    if pose is not None:
        need(pose, (4, 4), dtype=torch.float64, name='pose', device=dev)
    if stop is not None:
        need(stop, None, dtype=torch.int32, name='stop', device=dev)
    if out is None:
        out = dict(x=torch.empty((m, 3), dtype=torch.float64, device=dev), value=torch.empty((m,), dtype=torch.float64, device=dev),
                   grad=torch.empty((m, 3), dtype=torch.float64, device=dev), dist=torch.empty((m,), dtype=torch.float64, device=dev),
                   flag=torch.empty((m,), dtype=torch.uint8, device=dev))
    else:
        for name, shape, dt in (('x', (m, 3), torch.float64), ('value', (m,), torch.float64), ('grad', (m, 3), torch.float64),
                                ('dist', (m,), torch.float64), ('flag', (m,), torch.uint8)):
            need(out[name], shape, dtype=dt, name=name, device=dev)
    check(lib().dc_tsdf_sparse_sample(ptr(keys), ptr(slots), ptr(n_blocks), capacity, ptr(sum_), ptr(count), *origin, voxel, trunc, min_count,
                                      ptr(points), m, ptr(pose), ptr(stop), ptr(out['x']), ptr(out['value']), ptr(out['grad']),
                                      ptr(out['dist']), ptr(out['flag']), stream_ptr()), 'dc_tsdf_sparse_sample')
    return out


@on_device
def tsdf_icp_accumulate(sample, threshold, max_residual, state, status, partials, kept=None):
    """The pairs of one scan-to-TSDF iteration from ``sample`` (tsdf_sparse_sample's dict) -> block partials f64 [icp_blocks(M),
    DC_ICP_PARTIALS] for icp_finish (dc_tsdf_icp_accumulate): point i is a pair iff flag == 0, dist <= threshold (device f64 [1]) and
    dist < max_residual; ``kept`` (uint8 [M], optional) receives the flags."""
    x = sample['x']
    dev = x.device
    need(x, (None, 3), dtype=torch.float64, name='x')
    m = x.shape[0]
    need(sample['value'], (m,), dtype=torch.float64, name='value', device=dev)
    need(sample['grad'], (m, 3), dtype=torch.float64, name='grad', device=dev)
    need(sample['dist'], (m,), dtype=torch.float64, name='dist', device=dev)
    need(sample['flag'], (m,), dtype=torch.uint8, name='flag', device=dev)
    need(threshold, (1,), dtype=torch.float64, name='threshold', device=dev)
    _icp_state_args(state, status, dev)
    nb = icp_blocks(m)
    need(partials, (nb, nv.DC_ICP_PARTIALS), dtype=torch.float64, name='partials', device=dev)
    if kept is not None:
        need(kept, (m,), dtype=torch.uint8, name='kept', device=dev)
    max_residual = float(max_residual)
    if math.isnan(max_residual):
        raise ValueError('tsdf_icp_accumulate needs a max_residual that is a number')
    check(lib().dc_tsdf_icp_accumulate(ptr(x), ptr(sample['value']), ptr(sample['grad']), ptr(sample['dist']), ptr(sample['flag']), m,
                                       ptr(threshold), max_residual, ptr(state), ptr(status), ptr(partials), nb, ptr(kept), stream_ptr()),
          'dc_tsdf_icp_accumulate')


# ------------------------------------------------------------------------------------------------
# self-supervised training against the fused volume (csrc/dc_tsdf_loss.hip, loss.TsdfTarget)
# ------------------------------------------------------------------------------------------------
TSDF_LOSS_USED, TSDF_LOSS_INVALID, TSDF_LOSS_UNOBSERVED, TSDF_LOSS_GATED, TSDF_LOSS_MASKED = 0, 1, 2, 3, 255


class TsdfTables(object):
    """A sparse volume as tsdf_loss reads it: the table keys i64 [capacity] / slots i32 [capacity] / n_blocks i64 [1], the pool sum i64 /
    count i32 [capacity, 512], and the lattice (origin [3], voxel, trunc).  reconstruction.SparseTsdfVolume.tables() makes one."""

    def __init__(self, keys, slots, n_blocks, sum_, count, origin, voxel, trunc):
        self.keys, self.slots, self.n_blocks, self.sum, self.count = keys, slots, n_blocks, sum_, count
        self.origin, self.voxel, self.trunc = tuple(float(v) for v in origin), float(voxel), float(trunc)
        self.device = keys.device


class TsdfOwnTables(object):
    """The volumes of the single scans of a sequence as ONE structure: keys i64 [sum nb_s], ascending within each scan's segment, slots
    i32 already offset into the shared pool sum i64 / count i32 [cap_own, 512], ptr i64 [S+1] (scan s owns keys[ptr[s]:ptr[s+1]])."""

    def __init__(self, keys, slots, ptr_, sum_, count):
        self.keys, self.slots, self.ptr, self.sum, self.count = keys, slots, ptr_, sum_, count


def tsdf_loss_workspace(n, n_scans, n_terms, device):
    """Workspace of tsdf_loss for the given sizes (uint8 tensor)."""
    return _ws(lib().dc_tsdf_loss_workspace_bytes(int(n), int(n_scans), int(n_terms)), device)


@on_device
def tsdf_loss(volume_dev, ps, scan_ptr, poses12, model_kind=None, w=None, e=None, mask=None, own=None, squared=True, max_residual=None,
              min_count=1, want_exponent=False, want_points=False, out=None, ws=None):
    """Mean squared (``squared``) or absolute trilinear distance of the corrected, posed points of a sequence to the surface held by
    the sparse volume ``volume_dev`` (TsdfTables), with its gradient, in one host call of two launches (dc_tsdf_loss; the rule:
    csrc/dc_tsdf_loss_math.h).  ``ps``, ``scan_ptr``, ``poses12``, ``mask`` as for mesh_loss.  ``own`` (TsdfOwnTables): scan s is scored
    against the volume minus its own contribution (leave-one-out); None: no exclusion.  ``max_residual`` (None: the truncation): points
    with |phi| >= it are gated; a voxel counts as observed from ``min_count`` samples on.  Returns out f64 [5 + 2P + 12 S] = {mean
    loss, used, gated, unobserved, invalid, dL/dw, dL/dexponent (zero unless ``want_exponent``), dL/d[R|t]}; with ``want_points``
    also (value f64 [N]: phi, NaN unless observed; flag u8 [N]: TSDF_LOSS_*; x f64 [N,3]: the points, NaN outside the mask)."""
    if not isinstance(volume_dev, TsdfTables):
        raise TypeError('tsdf_loss takes the volume as ops.TsdfTables, got %s' % type(volume_dev).__name__)
    dev, capacity = _tsdf_sparse_table(volume_dev.keys, volume_dev.slots, volume_dev.n_blocks, 'tsdf_loss')
    if ps.device != dev:
        raise RuntimeError('points are on %s, the volume on %s' % (ps.device, dev))
    kind, nt, w, e, ns = _scan_loss_args(ps, scan_ptr, poses12, model_kind, w, e, mask, dev)
    need(volume_dev.sum, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='sum', device=dev)
    need(volume_dev.count, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='count', device=dev)
    origin, voxel, trunc, min_count = volume_dev.origin, volume_dev.voxel, volume_dev.trunc, int(min_count)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin) or not (voxel > 0.0 and math.isfinite(voxel)) or \
            not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('tsdf_loss needs a finite origin of 3 values, a voxel size and a truncation > 0, got %r, %r and %r'
                         % (origin, voxel, trunc))
    if min_count < 1:
        raise ValueError('tsdf_loss needs min_count >= 1, got %d' % min_count)
    mr = trunc if max_residual is None else float(max_residual)
    if math.isnan(mr):
        raise ValueError('max_residual must not be NaN')
    own_args = _tsdf_own_args(own, ns, dev, 'tsdf_loss')
    n_out = 5 + 2 * nt + 12 * ns
    out = _out_arg(out, n_out, dev)
    ws = _ws_arg(ws, lib().dc_tsdf_loss_workspace_bytes(ps.n, ns, nt), dev)
    value = flag = x = None
    if want_points:
        value = torch.empty((ps.n,), dtype=torch.float64, device=dev)
        flag = torch.empty((ps.n,), dtype=torch.uint8, device=dev)
        x = torch.empty((ps.n, 3), dtype=torch.float64, device=dev)
    check(lib().dc_tsdf_loss(ptr(volume_dev.keys), ptr(volume_dev.slots), ptr(volume_dev.n_blocks), capacity, ptr(volume_dev.sum),
                             ptr(volume_dev.count), *own_args, *origin, voxel, trunc, min_count, ptr(ps.vps), ptr(ps.dirs), ptr(ps.depth),
                             ptr(ps.inc), ptr(ps.lmask), ptr(mask), dtype_code(ps.dirs), ps.n, ptr(scan_ptr), ptr(poses12), ns, kind, nt,
                             ptr(w), ptr(e), int(bool(want_exponent)), int(bool(squared)), mr, ptr(value), ptr(flag), ptr(x), ptr(out),
                             ptr(ws), ws.shape[0], stream_ptr()), 'dc_tsdf_loss')
    return (out, value, flag, x) if want_points else out


# ------------------------------------------------------------------------------------------------
# ray casting the fused volume (csrc/dc_tsdf_cast.hip, reconstruction.SparseTsdfVolume.raycast)
# ------------------------------------------------------------------------------------------------
TSDF_CAST_HIT, TSDF_CAST_SKIPPED, TSDF_CAST_MISS, TSDF_CAST_BEHIND, TSDF_CAST_LOST = 0, 1, 2, 3, 4
TSDF_CAST_MAX_STEPS = 2 ** 24
_TSDF_CAST_OUT = (('face', (), torch.int32), ('t', (), torch.float64), ('inc', (), torch.float64), ('normal', (3,), torch.float64),
                  ('phi', (), torch.float64), ('status', (), torch.uint8), ('samples', (), torch.int32))


def _tsdf_own_args(own, ns, dev, who):
    """The seven exclusion arguments of dc_tsdf_loss / dc_tsdf_sparse_cast_rays from ``own`` (TsdfOwnTables of ``ns`` scans, or None)."""
    if own is None:
        return (None, None, None, 0, 0, None, None)
    if not isinstance(own, TsdfOwnTables):
        raise TypeError('%s takes own as ops.TsdfOwnTables, got %s' % (who, type(own).__name__))
    need(own.keys, (None,), dtype=torch.int64, name='own keys', device=dev)
    nk = own.keys.shape[0]
    need(own.slots, (nk,), dtype=torch.int32, name='own slots', device=dev)
    need(own.ptr, (ns + 1,), dtype=torch.int64, name='own ptr', device=dev)
    need(own.sum, (None, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='own sum', device=dev)
    cap_own = own.sum.shape[0]
    need(own.count, (cap_own, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='own count', device=dev)
    if cap_own < 1:
        raise ValueError('%s needs an own pool of at least one block' % who)
    # (keys of an empty tensor have no address: a table without keys is still a table, so it gets the pool's)
    return (ptr(own.keys) if nk else ptr(own.sum), ptr(own.slots) if nk else ptr(own.sum), ptr(own.ptr), nk, cap_own, ptr(own.sum),
            ptr(own.count))


@on_device
def tsdf_sparse_cast_rays(tables, vps, dirs, scan_offset, poses, t_min=0.0, t_max=100.0, step=None, refine=2, min_count=1, mask=None,
                          own=None, skip=True, out=None):
    """The rays of raycast_rays (vps, dirs f32 | f64 [N,3] in the sensor frame, scan-major; scan_offset, poses f64 [S,4,4] as there)
    marched through the sparse volume ``tables`` (TsdfTables) to the zero crossing of its trilinear interpolant (dc_tsdf_sparse_cast_rays;
    the rule: csrc/dc_tsdf_cast_math.h): samples at t_min + j step (``step`` None: voxel / 2; 0 < step <= trunc) up to ``t_max``, in units
    of |dirs[i]|; the crossing is refined by ``refine`` rounds of regula falsi.  ``own`` (TsdfOwnTables): scan s is cast against the
    volume minus its own contribution; ``mask`` bool / uint8 [N]: rays to skip.  Returns dict(face i32 [N] (the block's table position;
    -1 unless hit), t f64 [N] (+inf unless hit), inc f64 [N] (NaN unless hit), normal f64 [N,3] (the field's unit gradient, NaN unless
    hit), phi f64 [N] (the residual at t; NaN unless hit), status u8 [N] (TSDF_CAST_*), samples i32 [N]); face, t and inc follow
    raycast_rays' miss conventions.  ``skip`` False marches every sample (same outputs but ``samples``; for timing and tests).  ``out``:
    such a dict to write into.  One launch, nothing is read back."""
    if not isinstance(tables, TsdfTables):
        raise TypeError('tsdf_sparse_cast_rays takes the volume as ops.TsdfTables, got %s' % type(tables).__name__)
    dev, capacity = _tsdf_sparse_table(tables.keys, tables.slots, tables.n_blocks, 'tsdf_sparse_cast_rays')
    need(tables.sum, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int64, name='sum', device=dev)
    need(tables.count, (capacity, TSDF_BLOCK_VOXELS), dtype=torch.int32, name='count', device=dev)
    origin, voxel, trunc, min_count, refine = tables.origin, tables.voxel, tables.trunc, int(min_count), int(refine)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin) or not (voxel > 0.0 and math.isfinite(voxel)) or \
            not (trunc > 0.0 and math.isfinite(trunc)):
        raise ValueError('tsdf_sparse_cast_rays needs a finite origin of 3 values, a voxel size and a truncation > 0, got %r, %r and %r'
                         % (origin, voxel, trunc))
    if min_count < 1 or refine < 0:
        raise ValueError('tsdf_sparse_cast_rays needs min_count >= 1 and refine >= 0, got %d and %d' % (min_count, refine))
    t_min, t_max, step = float(t_min), float(t_max), 0.5 * voxel if step is None else float(step)
    if not (0.0 <= t_min < t_max and math.isfinite(t_max)):
        raise ValueError('tsdf_sparse_cast_rays needs 0 <= t_min < t_max, both finite, got %r and %r' % (t_min, t_max))
    if not 0.0 < step <= trunc:
        raise ValueError('tsdf_sparse_cast_rays needs 0 < step <= the truncation %g, got %r' % (trunc, step))
    if math.floor((t_max - t_min) / step) > TSDF_CAST_MAX_STEPS:
        raise ValueError('tsdf_sparse_cast_rays marches 2^24 steps at the most, got (%g - %g) / %g' % (t_max, t_min, step))
    n, code, ns, off = _measured_rays_arg(dev, vps, dirs, scan_offset, poses)
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError('mask must be bool or uint8, got %s' % mask.dtype)
        need(mask, (n,), name='mask', device=dev)
    own_args = _tsdf_own_args(own, ns, dev, 'tsdf_sparse_cast_rays')
    if out is None:
        out = {name: torch.empty((n,) + shape, dtype=dt, device=dev) for name, shape, dt in _TSDF_CAST_OUT}
    else:
        for name, shape, dt in _TSDF_CAST_OUT:
            need(out[name], (n,) + shape, dtype=dt, name=name, device=dev)
    if n == 0:
        return out
    off = off.to(dev)
    check(lib().dc_tsdf_sparse_cast_rays(ptr(tables.keys), ptr(tables.slots), ptr(tables.n_blocks), capacity, ptr(tables.sum),
                                         ptr(tables.count), *own_args, *origin, voxel, trunc, min_count, ptr(vps), ptr(dirs), ptr(mask),
                                         code, n, ptr(off), ptr(poses), ns, t_min, t_max, step, refine, 1 if skip else 0, ptr(out['face']),
                                         ptr(out['t']), ptr(out['inc']), ptr(out['normal']), ptr(out['phi']), ptr(out['status']),
                                         ptr(out['samples']), stream_ptr()), 'dc_tsdf_sparse_cast_rays')
    return out
