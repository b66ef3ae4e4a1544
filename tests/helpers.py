"""Shared helpers of the parity tests (test infrastructure)."""
import numpy as np
import torch


def t(x, dev=None, dtype=None):
    x = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None and x.dtype.is_floating_point:
        x = x.to(dtype)
    return x.to(dev) if dev is not None else x


def npy(x):
    return x.detach().cpu().numpy()


def scans_from_golden(g, dtype=torch.float64):
    """Per-scan local inputs of a fixture as CPU tensors (vps are zeros: the sensor frame)."""
    scans = []
    for s in range(int(g['n_scans'])):
        dirs = t(g['scan%d_dirs' % s], dtype=dtype)
        scans.append(dict(vps=torch.zeros_like(dirs), dirs=dirs, depth=t(g['scan%d_depth' % s], dtype=dtype),
                          inc=t(g['scan%d_inc_angles' % s], dtype=dtype), mask=t(g['scan%d_mask' % s])))
    return scans


def concat_scans(scans, dev):
    """Sequence layout of the kernels: local scans concatenated + scan ids."""
    from depth_correction_amd.ops import PointSet
    cat = lambda k: torch.cat([s[k] for s in scans]).contiguous().to(dev)
    sid = torch.cat([torch.full((len(s['dirs']),), i, dtype=torch.int32) for i, s in enumerate(scans)]).to(dev)
    return PointSet(cat('vps'), cat('dirs'), cat('depth'), cat('inc'), cat('mask'), sid)


def poses12(poses, dev):
    return torch.as_tensor(poses, dtype=torch.float64)[..., :3, :].reshape(-1, 12).contiguous().to(dev)


def rel_err(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def assert_eigvals_close(lam, ref, rtol, what=''):
    """|dlam| <= rtol |lam| + 1e-12 |C|: relative bar plus LAPACK's own absolute noise floor (eps * norm)."""
    lam, ref = np.asarray(lam, np.float64), np.asarray(ref, np.float64)
    tol = rtol * np.abs(ref) + 1e-12 * np.abs(ref).max(axis=-1, keepdims=True)
    bad = np.abs(lam - ref) > tol
    assert not bad.any(), '%s: %d eigenvalues off, worst rel %.3g' % (what, bad.sum(), (np.abs(lam - ref) / np.abs(ref))[bad].max())


# ---- SLAM tests (test_slam_host.py, test_slam_reference_host.py, test_gpu_slam_parity.py) -------------------------------------------
def slam_pose(yaw, t, roll=0.0, pitch=0.0):
    """4 x 4 pose from euler angles and a translation."""
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(roll, pitch, yaw)
    T[:3, 3] = t
    return T


def hostcheck_lib():
    """libdc_hostcheck.so (the test-only host build of the per-point math), built when it is missing."""
    import ctypes
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')
    if not os.path.exists(path):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(path)
    lib.dc_host_icp_finish.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64] + 2 * [ctypes.c_double] + 2 * [ctypes.c_int] + \
        2 * [ctypes.c_double] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_icp_finish(lib, partials, m, prm, state, status):
    """dc_host_icp_finish on partials [n_blocks, 30] with the parameters of slam_reference.params; state f64 [64] and status i32 [4]
    are numpy arrays changed in place."""
    partials = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, 30)
    rc = lib.dc_host_icp_finish(partials.ctypes.data, partials.shape[0], m, prm.icp_min_diff_rot, prm.icp_min_diff_trans,
                                int(prm.icp_smooth_length), int(prm.icp_max_iters), prm.icp_max_rotation, prm.icp_max_translation,
                                int(prm.min_pairs), state.ctypes.data, status.ctypes.data)
    assert rc == 0


# ---- the ray caster's host build (dc_raymath.h; test_raycast_host.py, test_gpu_raycast_edge.py) -------------------------------------
def raycast_host_lib():
    """hostcheck_lib() with the ray exports (rebuilt when the library at hand predates them)."""
    import ctypes
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_ray_cast_walk'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.dc_host_ray_boxes.restype = None
    lib.dc_host_ray_boxes.argtypes = [vp, i64, vp]
    lib.dc_host_ray_box_entry.restype = None
    lib.dc_host_ray_box_entry.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.dc_host_ray_prune_far.restype = None
    lib.dc_host_ray_prune_far.argtypes = [vp, i64, vp]
    lib.dc_host_ray_cast_brute.restype = None
    lib.dc_host_ray_cast_brute.argtypes = [vp, vp, i64, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp]
    lib.dc_host_ray_test_pairs.restype = None
    lib.dc_host_ray_test_pairs.argtypes = [vp, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp]
    lib.dc_host_ray_cast_walk.restype = None
    lib.dc_host_ray_cast_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp]
    return lib


def _c64(a, cols):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, cols))


def host_ray_boxes(lib, tri):
    """Leaf boxes f32 [n,6] of the triangles tri [n,9] (or [n,3,3])."""
    tri = _c64(tri, 9)
    box = np.empty((tri.shape[0], 6), dtype=np.float32)
    lib.dc_host_ray_boxes(tri.ctypes.data, tri.shape[0], box.ctypes.data)
    return box


def host_ray_box_entry(lib, o, d, box, t_far):
    """box_entry of the pairs (ray (o, d) [n,3], box f32 [n,6]) with t_far f32 [n] or a scalar -> tn f32 [n], inf where rejected."""
    o, d = _c64(o, 3), _c64(d, 3)
    n = o.shape[0]
    box = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(n, 6))
    t_far = np.ascontiguousarray(np.broadcast_to(np.asarray(t_far, dtype=np.float32), (n,)))
    assert d.shape[0] == n
    tn = np.empty(n, dtype=np.float32)
    lib.dc_host_ray_box_entry(o.ctypes.data, d.ctypes.data, box.ctypes.data, t_far.ctypes.data, n, tn.ctypes.data)
    return tn


def host_ray_prune_far(lib, t):
    """The t_far f32 [n] the traversal prunes with after a hit at t f64 [n]."""
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1))
    out = np.empty(t.shape[0], dtype=np.float32)
    lib.dc_host_ray_prune_far(t.ctypes.data, t.shape[0], out.ctypes.data)
    return out


def host_ray_cast_brute(lib, tri, o, d, t_min, cull, face_id=None, threads=8):
    """The oracle: test_triangle on every face of tri [F,9] in index order for the rays (o, d) [R,3] (world frame), t_min [R] or a
    scalar -> (face i32 [R], t, u, v f64 [R]).  The rays are split over a few threads (the library call releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    tri, o, d = _c64(tri, 9), _c64(o, 3), _c64(d, 3)
    nf, n = tri.shape[0], o.shape[0]
    assert d.shape[0] == n
    ids = np.ascontiguousarray(np.arange(nf) if face_id is None else face_id, dtype=np.int32)
    t_min = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,)))
    face, t, u, v = np.empty(n, np.int32), np.empty(n), np.empty(n), np.empty(n)
    step = max(1, -(-n // threads))

    def run(s):
        m = min(step, n - s)
        lib.dc_host_ray_cast_brute(tri.ctypes.data, ids.ctypes.data, nf, o[s:].ctypes.data, d[s:].ctypes.data, t_min[s:].ctypes.data, m,
                                   1 if cull else 0, face[s:].ctypes.data, t[s:].ctypes.data, u[s:].ctypes.data, v[s:].ctypes.data)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(run, range(0, n, step)))
    return face, t, u, v


def host_ray_cast_walk(lib, child, node_box, leaf_tri, leaf_face, o, d, t_min, cull):
    """cast_ray on the host (dc::bvh_walk with the kernels' visitor) over the tree (child i32 [n-1,2], node_box f32 [2n-1,6], leaf_tri
    [n,9], leaf_face i32 [n]) -> (face i32 [R], t, u, v f64 [R]), as host_ray_cast_brute."""
    child, box = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(node_box, dtype=np.float32)
    tri, ids, o, d = _c64(leaf_tri, 9), np.ascontiguousarray(leaf_face, dtype=np.int32), _c64(o, 3), _c64(d, 3)
    nf, n = tri.shape[0], o.shape[0]
    assert child.shape == (nf - 1, 2) and box.shape == (2 * nf - 1, 6) and ids.shape == (nf,) and d.shape[0] == n
    t_min = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,)))
    face, t, u, v = np.empty(n, np.int32), np.empty(n), np.empty(n), np.empty(n)
    lib.dc_host_ray_cast_walk(child.ctypes.data, box.ctypes.data, tri.ctypes.data, ids.ctypes.data, nf, o.ctypes.data, d.ctypes.data,
                              t_min.ctypes.data, n, 1 if cull else 0, face.ctypes.data, t.ctypes.data, u.ctypes.data, v.ctypes.data)
    return face, t, u, v


def host_ray_test_pairs(lib, tri, o, d, t_min, cull):
    """test_triangle pair by pair: ray i against triangle i -> (hit bool [n], t, u, v f64 [n])."""
    tri, o, d = _c64(tri, 9), _c64(o, 3), _c64(d, 3)
    n = tri.shape[0]
    assert o.shape[0] == n and d.shape[0] == n
    t_min = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,)))
    hit, t, u, v = np.empty(n, np.uint8), np.empty(n), np.empty(n), np.empty(n)
    lib.dc_host_ray_test_pairs(tri.ctypes.data, o.ctypes.data, d.ctypes.data, t_min.ctypes.data, n, 1 if cull else 0, hit.ctypes.data,
                               t.ctypes.data, u.ctypes.data, v.ctypes.data)
    return hit.astype(bool), t, u, v


# ---- the plane neighbourhoods' host build (dc_planemath.h; test_planes_host.py, test_gpu_planes_edge.py) ----------------------------
def planes_host_lib():
    """hostcheck_lib() with the plane exports (rebuilt when the library at hand predates them)."""
    import ctypes
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_smallest_eigvec_jacobi'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, i64, ci, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    lib.dc_host_plane_from_points.argtypes = [vp, ci, vp]
    lib.dc_host_plane_inliers.restype = None
    lib.dc_host_plane_inliers.argtypes = [vp, vp, i64, f64, vp]
    lib.dc_host_ransac_round.argtypes = [vp, ci, vp, i64, i64, i64, ci, f64, vp, vp, vp, vp, vp]
    lib.dc_host_ransac_refit_partial_count.argtypes = [i64]
    lib.dc_host_ransac_refit.argtypes = [vp, ci, vp, i64, vp, vp, vp, f64, vp, vp, vp]
    lib.dc_host_smallest_eigvec_jacobi.restype = None
    lib.dc_host_smallest_eigvec_jacobi.argtypes = [vp, vp]
    lib.dc_host_plane_refit.restype = None
    lib.dc_host_plane_refit.argtypes = [vp, vp, vp]
    lib.dc_host_dbscan.argtypes = [vp, i64, ci, ci, vp, vp]
    lib.dc_host_plane_model.restype = None
    lib.dc_host_plane_model.argtypes = [ci, ci, vp, vp, f64, f64, vp]
    lib.dc_host_plane_moments_fwd.argtypes = [vp, vp, vp, ci, vp, i64, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.dc_host_plane_moments_bwd.argtypes = [vp, vp, vp, ci, vp, i64, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


def _cloud_arg(x):
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    return x, 0 if x.dtype == np.float32 else 1


def _signed64(v):
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def host_plane_from_points(lib, p, distinct=True):
    """(valid, pl f64 [4]) of the plane through the three points p [3,3]."""
    p = _c64(p, 9)
    pl = np.empty(4)
    ok = lib.dc_host_plane_from_points(p.ctypes.data, 1 if distinct else 0, pl.ctypes.data)
    return bool(ok), pl


def host_plane_inliers(lib, pl, x, thresh):
    pl, x = _c64(pl, 4), _c64(x, 3)
    out = np.empty(x.shape[0], dtype=np.uint8)
    lib.dc_host_plane_inliers(pl.ctypes.data, x.ctypes.data, x.shape[0], float(thresh), out.ctypes.data)
    return out.astype(bool)


def host_ransac_round(lib, x, rem, seed, m, H, thresh):
    """The brute-force oracle of one RANSAC round -> dict(hyp [H,4], anchor [H,3], valid [H], counts [H], best [2])."""
    x, dt = _cloud_arg(x)
    rem = np.ascontiguousarray(rem, dtype=np.int32)
    o = dict(hyp=np.empty((H, 4)), anchor=np.empty((H, 3)), valid=np.empty(H, np.int32), counts=np.empty(H, np.int32),
             best=np.empty(2, np.int32))
    rc = lib.dc_host_ransac_round(x.ctypes.data, dt, rem.ctypes.data, len(rem), _signed64(seed), int(m), int(H), float(thresh),
                                  o['hyp'].ctypes.data, o['anchor'].ctypes.data, o['valid'].ctypes.data, o['counts'].ctypes.data,
                                  o['best'].ctypes.data)
    assert rc == 0
    return o


def host_ransac_refit(lib, x, rem, rnd, thresh):
    """The refit oracle for the round `rnd` (a dict of host_ransac_round, or the device's buffers as numpy arrays): the moments in the
    kernel's block order -> (totals [10], params [4], mask bool [n_rem])."""
    x, dt = _cloud_arg(x)
    rem = np.ascontiguousarray(rem, dtype=np.int32)
    hyp, anchor = _c64(rnd['hyp'], 4), _c64(rnd['anchor'], 3)
    best = np.ascontiguousarray(rnd['best'], dtype=np.int32)
    tot, params, mask = np.empty(10), np.empty(4), np.empty(len(rem), np.uint8)
    rc = lib.dc_host_ransac_refit(x.ctypes.data, dt, rem.ctypes.data, len(rem), hyp.ctypes.data, anchor.ctypes.data, best.ctypes.data,
                                  float(thresh), tot.ctypes.data, params.ctypes.data, mask.ctypes.data)
    assert rc == 0
    return tot, params, mask.astype(bool)


def host_smallest_eigvec(lib, cov6):
    """The refit's eigenvector step on C (xx xy xz yy yz zz): the vector before the sign rule and the normalisation."""
    c, out = _c64(cov6, 6), np.empty(3)
    lib.dc_host_smallest_eigvec_jacobi(c.ctypes.data, out.ctypes.data)
    return out


def host_plane_refit(lib, moments, anchor):
    v, a, out = _c64(moments, 10), _c64(anchor, 3), np.empty(4)
    lib.dc_host_plane_refit(v.ctypes.data, a.ctypes.data, out.ctypes.data)
    return out


def host_dbscan(lib, table, min_points):
    """Sequential DBSCAN on the padded neighbour table int32 [m,K] -> (labels [m], best label, its size)."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    m, k = table.shape
    labels, best = np.empty(m, np.int32), np.empty(2, np.int32)
    assert lib.dc_host_dbscan(table.ctypes.data, m, k, int(min_points), labels.ctypes.data, best.ctypes.data) == 0
    return labels, int(best[0]), int(best[1])


def host_plane_model(lib, code, w, e, d, g):
    """model_eval / model_dw -> (d', dd'/dd, dd'/dg, dd'/dw [P])."""
    w, e = _c64(w, 1).reshape(-1), _c64(e, 1).reshape(-1)
    out = np.zeros(3 + len(w))
    lib.dc_host_plane_model(int(code), len(w), w.ctypes.data if len(w) else None, e.ctypes.data if len(e) else None, float(d), float(g),
                            out.ctypes.data)
    return out[0], out[1], out[2], out[3:]


def _model_arg(w, e):
    if w is None:
        return 0, None, None, None, None
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
    e = np.zeros_like(w) if e is None else np.ascontiguousarray(np.asarray(e, dtype=np.float64).reshape(-1))
    return len(w), w, e, w.ctypes.data, e.ctypes.data


def host_plane_moments(lib, vps, dirs, depth, idx, normal, code, w=None, e=None, gcov=None):
    """One plane through the host build: dict(cov [3,3], mean [3], x [n,3]) and, with gcov [3,3], g_vps / g_dirs [n,3], g_depth [n],
    g_w [P] (float64, before the rounding to the cloud's dtype)."""
    vps, dt = _cloud_arg(vps)
    dirs, depth = np.ascontiguousarray(dirs, dtype=vps.dtype), np.ascontiguousarray(depth, dtype=vps.dtype).reshape(-1)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    n = len(idx)
    nrm = _c64(normal, 3)
    nt, wv, ev, wp, ep = _model_arg(w, e)
    cov, mean, x = np.empty((3, 3)), np.empty(3), np.empty((n, 3))
    rc = lib.dc_host_plane_moments_fwd(vps.ctypes.data, dirs.ctypes.data, depth.ctypes.data, dt, idx.ctypes.data, n, nrm.ctypes.data,
                                       int(code), nt, wp, ep, cov.ctypes.data, mean.ctypes.data, x.ctypes.data)
    assert rc == 0
    out = dict(cov=cov, mean=mean, x=x)
    if gcov is not None:
        g = _c64(gcov, 9)
        gv, gd, gdep, gw = np.empty((n, 3)), np.empty((n, 3)), np.empty(n), np.zeros(max(nt, 1))
        rc = lib.dc_host_plane_moments_bwd(vps.ctypes.data, dirs.ctypes.data, depth.ctypes.data, dt, idx.ctypes.data, n, nrm.ctypes.data,
                                           int(code), nt, wp, ep, mean.ctypes.data, g.ctypes.data, gv.ctypes.data, gd.ctypes.data,
                                           gdep.ctypes.data, gw.ctypes.data)
        assert rc == 0
        out.update(g_vps=gv, g_dirs=gd, g_depth=gdep, g_w=gw[:nt])
    return out


def host_fit_planes(lib, x, distance_threshold, min_support=3, max_iterations=1000, max_models=10, eps=None, seed=0, min_points=10):
    """The loop of segmentation.fit_planes with every round's RANSAC and refit from the header oracle (the kernels' own arithmetic,
    bit for bit) and the clustering from planes_reference.dbscan -> (params list of f64 [4], indices list of int64 arrays)."""
    import planes_reference as R
    x = np.ascontiguousarray(x)
    rem = np.arange(len(x), dtype=np.int32)
    params, indices = [], []
    m = 0
    while len(rem) >= 3:
        rnd = host_ransac_round(lib, x, rem, seed, m, max_iterations, distance_threshold)
        m += 1
        if rnd['best'][1] < min_support:
            break
        _, plane, mask = host_ransac_refit(lib, x, rem, rnd, distance_threshold)
        support = rem[mask]
        if len(support) < min_support:
            break
        keep = support
        if eps:
            labels, lbl, size = R.dbscan(x[support].astype(np.float64), eps, min_points)
            if size < min_support:
                rem = rem[~mask]
                if len(rem) < min_support:
                    break
                continue
            keep = support[labels == lbl]
        params.append(plane)
        indices.append(keep.astype(np.int64))
        if max_models is not None and len(params) == max_models:
            break
        rem = rem[~np.isin(rem, keep)]
        if len(rem) < min_support:
            break
    return params, indices
