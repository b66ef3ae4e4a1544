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
    if not hasattr(lib, 'dc_host_ray_cast_brute'):
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
