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
