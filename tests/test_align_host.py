"""Survey registration on the host (no GPU): the closed-form solver of dc_align_finish through its host build (csrc/dc_align_math.h in
libdc_hostcheck.so, the header the kernel includes) against route A of tests/align_reference.py, the status rules, the accurate
rotation angle, the conditions of the reference scene the GPU tests rely on, and the Python surface that needs no device
(absolute_orientation, align_paths, the configuration keys).

Bars (align_reference.bars): bar_R and bar_t are 16 x the largest disagreement of route A (means + SVD) and route B (fsum moments +
eigh of Horn's matrix) along the 25-iteration reference trajectory of the noisy scene, floors 16 eps and 16 ulp of the largest
coordinate; the test prints them.  Measured on a CPU: dR 8.9e-16, dt 1.4e-14 m (n = 4099), so bar_R 1.4e-14 and bar_t 2.2e-13 m; in
the shifted scene (coordinates near 2e5 m) dt 5.0e-10 m, bar_t 7.9e-9 m: the translation is the image of an origin 2e5 m away from
the data, and both routes resolve it to a few ulp of that distance times the rotation's own rounding.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_reference as A  # noqa: E402

STATE_COUNT, POSE, THRESHOLD, PAIRS, RMS = 64, 0, 32, 33, 34
CONVERGED, MAX_ITERS, FAIL_PAIRS, FAIL_DEGENERATE, FAIL_NONFINITE = 1, 2, -1, -2, -3


def host_lib():
    """libdc_hostcheck.so with the registration exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_align_finish'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.dc_host_align_solve.argtypes = [vp, vp, vp, vp]
    lib.dc_host_align_angle.restype = f64
    lib.dc_host_align_angle.argtypes = [vp, vp]
    lib.dc_host_align_finish.argtypes = [vp, ci, vp, f64, f64, ci, ci, vp, vp, vp, ci]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def pair_origins(p, y):
    return np.concatenate([0.5 * (p.min(axis=0) + p.max(axis=0)), 0.5 * (y.min(axis=0) + y.max(axis=0))])


def pair_moments(p, y, o):
    return A.moments(p, y, np.linalg.norm(y - p, axis=1), o)


def host_finish(lib, partials, o, T0=None, min_rot=0.0, min_trans=0.0, min_pairs=3, max_iters=5, status=None):
    """dc_host_align_finish on partials [n_blocks, 17] -> (state [64], status [4], history [max_iters, 5])."""
    partials = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, 17)
    state = np.full(STATE_COUNT, np.nan)
    state[POSE:POSE + 16] = (np.eye(4) if T0 is None else T0).reshape(-1)
    state[THRESHOLD] = np.inf
    status = np.zeros(4, np.int32) if status is None else status
    hist = np.full((max_iters, 5), np.nan)
    o = np.ascontiguousarray(o, dtype=np.float64)
    rc = lib.dc_host_align_finish(partials.ctypes.data, partials.shape[0], o.ctypes.data, min_rot, min_trans, min_pairs, max_iters,
                                  state.ctypes.data, status.ctypes.data, hist.ctypes.data, max_iters)
    assert rc == 0
    return state, status, hist


def set_bars(name):
    return A.scene_bars(4099, shifted=(name == 'shifted'))


# ---- the solver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(A.pair_sets()))
def test_solver_against_route_a(lib, name):
    p, y = A.pair_sets()[name]
    Ta, s, d = A.fit_svd(p, y)
    if name == 'mirrored':
        assert d == -1.0 and (s[1] - s[2]) / s[0] > 1e-6            # the proper-rotation optimum is unique
    else:
        assert d == 1.0
    o = pair_origins(p, y)
    m = pair_moments(p, y, o)
    state, status, hist = host_finish(lib, m, o, max_iters=1)
    T = state[POSE:POSE + 16].reshape(4, 4)
    bar_R, bar_t = set_bars(name)
    dR, dt = np.abs(T - Ta)[:3, :3].max(), np.abs(T - Ta)[:3, 3].max()
    print('%s: |R - R_A| %.3g (bar %.3g), |t - t_A| %.3g m (bar %.3g m)' % (name, dR, bar_R, dt, bar_t))
    assert status[0] == MAX_ITERS and status[1] == 1
    assert dR <= bar_R and dt <= bar_t
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) <= 16 * A.EPS
    W = len(p)
    assert hist[0, 0] == W and hist[0, 2] == np.inf
    assert abs(hist[0, 1] - math.sqrt(np.mean(np.sum((y - p) ** 2, axis=1)))) <= 16 * A.EPS * max(1.0, hist[0, 1])
    d_rot, d_trans = A.increment(Ta, np.eye(4), o[:3])
    assert abs(hist[0, 3] - d_rot) <= 4 * bar_R and abs(hist[0, 4] - d_trans) <= 4 * bar_t + 4 * bar_R * np.abs(o[:3]).max()


def test_blocks_are_summed_in_the_finish_order(lib):
    """Partials of several blocks: lane l of eight adds the rows l, l + 8, ... in order, then the eight sums in order."""
    p, y = A.pair_sets()['generic']
    o = pair_origins(p, y)
    rows = np.stack([pair_moments(p[i:i + 2], y[i:i + 2], o) for i in range(0, 40, 2)])            # 20 rows
    lanes = [np.zeros(17) for _ in range(8)]
    for b, row in enumerate(rows):
        lanes[b % 8] = lanes[b % 8] + row
    tot = np.zeros(17)
    for lane in lanes:
        tot = tot + lane
    one = host_finish(lib, tot, o, max_iters=1)[0]
    many = host_finish(lib, rows, o, max_iters=1)[0]
    assert np.array_equal(one[:16], many[:16])


@pytest.mark.parametrize('name', sorted(A.degenerate_sets()))
def test_degenerate_pairs_leave_the_estimate(lib, name):
    p, y = A.degenerate_sets()[name]
    o = pair_origins(p, y)
    T0 = A.rigid(A.axis_angle((0.0, 0.0, 1.0), 0.1), (1.0, 2.0, 3.0))
    state, status, hist = host_finish(lib, pair_moments(p, y, o), o, T0=T0)
    assert status[0] == FAIL_DEGENERATE and status[1] == 1
    assert np.array_equal(state[POSE:POSE + 16].reshape(4, 4), T0)
    assert hist[0, 0] == len(p) and np.isnan(hist[0, 3:]).all() and np.isnan(hist[1:]).all()


def test_too_few_pairs_and_nonfinite_moments(lib):
    p, y = A.pair_sets()['generic']
    o = pair_origins(p, y)
    T0 = A.rigid(A.axis_angle((1.0, 0.0, 0.0), 0.2), (0.5, 0.0, -0.5))
    state, status, _ = host_finish(lib, pair_moments(p[:2], y[:2], o), o, T0=T0)
    assert status[0] == FAIL_PAIRS and np.array_equal(state[POSE:POSE + 16].reshape(4, 4), T0) and state[PAIRS] == 2
    state, status, _ = host_finish(lib, pair_moments(p[:5], y[:5], o), o, T0=T0, min_pairs=6)
    assert status[0] == FAIL_PAIRS
    for col in (1, 5, 9, 16):
        m = pair_moments(p, y, o)
        m[col] = np.nan
        state, status, hist = host_finish(lib, m, o, T0=T0)
        assert status[0] == FAIL_NONFINITE, col
        assert np.array_equal(state[POSE:POSE + 16].reshape(4, 4), T0)
    # a status word that is set: nothing is touched
    st = np.array([CONVERGED, 7, 0, 0], np.int32)
    state, status, hist = host_finish(lib, pair_moments(p, y, o), o, T0=T0, status=st)
    assert list(status) == [CONVERGED, 7, 0, 0] and np.array_equal(state[POSE:POSE + 16].reshape(4, 4), T0) and np.isnan(hist).all()


def test_status_order_converged_then_max_iters(lib):
    p, y = A.pair_sets()['identity']
    o = pair_origins(p, y)
    m = pair_moments(p, y, o)
    assert host_finish(lib, m, o, min_rot=1e-9, min_trans=1e-9, max_iters=1)[1][0] == CONVERGED       # before MAX_ITERS
    assert host_finish(lib, m, o, max_iters=1)[1][0] == MAX_ITERS                                     # 0 disables: strict <
    assert host_finish(lib, m, o, max_iters=2)[1][0] == 0
    p, y = A.pair_sets()['generic']
    o = pair_origins(p, y)
    assert host_finish(lib, pair_moments(p, y, o), o, min_rot=1e-9, min_trans=1e-9, max_iters=3)[1][0] == 0


def test_accurate_angle_resolves_tiny_rotations(lib):
    for angle in (1e-12, 3e-10, 1e-7, 0.5, math.pi - 1e-9):
        Ta = np.ascontiguousarray(A.rigid(A.axis_angle((0.3, -0.2, 1.0), 0.4 + angle), (1.0, 2.0, 3.0)))
        Tb = np.ascontiguousarray(A.rigid(A.axis_angle((0.3, -0.2, 1.0), 0.4), (0.0, 0.0, 0.0)))
        got = lib.dc_host_align_angle(Ta.ctypes.data, Tb.ctypes.data)
        D = Ta[:3, :3] @ Tb[:3, :3].T
        print('angle %.3g: atan2 form %.6g, arccos form %.6g' % (angle, got, math.acos(max(-1.0, min(1.0, 0.5 * (np.trace(D) - 1.0))))))
        # the matrices themselves carry eps-sized entries: 1e-3 relative at 1e-12 rad is what they allow
        assert abs(got - angle) <= 1e-3 * angle
    small = np.ascontiguousarray(A.rigid(A.axis_angle((0.0, 0.0, 1.0), 1e-12), (0.0, 0.0, 0.0)))
    eye = np.eye(4)
    assert math.acos(min(1.0, 0.5 * (np.trace(small[:3, :3]) - 1.0))) == 0.0                          # what arccos returns
    assert abs(lib.dc_host_align_angle(small.ctypes.data, eye.ctypes.data) - 1e-12) <= 1e-15


# ---- the scene conditions the GPU tests rely on, on the reference alone ----------------------------------------------------------------
@pytest.mark.parametrize('n', A.SIZES)
def test_noise_free_scene_converges_to_the_true_transform(n):
    sc = A.scene(n)
    r = A.icp(sc, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    fit = np.abs(A.move(r['T'], sc['query'][:n]) - sc['survey'][sc['inlier_idx']]).max()
    print('n = %d: %s after %d iterations, max |T p - y| %.3g m (bar %.3g m), A vs B: dR %.3g dt %.3g m'
          % (n, r['status'], r['iterations'], fit, A.BAR_PT, r['dR'], r['dt']))
    assert r['status'] == 'converged' and r['iterations'] <= 40 and fit <= A.BAR_PT
    assert np.isnan(r['history'][r['iterations']:]).all() and np.isfinite(r['history'][:r['iterations']]).all()


@pytest.mark.parametrize('n', A.SIZES)
def test_noisy_trajectory_decides_clearly(n):
    """At the iterations the GPU step test starts from: no matched distance within 2 bar_pt of the threshold other than one equal to
    it, none within 2 bar_pt of the gate, and the brute-force second-best neighbour clearly behind the best (the index rule of
    test_gpu_cloudloss.py) for all but a few points."""
    sc = A.scene(n, A.SIGMA)
    tr = A.trajectory(n)
    bar_R, bar_t = A.scene_bars(n)
    print('n = %d: A vs B along the trajectory: dR %.3g dt %.3g m -> bar_R %.3g bar_t %.3g m' % (n, tr['dR'], tr['dt'], bar_R, bar_t))
    assert tr['iterations'] == 25 and len(tr['poses']) == 26
    for k in A.STEPS:
        s = A.step(sc, tr['poses'][k])
        d = s['d'][s['idx'] >= 0]
        near = (np.abs(d - s['tau']) <= 2 * A.BAR_PT) & (d != s['tau'])
        assert not near.any(), (k, d[near])
        assert np.abs(d - A.MAX_DIST).min() > 2 * A.BAR_PT
        x = A.move(tr['poses'][k], sc['query'])
        idx, d2, second = A.nearest(sc['survey'], x)
        clear = second - d2 > 1e-9 * A.EXTENT ** 2
        matched = d2 < A.MAX_DIST ** 2
        assert np.array_equal(np.where(matched, idx, -1)[clear], s['idx'][clear])
        assert (~clear).mean() <= 0.01
        assert s['W'] >= 0.7 * n


def test_shifted_scene_needs_centred_moments():
    """With the scene moved by (1e5, -2e5, 3e4) m the reference still converges to a few ulp of 2e5 m."""
    n = A.SIZES[-1]
    sc = A.scene(n, 0.0, True)
    r = A.icp(sc, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    fit = np.abs(A.move(r['T'], sc['query'][:n]) - sc['survey'][sc['inlier_idx']]).max()
    print('shifted: %s after %d iterations, max |T p - y| %.3g m = %.1f ulp of 2e5' % (r['status'], r['iterations'], fit, fit / np.spacing(2e5)))
    assert r['status'] == 'converged' and r['iterations'] <= 40 and fit <= 64 * np.spacing(2e5)


# ---- the Python surface that needs no device ----------------------------------------------------------------------------------------
def test_absolute_orientation_is_route_a():
    from depth_correction_amd.registration import absolute_orientation
    bar_R, bar_t = A.scene_bars(4099)
    for name, (p, y) in A.pair_sets().items():
        if name in ('mirrored', 'shifted'):
            continue
        T = absolute_orientation(p.T, y.T)
        Ta = A.fit_svd(p, y)[0]
        assert np.abs(T - Ta)[:3, :3].max() <= bar_R and np.abs(T - Ta)[:3, 3].max() <= bar_t, name
        # a minimum: perturbing the result raises the residual
        res = lambda M: np.sum((p @ M[:3, :3].T + M[:3, 3] - y) ** 2)
        for axis in np.eye(3):
            for sign in (-1.0, 1.0):
                assert res(A.rigid(A.axis_angle(axis, sign * 1e-4), (0, 0, 0)) @ T) > res(T)
                assert res(A.rigid(np.eye(3), sign * 1e-4 * axis) @ T) > res(T)
    p2 = np.random.default_rng(1).normal(size=(2, 30))
    c, s = math.cos(0.3), math.sin(0.3)
    T2 = absolute_orientation(p2, np.array([[c, -s], [s, c]]) @ p2 + [[1.0], [2.0]])
    assert T2.shape == (3, 3) and np.allclose(T2, [[c, -s, 1.0], [s, c, 2.0], [0, 0, 1]], atol=1e-14)
    with pytest.raises(ValueError):
        absolute_orientation(np.zeros((3, 4)), np.zeros((3, 5)))


def test_absolute_orientation_raises_on_a_reflection():
    from depth_correction_amd.registration import absolute_orientation
    p, y = A.pair_sets()['mirrored']
    with pytest.raises(ValueError, match='reflection'):
        absolute_orientation(p.T, y.T)
    T = absolute_orientation(p.T, y.T, fix_reflection=True)
    Ta = A.fit_svd(p, y)[0]
    bar_R, bar_t = A.scene_bars(4099)
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-14
    assert np.abs(T - Ta)[:3, :3].max() <= bar_R and np.abs(T - Ta)[:3, 3].max() <= bar_t


def test_align_paths_recovers_a_known_transform():
    from depth_correction_amd.registration import align_paths
    rng = np.random.default_rng(3)
    pos = np.cumsum(rng.normal(0.0, 0.5, size=(30, 3)), axis=0)
    T = A.rigid(A.axis_angle((0.2, 0.1, 1.0), 0.8), (3.0, -2.0, 0.5))
    poses = np.tile(np.eye(4), (30, 1, 1))
    poses[:, :3, 3] = pos
    poses[:, :3, :3] = A.axis_angle((1.0, 0.0, 0.0), 0.3)
    moved = T @ poses
    out = align_paths(poses, moved)
    assert np.abs(out['T'] - T).max() < 1e-12 and out['errors'].shape == (30,) and out['rmse'] < 1e-12 and out['mean'] <= out['rmse']
    out = align_paths(pos, moved[:, :3, 3])
    assert np.abs(out['T'] - T).max() < 1e-12
    noisy = moved[:, :3, 3] + rng.normal(0.0, 0.01, size=(30, 3))
    out = align_paths(pos, noisy)
    assert 0.005 < out['rmse'] < 0.03 and abs(out['rmse'] - math.sqrt(np.mean(out['errors'] ** 2))) < 1e-15
    with pytest.raises(ValueError):
        align_paths(pos, noisy[:-1])


def test_config_round_trip_of_the_registration_keys(tmp_path):
    from depth_correction_amd.config import Config
    cfg = Config()
    assert cfg.map_eval_register is False
    assert cfg.register_kwargs == {'inlier_ratio': 0.8, 'max_dist': 1.0, 'n_iters': 50, 'min_rot': 1e-6, 'min_trans': 1e-6}
    cfg.map_eval_register = True
    cfg.register_kwargs = dict(cfg.register_kwargs, max_dist=0.5, n_iters=20)
    path = str(tmp_path / 'cfg.yaml')
    cfg.to_yaml(path)
    back = Config().from_yaml(path)
    assert back.map_eval_register is True and back.register_kwargs == cfg.register_kwargs
    assert set(back.non_default()) == {'map_eval_register', 'register_kwargs'}
    assert Config().copy().register_kwargs is not Config().register_kwargs
