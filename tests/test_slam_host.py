"""SLAM evaluation on the host (no GPU): the perturbed odometry of scripts/robot_data, the metric, the CSV line and file names of
eval_slam, the ICP's 6 x 6 solve and pose update (libdc_hostcheck.so, the header the finish kernel uses), the finish kernel's state
machine through its host export against scripted registrations (tests/slam_reference.py; tests/test_gpu_slam_parity.py runs the
same table on the device) and the new Config fields."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')


@pytest.fixture(scope='module')
def host():
    if not os.path.exists(LIB):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _euler_sxyz(ai, aj, ak):
    Rx = np.array([[1, 0, 0], [0, np.cos(ai), -np.sin(ai)], [0, np.sin(ai), np.cos(ai)]])
    Ry = np.array([[np.cos(aj), 0, np.sin(aj)], [0, 1, 0], [-np.sin(aj), 0, np.cos(aj)]])
    Rz = np.array([[np.cos(ak), -np.sin(ak), 0], [np.sin(ak), np.cos(ak), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    return T


def _gt_poses(n=12, seed=3):
    rng = np.random.default_rng(seed)
    poses = []
    for i in range(n):
        T = _euler_sxyz(*(0.1 * rng.normal(size=3)))
        T[:3, 3] = [0.7 * i, 0.2 * np.sin(i), 0.05 * i]
        poses.append(T)
    return np.stack(poses)


def _robot_data_odometry(gt, odom_cov):
    """robot_data.precompute_poses with its odom_cov handling (robot_data:56-68, 123-151), written out again."""
    cov = odom_cov
    if isinstance(cov, float):
        cov = 6 * [cov]
    if len(cov) == 2:
        cov = 3 * [cov[0]] + 3 * [cov[1]]
    cov = np.array(cov)
    if cov.shape == (6,):
        cov = np.diag(cov)
    rng = np.random.default_rng(135)
    odom = gt.copy()
    for i in range(1, len(gt)):
        delta = np.linalg.solve(gt[i - 1], gt[i])
        noise = rng.multivariate_normal(np.zeros((6,)), cov)
        T = _euler_sxyz(*noise[:3])
        T[:3, 3] = noise[3:]
        odom[i] = odom[i - 1] @ (delta @ T)
    return odom


@pytest.mark.parametrize('odom_cov', [[1e-4, 2e-4, 3e-4, 2.5e-3, 1e-3, 4e-3], 'full', 2e-3, [1e-4, 2.5e-3]])
def test_odometry_matches_robot_data(odom_cov):
    from depth_correction_amd.slam import odometry_poses
    if odom_cov == 'full':
        A = np.random.default_rng(7).normal(size=(6, 6)) * 0.01
        odom_cov = (A @ A.T + 1e-4 * np.eye(6)).tolist()
    gt = _gt_poses()
    odom = odometry_poses(gt, odom_cov)
    ref = _robot_data_odometry(gt, odom_cov)
    assert np.array_equal(odom[0], gt[0])
    np.testing.assert_allclose(odom, ref, rtol=0, atol=1e-12)
    assert np.abs(odom - gt).max() > 1e-3                 # the noise is there
    np.testing.assert_allclose(odometry_poses(gt, [0.0] * 6), gt, rtol=0, atol=1e-12)


def test_odometry_cov_forms():
    from depth_correction_amd.slam import odometry_cov
    assert np.array_equal(odometry_cov(0.5), 0.5 * np.eye(6))
    assert np.array_equal(odometry_cov([1.0, 2.0]), np.diag([1.0] * 3 + [2.0] * 3))
    assert np.array_equal(odometry_cov('[1.0, 2.0]'), np.diag([1.0] * 3 + [2.0] * 3))
    assert odometry_cov(None) is None
    with pytest.raises(ValueError):
        odometry_cov([1.0, 2.0, 3.0])


def test_slam_errors_match_direct_computation():
    from depth_correction_amd.slam import path_lengths, slam_errors
    gt = _gt_poses(8)
    slam = np.stack([p @ _euler_sxyz(0.01 * i, -0.02, 0.005 * i) for i, p in enumerate(gt)])
    for i in range(len(slam)):
        slam[i, :3, 3] += [0.01 * i, -0.02, 0.003]
    lengths = path_lengths(gt)
    steps = [np.linalg.norm(np.linalg.solve(gt[i - 1], gt[i])[:3, 3]) for i in range(1, len(gt))]
    np.testing.assert_allclose(lengths, np.concatenate([[0.0], np.cumsum(steps)]), rtol=1e-14, atol=0)
    r, t, ra, ro = [], [], [], []
    for s, g, length in zip(slam, gt, lengths):
        d = np.linalg.solve(s, g)
        a = np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))
        n = np.linalg.norm(d[:3, 3])
        r.append(a)
        t.append(n)
        ra.append(a / length if length > 0 else 0.0)
        ro.append(n / length if length > 0 else 0.0)
    np.testing.assert_allclose(slam_errors(slam, gt, lengths), [np.mean(r), np.mean(t), np.mean(ra), np.mean(ro)], rtol=1e-13)


def test_csv_line_and_paths_match_reference_strings(tmp_path):
    from depth_correction_amd.config import SLAM, PoseProvider, slam_eval_bag, slam_eval_csv, slam_poses_csv
    from depth_correction_amd.scan_io import read_poses_csv, write_poses_csv
    assert list(SLAM) == ['icp_mapper'] and list(PoseProvider) == ['ground_truth', 'icp_mapper']
    assert slam_eval_csv('/log', 'icp_mapper', 'test') == '/log/slam_eval_icp_mapper_test.csv'
    assert slam_eval_csv('', 'icp_mapper') == 'slam_eval_icp_mapper.csv'
    assert slam_eval_bag('/log', 'icp_mapper') == '/log/slam_eval_icp_mapper.bag'
    assert slam_poses_csv('/log', 'seq/00', 'icp_mapper') == '/log/seq/00/slam_poses_icp_mapper.csv'
    assert slam_poses_csv(None, '', 'icp_mapper') == 'slam_poses_icp_mapper.csv'
    # eval_slam's line (robot_data:187-188)
    assert '%s %.9f %.9f %.9f %.9f\n' % ('room', 0.1, 0.2, 0.3, 0.4) == 'room 0.100000000 0.200000000 0.300000000 0.400000000\n'
    gt = _gt_poses(4)
    path = str(tmp_path / 'poses.csv')
    write_poses_csv([0, 1, 2, 3], gt, path)
    ids, poses = read_poses_csv(path)
    assert ids == [0, 1, 2, 3]
    np.testing.assert_allclose(np.stack(poses), gt, atol=1e-9)


def test_eval_slam_rejects_unknown_mapper():
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_slam
    for name in ('norlab_icp_mapper', 'ethzasl_icp_mapper'):
        with pytest.raises(ValueError, match='icp_mapper'):
            eval_slam(Config(slam=name, slam_eval_csv='x.csv'))


def test_config_slam_fields_yaml_round_trip(tmp_path):
    from depth_correction_amd.config import Config
    cfg = Config(odom_cov=[1e-4] * 3 + [2.5e-3] * 3, slam_eval_csv='a.csv', slam_poses_csv='p.csv', icp_max_iters=50,
                 slam_min_overlap=0.8, pose_provider='icp_mapper')
    path = str(tmp_path / 'cfg.yaml')
    cfg.to_yaml(path)
    back = Config().from_yaml(path)
    assert back.to_dict() == cfg.to_dict()
    d = Config()
    assert d.odom_cov == [0.0] * 6 and d.slam == 'icp_mapper' and d.pose_provider == 'ground_truth' and d.eval_slams == ['icp_mapper']
    assert (d.icp_knn, d.icp_trim_ratio, d.icp_max_normal_angle, d.icp_max_dist) == (3, 0.8, 1.57, 10.0)
    assert (d.icp_min_diff_rot, d.icp_min_diff_trans, d.icp_smooth_length, d.icp_max_iters) == (0.001, 0.01, 2, 100)
    assert (d.icp_max_rotation, d.icp_max_translation, d.slam_normals_k) == (0.8, 30.0, 9)
    assert (d.slam_min_overlap, d.slam_min_dist_new_point, d.slam_sensor_max_range) == (0.9, 0.1, 25.0)


def _pack21(A):
    return np.array([A[r, c] for r in range(6) for c in range(r, 6)])


def test_icp_solve_matches_numpy(host):
    rng = np.random.default_rng(11)
    for _ in range(50):
        J = rng.normal(size=(200, 6)) * rng.uniform(0.1, 10.0, size=6)
        r = rng.normal(size=200)
        A, b = J.T @ J, J.T @ r
        x = np.zeros(6)
        assert host.dc_host_icp_solve(_p(np.ascontiguousarray(_pack21(A))), _p(np.ascontiguousarray(b)), _p(x)) == 0
        ref = -np.linalg.solve(A, b)
        assert np.abs(x - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    A = np.zeros((6, 6))
    A[:5, :5] = np.eye(5)                      # one unconstrained degree of freedom
    assert host.dc_host_icp_solve(_p(np.ascontiguousarray(_pack21(A))), _p(np.ones(6)), _p(np.zeros(6))) == 1


def test_icp_step_matches_numpy_rodrigues(host):
    import torch
    from depth_correction_amd.transform import xyz_axis_angle_to_matrix
    rng = np.random.default_rng(12)
    for scale in (1e-9, 1e-7, 1e-3, 0.1, 1.0):
        x = rng.normal(size=6) * scale
        T = _euler_sxyz(*rng.normal(size=3))
        T[:3, 3] = rng.normal(size=3)
        out = np.zeros(16)
        host.dc_host_icp_step(_p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(T.reshape(-1))), _p(out))
        a = np.linalg.norm(x[:3])
        K = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
        R = np.eye(3) + (np.sin(a) / a if a > 0 else 1.0) * K + ((1 - np.cos(a)) / a ** 2 if a > 0 else 0.5) * K @ K
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = R, x[3:]
        np.testing.assert_allclose(out.reshape(4, 4), D @ T, rtol=0, atol=1e-12)
        D2 = xyz_axis_angle_to_matrix(torch.as_tensor(np.concatenate([x[3:], x[:3]]))).numpy()
        np.testing.assert_allclose(out.reshape(4, 4), D2 @ T, rtol=0, atol=1e-12)


# ---- dc_icp_finish as a state machine (dc_host_icp_finish: the kernel's block sum and its single-thread tail, compiled for the host)
def _host_finish(host, partials, m, prm, state, status):
    from helpers import host_icp_finish, hostcheck_lib
    host_icp_finish(hostcheck_lib(), partials, m, prm, state, status)


def _finish_cases():
    import slam_reference as R
    return R.finish_cases()


@pytest.mark.parametrize('case', _finish_cases(), ids=lambda c: c[0])
def test_icp_finish_scripted_registrations(host, case):
    """Every step of a scripted registration: status, iteration count, pairs / SSE / overlap and the history bit-equal to the Python
    restatement (slam_reference.finish), the pose within 1e-14 (numpy's Rodrigues formula against the header's quaternion form, at
    most eleven steps); a failure leaves the 16 pose words bit-identical; after the end one more call changes no byte."""
    import slam_reference as R
    name, over, steps, expect = case
    prm = R.script_params(over)
    ref = R.new_state(R.SCRIPT_PRIOR)
    state, status = R.state_vector(ref), np.zeros(4, dtype=np.int32)
    codes = []
    for step in steps:
        if status[0] != 0:
            break
        tot, m = R.script_totals(step)
        before = state.copy()
        _host_finish(host, tot, m, prm, state, status)
        R.finish(tot, m, prm, ref)
        codes.append(int(status[0]))
        want = R.state_vector(ref)
        assert status[0] == ref.code and status[1] == ref.iters == len(codes), (name, codes)
        assert state[16:].tobytes() == want[16:].tobytes(), (name, len(codes), state[32:51], want[32:51])
        assert np.abs(state[:16] - want[:16]).max() <= 1e-14, (name, len(codes))
        if status[0] < 0:
            assert state[:16].tobytes() == before[:16].tobytes(), name
        elif len(codes) > 0:
            assert state[:16].tobytes() != before[:16].tobytes(), name          # the estimate moved (max_iters keeps the update)
    assert codes == expect, (name, codes)
    frozen = (state.tobytes(), status.tobytes())
    _host_finish(host, R.script_totals(steps[0])[0], 50, prm, state, status)
    assert (state.tobytes(), status.tobytes()) == frozen, name


def test_icp_finish_bound_is_measured_from_the_prior(host):
    """Ten steps of 0.1 rad with max_rot 0.85: every single step is inside the bound, the ninth total (0.9) is not, and the estimate
    left in the state is the eighth's."""
    import slam_reference as R
    prm = R.script_params(dict(icp_max_rotation=0.85, icp_min_diff_rot=2.0 ** -30, icp_min_diff_trans=2.0 ** -30))
    state, status = R.state_vector(R.new_state(R.SCRIPT_PRIOR)), np.zeros(4, dtype=np.int32)
    x = np.zeros(6)
    x[2] = 0.1
    for _ in range(10):
        _host_finish(host, R.script_totals(x)[0], 50, prm, state, status)
    assert status[0] == R.FAIL_BOUND and status[1] == 9
    C = state[:16].reshape(4, 4) @ R.rigid_inv(R.SCRIPT_PRIOR)
    assert abs(R.rotation_angle(C) - 0.8) <= 1e-14


@pytest.mark.parametrize('n_blocks', [1, 7, 8, 9, 64, 511, 512])
def test_icp_finish_block_sum_order_is_bit_exact(host, n_blocks):
    """The documented order of the block sum (lane l of eight: blocks l, l + 8, ...; then the eight sums in order) emulated in numpy
    fp64: pairs / SSE / overlap and the pose after a step with JtJ = 2^4 I are bit-equal.  An IEEE statement, not a tolerance: the
    step rotates about z by an angle below 1e-9 from the identity, where every product of the update is exact.  The host build
    shares the per-lane loop (rows_lane_sum of dc_rowsum.h) with the finish kernel but adds the eight lane sums in a loop of its own: the kernel's
    second stage is pinned by the same case on the device (tests/test_gpu_slam_parity.py)."""
    import slam_reference as R
    partials, want_state = _block_sum_case(n_blocks)
    prm = R.script_params(dict(min_pairs=-2 ** 31 + 1, icp_max_rotation=3.0, icp_max_translation=1e30))
    state, status = R.state_vector(R.new_state(np.eye(4))), np.zeros(4, dtype=np.int32)
    _host_finish(host, partials, 64, prm, state, status)
    assert status[1] == 1 and status[0] in (0, 1)
    assert state[:16].tobytes() == want_state[:16].tobytes(), (state[:16], want_state[:16])
    assert state[48:51].tobytes() == want_state[48:51].tobytes()


def _block_sum_case(n_blocks, seed=21):
    import slam_reference as R
    return R.block_sum_case(n_blocks, seed)
