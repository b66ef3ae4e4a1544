"""Sweep-aware registration on the host (no GPU): the left Jacobian of csrc/dc_sweepmath.h against numpy longdouble with the header's
rounding count, the Jacobian row of tests/slam_ct_reference.py against central differences of its own residual, dc_icp_ct_finish's
state machine through its host export against scripted registrations, the new kernels' code-object notes, the Config fields and the
refusals that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import slam_ct_reference as C
import slam_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52
LD = np.longdouble


@pytest.fixture(scope='module')
def host():
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_icp_ct_finish'):
        import __graft_entry__ as ge
        ge.build()
        lib = ctypes.CDLL(os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so'))
    vp, f64, i32, i64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int64
    lib.dc_host_sweep_left_jacobian.argtypes = [vp, vp, vp, vp]
    lib.dc_host_sweep_left_jacobian.restype = None
    lib.dc_host_icp_ct_finish.argtypes = [vp, i32, i64, f64, f64, i32, i32, f64, f64, i32, f64, f64, f64, f64, vp, vp, vp]
    lib.dc_host_icp_ct_finish.restype = i32
    return lib


def _host_jl(host, a, u=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    J, out = np.zeros(9), np.zeros(3)
    if u is None:
        host.dc_host_sweep_left_jacobian(a.ctypes.data, J.ctypes.data, None, None)
        return J.reshape(3, 3)
    u = np.ascontiguousarray(u, dtype=np.float64)
    host.dc_host_sweep_left_jacobian(a.ctypes.data, J.ctypes.data, u.ctypes.data, out.ctypes.data)
    return J.reshape(3, 3), out


def host_ct_finish(host, partials, m, prm, state, ct, status):
    partials = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, C.N_TOT)
    rc = host.dc_host_icp_ct_finish(partials.ctypes.data, partials.shape[0], m, prm.icp_min_diff_rot, prm.icp_min_diff_trans,
                                    int(prm.icp_smooth_length), int(prm.icp_max_iters), prm.icp_max_rotation, prm.icp_max_translation,
                                    int(prm.min_pairs), prm.slam_ct_prior[0], prm.slam_ct_prior[1], prm.slam_ct_max_twist[0],
                                    prm.slam_ct_max_twist[1], state.ctypes.data, ct.ctypes.data, status.ctypes.data)
    assert rc == 0


# ---- 1. the left Jacobian ------------------------------------------------------------------------------------------------------------
def _jl_angles():
    rng = np.random.default_rng(41)
    unit = lambda v: v / np.linalg.norm(v)
    out = [np.zeros(3)]
    for th in (2.0 ** -27, np.nextafter(2.0 ** -26, 0.0), 2.0 ** -26, np.nextafter(2.0 ** -26, 1.0), 1e-6, 1e-3, np.nextafter(1.0, 0.0), 1.0,
               np.nextafter(1.0, 2.0), math.pi / 2, 3.0, np.nextafter(math.pi, 0.0), math.pi):
        out += [th * np.eye(3)[k] for k in range(3)] + [th * unit(rng.normal(size=3)) for _ in range(8)]
    out += [unit(rng.normal(size=3)) * th for th in rng.uniform(0.0, math.pi, size=3000)]
    out += [unit(rng.normal(size=3)) * th for th in 10.0 ** rng.uniform(-9, 0, size=1000)]
    return out


def test_left_jacobian_holds_the_headers_count(host):
    """Every entry of J_l(a) and of J_l(a)^T u within the count of csrc/dc_sweepmath.h, (1 + 4.75 th + 3.7 th^2) 2^-52 (times |u|
    for the product, plus its own three roundings), of the longdouble matrix for the same doubles a; th from 0 over both branch
    points (2^-26, 1) to pi.  Measured on the CPU build: the largest error is 0.25 of the count for the matrix and 1.55 u in absolute
    terms -- libm's sin is far inside the 2 u the count allows the device's."""
    rng = np.random.default_rng(42)
    worst = 0.0
    worst_u = 0.0
    for a in _jl_angles():
        th = float(np.linalg.norm(a))
        u = rng.normal(size=3)
        J, jtu = _host_jl(host, a, u)
        ref = C.left_jacobian(a, dtype=LD)
        count = (1.0 + 4.75 * th + 3.7 * th * th) * U
        err = float(np.abs(J.astype(LD) - ref).max())
        worst, worst_u = max(worst, err / count), max(worst_u, err / U)
        assert err <= count, (a, err / U, count / U)
        ref_u = ref.T @ u.astype(LD)
        err_u = float(np.abs(jtu.astype(LD) - ref_u).max())
        assert err_u <= (count + 3 * U * (1 + th + th * th)) * float(np.abs(u).sum()), (a, err_u / U)
    print('left Jacobian: largest error %.3g of the count, %.3g u' % (worst, worst_u))
    J = _host_jl(host, np.array([3e-9, -4e-9, 0.0]))                 # below 2^-26: exactly I + [a]x / 2
    assert np.array_equal(J, np.eye(3) + 0.5 * C.hat(np.array([3e-9, -4e-9, 0.0])))
    assert np.isnan(_host_jl(host, np.array([np.nan, 0.0, 0.0]))).any()


def test_left_jacobian_is_the_derivative_of_the_exponential():
    """Exp(a + da) Exp(a)^T = Exp(J_l(a) da) to first order, in longdouble: what the name means."""
    rng = np.random.default_rng(43)
    for _ in range(20):
        a, da = rng.normal(size=3), rng.normal(size=3) * 1e-7
        lhs = C.sweep_rotation(a + da, LD) @ C.sweep_rotation(a, LD).T
        rhs = C.sweep_rotation(np.asarray(C.left_jacobian(a, LD) @ da.astype(LD)), LD)
        assert float(np.abs(lhs - rhs).max()) < 1e-13


# ---- 2. the Jacobian row against central differences -----------------------------------------------------------------------------------
FD_MEASURED = 2.6e-9          # the largest disagreement measured on the CPU (step 1e-6)
FD_BAR = 10 * FD_MEASURED


def test_jacobian_row_against_central_differences():
    """The row of slam_ct_reference.jacobian_rows against central differences (step 1e-6) of slam_ct_reference.residual in all twelve
    unknowns: tau in {0, 0.3, 1, -0.2}, rotations over the sweep up to 0.3 rad, points within 10 m.  The largest disagreement
    measured on the CPU is 2.6e-9 (the step's own error: h^2 / 6 times a third derivative of the order of the 10 m lever, plus the
    rounding of the residual, 2^-53 x 20 / h); the bar is ten times that, 2.6e-8."""
    rng = np.random.default_rng(44)
    unit = lambda v: v / np.linalg.norm(v)
    h, worst = 1e-6, 0.0
    for trial in range(40):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.rotation(rng.normal(size=3) * 0.5), rng.normal(size=3) * 2.0
        twist = np.concatenate([rng.normal(size=3) * 0.3, unit(rng.normal(size=3)) * rng.uniform(0.0, 0.3)])
        tau = np.array([0.0, 0.3, 1.0, -0.2])
        p = rng.uniform(-10, 10, size=(4, 3))
        n = np.stack([unit(rng.normal(size=3)) for _ in range(4)])
        y = rng.uniform(-10, 10, size=(4, 3))
        J = C.jacobian_rows(p, tau, T, twist, n)

        def res(d):
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = R.rotation(d[:3]), d[3:6]
            return C.residual(p, tau, D @ T, twist + d[6:], n, y)
        for k in range(12):
            d = np.zeros(12)
            d[k] = h
            fd = (res(d) - res(-d)) / (2 * h)
            worst = max(worst, float(np.abs(fd - J[:, k]).max()))
    print('Jacobian row against central differences: largest disagreement %.3g (bar %.3g)' % (worst, FD_BAR))
    assert worst <= FD_BAR


# ---- 3. dc_icp_ct_finish as a state machine -------------------------------------------------------------------------------------------
def _pose_terms(x, T):
    """Sum of |terms| of every entry of the updated pose [R(x[:3]) | x[3:6]] T."""
    Rm = np.abs(R.rotation(x[:3]))
    out = np.zeros((4, 4))
    out[:3, :] = Rm @ np.abs(T[:3, :])
    out[:3, 3] += np.abs(x[3:6])
    return out


@pytest.mark.parametrize('case', C.finish_cases(), ids=lambda c: c[0])
def test_ct_finish_scripted_registrations(host, case):
    """Every step of a scripted registration: status, iteration count, pairs / SSE / overlap, the history and the prior twist bit-equal
    to the reference (slam_ct_reference.finish), pose and twist within 4 ulp of the sum of their entries' terms; a failure leaves the
    16 pose words and the twist bit-identical; after the end one more call changes no byte."""
    name, over, steps, expect = case
    prm = C.script_params(over)
    ref = C.new_state(R.SCRIPT_PRIOR, C.SCRIPT_TWIST)
    (state, ct), status = C.state_vectors(ref), np.zeros(4, dtype=np.int32)
    codes = []
    for step in steps:
        if status[0] != 0:
            break
        tot, m = C.script_totals(step)
        before, ct_before = state.copy(), ct.copy()
        host_ct_finish(host, tot, m, prm, state, ct, status)
        x, _ = C.finish(tot, m, prm, ref)
        codes.append(int(status[0]))
        want, want_ct = C.state_vectors(ref)
        assert status[0] == ref.code and status[1] == ref.iters == len(codes), (name, codes)
        assert state[16:].tobytes() == want[16:].tobytes(), (name, len(codes), state[32:51], want[32:51])
        assert ct[6:].tobytes() == want_ct[6:].tobytes()
        if status[0] < 0:
            assert state[:16].tobytes() == before[:16].tobytes() and ct.tobytes() == ct_before.tobytes(), name
        else:
            bar = 4 * U * _pose_terms(x, before[:16].reshape(4, 4))
            assert (np.abs(state[:16].reshape(4, 4) - want[:16].reshape(4, 4)) <= bar).all(), (name, len(codes))
            assert (np.abs(ct[:6] - want_ct[:6]) <= 4 * U * (np.abs(ct_before[:6]) + np.abs(x[6:]))).all(), (name, len(codes))
            # the estimate moved (max_iters keeps the update)
            assert state[:16].tobytes() != before[:16].tobytes() or ct[:6].tobytes() != ct_before[:6].tobytes(), name
    assert codes == expect, (name, codes)
    frozen = (state.tobytes(), ct.tobytes(), status.tobytes())
    host_ct_finish(host, C.script_totals(steps[0])[0], 50, prm, state, ct, status)
    assert (state.tobytes(), ct.tobytes(), status.tobytes()) == frozen, name


def _well_posed(seed, n=400):
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(n, 12)) * np.array([3.0] * 3 + [1.0] * 3 + [0.5] * 3 + [1.5] * 3)
    J[:, 6:9] = J[:, 3:6] * rng.uniform(0.0, 1.0, size=(n, 1))            # J_v = tau n_s: the coupling the prior is there for
    r = rng.normal(size=n) * 0.01
    tot = np.zeros(C.N_TOT)
    tot[:78], tot[78:90] = C.pack78(J.T @ J), J.T @ r
    tot[90], tot[91], tot[92] = n, float(r @ r), n
    return tot


@pytest.mark.parametrize('beta', [(0.0, 0.0), (0.01, 0.01), (1.0, 0.25)])
def test_ct_finish_well_posed_system_and_prior(host, beta):
    """A well-posed 12 x 12 system with the prior: the step the host build solved (read off the twist, which is updated additively)
    against the extended-precision solve within 1e-12 max(1, |x|), the bar of the 6 x 6 solve in test_slam_host.py; with beta > 0 and
    a twist away from its prior the step differs from the one without the prior."""
    prm = C.script_params(dict(slam_ct_prior=beta, icp_max_rotation=3.0, slam_ct_max_twist=(30.0, 3.0)))
    steps = []
    for seed in range(5):
        tot = _well_posed(seed)
        ref = C.new_state(R.SCRIPT_PRIOR, C.SCRIPT_TWIST)
        ref.twist = ref.twist + np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.001])     # the estimate has left the prior
        (state, ct), status = C.state_vectors(ref), np.zeros(4, dtype=np.int32)
        before = ct.copy()
        host_ct_finish(host, tot, 400, prm, state, ct, status)
        x, _ = C.finish(tot, 400, prm, ref)
        want, want_ct = C.state_vectors(ref)
        assert status[0] == ref.code == 0
        got_x = ct[:6] - before[:6]
        assert np.abs(got_x - x[6:]).max() <= 1e-12 * max(1.0, np.abs(x).max())
        assert np.abs(state[:16] - want[:16]).max() <= 1e-12 * max(1.0, np.abs(x).max()) * 4
        steps.append(x)
    if beta != (0.0, 0.0):
        free = C.script_params(dict(slam_ct_prior=(0.0, 0.0), icp_max_rotation=3.0, slam_ct_max_twist=(30.0, 3.0)))
        for seed, x in enumerate(steps):
            ref = C.new_state(R.SCRIPT_PRIOR, C.SCRIPT_TWIST)
            ref.twist = ref.twist + np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.001])
            x0, _ = C.finish(_well_posed(seed), 400, free, ref)
            assert np.abs(x - x0).max() > 1e-6


def test_ct_finish_prior_makes_equal_times_solvable(host):
    """All sweep times equal: singular without the prior (a scripted case above), solved with it; the twist moves toward its prior."""
    A = np.eye(12)
    A[6:9, 6:9], A[3:6, 6:9], A[6:9, 3:6] = 0.25 * np.eye(3), 0.5 * np.eye(3), 0.5 * np.eye(3)
    prm = C.script_params(dict(slam_ct_prior=(2.0 ** -7, 2.0 ** -7)))
    ref = C.new_state(R.SCRIPT_PRIOR, C.SCRIPT_TWIST)
    ref.twist = ref.twist + np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0])
    (state, ct), status = C.state_vectors(ref), np.zeros(4, dtype=np.int32)
    tot, m = C.script_totals(dict(x=np.zeros(12), A=A, pairs=128.0))
    host_ct_finish(host, tot, m, prm, state, ct, status)
    x, _ = C.finish(tot, m, prm, ref)
    assert status[0] == ref.code == 0 and x is not None
    assert abs(ct[0] - C.SCRIPT_TWIST[0]) < 0.5 and np.abs(ct[:6] - ref.twist).max() <= 1e-12


def test_ct_finish_refuses_bad_arguments(host):
    prm = C.script_params({})
    (state, ct), status = C.state_vectors(C.new_state(np.eye(4))), np.zeros(4, dtype=np.int32)
    tot = np.zeros((1, C.N_TOT))
    call = lambda **kw: host.dc_host_icp_ct_finish(tot.ctypes.data, kw.get('nb', 1), 50, 1e-3, 1e-2, kw.get('smooth', 2), 100, 0.8, 30.0, 6,
                                                   kw.get('beta', 0.0), 0.0, 1.0, 1.0, state.ctypes.data, ct.ctypes.data, status.ctypes.data)
    assert call() == 0
    assert call(nb=0) == 1 and call(nb=513) == 1 and call(smooth=0) == 1 and call(smooth=9) == 1
    assert call(beta=-1.0) == 1 and call(beta=float('nan')) == 1
    assert prm.slam_ct_prior == (0.0, 0.0)


@pytest.mark.parametrize('n_blocks', [1, 7, 8, 9, 511, 512])
def test_ct_finish_block_sum_order(host, n_blocks):
    """The documented order of the block sum over rows of 93 values: pairs, SSE and overlap bit-equal to the numpy emulation."""
    rng = np.random.default_rng(50 + n_blocks)
    part = np.zeros((n_blocks, C.N_TOT))
    part[:, 90:93] = 10.0 ** rng.uniform(-6, 6, size=(n_blocks, 3))
    part[0, :78] = C.pack78(16.0 * np.eye(12))
    tot = C.block_sum(part)
    prm = C.script_params(dict(min_pairs=0))
    (state, ct), status = C.state_vectors(C.new_state(np.eye(4))), np.zeros(4, dtype=np.int32)
    host_ct_finish(host, part, 64, prm, state, ct, status)
    assert status[1] == 1
    assert state[48] == tot[90] and state[49] == tot[91] and state[50] == tot[92] / 64.0


# ---- 4. the code object ---------------------------------------------------------------------------------------------------------------
def test_ct_kernels_have_no_private_segment():
    """icp_ct_accumulate_kernel keeps its 93 fp64 sums in registers: no private segment in the pair and finish kernels of either
    registration nor in icp_ct_init_kernel, at most 512 registers per lane (one wavefront per SIMD); the pair kernels' LDS is the
    block sum's one row per wavefront (4 x 30 and 4 x 93 doubles).  Metadata notes of the built library only."""
    from test_step_kernel_resources import _code_objects, _kernels
    import __graft_entry__ as ge
    ge.build()
    from depth_correction_amd import _native
    blob = open(_native.lib_path(), 'rb').read()
    found = {}
    for elf in _code_objects(blob):
        for k in _kernels(elf):
            m = re.search(r'\d+(icp_accumulate_kernel|icp_finish_kernel|icp_ct_init_kernel|icp_ct_accumulate_kernel|icp_ct_finish_kernel)E',
                          k['.name'])
            if m:
                found[m.group(1)] = k
    assert len(found) == 5, sorted(found)
    for name, k in sorted(found.items()):
        print('%s: vgpr %d sgpr %d scratch %d lds %d' % (name, k['.vgpr_count'], k['.sgpr_count'], k['.private_segment_fixed_size'],
                                                         k['.group_segment_fixed_size']))
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_count'] <= 512, name
    assert found['icp_accumulate_kernel']['.group_segment_fixed_size'] == 4 * 30 * 8
    assert found['icp_ct_accumulate_kernel']['.group_segment_fixed_size'] == 4 * 93 * 8


# ---- 5. configuration and refusals ----------------------------------------------------------------------------------------------------
def test_config_fields_and_defaults(tmp_path):
    from depth_correction_amd.config import Config
    d = Config()
    assert d.slam_ct is False and list(d.slam_ct_prior) == [1e-4, 1e-4] and d.slam_ct_max_twist is None
    cfg = Config(slam_ct=True, slam_ct_prior=[0.5, 0.25], slam_ct_max_twist=[1.0, 0.5])
    path = str(tmp_path / 'cfg.yaml')
    cfg.to_yaml(path)
    assert Config().from_yaml(path).to_dict() == cfg.to_dict()


def test_run_slam_refuses_ct_with_deskew():
    from depth_correction_amd.config import Config
    from depth_correction_amd.slam import run_slam
    with pytest.raises(ValueError, match='slam_ct'):
        run_slam([], None, Config(slam_ct=True, slam_deskew=True))


def test_mapper_scan_keeps_its_signature():
    from depth_correction_amd.slam import MapperScan
    s = MapperScan(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2))
    assert s.t is None and len(s) == 2
    assert MapperScan(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2), t=np.zeros(2)).t is not None


def test_depth_cloud_carries_sweep_times():
    """DepthCloud.sweep_t is a per-row field: copy, clone, to and every row selection take it along; a cloud without it has None."""
    import torch
    from depth_correction_amd.depth_cloud import DepthCloud
    pts = torch.arange(30, dtype=torch.float64).reshape(10, 3) + 1.0
    dc = DepthCloud.from_points(pts, dtype=torch.float64)
    assert dc.sweep_t is None and dc.copy().sweep_t is None and dc[2:5].sweep_t is None
    t = torch.linspace(0.0, 0.9, 10, dtype=torch.float64)
    dc.sweep_t = t
    assert dc.copy().sweep_t is t
    assert torch.equal(dc.clone().sweep_t, t) and dc.clone().sweep_t is not t
    assert torch.equal(dc.to(dtype=torch.float32).sweep_t, t) and dc.to(dtype=torch.float32).sweep_t.dtype == torch.float64
    assert torch.equal(dc[2:5].sweep_t, t[2:5]) and torch.equal(dc[torch.tensor([7, 1])].sweep_t, t[[7, 1]])
    keep = torch.arange(10) % 3 == 0
    assert torch.equal(dc[keep].sweep_t, t[keep]) and len(dc[keep]) == 4
    assert dc[['vps', 'dirs', 'depth']].sweep_t is t
    with pytest.raises(AssertionError):
        DepthCloud(dc.vps, dc.dirs, dc.depth, sweep_t=t[:5])


# ---- 6. where the per-iteration bar of the GPU parity test comes from -------------------------------------------------------------------
def _host_cast_scene():
    """The parity scene of tests/test_gpu_slam_ct.py built without a GPU: the pillared room cast by the host build's brute-force
    oracle, the static scan of pose 0 as the map and the swept scan of pose 1 as the reading, normals from slam_reference.normals."""
    import sweep_reference as S
    from helpers import host_ray_cast_brute, raycast_host_lib, slam_pose
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.sweep import sweep_matrix, sweep_times
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    tri = np.asarray(mesh.vertices, dtype=np.float64)[np.asarray(mesh.faces)].reshape(-1, 9)
    lib = raycast_host_lib()
    dirs, tmin = lidar_directions((16, 256), (45.0, 360.0), 16)
    tau = sweep_times(dirs, (45.0, 360.0))
    twist = np.array([0.25, 0.05, 0.0, 0.0, 0.0, 0.08])
    poses = S.constant_twist_poses(slam_pose(0.1, (-1.5, -0.3, 0.2), 0.02, -0.015), twist, 2)

    def scan(T, tw):
        W = np.stack([T @ (sweep_matrix(tw, t) if tw is not None else np.eye(4)) for t in tau])
        face, t, _, _ = host_ray_cast_brute(lib, tri, W[:, :3, 3], np.einsum('nij,nj->ni', W[:, :3, :3], dirs), tmin, True)
        ok = (face >= 0) & (t >= 0.5)
        return dirs[ok] * t[ok, None], tau[ok]
    mp, _ = scan(poses[0], None)
    p, pt = scan(poses[1], twist)
    mn, pn = R.normals(mp, 9)[0], R.normals(p, 9)[0]
    return R.moved(poses[0], mp), mn @ poses[0][:3, :3].T, p, pn, pt, poses[1], twist


def test_reference_sensitivity_behind_the_parity_bar():
    """The per-iteration bar of test_gpu_slam_ct.test_parity_iteration_by_iteration is 2 000 x C.REF_SENSITIVITY, the largest change of
    the reference's own poses and twists when the order of its extended-precision sums is permuted (3.61e-16 over 200 random orders
    of this scene).  Recomputed here over eight orders on the host-cast scene: the same registration (status, iterations, twist
    within a tenth of its norm, margins) and no change above the constant."""
    from scipy.spatial import cKDTree
    from helpers import slam_pose
    mp, mn, p, pn, tau, gt, twist = _host_cast_scene()
    prm = C.params(slam_ct_prior=(0.001, 0.001), icp_max_normal_angle=0.3)
    prior = gt @ slam_pose(0.03, (0.1, -0.05, 0.02))
    tree = cKDTree(mp)
    reg = C.register(mp, mn, p, pn, tau, prior, np.zeros(6), prm, tree)
    assert reg.status == 'converged' and np.linalg.norm(reg.twist - twist) <= 0.1 * np.linalg.norm(twist)
    for r in reg.records:
        assert min(r.margins['thr'], r.margins['normal'], r.margins.get('conv_rot', 1.0), r.margins.get('conv_trans', 1.0)) >= 1e-9
    worst = 0.0
    for seed in range(100, 1700, 200):
        other = C.register(mp, mn, p, pn, tau, prior, np.zeros(6), prm, tree, order_seed=seed)
        assert other.iterations == reg.iterations and other.status == reg.status
        for a, b in zip(reg.records, other.records):
            worst = max(worst, float(np.abs(a.pose - b.pose).max()), float(np.abs(a.twist - b.twist).max()))
    print('reference sensitivity to the order of its sums over 8 orders: %.3g (constant %.3g)' % (worst, C.REF_SENSITIVITY))
    assert worst <= C.REF_SENSITIVITY
