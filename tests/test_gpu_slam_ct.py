"""Sweep-aware registration on the device against tests/slam_ct_reference.py (numpy + cKDTree, fp64, sums in extended precision):
dc_icp_ct_accumulate on hand-written tables at the sizes where it can go wrong, dc_icp_ct_finish's state machine on scripted
registrations, zero motion against the 6-dof path, a whole registration of a swept scan iteration by iteration, the sweep times
through mapper_input and prepare, and run_slam on the six-pose arc of tests/test_gpu_sweep.py raw, de-skewed by the odometry and
sweep-aware.

The bars.  Totals: (n + 16) 2^-53 sum|term|, what dc_icp_accumulate is held to.  Pose and twist entries per iteration: 2 000 x the
largest change of the reference's own result on the parity scene when the order of its sums is permuted (DESIGN "SLAM evaluation"
makes the 6-dof bar the same way); measured on the CPU over 200 random orders: slam_ct_reference.REF_SENSITIVITY.  Every discrete decision of the
reference (threshold, normal gate, convergence) must keep a relative margin of MARGIN_FLOOR, asserted on the data the device used.
"""
import math

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import slam_ct_reference as C
import slam_reference as R
import sweep_reference as S
from helpers import slam_pose
from test_slam_ct_host import host, host_ct_finish          # noqa: F401 (host is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN_FLOOR = 1e-9
CT_BAR = 2000 * C.REF_SENSITIVITY                        # 7.2e-13; tests/test_slam_ct_host.py recomputes the sensitivity
TWIST = np.array([0.25, 0.05, 0.0, 0.0, 0.0, 0.08])
OFFSET = slam_pose(0.03, (0.1, -0.05, 0.02))
PARITY = dict(slam_ct_prior=[0.001, 0.001], icp_max_normal_angle=0.3)       # chosen on the CPU: see test_parity_iteration_by_iteration
PIN = 2.0 ** 36                                                             # a prior weight that pins the twist (zero-motion tests)


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.0, nn_k=0, nn_r=0.25, slam_ct=True)
    base.update(kw)
    return Config(**base)


def _np(x):
    return x.detach().cpu().numpy()


def _t(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _totals_bound(n_pairs, abs_totals):
    return (n_pairs + 16) * 2.0 ** -53 * abs_totals


# ---- 1. dc_icp_ct_accumulate on hand-written tables --------------------------------------------------------------------------------
def _case(m, knn, seed, n_map=5000, cos_min=math.cos(1.2)):
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    mp, mn = rng.uniform(-5, 5, size=(n_map, 3)), unit(rng.normal(size=(n_map, 3)))
    p, pn = rng.uniform(-5, 5, size=(m, 3)), unit(rng.normal(size=(m, 3)))
    tau = rng.uniform(-0.2, 1.0, size=m)
    tau[::7] = 0.0
    twist = np.array([0.25, 0.05, -0.1, 0.02, -0.03, 0.08])
    idx = rng.integers(0, n_map, size=(m, knn)).astype(np.int32)
    idx[rng.random((m, knn)) < (0.1 if m * knn < 100000 else 0.9)] = -1          # (keeps the reference's pair list small at 131 073)
    dist = rng.uniform(0.0, 1.0, size=(m, knn))
    dist[idx < 0] = np.inf
    T = slam_pose(0.4, (0.3, -0.2, 0.1), 0.1, -0.05)
    return dict(mp=mp, mn=mn, p=p, pn=pn, tau=tau, twist=twist, idx=idx, dist=dist, thr=0.8, T=T, cos_min=cos_min)


def _deskew_on_device(c):
    from depth_correction_amd import ops
    m = len(c['p'])
    q, nq = torch.empty((m, 3), dtype=torch.float64, device=DEV), torch.empty((m, 3), dtype=torch.float64, device=DEV)
    ops.deskew_device_twist(_t(c['p']), _t(c['pn']), _t(c['tau']), _t(c['twist']), torch.tensor([0, m], dtype=torch.int64, device=DEV), q, nq)
    return q, nq


def _run(c, q, nq, thr=None, want_kept=True, status_code=0, fill=None):
    from depth_correction_amd import _native as nv, ops
    m, knn = c['idx'].shape
    state = _t(R.state_vector(R.new_state(c['T'])))
    ct = torch.zeros((nv.DC_ICP_CT_STATE_COUNT,), dtype=torch.float64, device=DEV)
    ct[:6] = _t(c['twist'])
    status = torch.tensor([status_code, 0, 0, 0], dtype=torch.int32, device=DEV)
    nb = ops.icp_blocks(m)
    partials = torch.full((nb, nv.DC_ICP_CT_PARTIALS), float('nan') if fill is None else fill, dtype=torch.float64, device=DEV)
    kept = torch.full((m, knn), 7, dtype=torch.uint8, device=DEV) if want_kept else None
    ops.icp_ct_accumulate(_t(c['p']), q, nq, _t(c['tau']), _t(c['mp']), _t(c['mn']), _t(c['idx'], torch.int32), _t(c['dist']),
                          _t(np.array([c['thr'] if thr is None else thr])), c['cos_min'], state, ct, status, partials, kept=kept)
    torch.cuda.synchronize()
    return _np(partials), (_np(kept) if want_kept else None)


def _reference(c, q, nq, thr=None):
    return C.totals(c['mp'], c['mn'], c['p'], c['pn'], c['tau'], c['T'], c['twist'], c['idx'], c['dist'], c['thr'] if thr is None else thr,
                    c['cos_min'], q=_np(q), nq=_np(nq))


@pytest.mark.parametrize('knn', [1, 3])
@pytest.mark.parametrize('m', [1, 255, 256, 257, 131073])
def test_ct_accumulate_matches_reference(m, knn):
    """m = 131 073 = 512 x 256 + 1 is the first size at which the grid-stride loop takes a second trip (tests/test_gpu_slam_parity.py).
    The de-skewed points and normals are the device's own (dc_deskew, held to numpy in tests/test_gpu_sweep.py); the threshold is
    exactly the distance of a pair that passes the normal gate."""
    from depth_correction_amd import ops
    assert ops.icp_blocks(131072) == 512 and ops.icp_blocks(257) == 2
    c = _case(m, knn, seed=2000 * knn + m % 991)
    q, nq = _deskew_on_device(c)
    q_ref, nq_ref, _ = C.deskew(c['p'], c['pn'], c['tau'], c['twist'])
    assert np.abs(_np(q) - q_ref).max() <= 34 * 2.0 ** -52 * 10.0 and np.abs(_np(nq) - nq_ref).max() <= 34 * 2.0 ** -52
    nr = _np(nq) @ c['T'][:3, :3].T
    flat = np.flatnonzero((c['dist'].reshape(-1) <= c['thr']))
    for e in flat[np.argsort(-c['dist'].reshape(-1)[flat])][:64]:
        i, j = divmod(int(e), knn)
        if abs(nr[i] @ c['mn'][c['idx'][i, j]]) >= c['cos_min'] + 1e-6:
            c['thr'] = float(c['dist'][i, j])
            break
    ref = _reference(c, q, nq)
    assert ref['normal_margin'] >= MARGIN_FLOOR
    part, kept = _run(c, q, nq)
    part2, none = _run(c, q, nq, want_kept=False)
    assert part.tobytes() == part2.tobytes() and none is None                  # two runs: bit-identical
    assert np.array_equal(kept.astype(bool), ref['kept']) and set(np.unique(kept)) <= {0, 1}
    tot = C.block_sum(part)
    bound = _totals_bound(ref['n_pairs'], ref['abs_totals'])
    err = np.abs(tot - ref['totals'])
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    print('m %d knn %d: %d pairs, largest error / bound %.3g' % (m, knn, ref['n_pairs'], ratio))
    assert (err <= bound).all(), (np.flatnonzero(err > bound), ratio)
    assert tot[90] == ref['n_pairs'] and tot[92] == ref['kept'].any(axis=1).sum()
    if m * knn >= 64:
        at = (c['dist'] == c['thr']) & (c['idx'] >= 0)
        assert ref['n_pairs'] > 0 and at.sum() == 1 and ref['kept'][at].all()   # the pair whose distance equals the threshold is kept


def test_ct_accumulate_edges():
    c = _case(1000, 3, seed=5)
    q, nq = _deskew_on_device(c)
    for name, t in (('all rejected', -1.0), ('nan threshold', float('nan'))):
        part, kept = _run(c, q, nq, thr=t)
        assert (part == 0.0).all() and (kept == 0).all(), name
    part, kept = _run(c, q, nq, thr=float('inf'))
    ref = _reference(c, q, nq, thr=float('inf'))
    assert np.array_equal(kept.astype(bool), ref['kept']) and C.block_sum(part)[90] == ref['n_pairs'] > 0.5 * (c['idx'] >= 0).sum()
    none = dict(c, idx=np.full_like(c['idx'], -1))
    part, kept = _run(none, q, nq, thr=float('inf'))
    assert (part == 0.0).all() and (kept == 0).all()
    # cos_min exactly equal to a dot product of axis vectors (w = 0, identity pose: every product exact): kept (>=), rejected one ulp above
    for cm, keeps in ((0.6, True), (float(np.nextafter(0.6, 1.0)), False)):
        e = dict(c, mn=np.tile([0.6, 0.8, 0.0], (len(c['mp']), 1)), pn=np.tile([1.0, 0.0, 0.0], (len(c['p']), 1)), T=np.eye(4),
                 twist=np.array([0.1, 0.2, 0.3, 0.0, 0.0, 0.0]), cos_min=cm)
        qe, nqe = _deskew_on_device(e)
        part, kept = _run(e, qe, nqe)
        want = (e['idx'] >= 0) & (e['dist'] <= e['thr']) & keeps
        assert np.array_equal(kept.astype(bool), want) and C.block_sum(part)[90] == want.sum()
    # a status word that is set: partials and kept flags keep their bytes
    part, kept = _run(c, q, nq, status_code=1, fill=3.25)
    assert (part == 3.25).all() and (kept == 7).all()


# ---- 1b. dc_icp_ct_finish as a state machine on the device -------------------------------------------------------------------------
def _dev_ct_finish(partials, m, prm, state, ct, status):
    from depth_correction_amd import ops
    ops.icp_ct_finish(partials, m, state, ct, status, prm.icp_min_diff_rot, prm.icp_min_diff_trans, int(prm.icp_smooth_length),
                      int(prm.icp_max_iters), prm.icp_max_rotation, prm.icp_max_translation, prm.slam_ct_prior[0], prm.slam_ct_prior[1],
                      prm.slam_ct_max_twist[0], prm.slam_ct_max_twist[1], min_pairs=int(prm.min_pairs))
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', C.finish_cases(), ids=lambda c: c[0])
def test_ct_finish_scripted_registrations_on_device(host, case):
    """The table of tests/test_slam_ct_host.py through ops.icp_ct_finish with hand-made [1, 93] partials, what
    tests/test_gpu_slam_parity.py does for the 6-unknown finish.  Against the numpy restatement: status, iterations, pairs / SSE /
    overlap, history and prior twist bit-equal, pose and twist 1e-14.  Against the host build of the same header, which takes every
    step from the state the device took it from: the same words equal, pose and twist within 4 ulp (libm against the device's sin /
    cos / sqrt), the ulp being that of the entry's terms: sum_k |D_rk| |T_kc| for the pose update D T, |twist| + |step| for the
    twist.  A failure leaves pose and twist byte for byte; a launch after the end changes nothing."""
    name, over, steps, expect = case
    prm = C.script_params(over)
    ref = C.new_state(R.SCRIPT_PRIOR, C.SCRIPT_TWIST)
    state, ct = (_t(a) for a in C.state_vectors(ref))
    status = torch.zeros((4,), dtype=torch.int32, device=DEV)
    codes = []
    for step in steps:
        if codes and codes[-1] != 0:
            break
        tot, m = C.script_totals(step)
        before, ct_before = _np(state).copy(), _np(ct).copy()
        h_state, h_ct, h_status = before.copy(), ct_before.copy(), _np(status).copy()
        _dev_ct_finish(_t(tot.reshape(1, C.N_TOT)), m, prm, state, ct, status)
        host_ct_finish(host, tot, m, prm, h_state, h_ct, h_status)
        x_step, _ = C.finish(tot, m, prm, ref)
        got, got_ct, word = _np(state), _np(ct), _np(status)
        want, want_ct = C.state_vectors(ref)
        codes.append(int(word[0]))
        assert word[0] == ref.code == h_status[0] and word[1] == ref.iters == h_status[1] == len(codes), (name, codes)
        assert got[16:].tobytes() == want[16:].tobytes() == h_state[16:].tobytes(), (name, len(codes), got[32:51], want[32:51])
        assert got_ct[6:].tobytes() == want_ct[6:].tobytes() == h_ct[6:].tobytes(), (name, len(codes))
        assert np.abs(got[:16] - want[:16]).max() <= 1e-14 and np.abs(got_ct[:6] - want_ct[:6]).max() <= 1e-14, (name, len(codes))
        if word[0] < 0:                                    # a failure: the estimate it was given, byte for byte
            assert got[:16].tobytes() == before[:16].tobytes() == h_state[:16].tobytes(), name
            assert got_ct.tobytes() == ct_before.tobytes() == h_ct.tobytes(), name
        else:
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = R.rotation(x_step[:3]), x_step[3:6]
            terms = (np.abs(D) @ np.abs(before[:16].reshape(4, 4))).reshape(-1)
            unit = np.spacing(np.maximum(terms, np.abs(h_state[:16])))
            big = np.abs(h_state[:16]) >= 0.5
            assert (unit[big] <= 2 * np.spacing(np.abs(h_state[:16]))[big]).all()        # no cancellation there: the entry's own ulp
            assert (np.abs(got[:16] - h_state[:16]) <= 4 * unit).all(), (name, got[:16] - h_state[:16])
            unit_tw = np.spacing(np.maximum(np.abs(ct_before[:6]) + np.abs(x_step[6:]), np.abs(h_ct[:6])))
            assert (np.abs(got_ct[:6] - h_ct[:6]) <= 4 * unit_tw).all(), (name, got_ct[:6] - h_ct[:6])
            assert got[:16].tobytes() != before[:16].tobytes() or got_ct[:6].tobytes() != ct_before[:6].tobytes(), name
    assert codes == expect, (name, codes)
    frozen = (_np(state).tobytes(), _np(ct).tobytes(), _np(status).tobytes())
    _dev_ct_finish(_t(C.script_totals(steps[0])[0].reshape(1, C.N_TOT)), 50, prm, state, ct, status)
    assert (_np(state).tobytes(), _np(ct).tobytes(), _np(status).tobytes()) == frozen, name


# ---- 2. the pillared room -------------------------------------------------------------------------------------------------------------
class _Room(object):
    """Three poses of the constant-twist arc through the pillared room of tests/test_gpu_sweep.py (16 x 256 rays), rendered static and
    swept, prepared once; the first pose stands off the room's planes of symmetry (z = 0.2, a little roll and pitch): from z = 0 the
    floor and the ceiling give pairs of equal distances, and the trimmed threshold falls between two of them."""

    def __init__(self, tmp):
        from depth_correction_amd.dataset import RenderedMeshDataset
        from depth_correction_amd.mesh import room_mesh
        from depth_correction_amd.render import SweepModel
        from depth_correction_amd.slam import IcpMapper, mapper_input
        path = str(tmp / 'pillared_room.ply')
        room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))]).save_ply(path)
        self.poses = S.constant_twist_poses(slam_pose(0.1, (-1.5, -0.3, 0.2), 0.02, -0.015), TWIST, 3)
        self.kw = dict(poses=self.poses, size=(16, 256), fov=(45.0, 360.0), num_segments=16, device=DEV)
        self.moving = RenderedMeshDataset(path, sweep=SweepModel(), **self.kw)
        self.static = RenderedMeshDataset(path, **self.kw)
        self.cfg = _cfg()
        mapper = IcpMapper(self.cfg)
        self.map_scan = mapper.prepare(mapper_input(self.static[0][0], None, self.cfg))
        self.static_scan = mapper.prepare(mapper_input(self.static[1][0], None, self.cfg))
        self.swept_scan = mapper.prepare(mapper_input(self.moving[1][0], None, self.cfg))

    def mapper(self, **kw):
        from depth_correction_amd.slam import IcpMapper
        mapper = IcpMapper(_cfg(**kw))
        assert mapper.update(self.map_scan, self.poses[0]) == len(self.map_scan)
        return mapper


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    return _Room(tmp_path_factory.mktemp('slam_ct'))


def _buffers(mapper, scan):
    from depth_correction_amd import ops
    m, k = len(scan), mapper.knn
    mapper._ensure_grid(m)
    return dict(idx=torch.empty((m, k), dtype=torch.int32, device=DEV), dist=torch.empty((m, k), dtype=torch.float64, device=DEV),
                thr=torch.full((1,), -7.0, dtype=torch.float64, device=DEV), kept=torch.empty((m, k), dtype=torch.uint8, device=DEV),
                ct=mapper.ct_buffers(m), partials6=torch.empty((ops.icp_blocks(m), 30), dtype=torch.float64, device=DEV))


def _start_ct(mapper, buf, prior, twist0):
    from depth_correction_amd import ops
    ops.icp_init(_t(prior), mapper.state, mapper.status)
    ops.icp_ct_init(_t(twist0), buf['ct']['ct'])


def _iterate_ct(mapper, scan, buf, cos_min):
    map_pts, map_nrm = mapper.map_points()
    mapper.iteration_ct(scan, mapper.state[:16].view(4, 4), buf['idx'], buf['dist'], buf['thr'], buf['ct'], map_pts, map_nrm, cos_min,
                        mapper.ct_params(), kept=buf['kept'])
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', ['all_tau_zero', 'static_scan'])
def test_zero_motion_is_the_six_dof_path(room, case):
    """No motion to find: every tau = 0, or a static scan with its real sweep times, with a zero prior twist held by a prior weight of
    2^36 per pair (the largest that keeps the pose block's pivots above 1e-12 of the largest diagonal entry by two decades).  The pose
    after every iteration is the 6-dof path's and the twist stays zero, both within the per-iteration bar."""
    from depth_correction_amd import ops
    from depth_correction_amd.slam import MapperScan
    scan = room.static_scan
    t = torch.zeros((len(scan),), dtype=torch.float64, device=DEV) if case == 'all_tau_zero' else None
    if t is None:
        from depth_correction_amd.sweep import sweep_times
        pts = _np(scan.points)
        t = _t(sweep_times(pts / np.linalg.norm(pts, axis=1, keepdims=True), (45.0, 360.0)))
    scan = MapperScan(scan.points, scan.normals, scan.depth, t)
    six, ct = room.mapper(slam_ct=False), room.mapper(slam_ct_prior=[PIN, PIN])
    prior = room.poses[1] @ OFFSET
    b6, bc = _buffers(six, scan), _buffers(ct, scan)
    cos_min = math.cos(six.cfg.icp_max_normal_angle)
    ops.icp_init(_t(prior), six.state, six.status)
    _start_ct(ct, bc, prior, np.zeros(6))
    map_pts, map_nrm = six.map_points()
    worst = 0.0
    for it in range(1, 40):
        six.iteration(scan, six.state[:16].view(4, 4), b6['idx'], b6['dist'], b6['thr'], b6['partials6'], map_pts, map_nrm, cos_min)
        _iterate_ct(ct, scan, bc, cos_min)
        s6, sc, tw = _np(six.state), _np(ct.state), _np(bc['ct']['ct'])[:6]
        d = max(float(np.abs(s6[:16] - sc[:16]).max()), float(np.abs(tw).max()))
        worst = max(worst, d)
        assert d <= CT_BAR, (case, it, d)
        assert np.array_equal(_np(b6['idx']), _np(bc['idx'])) and _np(six.status).tolist() == _np(ct.status).tolist(), (case, it)
        if int(six.status[0]) != 0:
            break
    print('%s: %d iterations, status %d, largest pose / twist difference %.3g (bar %.3g)' % (case, it, int(six.status[0]), worst, CT_BAR))
    assert int(six.status[0]) == R.CONVERGED


def test_parity_iteration_by_iteration(room):
    """A whole sweep-aware registration of the swept scan of pose 1 against the static scan of pose 0, the prior off by 0.03 rad / 0.1 m
    and by the whole twist (v0 = w0 = 0).  beta = 0.001 and a normal gate of 0.3 rad were chosen on the CPU (host-cast scans of the
    same room): there the reference converges in 4 iterations to a twist 0.0087 from the true one (a tenth of its norm is 0.027) with
    margins of 1e-5 and more; with the default gate of 1.57 rad the sparse 16-ring map pulls v_z to -0.05 whatever beta is, and with
    beta = 0.01 against a zero prior the twist keeps a bias of 0.056.  The reference's own sensitivity to the order of its sums on
    that scene is 3.61e-16 (the largest over 200 random orders, tests/test_slam_ct_host.py), the bar 2 000 x that, 7.2e-13."""
    mapper = room.mapper(**PARITY)
    scan = room.swept_scan
    prm = C.params(mapper.cfg)
    assert prm.slam_ct_prior == (0.001, 0.001) and prm.icp_max_normal_angle == 0.3
    p, pn, tau = _np(scan.points), _np(scan.normals), _np(scan.t)
    mp, mn = (_np(a) for a in mapper.map_points())
    prior = room.poses[1] @ OFFSET
    buf = _buffers(mapper, scan)
    _start_ct(mapper, buf, prior, np.zeros(6))
    st, tree = C.new_state(prior, np.zeros(6)), cKDTree(mp)
    cos_min = math.cos(mapper.cfg.icp_max_normal_angle)
    worst, recs = 0.0, []
    while True:
        _iterate_ct(mapper, scan, buf, cos_min)
        rec = C.iteration(mp, mn, p, pn, tau, st, prm, tree)
        recs.append(rec)
        it = len(recs)
        state, status, ct = _np(mapper.state), _np(mapper.status), _np(buf['ct']['ct'])
        d_idx, d_dist, d_kept = _np(buf['idx']), _np(buf['dist']), _np(buf['kept']).astype(bool)
        assert rec.margins['thr'] >= MARGIN_FLOOR and rec.margins['normal'] >= MARGIN_FLOOR, (it, rec.margins)
        assert rec.margins.get('conv_rot', 1.0) >= MARGIN_FLOOR and rec.margins.get('conv_trans', 1.0) >= MARGIN_FLOOR, (it, rec.margins)
        assert np.array_equal(d_idx, rec.idx), it
        assert np.array_equal(np.isinf(d_dist), np.isinf(rec.dist)), it
        assert np.array_equal(d_kept, rec.kept), (it, int((d_kept != rec.kept).sum()))
        assert state[48] == rec.pairs and state[50] == rec.overlap
        assert status[1] == rec.iters == it and status[0] == rec.code, (it, status, rec.code)
        d = max(float(np.abs(state[:16].reshape(4, 4) - rec.pose).max()), float(np.abs(ct[:6] - rec.twist).max()))
        worst = max(worst, d)
        print('iteration %d: pairs %d, pose / twist deviation %.3g, margins thr %.2g normal %.2g' % (it, rec.pairs, d, rec.margins['thr'],
                                                                                                    rec.margins['normal']))
        assert d <= CT_BAR, (it, d, CT_BAR)
        assert np.array_equal(ct[6:12], np.zeros(6)) and np.array_equal(state[16:32].reshape(4, 4), prior)
        if status[0] != 0:
            break
        assert it < 60
    print('parity: %d iterations, largest deviation %.3g (bar %.3g); twist %s' % (len(recs), worst, CT_BAR, recs[-1].twist))
    assert status[0] == R.CONVERGED
    assert np.linalg.norm(recs[-1].twist - TWIST) <= 0.1 * np.linalg.norm(TWIST)


def test_register_returns_twist_and_deskewed_scan(room):
    """IcpMapper.register through its public path: the pose at sweep time 0, info['twist'], the launch count of this path, and the
    scan handed on to the map de-skewed by the estimated twist (dc_deskew of the reading by info['twist'], bit for bit)."""
    from depth_correction_amd import ops
    from depth_correction_amd.slam import LAUNCHES_PER_ITERATION, LAUNCHES_PER_ITERATION_CT
    mapper = room.mapper(**PARITY)
    scan = room.swept_scan
    pose, info = mapper.register(scan, room.poses[1] @ OFFSET)
    assert info['ok'] and info['status'] == 'converged' and info['launches_per_iteration'] == LAUNCHES_PER_ITERATION_CT == 24
    assert np.linalg.norm(info['twist'] - TWIST) <= 0.1 * np.linalg.norm(TWIST)
    d = np.linalg.solve(pose, room.poses[1])
    assert np.linalg.norm(d[:3, 3]) < 0.02 and R.rotation_angle(d) < 0.01
    flat = info['deskewed']
    x, _, nx = ops.deskew(scan.points, scan.t, [0, len(scan)], info['twist'][None], normals=scan.normals)
    assert torch.equal(flat.points, x) and torch.equal(flat.normals, nx) and flat.depth is scan.depth
    raw_pose, raw_info = room.mapper(slam_ct=False).register(scan, room.poses[1] @ OFFSET)
    assert raw_info['launches_per_iteration'] == LAUNCHES_PER_ITERATION and 'twist' not in raw_info
    # a scan without sweep times takes the 6-dof path whatever cfg.slam_ct says
    _, info6 = mapper.register(room.static_scan, room.poses[1] @ OFFSET)
    assert info6['launches_per_iteration'] == LAUNCHES_PER_ITERATION and 'twist' not in info6


# ---- 3. the sweep times follow their points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_model', [False, True])
def test_times_follow_their_points(room, with_model):
    """After mapper_input (depth filter, grid filter, and with a model the correction with its shadow filter) and prepare, scan.t[i] is
    sweep_times of the direction of the raw point i to the rounding of that function.  Everything is float64 here (the rendered
    cloud's fields, the configuration): the direction recomputed from the point is off by a rounding per component, atan2 by one
    of an angle up to pi, the shift and the mod by one each of an angle up to 2 pi -- below 1.3e-15 rad together, 2e-16 of the sweep
    -- and the division rounds once more.  The bar is 4 x 2^-52 = 8.9e-16 (measured 2.2e-16).  With a model this is the check; without
    one the times are also bit-equal to the raw cloud's field.  A configuration without slam_ct does not carry the times."""
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.slam import IcpMapper, mapper_input
    from depth_correction_amd.sweep import sweep_times
    cloud = room.moving[1][0]
    kw = dict(grid_res=0.1, min_depth=1.0)
    if with_model:
        kw.update(shadow_angle_bounds=[0.2, 2.9], shadow_neighborhood_angle=0.06, nn_r=0.4)
    cfg = _cfg(**kw)
    model = ScaledPolynomial(w=[-0.002], exponent=[2.0], device=DEV) if with_model else None
    assert cloud['x'].dtype == np.float64 and cloud['t'].dtype == np.float64
    scan = IcpMapper(cfg).prepare(mapper_input(cloud, model, cfg))
    assert scan.t is not None and scan.t.dtype == torch.float64 and 0.3 * len(cloud) < len(scan) < len(cloud)
    plain = _cfg(slam_ct=False, **kw)
    assert IcpMapper(plain).prepare(mapper_input(cloud, model, plain)).t is None
    raw = np.stack([cloud[f] for f in 'xyz'], axis=1).astype(np.float64)
    if with_model:
        # the correction changes depths, not directions: the direction of the corrected point is the raw point's
        pts = _np(scan.points)
    else:
        pts = _np(scan.points)
        rows = cKDTree(raw).query(pts)[1]
        assert np.abs(raw[rows] - pts).max() <= 1e-6 and np.array_equal(_np(scan.t), cloud['t'][rows].astype(np.float64))
    want = sweep_times(pts / np.linalg.norm(pts, axis=1, keepdims=True), (45.0, 360.0))
    d = np.abs(_np(scan.t) - want)
    d = np.minimum(d, 1.0 - d)
    print('times follow their points (%s): %d of %d rows, largest difference %.3g' % ('model' if with_model else 'filters', len(scan),
                                                                                       len(cloud), d.max()))
    assert d.max() <= 4 * 2.0 ** -52


def test_clear_empties_the_map(room):
    mapper = room.mapper()
    builds = mapper.grid_builds
    assert mapper.n_map == len(room.map_scan) and builds >= 1
    mapper.clear()
    assert mapper.n_map == 0 and mapper.map_points()[0].shape[0] == 0 and mapper.grid is None
    pose, info = mapper.register(room.static_scan, room.poses[1])
    assert info['status'] == 'init' and np.array_equal(pose, room.poses[1])
    assert mapper.update(room.map_scan, room.poses[0]) == len(room.map_scan) and mapper.grid_builds == builds + 1
    pose, info = mapper.register(room.static_scan, room.poses[1] @ OFFSET)
    assert info['ok'] and np.linalg.norm(np.linalg.solve(pose, room.poses[1])[:3, 3]) < 0.02


# ---- 4. run_slam -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('odometry', ['exact', 'noisy'])
def test_run_slam_three_ways(tmp_path, odometry):
    """The six-pose arc of test_slam_deskew, raw / de-skewed by the odometry's twist (slam_deskew) / sweep-aware (slam_ct), with exact
    odometry and with the noise of tests/test_gpu_slam.py (variances 1e-4 rad^2 and 2.5e-3 m^2 per step).  Every registration is ok;
    under noisy odometry slam_ct is no worse than slam_deskew; slam_ct at least halves the raw run's mean translation error.

    Measured on the MI355X (mean translation error, raw / slam_deskew / slam_ct with the default prior 1e-4; all 36 registrations
    converged): exact odometry 13.0 / 1.8 / 4.0 mm; noisy odometry 13.1 / 49.9 / 5.1 mm.  Before run_slam de-skewed the first scan
    again by the twist of the registered first step (the first assertion inside the loop), the noisy run gave 11.6 mm, above half
    the raw run's 13.1, at every prior weight (9.6 mm at best): the first scan, which cannot be registered, entered the map bent by
    the odometry's error (0.041 in the twist; 0.007 after the redo), and with the true twist for that scan alone the run gave 4.5 mm.
    """
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import RenderedMeshDataset
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import SweepModel
    from depth_correction_amd.slam import run_slam, slam_errors
    path = str(tmp_path / 'pillared_room.ply')
    room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))]).save_ply(path)
    poses = S.constant_twist_poses(slam_pose(0.0, (-1.5, -0.3, 0.0)), TWIST, 6)
    moving = RenderedMeshDataset(path, sweep=SweepModel(), poses=poses, size=(16, 256), fov=(45.0, 360.0), num_segments=16, device=DEV)
    cov = [0.0] * 6 if odometry == 'exact' else [1e-4] * 3 + [2.5e-3] * 3
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25, odom_cov=cov)
    errs = {}
    for name, kw in (('raw', dict()), ('slam_deskew', dict(slam_deskew=True)), ('slam_ct', dict(slam_ct=True))):
        res = run_slam(moving, None, Config(**base, **kw))
        errs[name] = slam_errors(res['slam'], res['gt'], res['path_lengths'])[1]
        print('%s odometry, %s: mean translation error %.3g m, status %s' % (odometry, name, errs[name], [i['status'] for i in res['info']]))
        assert all(i['ok'] for i in res['info']), (name, [i['status'] for i in res['info']])
        if name == 'slam_ct':
            print('   twists: %s' % [np.round(i['twist'], 3).tolist() for i in res['info'] if 'twist' in i])
            # the first scan was de-skewed again by the twist of the registered first step: nearer the truth than the odometry's
            from depth_correction_amd.sweep import motion_twist
            odo = motion_twist(np.linalg.solve(res['odom'][0], res['odom'][1]))
            first = np.linalg.norm(res['info'][0]['twist'] - TWIST)
            print('   first scan: twist off by %.3g (the odometry\'s first step by %.3g)' % (first, np.linalg.norm(odo - TWIST)))
            assert first < 0.02 and (odometry == 'exact' or first < 0.5 * np.linalg.norm(odo - TWIST))
    if odometry == 'noisy':
        assert errs['slam_ct'] <= errs['slam_deskew'], errs
    assert errs['slam_ct'] < 0.5 * errs['raw'], errs
