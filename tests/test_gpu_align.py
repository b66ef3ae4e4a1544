"""Survey registration on the MI355X (csrc/dc_align.hip, ops.align_* / survey_align, registration.register_cloud, SurveyCloud.register /
transformed, eval_map with map_eval_register, eval_slam's aligned path) against tests/align_reference.py.

Bars (align_reference): bar_pt = 2^-40 x extent for a point; bar_R / bar_t = 16 x the largest disagreement of the reference's two
independent fp64 routes along its own trajectory of the scene at hand (floors 16 eps, 16 ulp of the largest coordinate), measured
and printed by the tests.  Sums are held to the worst case of any summation order: n eps sum |term|.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_reference as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STATE_COUNT, POSE, PRIOR, THRESHOLD, PAIRS, RMS = 64, 0, 16, 32, 33, 34
CONVERGED, MAX_ITERS, FAIL_PAIRS, FAIL_DEGENERATE, FAIL_NONFINITE = 1, 2, -1, -2, -3
_SURVEYS = {}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _survey(shifted=False):
    """The reference scene's survey as a SurveyCloud (one per process: the device copies and the grid are built once)."""
    from depth_correction_amd.survey import SurveyCloud
    if shifted not in _SURVEYS:
        pts, nrm = A.survey(shifted)
        _SURVEYS[shifted] = SurveyCloud(pts.copy(), nrm.copy())
    return _SURVEYS[shifted]


def _new_state(n_rows):
    return (torch.empty((STATE_COUNT,), dtype=torch.float64, device=DEV), torch.empty((4,), dtype=torch.int32, device=DEV),
            torch.empty((n_rows, 5), dtype=torch.float64, device=DEV))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _finish_one_row(m, o, T0=None, **kw):
    """ops.align_finish on the one-row partials m [17] -> (T [4,4], status [4], history [rows,5]) as numpy."""
    from depth_correction_amd import ops
    state, status, hist = _new_state(kw.get('max_iters', 1))
    ops.align_init(state, status, None if T0 is None else _t(T0), hist)
    ops.align_finish(_t(np.asarray(m).reshape(1, 17)), _t(o), state, status, history=hist, **kw)
    torch.cuda.synchronize()
    return state.cpu().numpy()[POSE:POSE + 16].reshape(4, 4), status.cpu().numpy(), hist.cpu().numpy()


# ---- 1. one step, piece by piece ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', A.STEPS)
@pytest.mark.parametrize('n', A.SIZES)
def test_step_parity(n, k):
    """From the reference's T_k of the noisy scene: the match against brute force, the threshold, the kept set, the moments, the fit
    against route A on the device's kept set, the history row; dc_survey_align with n_iters = 1 gives the same bits."""
    from depth_correction_amd import ops
    sc, tr = A.scene(n, A.SIGMA), A.trajectory(n)
    bar_R, bar_t = A.scene_bars(n)
    Tk = tr['poses'][k]
    sd = _survey().on_device(DEV)
    q, o = _t(sc['query']), A.origins(sc['query'], sc['survey'])
    nq = q.shape[0]
    sd.reserve(nq)
    dist, idx = ops.knn_grid_query(sd.grid, q, _t(Tk), 1, r=A.MAX_DIST)
    tau = ops.quantile(dist, A.RATIO)
    nb = ops.align_blocks(nq)
    assert nb == -(-nq // 256) and nb >= 2
    partials = torch.full((nb, 17), float('nan'), dtype=torch.float64, device=DEV)
    kept = torch.full((nq,), 7, dtype=torch.uint8, device=DEV)
    ops.align_accumulate(q, sd.points, idx, dist, tau, _t(o), partials, kept=kept)
    state, status, hist = _new_state(1)
    ops.align_init(state, status, _t(Tk), hist)
    state[THRESHOLD:THRESHOLD + 1].copy_(tau)
    ops.align_finish(partials, _t(o), state, status, max_iters=1, history=hist)
    torch.cuda.synchronize()
    idx_h, d_h, tau_h, kept_h = idx.cpu().numpy()[:, 0], dist.cpu().numpy()[:, 0], float(tau.item()), kept.cpu().numpy().astype(bool)
    # the match, by the rule of test_gpu_cloudloss.py
    bf_idx, bf_d2, bf_second = A.nearest(sc['survey'], A.move(Tk, sc['query']))
    clear = bf_second - bf_d2 > 1e-9 * A.EXTENT ** 2
    matched = bf_d2 < A.MAX_DIST ** 2
    assert np.array_equal(idx_h >= 0, matched)
    assert np.array_equal(idx_h[clear], np.where(matched, bf_idx, -1)[clear])
    assert np.abs(d_h[matched] - np.sqrt(bf_d2[matched])).max() <= A.BAR_PT and np.isinf(d_h[~matched]).all()
    # the threshold and the kept set
    assert tau_h == np.quantile(d_h[np.isfinite(d_h)], A.RATIO)
    assert np.array_equal(kept_h, (idx_h >= 0) & (d_h <= tau_h))
    # the moments: any summation order of W terms stays within W eps sum |term| of the exactly rounded sum
    p, y = sc['query'][kept_h], sc['survey'][idx_h[kept_h]]
    W = int(kept_h.sum())
    ref = A.moments(p, y, d_h[kept_h], o)
    pc, yc = np.abs(p - o[:3]), np.abs(y - o[3:])
    mag = np.concatenate([[W], pc.sum(axis=0), yc.sum(axis=0), (pc[:, :, None] * yc[:, None, :]).sum(axis=0).reshape(-1), [np.sum(d_h[kept_h] ** 2)]])
    rows = partials.cpu().numpy()
    lanes = [rows[l::8].sum(axis=0) if len(rows[l::8]) else np.zeros(17) for l in range(8)]
    tot = np.zeros(17)
    for lane in lanes:
        tot = tot + lane
    print('n = %d k = %d: W %d, largest |moment - fsum| / (W eps sum|term|) %.3g' % (n, k, W, (np.abs(tot - ref) / (W * A.EPS * mag)).max()))
    assert tot[0] == W and np.all(np.abs(tot - ref) <= W * A.EPS * mag)
    # the fit against route A on the device's kept set
    Ta, s, dsign = A.fit_svd(p, y)
    st = state.cpu().numpy()
    T = st[POSE:POSE + 16].reshape(4, 4)
    dR, dt = np.abs(T - Ta)[:3, :3].max(), np.abs(T - Ta)[:3, 3].max()
    print('n = %d k = %d: |R - R_A| %.3g (bar %.3g), |t - t_A| %.3g m (bar %.3g m)' % (n, k, dR, bar_R, dt, bar_t))
    assert dR <= bar_R and dt <= bar_t and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(st[PRIOR:PRIOR + 16].reshape(4, 4), Tk)
    # the history row and the status
    row = hist.cpu().numpy()[0]
    d_rot, d_trans = A.increment(Ta, Tk, o[:3])
    assert row[0] == W == st[PAIRS] and row[2] == tau_h == st[THRESHOLD]
    assert abs(row[1] - math.sqrt(ref[16] / W)) <= (0.5 * W + 4) * A.EPS * row[1] and row[1] == st[RMS]        # (E within W eps E, above)
    assert abs(row[3] - d_rot) <= 4 * bar_R and abs(row[4] - d_trans) <= 2 * bar_t + 3 * bar_R * np.abs(o[:3]).sum()
    assert list(status.cpu().numpy()[:2]) == [MAX_ITERS, 1]
    # the queued form
    state2, status2, hist2 = ops.survey_align(sd, q, _t(o), prior=_t(Tk), inlier_ratio=A.RATIO, max_dist=A.MAX_DIST, n_iters=1)
    torch.cuda.synchronize()
    assert _same(state2.cpu().numpy(), st) and _same(hist2.cpu().numpy(), hist.cpu().numpy())
    assert np.array_equal(status2.cpu().numpy(), status.cpu().numpy())


# ---- 2. the solver on the device ------------------------------------------------------------------------------------------------------
def _pair_origins(p, y):
    return np.concatenate([0.5 * (p.min(axis=0) + p.max(axis=0)), 0.5 * (y.min(axis=0) + y.max(axis=0))])


@pytest.mark.parametrize('name', sorted(A.pair_sets()))
def test_solver_on_device(name):
    p, y = A.pair_sets()[name]
    o = _pair_origins(p, y)
    m = A.moments(p, y, np.linalg.norm(y - p, axis=1), o)
    T, status, hist = _finish_one_row(m, o)
    Ta, s, d = A.fit_svd(p, y)
    bar_R, bar_t = A.scene_bars(4099, shifted=(name == 'shifted'))
    dR, dt = np.abs(T - Ta)[:3, :3].max(), np.abs(T - Ta)[:3, 3].max()
    print('%s: |R - R_A| %.3g (bar %.3g), |t - t_A| %.3g m (bar %.3g m)' % (name, dR, bar_R, dt, bar_t))
    assert d == (-1.0 if name == 'mirrored' else 1.0)
    assert list(status[:2]) == [MAX_ITERS, 1] and dR <= bar_R and dt <= bar_t
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) <= 16 * A.EPS
    assert hist[0, 0] == len(p) and np.isinf(hist[0, 2]) and np.isfinite(hist[0]).sum() == 4


def test_failure_codes_on_device():
    T0 = A.rigid(A.axis_angle((0.0, 0.0, 1.0), 0.1), (1.0, 2.0, 3.0))
    for name, (p, y) in A.degenerate_sets().items():
        o = _pair_origins(p, y)
        T, status, hist = _finish_one_row(A.moments(p, y, np.linalg.norm(y - p, axis=1), o), o, T0=T0, max_iters=3)
        assert list(status[:2]) == [FAIL_DEGENERATE, 1] and np.array_equal(T, T0), name
        assert hist[0, 0] == len(p) and np.isnan(hist[0, 3:]).all() and np.isnan(hist[1:]).all()
    p, y = A.pair_sets()['generic']
    o = _pair_origins(p, y)
    T, status, _ = _finish_one_row(A.moments(p[:2], y[:2], np.zeros(2), o), o, T0=T0)
    assert list(status[:2]) == [FAIL_PAIRS, 1] and np.array_equal(T, T0)
    T, status, _ = _finish_one_row(A.moments(p[:5], y[:5], np.zeros(5), o), o, T0=T0, min_pairs=6)
    assert status[0] == FAIL_PAIRS and np.array_equal(T, T0)
    for col in (1, 5, 9, 16):
        m = A.moments(p, y, np.zeros(len(p)), o)
        m[col] = np.nan
        T, status, _ = _finish_one_row(m, o, T0=T0)
        assert status[0] == FAIL_NONFINITE and np.array_equal(T, T0), col
    m = A.moments(p, y, np.zeros(len(p)), o)
    assert _finish_one_row(m, o, min_rot=10.0, min_trans=10.0)[1][0] == CONVERGED                  # checked before MAX_ITERS
    assert _finish_one_row(m, o, max_iters=2)[1][0] == 0


# ---- 3. whole runs --------------------------------------------------------------------------------------------------------------------
def _run(sc, shifted=False, **kw):
    from depth_correction_amd.registration import register_cloud
    args = dict(inlier_ratio=A.RATIO, max_dist=A.MAX_DIST, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    args.update(kw)
    return register_cloud(_t(sc['query']), _survey(shifted), **args)


def _fit(T, sc):
    n = sc['n_inliers']
    return np.abs(A.move(T, sc['query'][:n]) - sc['survey'][sc['inlier_idx']]).max()


@pytest.mark.parametrize('n', A.SIZES)
def test_noise_free_run_reaches_the_true_transform(n):
    sc = A.scene(n)
    reg = _run(sc)
    ref = A.icp(sc, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    print('n = %d: %r; max |T p - y| %.3g m (bar %.3g m); reference: %s after %d iterations'
          % (n, reg, _fit(reg.T, sc), A.BAR_PT, ref['status'], ref['iterations']))
    assert reg.status == 'converged' and reg.ok and reg.iterations <= 40
    assert _fit(reg.T, sc) <= A.BAR_PT
    h = reg.history
    assert h.shape == (60, 5) and np.isfinite(h[:reg.iterations]).all() and np.isnan(h[reg.iterations:]).all()
    assert h[reg.iterations - 1, 3] < 1e-9 and h[reg.iterations - 1, 4] < 1e-9
    assert reg.pairs == h[reg.iterations - 1, 0] and reg.rms == h[reg.iterations - 1, 1] and reg.threshold == h[reg.iterations - 1, 2]
    again = _run(sc, n_iters=reg.iterations)
    assert np.array_equal(again.T, reg.T) and again.iterations == reg.iterations and _same(again.history, h[:reg.iterations])
    short = _run(sc, n_iters=reg.iterations - 1)
    assert short.status == 'max_iterations' and short.ok and _same(short.history, h[:reg.iterations - 1])


def test_shifted_scene_reaches_the_true_transform():
    """The scene 2e5 m from the origin: 64 ulp of 2e5 m, which sums of raw coordinates cannot meet (their moments cancel to 1e-5)."""
    n = A.SIZES[-1]
    sc = A.scene(n, 0.0, True)
    reg = _run(sc, shifted=True)
    fit = _fit(reg.T, sc)
    print('shifted: %r; max |T p - y| %.3g m = %.1f ulp of 2e5 m' % (reg, fit, fit / np.spacing(2e5)))
    assert reg.status == 'converged' and fit <= 64 * np.spacing(2e5)


def test_two_calls_are_bit_equal_whatever_ran_between():
    sc = A.scene(A.SIZES[-1], A.SIGMA)
    first = _run(sc, n_iters=30)
    _run(A.scene(A.SIZES[0], A.SIGMA), n_iters=5)
    _run(A.scene(A.SIZES[-1], 0.0, True), shifted=True, n_iters=3)
    second = _run(sc, n_iters=30)
    assert np.array_equal(first.T, second.T) and _same(first.history, second.history) and first.status == second.status


def test_noisy_run_follows_the_reference():
    """sigma = 0.01: the device's trajectory stays with the reference's (same pair counts, thresholds within bar_pt) and ends where
    it ends, within bar_R / bar_t."""
    n = A.SIZES[-1]
    sc, tr = A.scene(n, A.SIGMA), A.trajectory(n)
    reg = _run(sc, n_iters=25, min_rot=0.0, min_trans=0.0)
    assert reg.status == 'max_iterations' and reg.iterations == 25
    for k in A.STEPS:
        assert reg.history[k, 0] == tr['history'][k, 0] and abs(reg.history[k, 2] - tr['history'][k, 2]) <= A.BAR_PT, k
    # the reference has reached its fixed point (its last increment is exactly zero): both ends are the fit of one kept set
    assert tr['history'][24, 3] == 0.0 and tr['history'][24, 4] == 0.0
    bar_R, bar_t = A.scene_bars(n)
    assert np.abs(reg.T - tr['T'])[:3, :3].max() <= bar_R and np.abs(reg.T - tr['T'])[:3, 3].max() <= bar_t


def test_small_clouds_and_gates():
    from depth_correction_amd.registration import register_cloud
    sv, sc = _survey(), A.scene(A.SIZES[0])
    Tt = sc['T_true']
    near = A.rigid(A.axis_angle((0.0, 1.0, 0.0), 1e-3), (1e-3, 0.0, -1e-3)) @ Tt
    kw = dict(max_dist=A.MAX_DIST, n_iters=10, min_rot=1e-9, min_trans=1e-9)
    empty = register_cloud(_t(np.zeros((0, 3))), sv, init=near, **kw)
    assert empty.status == 'empty' and not empty.ok and np.array_equal(empty.T, near) and empty.iterations == 0 and empty.pairs == 0
    for m in (1, 2):
        reg = register_cloud(_t(sc['query'][:m]), sv, init=near, **kw)
        assert reg.status == 'too_few_pairs' and not reg.ok and np.array_equal(reg.T, near) and reg.iterations == 1 and reg.pairs == m
        assert np.isnan(reg.history[1:]).all() and reg.history[0, 0] == m
    three = register_cloud(_t(sc['query'][:3]), sv, init=near, **kw)
    fit = np.abs(A.move(three.T, sc['query'][:3]) - sc['survey'][sc['inlier_idx'][:3]]).max()
    print('three points: %r, max |T p - y| %.3g m' % (three, fit))
    assert three.ok and three.pairs == 3 and fit <= A.BAR_PT
    # the trimming quantile of three matched distances keeps two: too few
    assert register_cloud(_t(sc['query'][:3]), sv, init=near, inlier_ratio=0.5, **kw).status == 'too_few_pairs'
    # a NaN row is never matched
    full = _run(sc)
    q = np.concatenate([sc['query'], [[np.nan, 0.0, 0.0]]])
    bar_R, bar_t = A.scene_bars(A.SIZES[0])
    withnan = register_cloud(_t(q), sv, inlier_ratio=A.RATIO, max_dist=A.MAX_DIST, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    assert withnan.status == full.status and withnan.iterations == full.iterations and withnan.pairs == full.pairs
    assert np.abs(withnan.T - full.T)[:3, :3].max() <= bar_R and np.abs(withnan.T - full.T)[:3, 3].max() <= bar_t
    # nothing within max_dist
    far = register_cloud(_t(sc['query'] + (100.0, 0.0, 0.0)), sv, inlier_ratio=A.RATIO, **kw)
    assert far.status == 'too_few_pairs' and far.pairs == 0 and far.iterations == 1 and np.array_equal(far.T, np.eye(4))
    assert math.isnan(far.threshold) and math.isnan(far.rms)
    far1 = register_cloud(_t(sc['query'] + (100.0, 0.0, 0.0)), sv, **kw)
    assert far1.status == 'too_few_pairs' and math.isinf(far1.threshold)
    # a mask: the rows outside it are compacted away
    rng = np.random.default_rng(2)
    mask = np.ones(len(q) + 50, bool)
    mask[-50:] = False
    mask[len(sc['query'])] = False
    junk = np.concatenate([q, rng.uniform(0.0, 3.0, size=(50, 3))])
    masked = register_cloud(_t(junk), sv, mask=torch.as_tensor(mask, device=DEV), inlier_ratio=A.RATIO, max_dist=A.MAX_DIST, n_iters=60,
                            min_rot=1e-9, min_trans=1e-9)
    assert np.array_equal(masked.T, full.T) and _same(masked.history, full.history)
    # the argument contract
    with pytest.raises(ValueError, match='max_dist'):
        register_cloud(_t(sc['query']), sv)
    for bad in (dict(max_dist=float('inf')), dict(max_dist=0.5, inlier_ratio=0.0), dict(max_dist=0.5, n_iters=0), dict(max_dist=0.5, min_pairs=2),
                dict(max_dist=0.5, min_rot=-1.0)):
        with pytest.raises(ValueError):
            register_cloud(_t(sc['query']), sv, **bad)


# ---- 4. the surface -------------------------------------------------------------------------------------------------------------------
def test_transformed_survey_registers_back():
    sv = _survey()
    Tm = A.rigid(A.axis_angle((0.2, -0.1, 1.0), math.radians(2.0)), (0.06, -0.04, 0.03))
    moved = sv.transformed(Tm)
    assert len(moved) == len(sv) and moved._device == {} and moved is not sv
    assert np.abs(moved.points.numpy() - (A.survey()[0] @ Tm[:3, :3].T + Tm[:3, 3])).max() <= A.BAR_PT
    assert np.abs(moved.normals.numpy() - A.survey()[1] @ Tm[:3, :3].T).max() <= 4 * A.EPS
    reg = sv.register(moved.points[::5].to(DEV), max_dist=A.MAX_DIST, n_iters=60, min_rot=1e-9, min_trans=1e-9)
    bar_R, bar_t = A.scene_bars(A.SIZES[-1])
    want = np.linalg.inv(Tm)
    dR, dt = np.abs(reg.T - want)[:3, :3].max(), np.abs(reg.T - want)[:3, 3].max()
    print('%r: |R - R_m^-1| %.3g (bar %.3g), |t| %.3g m (bar %.3g m)' % (reg, dR, bar_R, dt, bar_t))
    assert reg.status == 'converged' and dR <= bar_R and dt <= bar_t
    assert moved.on_device(DEV).grid is not sv.on_device(DEV).grid


class _HandDataset(object):
    """Two scans of a hand-made lattice room: (structured cloud in the sensor frame, pose) pairs and the survey of the map."""

    def __init__(self, clouds, poses, survey):
        self.clouds, self.poses, self.survey = clouds, poses, survey

    def __iter__(self):
        return iter(zip(self.clouds, self.poses))

    def __len__(self):
        return len(self.clouds)

    def __str__(self):
        return 'lattice_room'


def _lattice():
    """World points on a 0.25 m lattice over the floor, two walls and the faces of two unequal pillars."""
    g = lambda a, b: np.arange(a, b + 1e-9, 0.25)
    parts = [np.stack(np.meshgrid(g(0.25, 7.75), g(0.25, 5.75), [0.0], indexing='ij'), -1).reshape(-1, 3),
             np.stack(np.meshgrid(g(0.25, 7.75), [0.0], g(0.25, 2.75), indexing='ij'), -1).reshape(-1, 3),
             np.stack(np.meshgrid([0.0], g(0.25, 5.75), g(0.25, 2.75), indexing='ij'), -1).reshape(-1, 3),
             np.stack(np.meshgrid([2.0], g(1.25, 2.0), g(0.25, 2.0), indexing='ij'), -1).reshape(-1, 3),
             np.stack(np.meshgrid(g(5.0, 6.0), [4.0], g(0.25, 2.75), indexing='ij'), -1).reshape(-1, 3)]
    return np.concatenate(parts)


def test_eval_map_registers_an_offset_map(tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_map
    from depth_correction_amd.model import BaseModel
    from depth_correction_amd.slam import mapper_input
    from depth_correction_amd.survey import SurveyCloud
    world = _lattice()
    true_poses = [A.rigid(A.axis_angle((0, 0, 1), 0.3), (2.0, 3.0, 1.0)), A.rigid(A.axis_angle((0, 0, 1), -0.8), (6.0, 2.0, 1.2))]
    halves = [world[0::2], world[1::2]]
    clouds = []
    for pts, T in zip(halves, true_poses):
        local = (pts - T[:3, 3]) @ T[:3, :3]
        arr = np.zeros(len(local), dtype=[('x', 'f8'), ('y', 'f8'), ('z', 'f8')])
        arr['x'], arr['y'], arr['z'] = local.T
        clouds.append(arr)
    cfg = Config(device=DEV, float_type='float64', min_depth=0.0, max_depth=float('inf'), grid_res=0.0, nn_k=0, nn_r=0.25,
                 map_eval_csv=str(tmp_path / 'map.csv'))
    model = BaseModel()
    # the unperturbed map, formed as eval_map forms it: the survey is exactly that
    moved = []
    for arr, T in zip(clouds, true_poses):
        pts = mapper_input(arr, model, cfg).get_points().detach().to(device=DEV, dtype=torch.float64)
        Tt = torch.as_tensor(T, device=DEV)
        moved.append(pts @ Tt[:3, :3].t() + Tt[:3, 3])
    truth = torch.cat(moved)
    survey = SurveyCloud(truth.cpu(), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(truth.shape[0], 3).clone())
    offset = A.rigid(np.eye(3), (0.03, -0.02, 0.01))
    ds = _HandDataset(clouds, [offset @ T for T in true_poses], survey)
    size = float(np.linalg.norm(offset[:3, 3]))
    off = eval_map(cfg, test_datasets=[ds], model=model)[0]
    assert 'registration' not in off and off['n'] == truth.shape[0] == len(world)
    assert abs(off['mean'] - size) <= A.BAR_PT and abs(off['max'] - size) <= A.BAR_PT
    cfg_on = cfg.copy()
    cfg_on.map_eval_register = True
    on = eval_map(cfg_on, test_datasets=[ds], model=model)[0]
    reg = on['registration']
    print('offset %.6f m: mean off %.9g, on %.3g (bar %.3g); %r' % (size, off['mean'], on['mean'], A.BAR_PT, reg))
    assert reg.ok and reg.status == 'converged' and on['n'] == len(world)
    assert on['mean'] <= A.BAR_PT and on['max'] <= A.BAR_PT
    assert np.abs(reg.T - np.linalg.inv(offset)).max() <= 1e-12
    lines = open(cfg.map_eval_csv).read().splitlines()
    assert len(lines) == 2
    for line, res in zip(lines, (off, on)):
        parts = line.split(' ')
        assert len(parts) == 7 and parts[0] == 'lattice_room' and int(parts[1]) == res['n']
        assert all(len(p.split('.')[1]) == 9 for p in parts[2:6]) and parts[6] == 'nan'            # (a survey has no side: signed_mean)
        assert parts[2] == '%.9f' % res['mean']


def test_eval_slam_reports_the_aligned_path(tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import RenderedMeshDataset, euler_matrix
    from depth_correction_amd.eval import eval_slam
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.registration import align_paths
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = str(tmp_path / 'pillared_room.ply')
    mesh.save_ply(path)
    poses = []
    for i in range(8):
        T = euler_matrix(0.0, 0.0, 0.04 * i)
        T[:3, 3] = (-3.0 + 0.25 * i, 0.3 * math.sin(i / 3.0), 0.02 * math.sin(i / 2.0))
        poses.append(T)
    ds = RenderedMeshDataset(path, poses=np.stack(poses), size=(64, 512), fov=(45.0, 360.0), num_segments=16, device=DEV)
    cfg = Config(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25,
                 slam_eval_csv=str(tmp_path / 'slam.csv'), odom_cov=[1e-4] * 3 + [2.5e-3] * 3)
    res = eval_slam(cfg, test_datasets=[ds], model=None)[0]
    al = res['aligned']
    assert set(al) == {'T', 'errors', 'mean', 'rmse'} and al['T'].shape == (4, 4) and al['errors'].shape == (8,)
    want = align_paths(res['slam'], res['gt'], fix_reflection=True)
    assert np.array_equal(al['T'], want['T']) and al['rmse'] == want['rmse']
    raw = np.linalg.norm(np.stack(res['slam'])[:, :3, 3] - np.stack(res['gt'])[:, :3, 3], axis=1)
    print('SLAM path: raw rmse %.6f m, aligned rmse %.6f m' % (math.sqrt(np.mean(raw ** 2)), al['rmse']))
    assert al['rmse'] <= math.sqrt(np.mean(raw ** 2)) + 1e-12              # the identity is one of the candidates
    line = open(cfg.slam_eval_csv).read().splitlines()
    assert len(line) == 1 and len(line[0].split(' ')) == 5
