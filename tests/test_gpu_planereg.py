"""Plane registration on the MI355X (csrc/dc_planereg.hip, ops.planereg_*, registration.register_planes, register_cloud(init='planes'),
SurveyCloud.register_planes, eval_map with map_eval_register_init = 'planes') against tests/planereg_reference.py, which takes every
discrete decision with an asserted margin, and against the host build of the rules (test_planereg_host.py).

Bars.  The valid lists, hypothesis numbers, scores, block counts, kept rows, fitnesses and candidate tables are compared for
EQUALITY, and so are the bits of the kernels' transforms and the host build's.  A fitted transform is held to
planereg_reference.T_BAR = 16 x what the oracle's own two routes (SVD + LU; Horn + eigh + Cramer) differ by over every valid
hypothesis of every input used here (asserted inside the oracle).  The refined transform is held to
align_reference.bars of the oracle's own refinement from the same prior, as tests/test_gpu_globalreg.py does.  On the scenes the
device's own planes are fed to the oracle, so the plane fits' last bits do not enter the comparison of the later stages.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_reference as A  # noqa: E402
import globalreg_reference as G  # noqa: E402
import planereg_reference as P  # noqa: E402
import test_planereg_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REFINE = dict(inlier_ratio=A.RATIO, max_dist=A.MAX_DIST, n_iters=25)
PROTOTYPE = dict(plane_voxel=None)                  # planes on the unfiltered clouds; everything else is the default
CHUNK = 16384                                       # hypotheses a block owns (include/dc_hip.h)
_SURVEY = []


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _survey():
    from depth_correction_amd.survey import SurveyCloud
    if not _SURVEY:
        pts, nrm = A.survey()
        _SURVEY.append(SurveyCloud(pts.copy(), nrm.copy()))
    return _SURVEY[0]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _device_lists(cp, cs, sp, tri, h0=0, h1=None, prm=None):
    """(counts, h, T, score) as numpy arrays from planereg_count, the scan and planereg_fill; every result of a second run has the same
    bits."""
    from depth_correction_amd import ops
    prm = dict(P.PARAMS, **(prm or {}))
    args = (_t(cp), _t(cs, torch.int64), _t(sp), _t(tri, torch.int32).reshape(-1, 3), prm['min_det'], prm['tol_dot'], prm['cos_tol'],
            prm['tol_d'])
    runs = []
    for _ in range(2):
        counts = ops.planereg_count(*args, h_begin=h0, h_end=h1)
        h, T, score = ops.planereg_hypotheses(*args, h_begin=h0, h_end=h1)
        torch.cuda.synchronize()
        runs.append([v.cpu().numpy() for v in (counts, h, T, score)])
    assert all(_bits(a, b) for a, b in zip(*runs))
    return runs[0]


def _check_lists(cp, cs, sp, want, host, h0=0, h1=None, prm=None, what=''):
    counts, h, T, score = _device_lists(cp, cs, sp, want['tri'], h0, h1, prm)
    got = dict(h=h, T=T, score=score)
    worst = H.assert_equal_lists(got, want, what)
    assert h.tolist() == host['h'].tolist() and score.tolist() == host['score'].tolist()
    vs_host = float(np.abs(T - host['T']).max()) if len(h) else 0.0
    assert _bits(T, host['T'])                      # the same header, contraction off on both sides: the same bits
    # count and fill agree: every block's count is the number of listed hypotheses in its range
    h1 = want['n_enumerated'] + h0 if h1 is None else h1
    assert len(counts) == -(-(h1 - h0) // CHUNK) and counts.dtype == np.int32
    assert counts.tolist() == np.bincount((h - h0) // CHUNK, minlength=len(counts)).tolist()
    print('%s: %d valid of %d in %d blocks; |T - oracle| %.3g, |T - host build| %.3g, routes differ by %.3g, bar %.3g'
          % (what, len(h), h1 - h0, len(counts), worst, vs_host, want['routes'], P.T_BAR))
    return got


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pc,ps', sorted(H.CASES))
def test_kernels_equal_oracle_and_host_build(pc, ps):
    from depth_correction_amd import ops
    cp, cs, sp, _, want = H.random_case(pc, ps)
    host = H.host_enumerate(H.host_lib(), cp, cs, sp, want['tri'])
    assert ops.planereg_triples(_t(cp), P.MIN_DET).cpu().numpy().tolist() == want['tri'].tolist()
    got = _check_lists(cp, cs, sp, want, host, what='(%d, %d)' % (pc, ps))
    assert len(got['h']) >= 1
    # a range that starts and ends inside a block and inside an (i, j) row
    lo, hi = 5 * 8 + 3, want['n_enumerated'] - 11
    sub = _device_lists(cp, cs, sp, want['tri'], lo, hi)
    keep = (want['h'] >= lo) & (want['h'] < hi)
    assert sub[1].tolist() == want['h'][keep].tolist() and sub[3].tolist() == want['score'][keep].tolist()
    assert _bits(sub[2], got['T'][keep])


def test_kernels_past_32_bits_with_33_survey_planes():
    """Ps = 33: 16 384 is no multiple of 33 x 8, so block boundaries fall inside (i, j) rows; the range is the triple whose numbers
    straddle 2^32."""
    cp, cs, sp, tri, h0, h1, prm = H.big_case(52, 33)
    assert h0 < 1 << 32 < h1 and (h1 - h0) % CHUNK != 0 and CHUNK % (33 * 8) != 0
    want = P.hypotheses(cp, cs, sp, min_det=0.05, h_begin=h0, h_end=h1, tri=tri)
    host = H.host_enumerate(H.host_lib(), cp, cs, sp, tri, h0, h1, prm)
    got = _check_lists(cp, cs, sp, want, host, h0, h1, prm, what='(52, 33) around 2^32')
    assert (got['h'] < 1 << 32).any() and (got['h'] > 1 << 32).any()


def test_no_valid_hypothesis_and_the_argument_contract():
    from depth_correction_amd import _native as nv
    from depth_correction_amd import ops
    cp, cs, sp, _ = P.random_planes(4, 4, 1)
    sp[1, :3] = sp[0, :3]
    sp3 = np.ascontiguousarray(sp[:3])              # two of three survey planes parallel: rule 2 rejects everything
    want = P.hypotheses(cp, cs, sp3)
    counts, h, T, score = _device_lists(cp, cs, sp3, want['tri'])
    assert len(want['tri']) > 0 and not counts.any() and h.shape == (0,) and T.shape == (0, 4, 4) and score.shape == (0,)
    # an empty range launches nothing
    args = (_t(cp), _t(cs, torch.int64), _t(sp), _t(want['tri'], torch.int32), P.MIN_DET, P.TOL_DOT, P.COS_TOL, P.OFFSET_TOL)
    assert ops.planereg_count(*args, h_begin=7, h_end=7).shape == (0,)
    assert ops.planereg_hypotheses(*args, h_begin=7, h_end=7)[0].shape == (0,)
    assert ops.planereg_triples(_t(np.tile(cp[:1], (3, 1))), P.MIN_DET).shape == (0, 3)
    # the C ABI refuses what is out of range before it looks at a pointer
    lib = nv.lib()
    tol = (P.MIN_DET, P.TOL_DOT, P.COS_TOL, P.OFFSET_TOL)

    def count(pc, ps, u, h0, h1, tol=tol):
        return lib.dc_planereg_count(None, None, pc, None, ps, None, u, h0, h1, *tol, None, None)

    assert count(3, 3, 1, 0, 0) == 0
    for bad in ((2, 3, 1, 0, 8), (3, 2, 1, 0, 8), (65, 3, 1, 0, 8), (3, 65, 1, 0, 8), (3, 3, 1, 0, 27 * 8 + 1), (3, 3, 1, -1, 8), (3, 3, 1, 9, 8),
                (3, 3, -1, 0, 0), (3, 3, 41665, 0, 8)):
        assert count(*bad) == nv.DC_ERR_ARG, bad
        assert lib.dc_planereg_fill(None, None, bad[0], None, bad[1], None, *bad[2:], *tol, None, 0, None, None, None, None) == nv.DC_ERR_ARG
    for q in range(4):
        for v in (float('nan'), float('inf')) + ((-1.0,) if q != 2 else ()):
            assert count(3, 3, 1, 0, 8, tol[:q] + (v,) + tol[q + 1:]) == nv.DC_ERR_ARG
    assert count(3, 3, 1, 0, 8) == nv.DC_ERR_ARG                    # a real range and no tables
    assert lib.dc_planereg_blocks(0) == 0 and lib.dc_planereg_blocks(1) == 1 and lib.dc_planereg_blocks(CHUNK + 1) == 2
    for bad in (dict(min_det=float('nan')), dict(h_begin=-1), dict(h_end=10 ** 12)):
        with pytest.raises(ValueError):
            ops.planereg_count(*args[:4], **dict(dict(min_det=P.MIN_DET, tol_dot=P.TOL_DOT, cos_tol=P.COS_TOL, tol_d=P.OFFSET_TOL), **bad))
    with pytest.raises(ValueError):
        ops.planereg_count(args[0][:2], args[1][:2], *args[2:])


# ---- suppression --------------------------------------------------------------------------------------------------------------------
def _select_without_reading_back(*args):
    """ops.planereg_select with every synchronising call of torch turned into an error: nothing is read back, inside the loop or out."""
    from depth_correction_amd import ops
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows = ops.planereg_select(*args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return rows.cpu().numpy()


def test_suppression_equals_the_oracles_walk():
    cp, cs, sp, _, want = H.random_case(12, 14)
    _, h, T, score = _device_lists(cp, cs, sp, want['tri'])
    centre = np.array([0.3, -0.2, 0.1])
    for M in (1, 5, 64, 400):
        rows, _, _ = P.select(want['h'], want['score'], want['T'], centre, M)
        got = _select_without_reading_back(_t(score, torch.int64), _t(T), _t(centre), M, P.DEDUPE_ROT, P.DEDUPE_TRANS)
        assert got.shape == (M,) and got[:len(rows)].tolist() == rows.tolist() and (got[len(rows):] == -1).all()
    assert len(rows) < 400                          # the walk ran out of hypotheses before 400 distinct poses
    hd, sd, Td = H.designed_list()
    got = _select_without_reading_back(_t(sd, torch.int64), _t(Td), _t(np.zeros(3)), 8, P.DEDUPE_ROT, P.DEDUPE_TRANS)
    assert got.tolist() == [1, 4, 0, 6, -1, -1, -1, -1]
    assert _select_without_reading_back(_t(sd[:0], torch.int64), _t(Td[:0]), _t(np.zeros(3)), 3, 0.1, 0.1).tolist() == [-1, -1, -1]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _device_planes(sc):
    """The device's own planes of a scene's cloud and of the survey, as register_planes computes them with PROTOTYPE."""
    from depth_correction_amd.registration import cloud_planes
    cp, cs = cloud_planes(_t(sc['query']), None, P.THRESH, P.MIN_SUPPORT, P.RANSAC_ITERS, P.CLUSTER_EPS, P.MAX_PLANES, 0)
    sp, ss = _survey().planes(DEV, None, P.THRESH, P.SURVEY_MIN_SUPPORT, P.RANSAC_ITERS, P.CLUSTER_EPS, P.MAX_PLANES, 0)
    return cp.cpu().numpy(), cs.cpu().numpy(), sp.cpu().numpy(), ss.cpu().numpy()


@pytest.mark.parametrize('name', P.SCENES)
def test_end_to_end(name):
    """register_planes on a scene with the prototype's parameters: the counts, the winner, its score and fitness, the runner-up and the
    whole candidate table equal the oracle's on the device's own planes; the coarse T within the bar; the refined result equals
    align_reference.icp from the oracle's prior within that run's bars; the refined error to the truth is at most twice the oracle's."""
    from depth_correction_amd.registration import register_planes
    sc = P.scene(name)
    got = register_planes(_t(sc['query']), _survey(), refine_kwargs=REFINE, **PROTOTYPE)
    cp, cs, sp, _ = _device_planes(sc)
    want = P.coarse_from_planes(sc, cp, cs, sp)
    rp, rs = P.cloud_planes(name)
    print('%s: %r; coarse error %.4f m (oracle %.4f m), routes differ by %.3g; the restated plane fit finds %d planes, supports equal: %s'
          % (name, got, G.point_error(got.T_coarse, sc), want['error'], want['hyp']['routes'], len(rp),
             rs.tolist() == cs.tolist()))
    assert got.method == 'planes' and got.n_planes == (len(cp), len(sp)) and got.n_correspondences == 0
    assert (got.n_points, got.n_valid, got.n_triples, got.n_enumerated) == (want['n_points'], want['n_valid'], want['n_triples'],
                                                                            want['n_enumerated'])
    assert got.candidates.dtype == np.int64 and np.array_equal(got.candidates, want['candidates'])
    assert (got.hypothesis, got.score, got.fitness, got.runner_up) == (want['hypothesis'], want['score'], want['fitness'], want['runner_up'])
    assert got.status == 'ok' and got.ok
    assert np.abs(got.T_coarse - want['T']).max() <= P.T_BAR
    assert G.point_error(got.T_coarse, sc) <= A.MAX_DIST / 2
    ref = A.icp(sc, init=want['T'], ratio=REFINE['inlier_ratio'], max_dist=REFINE['max_dist'], n_iters=REFINE['n_iters'])
    bar_R, bar_t = A.bars(ref, float(np.abs(sc['survey']).max()))
    dR, dt = np.abs(got.T - ref['T'])[:3, :3].max(), np.abs(got.T - ref['T'])[:3, 3].max()
    e_got, e_ref = G.point_error(got.T, sc), G.point_error(ref['T'], sc)
    print('  refined %r: |R - ref| %.3g (bar %.3g), |t - ref| %.3g m (bar %.3g m); error to the truth %.5f m, the oracle\'s own %.5f m'
          % (got.refined, dR, bar_R, dt, bar_t, e_got, e_ref))
    assert got.refined.status == ref['status'] and got.refined.iterations == ref['iterations']
    assert dR <= bar_R and dt <= bar_t
    assert e_got <= 2.0 * e_ref


def test_sixteen_candidates_select_a_wrong_pose():
    from depth_correction_amd.registration import register_planes
    sc = P.scene('last60')
    few = register_planes(_t(sc['query']), _survey(), n_candidates=16, refine=False, **PROTOTYPE)
    cp, cs, sp, _ = _device_planes(sc)
    want = P.coarse_from_planes(sc, cp, cs, sp, M=16)
    assert np.array_equal(few.candidates, want['candidates']) and few.hypothesis == want['hypothesis']
    assert G.point_error(few.T, sc) > 1.0 and few.candidates.shape == (16, 3)


# ---- the surface --------------------------------------------------------------------------------------------------------------------
def test_register_cloud_from_the_plane_prior():
    from depth_correction_amd.registration import register_cloud, register_planes
    sc, sv = P.scene('turn75'), _survey()
    q = _t(sc['query'])
    direct = register_planes(q, sv, refine_kwargs=REFINE, **PROTOTYPE)
    reg = register_cloud(q, sv, init='planes', global_kwargs=PROTOTYPE, **REFINE)
    assert reg.coarse is not None and reg.coarse.method == 'planes' and reg.coarse.refined is None
    assert reg.coarse.hypothesis == direct.hypothesis and np.array_equal(reg.coarse.T, direct.T_coarse)
    assert np.array_equal(reg.T, direct.T) and np.array_equal(reg.history, direct.refined.history, equal_nan=True)
    via = sv.register(q, init='planes', global_kwargs=PROTOTYPE, **REFINE)
    both = sv.register_planes(q, refine_kwargs=REFINE, **PROTOTYPE)
    assert np.array_equal(via.T, reg.T) and np.array_equal(both.T, reg.T) and np.array_equal(both.candidates, direct.candidates)
    assert G.point_error(reg.T, sc) < 0.01
    # the survey's planes are computed once per device and argument set
    n_sets = len(sv._planes)
    sv.register_planes(q, refine=False, **PROTOTYPE)
    assert len(sv._planes) == n_sets and n_sets >= 1
    a, b = sv.planes(DEV, None, P.THRESH, P.SURVEY_MIN_SUPPORT, P.RANSAC_ITERS, P.CLUSTER_EPS, P.MAX_PLANES, 0)
    assert sv.planes(DEV, None, P.THRESH, P.SURVEY_MIN_SUPPORT, P.RANSAC_ITERS, P.CLUSTER_EPS, P.MAX_PLANES, 0)[0] is a
    assert a.shape == (b.shape[0], 4) and b.dtype == torch.int64
    # filtered planes (the default plane_voxel): another argument set, the same place
    filt = register_planes(q, sv, refine_kwargs=REFINE)
    print('plane_voxel 0.1: %r, coarse error %.4f m, refined %.4f m' % (filt, G.point_error(filt.T_coarse, sc), G.point_error(filt.T, sc)))
    assert len(sv._planes) == n_sets + 1 and filt.ok and G.point_error(filt.T, sc) < 0.01
    # a mask leaves rows out; the report
    half = register_planes(q, sv, mask=_t(np.arange(len(sc['query'])) % 2 == 0, torch.bool), refine=False, **PROTOTYPE)
    assert half.n_points < direct.n_points and half.status == 'ok'
    d = direct.as_dict()
    assert d['method'] == 'planes' and d['runner_up'] == direct.runner_up and d['n_planes'] == direct.n_planes and 'planes' in repr(direct)
    # the argument contract
    with pytest.raises(ValueError):
        register_cloud(q, sv, init='plane', **REFINE)
    with pytest.raises(ValueError):
        register_cloud(q, sv, init=np.eye(4), global_kwargs={}, **REFINE)
    for bad in (dict(voxel=0.0), dict(max_planes=65), dict(max_planes=2), dict(n_candidates=0), dict(eps=-1.0), dict(tol_dot=float('nan')),
                dict(min_det=-0.5)):
        with pytest.raises(ValueError):
            register_planes(q, sv, **bad)


def test_statuses():
    from depth_correction_amd.registration import register_planes
    sv = _survey()
    empty = register_planes(_t(np.zeros((0, 3))), sv)
    assert empty.status == 'empty' and not empty.ok and np.array_equal(empty.T, np.eye(4)) and empty.candidates.shape == (0, 3)
    assert empty.method == 'planes' and register_planes(_t(np.full((5, 3), np.nan)), sv).status == 'empty'
    rng = np.random.default_rng(G.SEED)
    wall = np.stack([rng.uniform(0, 4, 3000), rng.uniform(0, 4, 3000), rng.normal(0, 0.005, 3000)], axis=1)
    one = register_planes(_t(wall), sv, **PROTOTYPE)
    assert one.status == 'too_few_planes' and not one.ok and one.n_planes[0] == 1 and one.n_planes[1] >= 3 and one.n_valid == 0
    assert np.array_equal(one.T, np.eye(4)) and one.refined is None
    # three planes that are not independent (two of them parallel): no triple
    walls = np.concatenate([wall, wall + (0, 0, 2.0), wall[:, [2, 0, 1]] + (0, 0, 0)])
    par = register_planes(_t(walls), sv, **PROTOTYPE)
    assert par.n_planes[0] == 3 and par.status == 'too_few_planes'
    # a pose, but not one that the caller's bar on the fitness accepts
    sc = P.scene('part_low')
    low = register_planes(_t(sc['query']), sv, min_fitness=1.01, refine=False, **PROTOTYPE)
    assert low.status == 'low_fitness' and not low.ok and np.isfinite(low.T).all() and 1 <= low.candidates.shape[0] <= 64


class _TwoScans(object):
    """The cloud of a scene as two scans in one sensor frame, with the room's survey."""

    def __init__(self, clouds, poses, survey):
        self.clouds, self.poses, self.survey = clouds, poses, survey

    def __iter__(self):
        return iter(zip(self.clouds, self.poses))

    def __len__(self):
        return len(self.clouds)

    def __str__(self):
        return 'moved_room'


def test_eval_map_registers_a_map_by_its_planes(tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_map
    from depth_correction_amd.model import BaseModel
    sc = P.scene('turn140')
    pts = sc['query']
    clouds = []
    for part in (pts[:len(pts) // 2], pts[len(pts) // 2:]):
        arr = np.zeros(len(part), dtype=[('x', 'f8'), ('y', 'f8'), ('z', 'f8')])
        arr['x'], arr['y'], arr['z'] = part.T
        clouds.append(arr)
    ds = _TwoScans(clouds, [np.eye(4), np.eye(4)], _survey())
    cfg = Config(device=DEV, float_type='float64', min_depth=0.0, max_depth=float('inf'), grid_res=0.0, nn_k=0, nn_r=0.25,
                 map_eval_csv=str(tmp_path / 'map.csv'))
    assert cfg.map_eval_register_init is None and cfg.register_planes_kwargs == {} and cfg.register_global_kwargs == {}
    cfg.map_eval_register = True
    cfg.register_kwargs = dict(REFINE)
    model = BaseModel()
    plain = eval_map(cfg, test_datasets=[ds], model=model)[0]
    assert 'registration_coarse' not in plain and G.point_error(plain['registration'].T, sc) > 1.0
    cfg_p = cfg.copy()
    cfg_p.map_eval_register_init = 'planes'
    cfg_p.register_planes_kwargs = dict(PROTOTYPE)
    on = eval_map(cfg_p, test_datasets=[ds], model=model)[0]
    coarse, reg = on['registration_coarse'], on['registration']
    print('without the prior: mean %.4f m; with it: %r, %r, mean %.5f m' % (plain['mean'], coarse, reg, on['mean']))
    assert reg.coarse is coarse and coarse.method == 'planes' and coarse.ok and reg.ok
    assert G.point_error(reg.T, sc) < 0.02 and on['mean'] < 0.1 and plain['mean'] > 2.0 * on['mean']
    cfg_bad = cfg.copy()
    cfg_bad.map_eval_register_init = 'plane'
    with pytest.raises(ValueError):
        eval_map(cfg_bad, test_datasets=[ds], model=model)


def test_descriptor_registration_is_unchanged():
    """register_global and register_cloud(init='global') on one placement: the oracle's candidate table and winner as before (2^16
    hypotheses, a prefix of the enumeration the existing tests use), the report and the printed form without the new fields."""
    from depth_correction_amd.registration import register_cloud, register_global
    name, K = 'turn75', 1 << 16
    sc, sv = G.placement(name), _survey()
    want = G.coarse(name, K)
    q, gk = _t(sc['query']), dict(normals=_t(sc['query_normals']), n_hypotheses=K)
    got = register_global(q, sv, seed=G.SEED, refine=False, **gk)
    assert np.array_equal(got.candidates, want['candidates']) and got.hypothesis == want['hypothesis']
    assert (got.n_points, got.n_correspondences, got.n_valid) == (want['n_points'], want['n_correspondences'], want['n_valid'])
    assert got.method == 'descriptors' and got.runner_up is None and got.n_planes is None
    assert sorted(got.as_dict()) == sorted(['T', 'T_coarse', 'status', 'ok', 'hypothesis', 'score', 'fitness', 'n_points',
                                            'n_correspondences', 'n_valid', 'candidates'])
    assert repr(got) == 'GlobalRegistration(%s, hypothesis %d, score %d of %d matches, fitness %d of %d points)' % (
        got.status, got.hypothesis, got.score, got.n_correspondences, got.fitness, got.n_points)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')            # (a prior of low fitness is warned about: 2^16 hypotheses are few)
        reg = register_cloud(q, sv, init='global', global_kwargs=gk, **REFINE)
    assert reg.coarse.hypothesis == want['hypothesis'] and np.array_equal(reg.coarse.T, got.T)
    direct = register_cloud(q, sv, init=got.T, **REFINE)
    assert np.array_equal(reg.T, direct.T)

