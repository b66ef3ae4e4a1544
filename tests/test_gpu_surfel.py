"""Surfel ray casting on the GPU (dc_surfel_bvh_build / dc_surfel_cast_rays): the tree's invariants, the cast against the host build's
brute force (bit for bit) and the numpy oracle (tests/surfel_reference.py), ties and edges on dyadic coordinates, the blend and its
normal gate, and depth_bias / eval_bias against a surveyed cloud."""
import math

import numpy as np
import pytest
import torch

import surfel_reference as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
COS45 = math.cos(math.pi / 4)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _build(pts, nrm, rho, box=None):
    from depth_correction_amd import ops
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    box = np.concatenate([pts.min(axis=0), pts.max(axis=0)]) if box is None else box
    return ops.surfel_bvh_build(_dev(pts), _dev(np.asarray(nrm, dtype=np.float64).reshape(-1, 3)), _dev(np.asarray(rho, dtype=np.float64).reshape(-1)), box)


def _cast(bvh, vps, dirs, off, poses, dtype=torch.float64, **kw):
    from depth_correction_amd import ops
    out = ops.surfel_cast_rays(bvh, _dev(vps, dtype), _dev(dirs, dtype), off, _dev(poses), **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


@pytest.fixture(scope='module')
def lib():
    return S.surfel_host_lib()


@pytest.fixture(scope='module')
def room():
    pts, nrm, rho = S.room_survey()
    return pts, nrm, rho, _build(pts, nrm, rho)


# ---- 1. the tree ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['one', 'two', 'three', 'room', 'duplicates', 'coplanar'])
def test_tree_invariants(lib, kind):
    rng = np.random.default_rng(8)
    n = dict(one=1, two=2, three=3).get(kind, 1000)
    pts, nrm, rho = S.room_survey(seed=9, m=n)
    if kind == 'duplicates':                                # every centre four times (and whole disks twice)
        pts[250:] = np.tile(pts[:250], (3, 1))
        nrm[500:750], rho[500:750] = nrm[:250], rho[:250]
    if kind == 'coplanar':                                  # a flat scene-box axis
        pts[:, 2] = 0.75
        nrm = np.tile([0.0, 0.0, 1.0], (n, 1)) + rng.normal(scale=0.01, size=(n, 3))
    one, two = _build(pts, nrm, rho), _build(pts, nrm, rho)
    torch.cuda.synchronize()
    for name in ('leaf_index', 'child', 'parent', 'node_box', 'leaf_disk'):
        assert torch.equal(getattr(one, name), getattr(two, name)), name
    leaf_index, child, parent, node_box, leaf_disk = (getattr(one, k).cpu().numpy() for k in ('leaf_index', 'child', 'parent', 'node_box', 'leaf_disk'))
    assert one.n_disks == n and node_box.shape == (2 * n - 1, 6) and leaf_disk.shape == (n, 8) and child.shape == (max(n - 1, 0), 2)
    S.check_tree(leaf_index, child, parent, node_box, n)
    # the leaves: the disks' rows in leaf order, and the boxes of the host build, bit for bit
    assert np.array_equal(leaf_disk, S.disk_rows(pts, nrm, rho)[leaf_index])
    assert np.array_equal(node_box[n - 1:], S.host_boxes(lib, pts, nrm, rho)[leaf_index])
    # every leaf's box inside every ancestor's (climbing; check_tree has the single steps)
    for leaf in range(0, n, max(1, n // 50)):
        node = n - 1 + leaf
        while parent[node] >= 0:
            node = parent[node]
            assert (node_box[n - 1 + leaf, :3] >= node_box[node, :3]).all() and (node_box[n - 1 + leaf, 3:] <= node_box[node, 3:]).all()
        assert node == 0


# ---- 2. the cast against the host build's brute force -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('n_rays', [4096, 129, 0])
def test_cast_is_the_brute_force_bit_for_bit(lib, room, dtype, n_rays):
    pts, nrm, rho, bvh = room
    vps, dirs, off, poses = S.room_rays(n=max(n_rays, 2))
    if n_rays == 0:
        vps, dirs, off = vps[:0], dirs[:0], np.zeros(3, dtype=np.int64)
    o, d = S.world_rays(vps, dirs, off, poses)
    rows = S.disk_rows(pts, nrm, rho)
    for t_min, window in ((0.0, 0.0), (1.5, 0.0), (0.0, 0.1)):
        idx, t1, t, inc, cnt = _cast(bvh, vps, dirs, off, poses, dtype, t_min=t_min, window=window)
        assert idx.shape == (n_rays,) and idx.dtype == np.int32 and cnt.dtype == np.int32
        if n_rays == 0:
            continue
        r_idx, r_t1, r_t, r_inc, r_cnt = S.host_cast_brute(lib, rows, o, d, t_min, window, COS45)
        assert (idx >= 0).sum() > 0.4 * n_rays
        assert np.array_equal(idx, r_idx) and np.array_equal(t1, r_t1) and np.array_equal(cnt, r_cnt)
        if window == 0.0:
            assert np.array_equal(t, r_t) and np.array_equal(inc, r_inc, equal_nan=True) and np.array_equal(t, t1)
            assert np.array_equal(cnt, (idx >= 0).astype(np.int32))


# ---- 3. edges, on dyadic coordinates ------------------------------------------------------------------------------------------------------
def test_edges_and_ties(lib):
    inf, nan = np.inf, np.nan
    pts = [[0, 0, 4], [0, 0, 4], [8, 0, 4], [8.5, 0, 4], [0, 0, 6]]         # 0 = 1; 2 and 3 overlap in one plane; 4 behind 0
    nrm = [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, -2]]
    rho = [1.25, 1.25, 1.0, 1.0, 1.0]
    bvh = _build(pts, nrm, rho)
    up = np.nextafter(0.75, 1.0)
    o = np.array([[0, 0, 0], [8.25, 0, 0], [-5, 0, 4], [0.75, 1, 0], [up, 1, 0], [0, 0, 0], [inf, 0, 0], [0, 0, 9], [8.25, 0, 4]], dtype=np.float64)
    d = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 0, 1], [nan, 0, 1], [0, 0, 1], [0, 0, -0.5], [0, 0, 1]], dtype=np.float64)
    off, poses = [0, len(o)], np.eye(4)[None]
    rows = S.disk_rows(pts, nrm, rho)

    def both(**kw):
        got = _cast(bvh, o, d, off, poses, **kw)                            # the origins as view points: the identity pose is exact
        want = S.host_cast_brute(lib, rows, o, d, kw.get('t_min', 0.0), kw.get('window', 0.0), kw.get('min_cos', COS45))
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)
        return got

    idx, t1, t, inc, cnt = both()
    #                    identical  coplanar  in-plane  rim  outside  NaN  inf  from behind (t in units of |d|)  on the disk itself
    assert idx.tolist() == [0, 2, -1, 0, -1, -1, -1, 4, -1]
    assert t1.tolist() == [4.0, 4.0, inf, 4.0, inf, inf, inf, 6.0, inf] and np.array_equal(t, t1)
    assert cnt.tolist() == [1, 1, 0, 1, 0, 0, 0, 1, 0]
    assert np.array_equal(np.isnan(inc), idx < 0) and (inc[idx >= 0] == 0.0).all()
    # t_min equal to t: the disks at t = 4 no longer count, the one behind does
    idx, t1, t, inc, cnt = both(t_min=4.0)
    assert idx.tolist() == [4, -1, -1, -1, -1, -1, -1, 4, -1] and t1[0] == 6.0
    assert both(t_min=float(np.nextafter(4.0, 0.0)))[0].tolist() == [0, 2, -1, 0, -1, -1, -1, 4, -1]
    # the blend: both copies of the identical disk, then the disk behind them once the window reaches it
    idx, t1, t, inc, cnt = both(window=0.1)
    assert idx.tolist() == [0, 2, -1, 0, -1, -1, -1, 4, -1] and cnt.tolist() == [2, 2, 0, 2, 0, 0, 0, 1, 0] and np.array_equal(t, t1)
    idx, t1, t, inc, cnt = both(window=2.0)
    assert cnt.tolist() == [3, 2, 0, 2, 0, 0, 0, 1, 0] and t[0] == 4.0 + (1.0 * 2.0) / 3.0 and t1[0] == 4.0
    assert t[3] == 4.0                                                     # on the rim: every weight 0, the first hit's values
    # one disk: the root is the leaf
    single = _build(pts[:1], nrm[:1], rho[:1])
    got = _cast(single, o, d, off, poses, window=0.1)
    assert got[0].tolist() == [0, -1, -1, 0, -1, -1, -1, 0, -1] and got[4].tolist() == [1, 0, 0, 1, 0, 0, 0, 1, 0]


# ---- 4. the blend ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_blend_matches_the_oracle_within_the_error_count(room, dtype):
    pts, nrm, rho, bvh = room
    vps, dirs, off, poses = S.room_rays()
    o, d = S.world_rays(vps, dirs, off, poses)
    counts = {}
    for min_cos in (COS45, 0.0):
        got = _cast(bvh, vps, dirs, off, poses, dtype, window=0.1, min_cos=min_cos)
        again = _cast(bvh, vps, dirs, off, poses, dtype, window=0.1, min_cos=min_cos)
        for a, b in zip(got, again):
            assert np.array_equal(a, b, equal_nan=True)
        idx, t1, t, inc, cnt = got
        ref = S.oracle(pts, nrm, rho, o, d, window=0.1, min_cos=min_cos)
        assert np.array_equal(idx, ref.index) and np.array_equal(t1, ref.t_first) and np.array_equal(cnt, ref.count)
        et, bt = S.t_err_units(t, ref)
        ec, bc = S.cos_err_units(inc, ref)
        print('min_cos %.3f: largest multiple of the error count: t %.3f, cos(inc) %.3f; k up to %d' % (min_cos, (et / bt).max(), (ec / bc).max(), cnt.max()))
        assert (et <= bt).all() and (ec <= bc).all()
        counts[min_cos] = cnt
    # the gate matters: near the room's edges the adjoining wall's disks lie inside the window
    assert (counts[0.0] >= counts[COS45]).all() and (counts[0.0] > counts[COS45]).sum() > 20


def test_corner_overhang_and_the_normal_gate():
    """Wall A (x = 2) is hit 5 cm from the corner with wall B (y = 1.5), whose disk overhangs behind A: the ray meets it 8.5 cm
    farther on, inside the window.  The gate keeps it out of the blend; min_cos = 0 lets it in."""
    pts = [[2, 1.4, 0], [2, 1.3, 0.1], [1.9, 1.5, 0]]
    nrm = [[1, 0, 0], [-1, 0, 0], [0, 1, 0]]
    rho = [0.3, 0.3, 0.3]
    bvh = _build(pts, nrm, rho)
    o, d = np.zeros((1, 3)), np.array([[2.0, 1.45, 0.0]])
    args = (bvh, o, d, [0, 1], np.eye(4)[None])
    for min_cos, members in ((COS45, [0, 1]), (0.0, [0, 1, 2])):
        idx, t1, t, inc, cnt = _cast(*args, window=0.1, min_cos=min_cos)
        ref = S.oracle(pts, nrm, rho, o, d, window=0.1, min_cos=min_cos)
        assert idx[0] == 0 and t1[0] == 1.0 and cnt[0] == len(members) == ref.count[0] and ref.members[1].tolist() == members
        et, bt = S.t_err_units(t, ref)
        ec, bc = S.cos_err_units(inc, ref)
        assert (et <= bt).all() and (ec <= bc).all()
        if min_cos > 0:
            assert t[0] == 1.0 and abs(math.cos(inc[0]) - 2.0 / math.hypot(2.0, 1.45)) < 1e-15
        else:
            assert 1.0 < t[0] < 1.0 + 0.0345 and math.cos(inc[0]) > 2.0 / math.hypot(2.0, 1.45) + 0.01
    assert _cast(*args, window=0.03, min_cos=0.0)[4][0] == 2                # the overhang lies 0.0345 behind: outside a 3 cm window


# ---- 5. depth_bias against a survey ------------------------------------------------------------------------------------------------------
def test_depth_bias_against_a_noisy_survey():
    """The wall scene of the host suite through metrics.depth_bias: clouds holding the exact depths of the plane, a survey with 5 mm
    of noise.  The first disk's depth is biased towards the sensor, growing with the angle; the blended depth is not."""
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.metrics import depth_bias
    from depth_correction_amd.survey import SurveyCloud
    pts, nrm, dirs, theta, depth = S.wall_scene()
    survey = SurveyCloud(pts, nrm)
    pose = np.eye(4)
    pose[:3, 3] = S.WALL_SENSOR
    cloud = DepthCloud(torch.zeros((1, 3), dtype=torch.float64, device=DEV), _dev(dirs), _dev(depth[:, None]))
    res = depth_bias([cloud], pose[None], survey, surfel_radius=S.WALL_RHO, surfel_window=S.WALL_WINDOW)
    idx, t, t1, cnt, inc = (res[k].cpu().numpy() for k in ('face', 't', 't_first', 'count', 'inc'))
    assert (idx >= 0).all() and res['before']['totals']['hits'] == len(dirs) and 8.0 < cnt.mean() < 11.0
    S.check_wall(theta, t1 - depth, t - depth)
    assert np.abs(inc - theta).max() < 1e-9                                  # every normal is the wall's
    assert abs(res['before']['overall']['rms']) < 0.005                      # the blend of ~10 disks of 5 mm noise
    first = depth_bias([cloud], pose[None], survey, surfel_radius=S.WALL_RHO, surfel_window=0.0)
    assert torch.equal(first['t'], res['t_first']) and torch.equal(first['t_first'], res['t_first']) and torch.equal(first['face'], res['face'])
    assert bool((first['count'] == 1).all())
    assert survey.surfels(DEV, radius=S.WALL_RHO) is survey.surfels(DEV, radius=S.WALL_RHO)        # cached per argument set
    auto = survey.surfels(DEV, k=10)
    assert auto is survey.surfels(DEV) and auto is not survey.surfels(DEV, k=10, scale=1.5)
    r = auto.radii.cpu().numpy()
    # 850 points / m^2: the tenth other point lies at about sqrt(10.5 / (850 pi)) = 6.3 cm
    assert 0.055 < np.median(r) < 0.07 and (r > 0).all()


# ---- 6. eval_bias ----------------------------------------------------------------------------------------------------------------------
def test_eval_bias_against_a_survey(tmp_path, capsys):
    from depth_correction_amd.eval import eval_bias
    from depth_correction_amd.survey import SurveyCloud
    from test_gpu_bias import _room_setup
    cfg, biased, model, poses = _room_setup(tmp_path, [0.05], [2.0])
    cfg.cloud_samples = 100000

    class SurveyOnly(object):
        """A sequence with a surveyed cloud and no mesh (the FEE corridor's shape)."""

        def __init__(self, ds):
            self.items = list(ds)
            self.survey = SurveyCloud.from_mesh(ds.get_mesh(), cfg.cloud_samples, device=DEV)

        def __iter__(self):
            return iter(self.items)

        def __str__(self):
            return 'survey_only/room'

    only = SurveyOnly(biased)
    assert not hasattr(only, 'get_mesh')
    cfg.bias_eval_csv, cfg.bias_eval_curve_csv = str(tmp_path / 'bias.csv'), str(tmp_path / 'curve.csv')
    res = eval_bias(cfg, test_datasets=[only], model=model)[0]
    assert 'Depth bias on survey_only/room:' in capsys.readouterr().out
    assert res['before']['totals']['used'] > 0 and 't_first' in res and 'count' in res and res['name'] == 'survey_only/room'
    line = open(cfg.bias_eval_csv).read().split()
    assert line[0] == 'survey_only/room' and int(line[1]) == res['before']['totals']['used'] and len(line) == 11
    assert len(open(cfg.bias_eval_curve_csv).read().splitlines()) == 1 + res['bins']
    # the validation path: the rendered room against the survey sampled from its own mesh, and against the mesh
    cfg.bias_eval_csv = cfg.bias_eval_curve_csv = None
    cfg.bias_eval_against = 'survey'
    on_survey = eval_bias(cfg, test_datasets=[biased], model=model)[0]
    cfg.bias_eval_against = 'mesh'
    on_mesh = eval_bias(cfg, test_datasets=[biased], model=model)[0]
    assert on_survey['before']['totals']['used'] > 0 and 'count' in on_survey and 'count' not in on_mesh
    with capsys.disabled():
        print('\nroom: used %d (survey) / %d (mesh); rms before %.5f / %.5f m, after %.5f / %.5f m; w at true angles %s / %s'
              % (on_survey['before']['totals']['used'], on_mesh['before']['totals']['used'], on_survey['before']['overall']['rms'],
                 on_mesh['before']['overall']['rms'], on_survey['after']['overall']['rms'], on_mesh['after']['overall']['rms'],
                 on_survey['fit']['w_true_angles'], on_mesh['fit']['w_true_angles']))
