"""Dynamic points in the map on the MI355X (csrc/dc_dynamic.hip, slam.IcpMapper.update_dynamic, render.MovingObjectDataset): the
kernels against the numpy + cKDTree oracle (tests/dynamic_reference.py) bit for bit, the angular match table, a scene in which a
box moves, and what the switches change and do not change in run_slam."""
import math

import numpy as np
import pytest
import torch

import dynamic_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _device_update(t):
    """ops.dyn_update on a table of dynamic_reference -> (P' [N], seen [N]) as numpy arrays."""
    from depth_correction_amd import ops
    prm = t.prm
    P = _t(np.array(t.prob, dtype=np.float64))
    seen = torch.zeros((P.shape[0],), dtype=torch.uint8, device=DEV)
    ops.dyn_update(_t(t.map_points, np.float64), _t(t.map_normals, np.float64), _t(t.pose, np.float64), _t(t.reading, np.float64),
                   _t(t.rows, np.int32), _t(t.match_idx, np.int32), _t(t.match_chord, np.float64), prm.chord_max, prm.epsilon_a, prm.epsilon_d,
                   prm.alpha, prm.beta, prm.threshold, prm.max_range, P, seen)
    return P.cpu().numpy(), seen.cpu().numpy()


def _hold(t):
    ref = R.update_rows(t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, t.prm, t.prob)
    P, seen = _device_update(t)
    bad = np.flatnonzero(~R.same_bits(P, ref.prob))
    print('rows %d: %d probabilities differ from the oracle' % (len(t.rows), bad.size))
    assert bad.size == 0, (bad[:10], P[bad[:10]], ref.prob[bad[:10]])          # expected difference: 0
    assert np.array_equal(seen, ref.seen)
    P2, seen2 = _device_update(t)
    assert R.same_bits(P, P2).all() and np.array_equal(seen, seen2)             # two runs are bit-identical
    return ref


def _hold_directions(points, pose, max_range):
    from depth_correction_amd import ops
    ref = R.direction(points, pose, max_range)
    dirs, depth, valid = ops.dyn_directions(_t(points, np.float64), None if pose is None else _t(pose, np.float64), max_range)
    dirs, depth, valid = dirs.cpu().numpy(), depth.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(valid, ref.valid)
    assert R.same_bits(dirs, ref.u).all() and R.same_bits(depth, ref.rho).all()
    assert np.isfinite(dirs).all()
    return ref


# ---- 1. kernels against the oracle ----------------------------------------------------------------------------------------------------
def test_hand_table_bit_for_bit():
    t = R.hand_table()
    ref = _hold(t)
    for i, name in enumerate(t.names):
        assert ref.seen[i] == t.expect[name], name
    extra = np.array([[np.nan, 0.0, 0.0], [np.inf, 1.0, 0.0], [0.0, -np.inf, 2.0], [1e-200, 0.0, 0.0], [1e200, 1e200, 0.0], [3.0, 4.0, 12.0]])
    for pose in (None, t.pose, R.random_pose(np.random.default_rng(3))):
        for pts, max_range in ((t.map_points, t.prm.max_range), (t.reading, 0.0), (extra, 0.0), (extra, math.inf), (extra, 13.0)):
            _hold_directions(pts, pose, max_range)


@pytest.mark.parametrize('m', [1, 1000])
@pytest.mark.parametrize('n_rows', [1, 255, 256, 257, 65537])
def test_random_rows_bit_for_bit(n_rows, m):
    t = R.random_rows(n_rows, m, seed=1000 * m + n_rows)
    ref = _hold(t)
    if n_rows >= 65537 and m > 1:
        for name, rows in ref.branch.items():
            assert name == 'reading_invalid' or rows.sum() >= 100, (name, int(rows.sum()))
    _hold_directions(t.map_points, t.pose, t.prm.max_range)
    _hold_directions(t.reading, None, 0.0)


def test_rows_that_skip_map_rows():
    t = R.random_rows(3001, 500, seed=6, skip=True)
    ref = _hold(t)
    others = np.setdiff1d(np.arange(t.prob.size), t.rows)
    assert R.same_bits(ref.prob[others], t.prob[others]).all() and (ref.seen[others] == 0).all()


def test_bad_parameters_and_empty_tables_are_refused_or_do_nothing():
    from depth_correction_amd import ops
    t = R.hand_table()
    for kw in (dict(chord_max=0.0), dict(chord_max=2.0), dict(epsilon_a=-1.0), dict(epsilon_d=math.inf), dict(alpha=1.0), dict(beta=0.0),
               dict(threshold=0.0), dict(threshold=1.5)):
        t.prm = R.params(**dict(R.TABLE_PRM, **kw))
        with pytest.raises(RuntimeError, match='invalid argument'):
            _device_update(t)
    t = R.hand_table()
    t.rows, t.match_idx, t.match_chord = t.rows[:0], t.match_idx[:0], t.match_chord[:0]
    P, seen = _device_update(t)                           # n_rows == 0 launches nothing
    assert R.same_bits(P, t.prob).all() and not seen.any()
    dirs, depth, valid = ops.dyn_directions(torch.empty((0, 3), dtype=torch.float64, device=DEV))
    assert dirs.shape == (0, 3) and depth.shape == (0,) and valid.shape == (0,)
    with pytest.raises(TypeError):
        ops.dyn_directions(torch.zeros((4, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.dyn_directions(torch.zeros((4, 2), dtype=torch.float64, device=DEV))


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    base.update(kw)
    return Config(**base)


def test_map_with_no_row_in_range_is_left_alone():
    from depth_correction_amd.slam import IcpMapper, MapperScan
    rng = np.random.default_rng(8)
    pts = rng.uniform(-2.0, 2.0, size=(500, 3))
    nrm = rng.normal(size=(500, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    scan = MapperScan(_t(pts), _t(nrm), _t(np.linalg.norm(pts, axis=1)))
    mapper = IcpMapper(_cfg(slam_compute_prob_dynamic=True))
    assert mapper.update(scan, np.eye(4)) == 500
    P0 = mapper.map_dynamic().clone()
    assert (P0 == 0.6).all()                             # the first scan's points get the prior
    far = np.eye(4)
    far[:3, 3] = (100.0, 0.0, 0.0)
    out = mapper.update_dynamic(scan, far)               # every map point is beyond slam_sensor_max_range from there
    assert out == dict(in_range=0, matched=0, occluded=0, updated=0, dynamic=0)
    assert torch.equal(mapper.map_dynamic(), P0)
    out = mapper.update_dynamic(scan, np.eye(4))         # the same scan from where it was taken: every point is seen where it is
    assert out['in_range'] == 500 and out['matched'] == 500 and out['updated'] == 500 and out['dynamic'] == 0
    assert (mapper.map_dynamic() < P0).all()


# ---- 2. match table -------------------------------------------------------------------------------------------------------------------
def test_match_table_equals_ckdtree():
    from depth_correction_amd import ops
    from depth_correction_amd.render import lidar_directions
    rng = np.random.default_rng(21)
    prm = R.params()
    dirs, _ = lidar_directions(size=(64, 512), fov=(45.0, 360.0), num_segments=16)
    reading = np.array(dirs) * rng.uniform(1.0, 9.0, size=(dirs.shape[0], 1))
    reading[::97] = 0.0                                  # rows without a direction: they must not enter the grid
    mp = rng.uniform(-6.0, 6.0, size=(20000, 3))
    mp[:, 2] = rng.uniform(-1.5, 1.5, size=20000)
    mp[::101] = 60.0                                     # out of range
    pose = R.random_pose(rng)
    pose[2, 3] = 0.2
    pose[:3, :3] = np.array([[math.cos(0.4), -math.sin(0.4), 0.0], [math.sin(0.4), math.cos(0.4), 0.0], [0.0, 0.0, 1.0]])
    tab = R.match_table(mp, pose, reading, prm)
    both = np.isfinite(tab.chord2)
    assert not (tab.chord[both] == tab.chord2[both]).any()           # no tie between the two nearest: the nearest is well defined
    u, _, u_ok = ops.dyn_directions(_t(mp), _t(pose), prm.max_range)
    v, _, v_ok = ops.dyn_directions(_t(reading), None, 0.0)
    (u,), rows = ops.compact_rows(u_ok, [u], want_index=True)
    (v,), vrows = ops.compact_rows(v_ok, [v], want_index=True)
    grid = ops.knn_grid_build(v, u.shape[0], 1)
    chord, idx = ops.knn_grid_query(grid, u, torch.eye(4, dtype=torch.float64, device=DEV), 1, r=prm.chord_max)
    idx = idx.reshape(-1).cpu().numpy()
    match = np.where(idx >= 0, vrows.cpu().numpy()[np.maximum(idx, 0)], -1)
    assert np.array_equal(rows.cpu().numpy(), tab.rows)
    assert np.array_equal(match, tab.idx)
    assert R.same_bits(chord.reshape(-1).cpu().numpy(), tab.chord).all()
    matched = (tab.idx >= 0).sum()
    print('match table: %d of %d map rows in range, %d matched' % (len(tab.rows), len(mp), matched))
    assert 0.1 * len(mp) < matched < len(tab.rows)


# ---- 3. a scene in which a box moves ---------------------------------------------------------------------------------------------------
def _box_dataset(n, moves_at, sensor, size=(64, 512)):
    from depth_correction_amd.mesh import box_mesh, room_mesh
    from depth_correction_amd.render import MovingObjectDataset
    room = room_mesh((4.0, 3.0, 1.5))
    box = box_mesh((0.0, 0.0, 0.0), (0.4, 0.4, 0.8))
    obj = np.tile(np.eye(4), (n, 1, 1))
    obj[:, :3, 3] = (1.9, 0.0, -0.7)                     # standing on the floor (z = -1.5)
    obj[moves_at:, :3, 3] = (-2.1, 1.4, -0.7)
    poses = np.stack([sensor(s) for s in range(n)])
    return room, MovingObjectDataset(room, [(box, obj)], poses, size=size, fov=(45.0, 360.0), num_segments=16, device=DEV)


def _sensor3(s):
    T = np.eye(4)
    T[:3, 3] = (-0.6 + 0.15 * s, 0.05 * s, 0.0)
    return T


def test_moving_box_scene_device_equals_oracle_and_the_box_is_found():
    from depth_correction_amd.metrics import point_to_mesh_distance
    from depth_correction_amd.slam import IcpMapper, mapper_input
    # no voxel filter: the conditions below are those of whole 64 x 512 scans (a numpy simulation of this scene with analytic rays
    # gives 72 % / 0.3 % / 0.00 %; with grid_res = 0.1 the map is coarser than the beams and 1 % of the static points are flagged)
    cfg = _cfg(slam_compute_prob_dynamic=True, grid_res=0.0)
    prm = R.params(cfg)
    room, ds = _box_dataset(10, 3, _sensor3)
    assert len(ds) == 10 and ds.get_mesh() is room
    mapper = IcpMapper(cfg)
    P_or = np.zeros((0,))
    for i in range(len(ds)):
        cloud, pose = ds[i]
        assert cloud.dtype == ds.cloud_dtype and len(cloud) > 20000
        scan = mapper.prepare(mapper_input(cloud, None, cfg))
        n0 = mapper.n_map
        mp, mn = (a.clone() for a in mapper.map_points())
        added = mapper.update(scan, pose, overlap=None)
        P_dev = mapper.map_dynamic().cpu().numpy()
        if n0 > 0:
            ref = R.update_map(mp.cpu().numpy(), mn.cpu().numpy(), pose, scan.points.cpu().numpy(), prm, P_or)
            bad = np.flatnonzero(~R.same_bits(P_dev[:n0], ref.prob))
            print('scan %d: map %d, %s, %d probabilities differ from the oracle' % (i, n0, ref.counts, bad.size))
            assert bad.size == 0, (i, bad[:10], P_dev[bad[:10]], ref.prob[bad[:10]])
            assert mapper.last_dyn == ref.counts, (mapper.last_dyn, ref.counts)
            assert int((ref.prob >= prm.threshold).sum()) == mapper.last_dyn['dynamic']
            P_or = ref.prob
        else:
            assert mapper.last_dyn is None
        P_or = np.concatenate([P_or, np.full(added, prm.prior)])
        assert mapper.n_map == n0 + added == P_or.shape[0]
        assert (P_dev[n0:] == prm.prior).all()
    # the conditions hold on the oracle's final P; the classes are distances to the static mesh
    pts = mapper.map_points()[0]
    dist = point_to_mesh_distance(pts, room).cpu().numpy()
    x = pts.cpu().numpy()[:, 0]
    dyn = P_or >= prm.threshold
    first, second, static = (dist > 0.05) & (x > 0.0), (dist > 0.05) & (x < 0.0), dist < 1e-3
    share = [float(dyn[c].mean()) for c in (first, second, static)]
    print('dynamic share: object at its first place %.4f (%d points), at its second %.4f (%d), static %.5f (%d)'
          % (share[0], first.sum(), share[1], second.sum(), share[2], static.sum()))
    assert first.sum() > 100 and second.sum() > 100 and static.sum() > 10000
    assert share[0] >= 0.5
    assert share[2] <= 0.01
    assert share[1] <= 0.05
    kept = mapper.map_points(static_only=True)[0]
    assert kept.shape[0] == int((~dyn).sum()) and torch.equal(kept, pts[_t(~dyn)])


# ---- 4. and 5. run_slam with the switches ----------------------------------------------------------------------------------------------
def _sensor24(s):
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(0.0, 0.0, 0.04 * s)
    T[:3, 3] = (-3.0 + 0.25 * s, 0.3 * math.sin(s / 3.0), 0.02 * math.sin(s / 2.0))
    return T


@pytest.fixture(scope='module')
def runs():
    """run_slam over one 24-pose sequence (the box moves before scan 8) with the switches off, with the probabilities on, and with
    the probabilities on every scan and the cut; the scans are rendered once."""
    from depth_correction_amd import ops
    from depth_correction_amd.slam import IcpMapper, run_slam
    _, ds = _box_dataset(24, 8, _sensor24)
    items = [ds[i] for i in range(len(ds))]
    calls = dict(dyn_directions=0, dyn_update=0)
    wrapped = {}
    for name in calls:
        def counting(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        wrapped[name] = getattr(ops, name)
        setattr(ops, name, counting)
    out = {}
    try:
        noise = [1e-4] * 3 + [2.5e-3] * 3                 # slam_eval.launch
        for key, kw in (('off', {}), ('prob', dict(slam_compute_prob_dynamic=True)),
                        ('cut', dict(slam_compute_prob_dynamic=True, slam_dynamic_every_scan=True, slam_cut_dynamic=True))):
            cfg = _cfg(odom_cov=noise, **kw)
            mapper = IcpMapper(cfg)
            before = dict(calls)
            res = run_slam(items, None, cfg, mapper=mapper)
            out[key] = dict(res=res, mapper=mapper, cfg=cfg, calls={k: calls[k] - before[k] for k in calls}, items=items)
    finally:
        for name, f in wrapped.items():
            setattr(ops, name, f)
    return out


def test_nothing_existing_moves(runs):
    off, prob = runs['off'], runs['prob']
    assert off['calls'] == dict(dyn_directions=0, dyn_update=0)              # switches off: no dyn_* op runs
    assert prob['calls']['dyn_update'] > 0 and prob['calls']['dyn_directions'] == 2 * prob['calls']['dyn_update']
    a, b = off['res'], prob['res']
    for key in ('slam', 'odom', 'gt', 'path_lengths'):
        assert np.array_equal(a[key], b[key]), key
    assert len(a['info']) == len(b['info']) == 24
    for ia, ib in zip(a['info'], b['info']):
        assert set(ia) == set(ib) and {'dynamic', 'dyn'} <= set(ia)
        for k in ia:
            if k not in ('dynamic', 'dyn'):
                assert ia[k] == ib[k], k
        assert ia['dynamic'] == 0 and ia['dyn'] is None
    assert any(i['dyn'] is not None for i in b['info'])
    assert torch.equal(off['mapper'].map_points()[0], prob['mapper'].map_points()[0])
    assert (off['mapper'].map_dynamic() == 0.6).all()
    print('probabilities on: final dynamic count %d of %d map points' % (b['info'][-1]['dynamic'], b['info'][-1]['map_size']))


def test_cut_keeps_dynamic_points_out_of_the_pairs(runs):
    from depth_correction_amd import _native as nv, ops
    from depth_correction_amd.slam import mapper_input, slam_errors
    cut = runs['cut']
    mapper, cfg, res = cut['mapper'], cut['cfg'], cut['res']
    thr = cfg.slam_threshold_dynamic
    for i, info in enumerate(res['info']):
        assert info['ok'] and info['status'] == ('init' if i == 0 else 'converged'), (i, info['status'])
        assert i == 0 or info['dyn'] is not None                            # slam_dynamic_every_scan
    P = mapper.map_dynamic()
    n_dyn = int((P >= thr).sum())
    assert n_dyn > 0 and n_dyn == mapper.n_dynamic == res['info'][-1]['dynamic']
    pts, nrm = mapper.map_points()
    static = P < thr
    sp, sn = mapper.map_points(static_only=True)
    assert torch.equal(sp, pts[static]) and torch.equal(sn, nrm[static])
    # one iteration of the last scan from its pose: every pair is formed with a row of the compacted static cloud
    scan = mapper.prepare(mapper_input(cut['items'][-1][0], None, cfg))
    m, k = len(scan), mapper.knn
    grid, rp, rn, rows = mapper.reference(m)
    assert rows is not None and torch.equal(rows.long(), torch.nonzero(static).reshape(-1))
    assert torch.equal(rp, sp) and torch.equal(rn, sn) and grid.n == sp.shape[0]
    idx = torch.empty((m, k), dtype=torch.int32, device=DEV)
    dist = torch.empty((m, k), dtype=torch.float64, device=DEV)
    thr_d = torch.empty((1,), dtype=torch.float64, device=DEV)
    kept = torch.empty((m, k), dtype=torch.uint8, device=DEV)
    partials = torch.empty((ops.icp_blocks(m), nv.DC_ICP_PARTIALS), dtype=torch.float64, device=DEV)
    ops.icp_init(_t(res['slam'][-1]), mapper.state, mapper.status)
    mapper.iteration(scan, mapper.state[:16].view(4, 4), idx, dist, thr_d, partials, rp, rn, math.cos(cfg.icp_max_normal_angle), kept=kept,
                     grid=grid)
    pairs = kept.bool()
    assert int(pairs.sum()) > m and int(idx[pairs].min()) >= 0 and int(idx[pairs].max()) < rows.shape[0]
    assert (P[rows[idx[pairs].long()].long()] < thr).all()
    # reported, not asserted: on a room this size the box is a small share of the pairs
    e_cut = slam_errors(res['slam'], res['gt'], res['path_lengths'])
    e_off = slam_errors(runs['off']['res']['slam'], res['gt'], res['path_lengths'])
    print('mean errors without the cut %.3e rad / %.3e m, with it %.3e rad / %.3e m; %d of %d map points dynamic'
          % (e_off[0], e_off[1], e_cut[0], e_cut[1], n_dyn, mapper.n_map))
