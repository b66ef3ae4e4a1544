"""Dynamic points in the map on the host (no GPU): csrc/dc_dynmath.h through its host build (libdc_hostcheck.so, the header the
kernels of csrc/dc_dynamic.hip include) against the numpy restatement (tests/dynamic_reference.py) bit for bit, the properties of
that restatement, the new Config fields and their checks, and MovingObjectDataset's scene meshes."""
import math

import numpy as np
import pytest

import dynamic_reference as R


@pytest.fixture(scope='module')
def host():
    return R.host_lib()


def _hold(host, t):
    """The host build and the oracle on one table: P', seen bit for bit; returns the oracle's result."""
    ref = R.update_rows(t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, t.prm, t.prob)
    rc, P, seen = R.host_update(host, t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, t.prm, t.prob)
    assert rc == 0
    bad = np.flatnonzero(~R.same_bits(P, ref.prob))
    assert bad.size == 0, (bad[:10], P[bad[:10]], ref.prob[bad[:10]])
    assert np.array_equal(seen, ref.seen)
    return ref


# ---- header against oracle ------------------------------------------------------------------------------------------------------------
def test_hand_table_bit_for_bit(host):
    t = R.hand_table()
    ref = _hold(host, t)
    for i, name in enumerate(t.names):
        assert ref.seen[i] == t.expect[name], (name, ref.seen[i])
        if t.expect[name] != R.UPDATED:
            assert R.same_bits(ref.prob[i], t.prob[i]), name                   # occluded / untouched: P as it was, to the bit
    P = dict(zip(t.names, ref.prob))
    br = {k: dict(zip(t.names, v)) for k, v in ref.branch.items()}
    pinned = R.ONE / (R.ONE + R.EPS)
    # both sides of every boundary took the branch the rule names
    assert br['wp2_one']['delta_below_eps_d'] and br['wd2_eps']['delta_below_eps_d']
    assert br['wp2_ramp']['delta_equals_eps_d'] and br['wd2_ramp']['delta_equals_eps_d']          # delta < epsilon_d is strict
    assert br['wd2_ramp']['offset_below_d_max'] and br['wd2_one']['offset_equals_d_max'] and br['wd2_one']['offset_above_d_max']
    assert br['wp2_eps']['offset_equals_d_max']                                                    # offset < d_max is strict
    assert br['wd2_one']['rho_far_in_front'] and br['wp2_eps']['rho_far_in_front']
    assert br['wd2_eps']['rho_equals_r'] and br['wp2_one']['rho_equals_r']                         # delta = 0
    assert br['wd2_eps']['rho_above_r_ramp'] and br['wp2_ramp']['rho_above_r_ramp']                # rho > r: no dynamic evidence
    assert br['wd2_eps']['reach_exact'] and br['wp2_eps']['reach_exact']
    assert br['occluded']['reach_one_ulp_behind'] and br['updated']['reach_exact'] and br['updated']['reach_one_ulp_inside']
    assert br['below_threshold']['P_one_ulp_below_threshold'] and br['dynamic']['P_at_threshold'] and br['dynamic']['P_one_ulp_above_threshold']
    assert br['map_invalid']['rho_one_ulp_above_max_range'] and br['updated']['rho_equals_max_range']
    assert br['chord_refused']['chord_equals_max'] and br['chord_refused']['chord_above_max'] and br['updated']['chord_one_ulp_below_max']
    assert br['unmatched']['unmatched'] and br['reading_invalid']['reading_at_origin'] and br['map_invalid']['map_point_at_sensor']
    for name in ('P_at_threshold', 'P_one_ulp_above_threshold', 'P_dynamic_static_evidence', 'P_one'):
        assert P[name] == pinned, name
    # evidence moves P the way the rule says
    assert P['rho_far_in_front'] > 0.6 and P['offset_above_d_max'] > 0.6                 # seen through: dynamic evidence
    assert P['rho_equals_r'] < 0.6 and P['delta_below_eps_d'] < 0.6                      # seen where it is: static evidence
    assert P['P_zero'] > 0.0
    # w_v = eps: a normal perpendicular to the ray, or none, all but switches the update off
    for name in ('normal_perpendicular', 'normal_zero'):
        assert abs(P[name] - 0.6) < 1e-3 and P[name] != 0.6, (name, P[name])
    assert P['normal_opposed'] == P['offset_above_d_max']                                  # |n . d|
    assert P['chord_one_ulp_below_max'] != P['chord_zero'] and abs(P['chord_one_ulp_below_max'] - 0.3) < 1e-3   # w_d1 -> eps at the rim


def test_hand_table_directions_bit_for_bit(host):
    t = R.hand_table()
    extra = np.array([[np.nan, 0.0, 0.0], [np.inf, 1.0, 0.0], [0.0, -np.inf, 2.0], [1e-200, 0.0, 0.0], [1e200, 1e200, 0.0], [3.0, 4.0, 12.0]])
    rng = np.random.default_rng(3)
    for pose in (None, t.pose, R.random_pose(rng)):
        for pts, max_range in ((t.map_points, t.prm.max_range), (t.reading, 0.0), (extra, 0.0), (extra, np.inf), (extra, 13.0)):
            ref = R.direction(pts, pose, max_range)
            dirs, depth, valid = R.host_directions(host, pts, pose, max_range)
            assert np.array_equal(valid, ref.valid)
            assert R.same_bits(dirs, ref.u).all() and R.same_bits(depth, ref.rho).all()
            assert np.isfinite(dirs).all() and (dirs[~valid] == 0.0).all()
    ref = R.direction(extra, None, 13.0)
    assert list(ref.valid) == [False, False, False, False, False, True] and ref.rho[5] == 13.0      # 1e-200 squared underflows to 0
    assert list(R.direction(extra, None, 0.0).valid) == [False, False, False, False, False, True]       # 1e200 squared overflows


def test_random_rows_bit_for_bit_and_every_branch(host):
    t = R.random_rows(20000, 3000, seed=5)
    ref = _hold(host, t)
    for name, rows in ref.branch.items():
        if name == 'reading_invalid':               # the generator makes no reading point at the origin (the hand table has it)
            continue
        assert rows.sum() >= 100, (name, int(rows.sum()))
    dm = R.direction(t.map_points, t.pose, t.prm.max_range)
    dirs, depth, valid = R.host_directions(host, t.map_points, t.pose, t.prm.max_range)
    assert np.array_equal(valid, dm.valid) and R.same_bits(dirs, dm.u).all() and R.same_bits(depth, dm.rho).all()
    assert 100 <= (~valid).sum() <= valid.size - 100


def test_rows_that_skip_map_rows_leave_the_others(host):
    t = R.random_rows(3000, 500, seed=6, skip=True)
    ref = _hold(host, t)
    others = np.setdiff1d(np.arange(t.prob.size), t.rows)
    assert R.same_bits(ref.prob[others], t.prob[others]).all() and (ref.seen[others] == 0).all()
    assert (ref.seen[t.rows] == R.UPDATED).sum() > 100


def test_host_update_refuses_bad_parameters(host):
    t = R.hand_table()
    bad = [dict(chord_max=0.0), dict(chord_max=2.0), dict(chord_max=math.nan), dict(epsilon_a=-1e-9), dict(epsilon_a=math.inf),
           dict(epsilon_d=-1e-9), dict(epsilon_d=math.nan), dict(alpha=0.0), dict(alpha=1.0), dict(beta=0.0), dict(beta=1.0),
           dict(threshold=0.0), dict(threshold=1.0000001), dict(max_range=math.nan)]
    for kw in bad:
        prm = R.params(**dict(R.TABLE_PRM, **kw))
        rc, P, seen = R.host_update(host, t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, prm, t.prob)
        assert rc == -1, kw
        assert R.same_bits(P, t.prob).all() and not seen.any()
    for kw in (dict(threshold=1.0), dict(epsilon_a=0.0), dict(epsilon_d=0.0), dict(max_range=0.0), dict(max_range=math.inf)):
        t.prm = R.params(**dict(R.TABLE_PRM, **kw))
        _hold(host, t)                                # the bounds themselves are accepted, and d_max = 0 divides nothing by zero
        assert np.isfinite(R.update_rows(t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, t.prm,
                                         t.prob).prob).all()


# ---- oracle properties ----------------------------------------------------------------------------------------------------------------
def test_oracle_probabilities_stay_in_range_and_untouched_rows_keep_their_bits():
    t = R.random_rows(20000, 3000, seed=9)
    ref = R.update_rows(t.map_points, t.map_normals, t.pose, t.reading, t.rows, t.match_idx, t.match_chord, t.prm, t.prob)
    assert (ref.prob >= 0.0).all() and (ref.prob <= 1.0).all()
    br = ref.branch
    kept = br['unmatched'] | br['chord_refused'] | br['map_invalid'] | br['occluded']
    assert kept.sum() > 1000
    assert R.same_bits(ref.prob[kept], t.prob[kept]).all()
    assert (ref.seen[br['occluded']] == R.OCCLUDED).all() and (ref.seen[br['unmatched'] | br['chord_refused'] | br['map_invalid']] == 0).all()
    dyn = br['dynamic']
    assert dyn.sum() > 100 and (ref.prob[dyn] == R.ONE / (R.ONE + R.EPS)).all()
    assert (br['updated'] == (br['below_threshold'] | br['dynamic'])).all()


def _one(prm, P, rho, r=4.0):
    """One update of a point at (rho, 0, 0) with its normal along the ray against the reading point (r, 0, 0), c = 0."""
    out = R.update_rows([[rho, 0.0, 0.0]], [[1.0, 0.0, 0.0]], np.eye(4), [[r, 0.0, 0.0]], [0], [0], [0.0], prm, [P])
    assert out.seen[0] == R.UPDATED
    return float(out.prob[0])


def test_oracle_static_updates_fall_and_dynamic_updates_cross_the_threshold():
    prm = R.params()
    P = [prm.prior]
    for _ in range(10):                                # c = 0, delta = 0, |cos| = 1: the beam ends on the point
        P.append(_one(prm, P[-1], 4.0))
    # the static update contracts toward its fixed point (2.5e-5 with these parameters) and reaches it, to the bit, at the sixth
    # step: the sequence falls strictly until then and never rises
    assert all(b <= a for a, b in zip(P, P[1:])), P
    assert all(b < a for a, b in zip(P[:6], P[1:6])) and P[10] < 1e-4, P
    steps = 0
    Pd = P[-1]
    while Pd < prm.threshold:                          # the beam passes through where the point was
        Pd = _one(prm, Pd, 2.0)
        steps += 1
        assert steps <= 4, (steps, Pd)
    assert _one(prm, Pd, 4.0) == R.ONE / (R.ONE + R.EPS)           # and static evidence no longer brings it back


def test_oracle_match_table_is_ckdtree_with_a_strict_bound():
    prm = R.params(max_range=0.0)
    a = prm.beam_half_angle
    reading = np.array([[5.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 0.0]])
    mp = np.array([[2.0 * math.cos(a), 2.0 * math.sin(a), 0.0], [math.cos(3 * a), math.sin(3 * a), 0.0], [0.0, 7.0, 0.0], [0.0, 0.0, 0.0]])
    tab = R.match_table(mp, np.eye(4), reading, prm)
    assert list(tab.rows) == [0, 1, 2] and list(tab.idx) == [0, -1, 1]          # the origin rows of both sides never enter the search
    assert tab.chord[0] < prm.chord_max and np.isinf(tab.chord[1]) and tab.chord[2] == 0.0
    assert abs(tab.chord[0] - 2.0 * math.sin(a / 2.0)) < 1e-15


# ---- configuration, mapper and dataset ------------------------------------------------------------------------------------------------
def test_config_defaults_are_slam_launch_with_the_switches_off():
    from depth_correction_amd.config import Config
    cfg = Config()
    assert (cfg.slam_compute_prob_dynamic, cfg.slam_dynamic_every_scan, cfg.slam_cut_dynamic) == (False, False, False)
    assert (cfg.slam_prior_dynamic, cfg.slam_threshold_dynamic, cfg.slam_beam_half_angle, cfg.slam_epsilon_a, cfg.slam_epsilon_d,
            cfg.slam_alpha, cfg.slam_beta, cfg.slam_sensor_max_range) == (0.6, 0.9, 0.01, 0.01, 0.01, 0.8, 0.99, 25.0)
    from depth_correction_amd.slam import dynamic_params
    p = dynamic_params(cfg)
    assert p['chord_max'] == 2.0 * math.sin(0.01) and p['max_range'] == 25.0
    ref = R.params(cfg)
    assert all(getattr(ref, k) == p[k] for k in ('prior', 'threshold', 'epsilon_a', 'epsilon_d', 'alpha', 'beta', 'max_range', 'chord_max'))


@pytest.mark.parametrize('field,value', [
    ('slam_beam_half_angle', 0.0), ('slam_beam_half_angle', math.pi / 2), ('slam_beam_half_angle', -0.01), ('slam_beam_half_angle', math.nan),
    ('slam_epsilon_a', -1e-9), ('slam_epsilon_a', math.inf), ('slam_epsilon_d', -1e-9), ('slam_epsilon_d', math.nan),
    ('slam_alpha', 0.0), ('slam_alpha', 1.0), ('slam_beta', 0.0), ('slam_beta', 1.0),
    ('slam_threshold_dynamic', 0.0), ('slam_threshold_dynamic', 1.0000001), ('slam_prior_dynamic', -1e-9), ('slam_prior_dynamic', 1.0000001)])
def test_parameter_validation(field, value):
    from depth_correction_amd.config import Config
    from depth_correction_amd.slam import dynamic_params
    cfg = Config()
    setattr(cfg, field, value)
    with pytest.raises(ValueError, match=field.replace('slam_', '').split('_dynamic')[0]):
        dynamic_params(cfg)


def test_parameter_bounds_themselves():
    from depth_correction_amd.config import Config
    from depth_correction_amd.slam import dynamic_params
    for field, value in (('slam_epsilon_a', 0.0), ('slam_epsilon_d', 0.0), ('slam_threshold_dynamic', 1.0), ('slam_prior_dynamic', 0.0),
                         ('slam_prior_dynamic', 1.0), ('slam_sensor_max_range', math.inf), ('slam_sensor_max_range', 0.0)):
        cfg = Config()
        setattr(cfg, field, value)
        dynamic_params(cfg)


def _scene():
    from depth_correction_amd.mesh import box_mesh, room_mesh
    from depth_correction_amd.render import MovingObjectDataset
    room = room_mesh((4.0, 3.0, 1.5))
    box = box_mesh((0.0, 0.0, 0.0), (0.4, 0.4, 0.8))
    n = 5
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, 0, 3] = np.arange(n) * 0.1
    obj = np.tile(np.eye(4), (n, 1, 1))
    c, s = math.cos(0.3), math.sin(0.3)
    obj[2:, :3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    obj[:, :3, 3] = [1.9, 0.0, -0.7]
    obj[2:, :3, 3] = [-2.1, 1.4, -0.7]
    return room, box, poses, obj, MovingObjectDataset(room, [(box, obj)], poses, device='cpu')


def test_moving_object_scene_mesh_is_a_numpy_merge():
    room, box, poses, obj, ds = _scene()
    assert len(ds) == 5 and ds.ids == [0, 1, 2, 3, 4] and ds.get_mesh() is room
    assert np.array_equal(ds.cloud_pose(3), poses[3])
    for id in (0, 3):
        scene = ds.scene_mesh(id)
        moved = box.vertices @ obj[id, :3, :3].T + obj[id, :3, 3]
        assert scene.faces.shape[0] == room.faces.shape[0] + box.faces.shape[0]
        assert scene.vertices.shape[0] == np.unique(np.concatenate([room.vertices, moved]), axis=0).shape[0]
        assert scene.vertices.shape[0] == room.vertices.shape[0] + box.vertices.shape[0]          # the box touches no room vertex
        tri = scene.vertices[scene.faces]
        nr = room.faces.shape[0]
        assert np.array_equal(tri[:nr], room.vertices[room.faces])                               # the room's faces first, untouched
        assert np.array_equal(tri[nr:], moved[box.faces])                                        # then the box's, offset and moved
        assert np.array_equal(tri[nr:].reshape(-1, 3).min(axis=0), moved.min(axis=0))
    assert np.array_equal(ds.get_mesh().vertices, room.vertices)                                 # the ground truth does not move


def test_moving_object_dataset_indexing_and_refusals():
    from depth_correction_amd.render import MovingObjectDataset
    room, box, poses, obj, ds = _scene()
    sub = ds[1:4]
    assert len(sub) == 3 and sub.ids == [1, 2, 3] and len(ds[[0, 4]]) == 2 and ds[[0, 4]].ids == [0, 4]
    assert np.array_equal(sub.cloud_pose(sub.ids[2]), poses[3])
    with pytest.raises(ValueError):
        ds['a']
    with pytest.raises(ValueError, match='poses'):
        MovingObjectDataset(room, [(box, obj[:3])], poses)
    with pytest.raises(TypeError):
        MovingObjectDataset(room, [(box.vertices, obj)], poses)
    with pytest.raises(TypeError):
        MovingObjectDataset(room, [(box, obj)], poses, beam='thin')
    with pytest.raises(ValueError):
        MovingObjectDataset(room, [(box, obj)], poses, size=(64, 8), num_segments=16)
    # construction needs no GPU; rendering refuses any other device with the package's usual error
    with pytest.raises(RuntimeError, match='no CPU path'):
        ds.local_cloud(0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ds[0]
