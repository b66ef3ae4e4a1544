"""Scan-to-TSDF registration on the host (no GPU): the rules of csrc/dc_tsdf_track_math.h through their host build (libdc_hostcheck.so,
the header the kernels inline) against tests/tsdf_track_reference.py, bit for bit on x, value, grad, dist and flag over the designed
volumes of tests/tsdf_track_cases.py, and against hand-written figures where the arithmetic is exact; the row's edges; and one analytic
check through the oracle alone: the reference mapper pulls a displaced scan of a plane back onto the fused plane.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import slam_reference as R  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
import tsdf_track_cases as C  # noqa: E402
import tsdf_track_reference as T  # noqa: E402

CASES = {name: rest for name, *rest in C.sample_cases()}


def host_lib():
    """libdc_hostcheck.so with the tracking exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_tsdf_sparse_sample'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_tsdf_sparse_sample.argtypes = [vp, vp, vp, i64, vp, vp, vp, f64, f64, ci, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.dc_host_tsdf_icp_accumulate.argtypes = [vp, vp, vp, vp, vp, i64, vp, f64, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_sample(lib, vol, points, pose=None, min_count=1, stop=None, fill=None):
    """dc_host_tsdf_sparse_sample on the oracle volume's arrays; ``fill``: what the outputs hold beforehand."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    m = p.shape[0]
    keys, slots = np.ascontiguousarray(vol.keys, np.uint64), np.ascontiguousarray(vol.slots, np.int32)
    nb = np.array([vol.n_blocks], np.int64)
    pose = None if pose is None else np.ascontiguousarray(pose, np.float64)
    stop = None if stop is None else np.array([stop], np.int32)
    out = dict(x=np.zeros((m, 3)), value=np.zeros(m), grad=np.zeros((m, 3)), dist=np.zeros(m), flag=np.zeros(m, np.uint8))
    if fill is not None:
        for a in out.values():
            a[...] = fill
    rc = lib.dc_host_tsdf_sparse_sample(_p(keys), _p(slots), _p(nb), vol.capacity, _p(vol.sum), _p(vol.count), _p(vol.origin), vol.voxel,
                                        vol.trunc, min_count, _p(p), m, _p(pose), _p(stop), _p(out['x']), _p(out['value']), _p(out['grad']),
                                        _p(out['dist']), _p(out['flag']))
    assert rc == 0
    return out


def host_row(lib, s, thr, max_residual, status=0, fill=None):
    """(row [30], kept [m]) of dc_host_tsdf_icp_accumulate."""
    m = len(s['flag'])
    arrs = [np.ascontiguousarray(s[k], np.float64) for k in ('x', 'value', 'grad', 'dist')] + [np.ascontiguousarray(s['flag'], np.uint8)]
    row, kept = np.full(30, np.nan if fill is None else fill), np.full(m, 7, np.uint8)
    st = np.array([status, 0, 0, 0], np.int32)
    rc = lib.dc_host_tsdf_icp_accumulate(*[_p(a) for a in arrs], m, _p(np.array([thr], np.float64)), max_residual, _p(st), _p(row), _p(kept))
    assert rc == 0
    return row, kept


def assert_same_sample(got, want, what=''):
    for k in ('x', 'value', 'grad', 'dist'):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    assert np.array_equal(got['flag'], want['flag']), (what, 'flag')


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_sampling_equals_oracle_and_hand(lib, name):
    blocks, min_count, points, pose, expected = CASES[name]
    vol = C.make_volume(blocks)
    want = T.sample(vol, points, pose, min_count)
    got = host_sample(lib, vol, points, pose, min_count)
    assert_same_sample(got, want, name)
    if expected is not None:
        assert np.array_equal(got['flag'], expected['flag']), name
        assert np.array_equal(got['value'], expected['value'], equal_nan=True), name
        assert np.array_equal(got['grad'], expected['grad']), name
        valid = expected['flag'] == 0
        assert np.array_equal(got['dist'][valid], np.abs(expected['value'][valid])) and np.isposinf(got['dist'][~valid]).all(), name
    else:
        assert (got['flag'] == 0).sum() > 100 and (got['flag'] == 2).sum() > 50, name


def test_pose_moves_before_sampling(lib):
    """With and without a pose: the same world points give the same sample, and x is the moved point in move_point's order."""
    blocks, _, points, pose, _ = CASES['exact_pose']
    vol = C.make_volume(blocks)
    posed = host_sample(lib, vol, points, pose)
    plain = host_sample(lib, vol, posed['x'])
    assert_same_sample(posed, plain)
    blocks, _, points, pose, _ = CASES['generic_pose_oracle_only']
    got = host_sample(lib, C.make_volume(blocks), points, pose)
    assert np.array_equal(got['x'], R.moved(pose, points))


def test_stop_leaves_the_outputs(lib):
    blocks, min_count, points, pose, _ = CASES['linear_inside_one_block']
    vol = C.make_volume(blocks)
    got = host_sample(lib, vol, points, pose, min_count, stop=1, fill=5)
    assert all((a == 5).all() for a in got.values())
    got = host_sample(lib, vol, points, pose, min_count, stop=0, fill=5)
    assert_same_sample(got, T.sample(vol, points, pose, min_count))


def test_empty_volume_and_no_points(lib):
    vol = S.SparseVolume(capacity=2, **C.VOLUME)
    got = host_sample(lib, vol, np.array([[1.0, 1.0, 1.0]]))
    assert got['flag'].tolist() == [2] and np.isnan(got['value'][0]) and np.isposinf(got['dist'][0]) and not got['grad'].any()
    assert host_sample(lib, vol, np.zeros((0, 3)))['flag'].shape == (0,)


# ---- the row ---------------------------------------------------------------------------------------------------------------------------
def test_row_edges_by_hand(lib):
    s = C.row_edge_sample()
    row, kept = host_row(lib, s, 0.5, 2.0)                      # dist == threshold is kept
    assert kept.tolist() == [1, 1, 0, 0, 0, 0]
    assert np.array_equal(row, C.row_by_hand())
    _, kept = host_row(lib, s, 10.0, 2.0)                       # dist == max_residual is dropped, whatever the threshold
    assert kept.tolist() == [1, 1, 1, 0, 0, 0]
    _, kept = host_row(lib, s, 10.0, np.nextafter(2.0, 3.0))
    assert kept.tolist() == [1, 1, 1, 1, 0, 0]
    _, kept = host_row(lib, s, np.inf, np.inf)                  # an invalid point is never a pair
    assert kept.tolist() == [1, 1, 1, 1, 0, 0]
    row, kept = host_row(lib, s, np.nan, 2.0)                   # a NaN threshold keeps nothing
    assert kept.tolist() == [0] * 6 and not row.any()
    row, kept = host_row(lib, s, 0.5, 2.0, status=1, fill=3.0)  # a registration that has ended: nothing is written
    assert (row == 3.0).all() and (kept == 7).all()
    empty = {k: v[:0] for k, v in s.items()}
    row, kept = host_row(lib, empty, 0.5, 2.0)                  # m = 0: a row of zeros
    assert row.shape == (30,) and not row.any() and kept.shape == (0,)


@pytest.mark.parametrize('m', [1, 63, 257, 5000])
def test_row_matches_extended_precision(lib, m):
    s = C.random_sample(m)
    thr = R.quantile_finite(s['dist'], 0.8)
    want = T.totals(s, thr, 0.29)
    row, kept = host_row(lib, s, thr, 0.29)
    assert np.array_equal(kept.astype(bool), want['kept'])
    assert row[27] == want['n_pairs'] == row[29]
    assert (np.abs(row - want['totals']) <= C.totals_bound(want['n_pairs'], want['abs_totals'])).all()


def test_clamped_sample_is_no_pair_at_max_residual_tau(lib):
    blocks, min_count, points, pose, _ = CASES['all_corners_clamped']
    vol = C.make_volume(blocks)
    s = host_sample(lib, vol, points, pose, min_count)
    row, kept = host_row(lib, s, np.inf, vol.trunc)
    assert kept.tolist() == [0, 0] and not row.any()


# ---- the analytic check, through the oracle alone --------------------------------------------------------------------------------------
def test_reference_mapper_pulls_a_displaced_scan_onto_the_plane():
    """A volume fused from two viewpoints of the plane z = 0; a scan of the plane whose prior is off by a third of the truncation and
    1 degree: the registered pose puts the scan's points closer to the plane than the prior does."""
    prm = T.params(slam_tsdf_voxel_size=0.1, slam_tsdf_trunc=0.3, icp_max_iters=30)
    vol = T.new_volume(prm)
    for vp in ((0.3, -0.2, 2.0), (-0.5, 0.4, 1.6)):
        sc = C.plane_scan(vp)
        S.fuse(vol, vps=sc['vps'], dirs=sc['dirs'], depth=sc['depth'])
    scan = C.plane_scan((0.1, 0.1, 1.8), n_side=30, half=1.5)
    a = np.deg2rad(1.0)
    prior = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a), 0.0], [0.0, np.sin(a), np.cos(a), 0.1], [0.0, 0.0, 0.0, 1.0]])
    reg = T.register(vol, scan['points'], prior, prm)
    assert reg.status in ('converged', 'max_iterations'), reg.status
    before = np.abs(R.moved(prior, scan['points'])[:, 2])
    after = np.abs(R.moved(reg.pose, scan['points'])[:, 2])
    print('plane: mean |z| %.4f -> %.4f, max %.4f -> %.4f, %d iterations (%s)' % (before.mean(), after.mean(), before.max(), after.max(),
                                                                                   reg.iterations, reg.status))
    assert after.mean() < 0.2 * before.mean() and after.max() < before.max()
    assert reg.records[0].margins['thr'] > 0.0


def test_pose_sensitivity_of_the_step_by_step_scene():
    """The figure the device's pose bar is made of, recomputed on the host-built copy of the scene over three orders of the sums: the
    reference registers the scan, and no order moves a pose entry of any iteration by more than the recorded largest change."""
    from helpers import slam_pose
    scans, gt = C.roombox_host_scene()
    prm = T.params(**C.STEP)
    vol = T.new_volume(prm)
    for i in C.STEP_FUSED:
        S.fuse(vol, vps=scans[i]['vps'], dirs=scans[i]['dirs'], depth=scans[i]['depth'], pose=gt[i], max_range=prm.slam_sensor_max_range)
    p, truth = scans[C.STEP_SCAN]['points'], gt[C.STEP_SCAN]
    prior = truth @ slam_pose(0.03, (0.1, -0.05, 0.02))
    base = T.register(vol, p, prior, prm)
    assert base.status == 'converged' and np.abs(base.pose - truth).max() < 0.1 * np.abs(prior - truth).max()
    worst = 0.0
    for seed in (5, 1005, 2005):
        again = T.register(vol, p, prior, prm, order_seed=seed)
        assert again.iterations == base.iterations
        worst = max(worst, max(np.abs(a - b).max() for a, b in zip(base.poses, again.poses)))
    print('largest change over three orders: %.3g (recorded over 200: %.3g)' % (worst, C.POSE_SENSITIVITY))
    assert worst <= C.POSE_SENSITIVITY


def test_python_layer_without_a_gpu():
    """Config's defaults keep the point map; make_mapper refuses an unknown map and TsdfMapper refuses the point map's switches before
    it touches a device."""
    from depth_correction_amd import slam
    from depth_correction_amd.config import Config, SLAM
    cfg = Config()
    assert SLAM == ['icp_mapper'] or list(SLAM) == ['icp_mapper']
    assert cfg.slam_map == 'points' and cfg.slam_tsdf_voxel_size == 0.1 and cfg.slam_tsdf_trunc is None and cfg.slam_tsdf_min_count == 1
    assert cfg.slam_tsdf_max_blocks is None and cfg.slam_tsdf_max_residual is None
    cfg.slam_map = 'octree'
    with pytest.raises(ValueError, match='slam_map'):
        slam.make_mapper(cfg)
    for name in ('slam_ct', 'slam_compute_prob_dynamic', 'slam_cut_dynamic'):
        cfg = Config()
        cfg.slam_map = 'tsdf'
        setattr(cfg, name, True)
        with pytest.raises(ValueError, match=name):
            slam.make_mapper(cfg)
    assert slam.LAUNCHES_PER_ITERATION_TSDF == slam.LAUNCHES_PER_ITERATION - 2
