"""Scan-to-TSDF registration on the MI355X (csrc/dc_tsdf_track.hip, slam.TsdfMapper) against tests/tsdf_track_reference.py.

Bars (none is taken from the device's output):
  * sampling (x, value, grad, dist, flag) equal to the oracle to the bit, on the designed cases and on the random posed scene;
  * discrete values (flags, kept flags, counts, status words, iteration counts) equal;
  * a total within (n + 16) 2^-53 sum|term| of the extended-precision sum, n the kept pairs (test_gpu_slam_parity's derived bound);
  * the trimmed threshold within 4 ulp of the rule applied to the device's own distances;
  * pose entries within POSE_BAR per iteration: 2 000 x the largest change of the reference's own poses over 200 random orders of its
    sums on the step-by-step scene, measured on the CPU (DESIGN "Scan-to-TSDF registration" has the figures);
  * after the first iteration the two sides' poses differ by up to POSE_BAR, so a moved point (coordinates below 30 m) by up to
    30 POSE_BAR and, the interpolant being continuous with a slope of at most 2 (tau / a) sqrt(3) in metres per metre, a sampled
    distance by up to 2 (tau / a) sqrt(3) 30 POSE_BAR.
Every step also asserts the reference's margins: no discrete decision compared sits within 1e-9 of its threshold.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import slam_reference as R  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
import tsdf_track_cases as C  # noqa: E402
import tsdf_track_reference as T  # noqa: E402
from helpers import slam_pose as _pose  # noqa: E402
from tsdf_sparse_cases import RANDOM, random_scans  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
POSE_BAR = 2000 * C.POSE_SENSITIVITY     # 3.47e-15: see tsdf_track_cases and DESIGN
MARGIN_FLOOR = 1e-9
WORST = dict(pose=0.0, thr_ulp=0.0, totals=0.0)
CASES = {name: rest for name, *rest in C.sample_cases()}


@pytest.fixture(scope='module', autouse=True)
def _report_largest_deviations():
    for key in WORST:
        WORST[key] = 0.0
    yield
    print('\nlargest device - reference deviation over the tests that ran: pose entry %.3g (bar %.3g), threshold %.3g ulp (bar 4), '
          'totals %.3g of their bound' % (WORST['pose'], POSE_BAR, WORST['thr_ulp'], WORST['totals']))


def up(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)), device=DEV)


def _np(x):
    return x.detach().cpu().numpy()


def device_volume(want):
    """A SparseTsdfVolume holding the oracle volume's table and pool."""
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    vol = SparseTsdfVolume(want.voxel, trunc=want.trunc, origin=want.origin, max_blocks=want.capacity, device=DEV)
    n = want.n_blocks
    vol._keys[:n] = up(want.keys.astype(np.int64))
    vol._slots[:n] = up(want.slots)
    vol._sum.copy_(up(want.sum))
    vol._count.copy_(up(want.count))
    vol._n_blocks[0] = n
    vol._n_host = n
    return vol


def host(sample):
    return {k: _np(v) for k, v in sample.items()}


def assert_same_sample(got, want, what=''):
    for k in ('x', 'value', 'grad', 'dist'):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    assert np.array_equal(got['flag'], want['flag']), (what, 'flag')


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_designed_sampling_cases(name):
    blocks, min_count, points, pose, expected = CASES[name]
    want_vol = C.make_volume(blocks)
    got = host(device_volume(want_vol).sample(points, pose=pose, min_count=min_count))
    assert_same_sample(got, T.sample(want_vol, points, pose, min_count), name)
    if expected is not None:
        assert np.array_equal(got['flag'], expected['flag']) and np.array_equal(got['value'], expected['value'], equal_nan=True), name
        assert np.array_equal(got['grad'], expected['grad']), name


def test_stop_leaves_the_outputs():
    blocks, min_count, points, pose, _ = CASES['linear_inside_one_block']
    want_vol = C.make_volume(blocks)
    vol = device_volume(want_vol)
    out = vol.sample(points)
    for v in out.values():
        v.fill_(5)
    vol.sample(points, stop=torch.ones(1, dtype=torch.int32, device=DEV), out=out)
    assert all(bool((v == 5).all()) for v in out.values())
    vol.sample(points, stop=torch.zeros(1, dtype=torch.int32, device=DEV), out=out)
    assert_same_sample(host(out), T.sample(want_vol, points, None, min_count))
    empty = vol.sample(np.zeros((0, 3)))
    assert empty['flag'].shape == (0,) and empty['x'].shape == (0, 3)


@pytest.fixture(scope='module')
def random_scene():
    """{dtype: (device volume, oracle, queries)} of the random posed scene of the sparse tests (negative blocks), fused once; 5000 query
    points scattered within +-1.5 tau of the scans' end points, some of them NaN."""
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    out = {}
    for dt in (np.float32, np.float64):
        vol = SparseTsdfVolume(RANDOM['voxel'], trunc=RANDOM['trunc'], origin=RANDOM['origin'], device=DEV)
        want = S.SparseVolume(capacity=8, **RANDOM)
        ends = []
        for b in random_scans():
            n = b['dirs'].shape[0]
            c = DepthCloud(up(np.broadcast_to(b['vps'], (n, 3)), dt), up(b['dirs'], dt), up(b['depth'], dt).reshape(n, 1))
            vol.integrate(c, pose=b['pose'], mask=up(b['mask']), min_depth=b['min_depth'], max_range=b['max_range'])
            S.fuse(want, **dict(b, vps=b['vps'].astype(dt), dirs=b['dirs'].astype(dt), depth=b['depth'].astype(dt)))
            with np.errstate(all='ignore'):
                e = np.broadcast_to(b['vps'], (n, 3)) + b['depth'][:, None] * b['dirs']
            e = e[np.isfinite(e).all(axis=1)]
            ends.append(R.moved(b['pose'], e) if b['pose'] is not None else e)
        ends = np.concatenate(ends)
        rng = np.random.default_rng(11)
        q = ends[rng.integers(0, len(ends), 5000)] + rng.uniform(-1.5, 1.5, (5000, 3)) * RANDOM['trunc']
        q[rng.integers(0, 5000, 20)] = np.nan
        out[dt] = (vol, want, q)
    return out


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('posed', [False, True])
def test_random_scene_sampling_equals_oracle(random_scene, dt, posed):
    vol, want, q = random_scene[dt]
    rows = min(vol.capacity, want.capacity)
    assert vol.n_blocks == want.n_blocks <= rows and np.array_equal(_np(vol._sum[:rows]), want.sum[:rows])
    pose = _pose(0.3, (0.05, -0.02, 0.04), roll=0.02, pitch=-0.01) if posed else None
    for min_count in (1, 2):
        ref = T.sample(want, q, pose, min_count)
        got = host(vol.sample(q, pose=pose, min_count=min_count))
        assert_same_sample(got, ref, (dt.__name__, posed, min_count))
    counts = np.bincount(ref['flag'], minlength=3)
    print('random scene %s posed %s: flags %s' % (dt.__name__, posed, counts.tolist()))
    assert counts[0] > 100 and counts[1] >= 15 and counts[2] > 500          # (the oracle's counts: every flag is exercised)


# ---- the row -------------------------------------------------------------------------------------------------------------------------
def _device_row(s, thr, max_residual, status_code=0, fill=None):
    from depth_correction_amd import _native as nv, ops
    m = len(s['flag'])
    d = dict(x=up(s['x']), value=up(s['value']), grad=up(s['grad']), dist=up(s['dist']), flag=up(s['flag'], np.uint8))
    state = torch.zeros(nv.DC_ICP_STATE_COUNT, dtype=torch.float64, device=DEV)
    status = torch.tensor([status_code, 0, 0, 0], dtype=torch.int32, device=DEV)
    partials = torch.full((ops.icp_blocks(m), nv.DC_ICP_PARTIALS), float('nan') if fill is None else fill, dtype=torch.float64, device=DEV)
    kept = torch.full((m,), 7, dtype=torch.uint8, device=DEV)
    ops.tsdf_icp_accumulate(d, up(np.array([thr])), max_residual, state, status, partials, kept=kept)
    return _np(partials), _np(kept)


@pytest.mark.parametrize('m', C.ROW_SIZES)
def test_row_matches_extended_precision(m):
    from depth_correction_amd import ops
    s = C.random_sample(m, seed=m % 97)
    thr = R.quantile_finite(s['dist'], 0.8)
    want = T.totals(s, thr, 0.29)
    partials, kept = _device_row(s, thr, 0.29)
    assert partials.shape[0] == ops.icp_blocks(m) == min(512, (m + 255) // 256)
    assert np.array_equal(kept.astype(bool), want['kept'])
    tot = R.block_sum(partials)
    assert tot[27] == want['n_pairs'] == tot[29]
    bound = C.totals_bound(want['n_pairs'], want['abs_totals'])
    err = np.abs(tot - want['totals'])
    with np.errstate(divide='ignore', invalid='ignore'):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    WORST['totals'] = max(WORST['totals'], worst)
    print('m %d: %d pairs, totals at %.3g of their bound' % (m, want['n_pairs'], worst))
    assert (err <= bound).all(), (m, err, bound)
    again, kept2 = _device_row(s, thr, 0.29)
    assert np.array_equal(partials, again) and np.array_equal(kept, kept2)


def test_row_edges():
    s = C.row_edge_sample()
    partials, kept = _device_row(s, 0.5, 2.0)
    assert kept.tolist() == [1, 1, 0, 0, 0, 0] and np.array_equal(partials[0], C.row_by_hand())
    assert _device_row(s, 10.0, 2.0)[1].tolist() == [1, 1, 1, 0, 0, 0]                 # dist == max_residual is dropped
    assert _device_row(s, 10.0, np.nextafter(2.0, 3.0))[1].tolist() == [1, 1, 1, 1, 0, 0]
    partials, kept = _device_row(s, float('nan'), 2.0)
    assert kept.tolist() == [0] * 6 and not partials.any()
    partials, kept = _device_row(s, 0.5, 2.0, status_code=1, fill=3.0)
    assert (partials == 3.0).all() and (kept == 7).all()
    partials, kept = _device_row({k: v[:0] for k, v in s.items()}, 0.5, 2.0)
    assert partials.shape == (1, 30) and not partials.any() and kept.shape == (0,)


# ---- step by step --------------------------------------------------------------------------------------------------------------------
STEP = C.STEP
OFFSET = _pose(0.03, (0.1, -0.05, 0.02))                          # test_gpu_slam_parity's; 0.36 m at the far wall, inside the truncation


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device='cuda:0', float_type='float64', min_depth=0.0, max_depth=float('inf'), grid_res=0.0, nn_k=0, nn_r=0.25, slam_map='tsdf')
    base.update(kw)
    return Config(**base)


class _Scene(object):
    """Six RoomBoxDataset scans prepared once on the device with their host copies; scans 0, 1 and 3 are fused at the ground truth."""

    def __init__(self):
        from depth_correction_amd.dataset import RoomBoxDataset
        from depth_correction_amd.slam import TsdfMapper, mapper_input
        self.cfg = _cfg(**STEP)
        ds = RoomBoxDataset(n_pts=20000, n_poses=6, dtype=np.float64)
        mapper = TsdfMapper(self.cfg)
        self.dev = [mapper.prepare(mapper_input(cloud, None, self.cfg)) for cloud, _ in ds]
        self.host = [dict(points=_np(s.points), vps=_np(s.vps), dirs=_np(s.dirs), depth=_np(s.depth).reshape(-1)) for s in self.dev]
        self.gt = np.stack([pose for _, pose in ds])
        self.prm = T.params(self.cfg)
        self.volume = T.new_volume(self.prm)
        for i in C.STEP_FUSED:
            S.fuse(self.volume, vps=self.host[i]['vps'], dirs=self.host[i]['dirs'], depth=self.host[i]['depth'], pose=self.gt[i],
                   max_range=self.prm.slam_sensor_max_range)

    def mapper(self, cfg=None, status_every=4):
        from depth_correction_amd.slam import TsdfMapper
        mapper = TsdfMapper(cfg or self.cfg, status_every=status_every)
        for i in C.STEP_FUSED:
            assert mapper.update(self.dev[i], self.gt[i]) == len(self.dev[i])
        return mapper


@pytest.fixture(scope='module')
def scene():
    return _Scene()


def _ulps(a, b):
    if math.isnan(a) and math.isnan(b):
        return 0.0
    return abs(a - b) / np.spacing(abs(b))


def test_fused_volume_equals_oracle(scene):
    vol, want = scene.mapper().volume, scene.volume
    n = want.n_blocks
    assert vol.n_blocks == n and np.array_equal(_np(vol._keys[:n]).astype(np.uint64), want.keys)
    m = min(vol.capacity, want.capacity)
    assert np.array_equal(_np(vol._sum[:m]), want.sum[:m]) and np.array_equal(_np(vol._count[:m]), want.count[:m])


def test_step_by_step_matches_reference(scene):
    from depth_correction_amd import _native as nv
    mapper = scene.mapper()
    cfg, prm, vol = scene.cfg, scene.prm, scene.volume
    scan_d, p = scene.dev[2], scene.host[2]['points']
    prior = scene.gt[2] @ OFFSET
    from depth_correction_amd import ops
    buf = mapper.buffers(len(scan_d))
    buf['thr'].fill_(-7.0)
    kept = torch.empty((len(scan_d),), dtype=torch.uint8, device=DEV)
    ops.icp_init(up(prior), mapper.state, mapper.status)
    pose_d = mapper.state[:16].view(4, 4)
    st = R.new_state(prior)
    slope = 2.0 * (vol.trunc / vol.voxel) * math.sqrt(3.0)
    it = 0
    while True:
        mapper.iteration(scan_d, pose_d, buf, kept=kept)
        torch.cuda.synchronize()
        rec = T.iteration(vol, p, st, prm)
        it += 1
        state, status = _np(mapper.state), _np(mapper.status)
        got = host({k: buf[k] for k in ('x', 'value', 'grad', 'dist', 'flag')})
        d_thr, d_kept = float(buf['thr'].item()), _np(kept).astype(bool)
        m = rec.margins
        assert min(m['thr'], m['max_residual'], m['cell'], m.get('conv_rot', 1.0), m.get('conv_trans', 1.0)) >= MARGIN_FLOOR, (it, m)
        assert np.array_equal(got['flag'], rec.sample['flag']), (it, int((got['flag'] != rec.sample['flag']).sum()))
        ok = rec.sample['flag'] == 0
        if it == 1:                                    # the same pose on both sides: the same sample to the bit
            assert_same_sample(got, rec.sample, it)
            assert _ulps(d_thr, rec.thr) <= 4, (it, d_thr, rec.thr)
        else:
            np.testing.assert_allclose(got['x'], rec.sample['x'], rtol=0, atol=30 * POSE_BAR)
            np.testing.assert_allclose(got['value'][ok], rec.sample['value'][ok], rtol=0, atol=slope * 30 * POSE_BAR)
            assert abs(d_thr - rec.thr) <= slope * 30 * POSE_BAR, (it, d_thr, rec.thr)
        own = _ulps(d_thr, R.quantile_finite(got['dist'], cfg.icp_trim_ratio))
        WORST['thr_ulp'] = max(WORST['thr_ulp'], own)
        assert own <= 4, (it, d_thr)
        assert np.array_equal(d_kept, rec.kept), (it, int((d_kept != rec.kept).sum()))
        ref = T.totals(got, d_thr, mapper.max_residual)             # extended precision at the device's own sample and threshold
        tot = R.block_sum(_np(buf['partials']))
        bound = C.totals_bound(ref['n_pairs'], ref['abs_totals'])
        err = np.abs(tot - ref['totals'])
        with np.errstate(divide='ignore', invalid='ignore'):
            WORST['totals'] = max(WORST['totals'], float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), (it, err, bound)
        assert tot[27] == ref['n_pairs'] == rec.pairs == tot[29]
        assert status[1] == rec.iters == it and status[0] == rec.code, (it, status, rec.code)
        dpose = np.abs(state[:16].reshape(4, 4) - rec.pose).max()
        WORST['pose'] = max(WORST['pose'], dpose)
        print('iteration %d: %d pairs, threshold %.4f, pose deviation %.3g, margins thr %.2e cell %.2e' % (it, rec.pairs, rec.thr, dpose,
                                                                                                          m['thr'], m['cell']))
        assert dpose <= POSE_BAR, (it, dpose)
        assert state[nv.DC_ICP_STATE_PAIRS] == rec.pairs and state[nv.DC_ICP_STATE_OVERLAP] == rec.overlap
        assert np.array_equal(state[16:32].reshape(4, 4), prior)
        if status[0] != 0:
            break
        assert it < 60
    assert status[0] == R.CONVERGED and it > cfg.icp_smooth_length
    e_prior, e_pose = np.abs(prior - scene.gt[2]).max(), np.abs(rec.pose - scene.gt[2]).max()
    print('registered from %.3f to %.4f of the ground truth in %d iterations' % (e_prior, e_pose, it))
    assert e_pose < 0.1 * e_prior


# ---- registration --------------------------------------------------------------------------------------------------------------------
def test_status_every_changes_only_the_host_reads(scene):
    prior = scene.gt[2] @ OFFSET
    results = []
    for every in (1, 4, 100):
        pose, info = scene.mapper(status_every=every).register(scene.dev[2], prior)
        results.append((pose, info))
        assert info['ok'] and info['launches_per_iteration'] == 21
        assert info['host_reads'] == (info['iterations'] + every - 1) // every if every < 100 else info['host_reads'] == 1
    for pose, info in results[1:]:
        assert np.array_equal(pose, results[0][0])
        assert {k: v for k, v in info.items() if k != 'host_reads'} == {k: v for k, v in results[0][1].items() if k != 'host_reads'}
    ref = T.register(scene.volume, scene.host[2]['points'], prior, scene.prm)
    assert results[0][1]['status'] == ref.status and results[0][1]['iterations'] == ref.iterations and results[0][1]['pairs'] == ref.pairs


def test_failure_paths_keep_prior_and_volume(scene):
    from depth_correction_amd.slam import TsdfMapper
    prior = scene.gt[2] @ OFFSET
    empty = TsdfMapper(scene.cfg)
    pose, info = empty.register(scene.dev[2], prior)                       # an empty volume: the first scan initialises the map
    assert info['status'] == 'init' and info['ok'] and np.array_equal(pose, prior) and empty.n_map == 0
    mapper = scene.mapper()
    vol = mapper.volume
    before = [t.clone() for t in (vol._keys, vol._slots, vol._sum, vol._count, vol._n_blocks)]
    pose, info = mapper.register(np.zeros((0, 3)), prior)
    assert info['status'] == 'empty' and not info['ok'] and np.array_equal(pose, prior)
    far = prior.copy()
    far[:3, 3] += 500.0                                                     # a scan wholly outside the volume: no valid sample
    pose, info = mapper.register(scene.dev[2], far)
    assert info['status'] == 'too_few_pairs' and not info['ok'] and info['pairs'] == 0 and np.array_equal(pose, far), info
    assert all(torch.equal(a, b) for a, b in zip(before, (vol._keys, vol._slots, vol._sum, vol._count, vol._n_blocks)))
    pts, nrm = mapper.map_points()
    assert pts.shape == nrm.shape and pts.shape[0] > 1000
    norms = torch.linalg.norm(nrm, dim=1)
    assert bool(((norms - 1.0).abs() < 1e-12)[norms > 0].all()) and float((norms > 0).double().mean()) > 0.5
    mapper.clear()
    assert mapper.n_map == 0


def test_refused_switches():
    from depth_correction_amd.slam import make_mapper, run_slam
    for name in ('slam_ct', 'slam_compute_prob_dynamic', 'slam_cut_dynamic'):
        with pytest.raises(ValueError, match=name):
            make_mapper(_cfg(**{name: True}))
        with pytest.raises(ValueError, match=name):
            run_slam([], None, _cfg(**{name: True}))
    assert type(make_mapper(_cfg(slam_map='points'))).__name__ == 'IcpMapper'
    assert type(make_mapper(_cfg(slam_deskew=True))).__name__ == 'TsdfMapper'


# ---- run_slam on the pillared room of test_gpu_slam.py ---------------------------------------------------------------------------------
ROOM = dict(slam_tsdf_voxel_size=0.1, slam_tsdf_trunc=0.3)


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = tmp_path_factory.mktemp('tsdf_slam') / 'pillared_room.ply'
    mesh.save_ply(str(path))
    return str(path), mesh


def _room_cfg(**kw):
    base = dict(min_depth=0.5, max_depth=25.0, grid_res=0.1, **ROOM)
    base.update(kw)
    return _cfg(**base)


def _dataset(path, n=24, size=(64, 512)):
    from depth_correction_amd.dataset import RenderedMeshDataset
    poses = np.stack([_pose(0.04 * i, (-3.0 + 0.25 * i, 0.3 * math.sin(i / 3.0), 0.02 * math.sin(i / 2.0))) for i in range(n)])
    return RenderedMeshDataset(path, poses=poses, size=size, fov=(45.0, 360.0), num_segments=16, device='cuda:0')


def test_sequence_odometry_noise(room):
    from depth_correction_amd.metrics import reconstruction_accuracy
    from depth_correction_amd.slam import make_mapper, run_slam, slam_errors
    path, gt_mesh = room
    cfg = _room_cfg(odom_cov=[1e-4] * 3 + [2.5e-3] * 3)
    ds = _dataset(path)
    mapper = make_mapper(cfg)
    res = run_slam(ds, None, cfg, mapper=mapper)
    e_slam = slam_errors(res['slam'], res['gt'], res['path_lengths'])
    e_odom = slam_errors(res['odom'], res['gt'], res['path_lengths'])
    overlaps = [i['overlap'] for i in res['info'][1:]]
    print('tsdf slam', e_slam, 'odom', e_odom, 'ratio %.3f / %.3f' % (e_slam[0] / e_odom[0], e_slam[1] / e_odom[1]),
          [i['status'] for i in res['info']], [i['iterations'] for i in res['info']], 'median overlap %.3f' % np.median(overlaps),
          '%d blocks' % mapper.n_map)
    assert all(i['ok'] for i in res['info']), [i['status'] for i in res['info']]
    assert e_slam[0] < e_odom[0] and e_slam[1] < e_odom[1], (e_slam, e_odom)
    assert np.median(overlaps) >= 0.5
    again = run_slam(ds, None, cfg)
    assert np.array_equal(res['slam'], again['slam'])
    acc = reconstruction_accuracy(mapper.extract_mesh(), gt_mesh, n_samples=20000)
    print('mesh of the final volume against the ground truth:', {k: acc[k] for k in ('accuracy', 'completeness')})


def test_eval_slam_files(room, tmp_path):
    from depth_correction_amd.eval import eval_slam
    from depth_correction_amd.scan_io import read_poses_csv
    ds = _dataset(room[0], n=5)
    cfg = _room_cfg(slam_eval_csv=str(tmp_path / 'eval.csv'), slam_poses_csv=str(tmp_path / 'seq' / 'slam_poses_icp_mapper.csv'))
    res = eval_slam(cfg, test_datasets=[ds], model=None)
    lines = open(cfg.slam_eval_csv).read().splitlines()
    assert len(lines) == 1 and lines[0].split(' ')[0] == str(ds) and len(lines[0].split(' ')) == 5
    ids, poses = read_poses_csv(cfg.slam_poses_csv)
    assert ids == list(range(5))
    np.testing.assert_allclose(np.stack(poses), res[0]['slam'], atol=1e-8)
    assert all(i['launches_per_iteration'] == 21 for i in res[0]['info'])
