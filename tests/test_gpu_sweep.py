"""Moving-sweep lidar on the GPU: dc_sweep_rays, dc_raycast_sweep and dc_deskew against the thin cast and the numpy restatement
(tests/sweep_reference.py), then the rendered dataset, preproc.deskew_cloud, DeskewedDataset and run_slam's constant-velocity de-skew
end to end against the mesh."""
import math

import numpy as np
import pytest
import torch

import sweep_reference as R
from helpers import slam_pose

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -52
COUNTS = (180, 0, 120)                     # 300 rays: one scan empty, no multiple of the cast's block of 128
T_MIN = 0.05


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _same(a, b):
    """torch.equal with the NaNs matched."""
    if a.dtype.is_floating_point:
        return bool(torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))
    return bool(torch.equal(a, b))


@pytest.fixture(scope='module')
def scene():
    """The box room with its tessellated wall and three scans of rays from inside it: view points N(0, 0.1), directions that are not
    unit, sweep times in [-0.2, 1), twists of about 0.5 m and 0.3 rad."""
    mesh = R.standard_scene()
    assert mesh.faces.shape[0] == 212
    rng = np.random.default_rng(21)
    n = sum(COUNTS)
    poses = np.stack([slam_pose(rng.uniform(-math.pi, math.pi), rng.uniform(-1.0, 1.0, size=3) * (2.0, 1.5, 0.5), roll=rng.uniform(-0.3, 0.3),
                                pitch=rng.uniform(-0.3, 0.3)) for _ in COUNTS])
    axis = rng.normal(size=(len(COUNTS), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    twists = np.concatenate([rng.normal(size=(len(COUNTS), 3)) * 0.3, 0.3 * axis], axis=1)
    return dict(mesh=mesh, bvh=mesh.on_device(DEV)[3], n=n, off=np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64),
                poses=_dev(poses), twists=twists, vps=rng.normal(scale=0.1, size=(n, 3)),
                dirs=rng.normal(size=(n, 3)) * rng.uniform(0.3, 3.0, size=(n, 1)), tau=rng.uniform(-0.2, 1.0, size=n),
                scan=np.repeat(np.arange(len(COUNTS)), COUNTS))


# ---- 1. zero motion is the thin cast ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_zero_motion_is_the_thin_cast(scene, dtype):
    from depth_correction_amd import ops
    vps, dirs = _dev(scene['vps'], dtype), _dev(scene['dirs'], dtype)
    thin = ops.raycast_rays(scene['bvh'], vps, dirs, scene['off'], scene['poses'], t_min=T_MIN)
    assert int((thin[0] >= 0).sum()) >= 0.9 * scene['n']
    still = ops.raycast_sweep(scene['bvh'], vps, dirs, _dev(scene['tau']), scene['off'], scene['poses'], np.zeros_like(scene['twists']),
                              t_min=T_MIN)
    start = ops.raycast_sweep(scene['bvh'], vps, dirs, torch.zeros(scene['n'], dtype=torch.float64, device=DEV), scene['off'],
                              scene['poses'], scene['twists'], t_min=T_MIN)
    for got in (still, start):
        assert got[0].dtype == torch.int32 and got[1].dtype == got[2].dtype == torch.float64
        for a, b in zip(got, thin):
            assert _same(a, b)
    # no rays: nothing is launched
    none = ops.raycast_sweep(scene['bvh'], vps[:0], dirs[:0], _dev(scene['tau'][:0]), [0, 0, 0, 0], scene['poses'], scene['twists'])
    assert [tuple(x.shape) for x in none] == [(0,), (0,), (0,)]


# ---- 2. fused equals composed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('cull', [True, False])
def test_fused_equals_composed(scene, cull, dtype):
    """raycast_sweep = raycast_rays on sweep_rays' rays, bit for bit, with per-ray near clips (raycast_rays takes one clip per call: the
    rays alternate between two clips and each takes its own call's answer), and again on a second run.  Three rays have sweep times
    that are not finite: NaN rays from sweep_rays, misses from both casts."""
    from depth_correction_amd import ops
    n = scene['n']
    vps, dirs = _dev(scene['vps'], dtype), _dev(scene['dirs'], dtype)
    tau_h = scene['tau'].copy()
    tau_h[[5, 200, 299]] = [float('nan'), float('inf'), -float('inf')]
    tau = _dev(tau_h)
    clips = (T_MIN, 0.8)
    which = np.arange(n) % 2
    t_min = _dev(np.asarray(clips)[which])
    fused = ops.raycast_sweep(scene['bvh'], vps, dirs, tau, scene['off'], scene['poses'], scene['twists'], t_min=t_min, cull=cull)
    o, D = ops.sweep_rays(vps, dirs, tau, scene['off'], scene['twists'])
    assert o.dtype == D.dtype == torch.float64 and o.shape == D.shape == (n, 3)
    per_clip = [ops.raycast_rays(scene['bvh'], o, D, scene['off'], scene['poses'], t_min=c, cull=cull) for c in clips]
    pick = _dev(which).bool()
    composed = [torch.where(pick, b, a) for a, b in zip(*per_clip)]
    for a, b in zip(fused, composed):
        assert _same(a, b)
    bad = [5, 200, 299]
    assert torch.isnan(o[bad]).all() and torch.isnan(D[bad]).all()
    assert (fused[0][bad] == -1).all() and torch.isinf(fused[1][bad]).all() and (fused[1][bad] > 0).all() and torch.isnan(fused[2][bad]).all()
    # the two clips and the motion both matter here: some rays change their answer with either
    assert not _same(per_clip[0][1], per_clip[1][1])
    thin = ops.raycast_rays(scene['bvh'], vps, dirs, scene['off'], scene['poses'], t_min=T_MIN, cull=cull)
    assert not _same(thin[1], per_clip[0][1])
    hit = fused[0] >= 0
    assert int(hit.sum()) >= 0.5 * n and (torch.isfinite(fused[2][hit])).all()
    again = ops.raycast_sweep(scene['bvh'], vps, dirs, tau, scene['off'], scene['poses'], scene['twists'], t_min=t_min, cull=cull)
    for a, b in zip(fused, again):
        assert _same(a, b)
    # a scalar clip goes the same way
    one = ops.raycast_sweep(scene['bvh'], vps, dirs, tau, scene['off'], scene['poses'], scene['twists'], t_min=0.8, cull=cull)
    for a, b in zip(one, per_clip[1]):
        assert _same(a, b)


# ---- 3. the kernels against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_kernels_against_numpy(scene, dtype):
    """sweep_rays and deskew within 34 * 2^-52 (|x| + |tau v|) of the longdouble restatement per component; de-skewing keeps the depth
    within 8 * 2^-52 (|x| + |vp|)."""
    from depth_correction_amd import _native as nv
    from depth_correction_amd import ops
    n = scene['n']
    vps_d, dirs_d, tau_d = _dev(scene['vps'], dtype), _dev(scene['dirs'], dtype), _dev(scene['tau'])
    vps, dirs = vps_d.double().cpu().numpy(), dirs_d.double().cpu().numpy()        # fp32 inputs are converted exactly
    tw = scene['twists'][scene['scan']]
    o, D = (x.cpu().numpy() for x in ops.sweep_rays(vps_d, dirs_d, tau_d, scene['off'], scene['twists']))
    for got, src, k in ((o, vps, 0), (D, dirs, 1)):
        want = R.apply(src, scene['tau'], tw)[k]
        err = np.abs(got.astype(R.LD) - want).astype(np.float64)
        print('sweep_rays %s: max error %.2f x 2^-52 (|x| + |tau v|)' % ('origin direction'.split()[k], (err / (R.bound(src, scene['tau'], tw) / R.BOUND_ULPS)).max()))
        assert (err <= R.bound(src, scene['tau'], tw)).all()
    # de-skew: the directions stand in for points (metres), the view points as they are, unit normals
    nrm_h = np.random.default_rng(2).normal(size=(n, 3))
    nrm_d = _dev(nrm_h / np.linalg.norm(nrm_h, axis=1, keepdims=True), dtype)
    nrm = nrm_d.double().cpu().numpy()
    x1, v1, m1 = (a.cpu().numpy() for a in ops.deskew(dirs_d, tau_d, scene['off'], scene['twists'], vps=vps_d, normals=nrm_d))
    for name, got, src, k in (('points', x1, dirs, 0), ('vps', v1, vps, 0), ('normals', m1, nrm, 1)):
        want = R.apply(src, scene['tau'], tw)[k]
        err = np.abs(got.astype(R.LD) - want).astype(np.float64)
        print('deskew %s: max error %.2f x 2^-52 (|x| + |tau v|)' % (name, (err / (R.bound(src, scene['tau'], tw) / R.BOUND_ULPS)).max()))
        assert (err <= R.bound(src, scene['tau'], tw)).all()
    rigid = np.abs(np.linalg.norm(x1 - v1, axis=1) - np.linalg.norm(dirs - vps, axis=1))
    print('deskew: max change of depth %.2f x 2^-52 (|x| + |vp|)' % (rigid / (EPS * (np.linalg.norm(dirs, axis=1) + np.linalg.norm(vps, axis=1)))).max())
    assert (rigid <= 8 * EPS * (np.linalg.norm(dirs, axis=1) + np.linalg.norm(vps, axis=1))).all()
    # points alone; no points at all
    only = ops.deskew(dirs_d, tau_d, scene['off'], scene['twists'])
    assert only[1] is None and only[2] is None and np.array_equal(only[0].cpu().numpy(), x1)
    empty = ops.deskew(dirs_d[:0], tau_d[:0], [0, 0, 0, 0], scene['twists'], vps=vps_d[:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2] is None
    if dtype == torch.float64:                                                  # in place: the outputs are the inputs
        xs, vs, ms = dirs_d.clone(), vps_d.clone(), nrm_d.clone()
        off = _dev(scene['off'])
        twd = _dev(scene['twists'])
        nv.check(nv.lib().dc_deskew(nv.ptr(xs), nv.ptr(vs), nv.ptr(ms), nv.DC_F64, nv.ptr(tau_d), n, nv.ptr(off), nv.ptr(twd), len(COUNTS),
                                    nv.ptr(xs), nv.ptr(vs), nv.ptr(ms), nv.stream_ptr()), 'dc_deskew')
        assert np.array_equal(xs.cpu().numpy(), x1) and np.array_equal(vs.cpu().numpy(), v1) and np.array_equal(ms.cpu().numpy(), m1)


# ---- 4. the rendered dataset and the round trip -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def room_file(tmp_path_factory):
    path = tmp_path_factory.mktemp('sweep') / 'room.ply'
    R.standard_scene().save_ply(str(path))
    return str(path)


def _posed(cloud, pose):
    pts = np.stack([cloud[f] for f in 'xyz'], axis=1)
    return _dev(pts @ pose[:3, :3].T + pose[:3, 3])


def _mesh_distance(ds, cloud, pose):
    from depth_correction_amd.metrics import point_to_mesh_distance
    return point_to_mesh_distance(_posed(cloud, pose), ds.get_mesh()).cpu().numpy()


def test_round_trip(room_file):
    """A scan taken under a twist of 0.5 m and 0.2 rad, de-skewed with that twist and posed by the dataset's pose, lies on the mesh
    (1e-9 m); posed as it is, it does not: the last column was taken 0.5 m and 0.2 rad from the pose, which moves a point on a wall 3
    to 5 m away by decimetres (the test asks for 1 cm)."""
    from depth_correction_amd.dataset import RenderedMeshDataset
    from depth_correction_amd.preproc import deskew_cloud
    from depth_correction_amd.render import SweepModel, lidar_directions
    twist = np.array([0.4, 0.3, 0.0, 0.0, 0.0, 0.2])
    assert abs(np.linalg.norm(twist[:3]) - 0.5) < 1e-12
    pose = slam_pose(0.4, (-0.5, 0.2, 0.1))
    kw = dict(poses=pose[None], size=(16, 64), fov=(45.0, 360.0), num_segments=16, device=DEV)
    ds = RenderedMeshDataset(room_file, sweep=SweepModel(twists=twist[None]), **kw)
    raw, T = ds[0]
    n_rays = lidar_directions(size=(16, 64), fov=(45.0, 360.0), num_segments=16)[0].shape[0]
    assert raw.dtype == ds.cloud_dtype and raw.dtype.names[-1] == 't' and np.array_equal(T, pose)
    assert len(raw) >= 0.9 * n_rays
    assert (raw['t'] >= 0).all() and (raw['t'] < 1).all() and np.ptp(raw['t']) > 0.9
    assert (raw['vp_x'] == 0).all() and (raw['vp_y'] == 0).all() and (raw['vp_z'] == 0).all()
    flat = deskew_cloud(raw, twist, device=DEV)
    assert flat.dtype == raw.dtype and np.array_equal(flat['t'], raw['t'])
    d_flat, d_raw = _mesh_distance(ds, flat, pose), _mesh_distance(ds, raw, pose)
    print('round trip: %d of %d rays hit; distance to the mesh de-skewed max %.3g m, raw max %.3g m' % (len(raw), n_rays, d_flat.max(), d_raw.max()))
    assert d_flat.max() <= 1e-9
    assert d_raw.max() > 0.01
    # the de-skewed view point is where the sensor stood: tau v in the pose's frame; depth and incidence angle are kept
    np.testing.assert_allclose(np.stack([flat['vp_x'], flat['vp_y'], flat['vp_z']], 1), raw['t'][:, None] * twist[None, :3], rtol=0, atol=1e-15)
    ray_raw = np.stack([raw[f] for f in 'xyz'], 1)
    ray_flat = np.stack([flat[f] - flat['vp_' + f] for f in 'xyz'], 1)
    np.testing.assert_allclose(np.linalg.norm(ray_flat, axis=1), np.linalg.norm(ray_raw, axis=1), rtol=1e-14)
    n_raw, n_flat = (np.stack([c['normal_' + f] for f in 'xyz'], 1) for c in (raw, flat))
    np.testing.assert_allclose((n_flat * ray_flat).sum(1), (n_raw * ray_raw).sum(1), rtol=0, atol=1e-13)
    # the de-skewed normals are the mesh's face normals in the pose's frame: axis-aligned in the world
    n_world = n_flat @ pose[:3, :3].T
    assert np.abs(np.abs(n_world).max(axis=1) - 1.0).max() <= 1e-14
    # points plus times
    pts = deskew_cloud((ray_raw, raw['t']), twist, device=DEV)
    assert np.array_equal(pts, np.stack([flat[f] for f in 'xyz'], 1))
    # no motion: the sweep renders what the thin renderer does, plus t
    still = RenderedMeshDataset(room_file, sweep=SweepModel(twists=np.zeros((1, 6))), **kw)[0][0]
    thin = RenderedMeshDataset(room_file, **kw)[0][0]
    assert len(still) == len(thin)
    for f in 'xyz':
        np.testing.assert_allclose(still[f], thin[f], rtol=0, atol=1e-12)
        np.testing.assert_allclose(still['normal_' + f], thin['normal_' + f], rtol=0, atol=1e-15)


@pytest.mark.parametrize('ref', [0.0, 0.5])
def test_deskewed_dataset(room_file, ref):
    """Four poses of a constant-twist trajectory, the twists taken from the poses: every de-skewed cloud is on the mesh."""
    from depth_correction_amd.dataset import DeskewedDataset, RenderedMeshDataset
    from depth_correction_amd.render import SweepModel
    twist = np.array([0.3, 0.1, 0.02, 0.01, -0.02, 0.15])
    poses = R.constant_twist_poses(slam_pose(-0.3, (-1.0, -0.5, 0.0)), twist, 4)
    raw = RenderedMeshDataset(room_file, poses=poses, size=(16, 64), fov=(45.0, 360.0), num_segments=16, device=DEV, sweep=SweepModel(ref=ref))
    ds = DeskewedDataset(raw, ref=ref)
    np.testing.assert_allclose(ds.twists, np.tile(twist, (4, 1)), rtol=0, atol=1e-13)
    assert len(ds) == 4
    worst_raw = 0.0
    for i, (cloud, pose) in enumerate(ds):
        assert np.array_equal(pose, poses[i]) and cloud.dtype == raw.cloud_dtype and len(cloud) >= 0.9 * 16 * 64
        d = _mesh_distance(raw, cloud, pose)
        worst_raw = max(worst_raw, _mesh_distance(raw, raw[i][0], pose).max())
        assert d.max() <= 1e-9, (i, d.max())
    assert worst_raw > 0.01
    by_id = ds.local_cloud(2)
    assert np.array_equal(by_id, ds[2][0])


# ---- 5. SLAM ----------------------------------------------------------------------------------------------------------------------------
def test_slam_deskew(tmp_path):
    """Six scans of a constant-twist arc through the pillared room, 16 x 256 rays, exact odometry.  Every registration is ok with and
    without de-skewing, and de-skewing at least halves the mean translation error.  Measured on the MI355X: 1.8 mm de-skewed, 13 mm
    raw, 3.1 mm for the same trajectory rendered without a sweep; all 18 registrations converged."""
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import RenderedMeshDataset
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import SweepModel
    from depth_correction_amd.slam import run_slam, slam_errors
    path = str(tmp_path / 'pillared_room.ply')
    room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))]).save_ply(path)
    twist = np.array([0.25, 0.05, 0.0, 0.0, 0.0, 0.08])
    poses = R.constant_twist_poses(slam_pose(0.0, (-1.5, -0.3, 0.0)), twist, 6)
    kw = dict(poses=poses, size=(16, 256), fov=(45.0, 360.0), num_segments=16, device=DEV)
    moving = RenderedMeshDataset(path, sweep=SweepModel(), **kw)
    static = RenderedMeshDataset(path, **kw)
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25, odom_cov=[0.0] * 6)
    errs = {}
    for name, ds, deskew in (('de-skewed', moving, True), ('raw', moving, False), ('no sweep', static, False)):
        res = run_slam(ds, None, Config(slam_deskew=deskew, **base))
        errs[name] = slam_errors(res['slam'], res['gt'], res['path_lengths'])[1]
        print('%s: mean translation error %.3g m, status %s' % (name, errs[name], [i['status'] for i in res['info']]))
        assert all(i['ok'] for i in res['info']), (name, [i['status'] for i in res['info']])
    assert errs['de-skewed'] < 0.5 * errs['raw'], errs
