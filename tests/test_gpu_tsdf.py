"""Surface reconstruction on the GPU: dc_tsdf_integrate / dc_tsdf_extract_* through reconstruction.TsdfVolume against the numpy oracle
tests/tsdf_reference.py, bit for bit -- on the designed cases of tests/tsdf_cases.py, on a random scene and on a rendered pillared room
--, reproducibility under ray order, the empty cases, and the layers above: reconstruct, metrics.reconstruction_accuracy, eval_recon.

Figures (printed by the tests): the end-to-end room at voxel 0.1 m and the effect of the correction are recorded in DESIGN "Surface
reconstruction".
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cases as C  # noqa: E402
import tsdf_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def device_volume(volume):
    from depth_correction_amd.reconstruction import TsdfVolume
    return TsdfVolume(volume['origin'], volume['dims'], volume['voxel'], trunc=volume['trunc'], device=DEV)


def cloud_of(b, dtype=None):
    """The DepthCloud of one batch of tsdf_cases (numpy arrays in the sensor frame)."""
    from depth_correction_amd.depth_cloud import DepthCloud
    dt = b['dirs'].dtype if dtype is None else dtype
    n = b['dirs'].shape[0]
    up = lambda a: torch.as_tensor(np.array(a, dtype=dt), device=DEV)
    return DepthCloud(up(np.broadcast_to(b['vps'], (n, 3))), up(b['dirs']), up(b['depth']).reshape(n, 1))


def integrate_both(vol, want, b, dtype=None):
    """One batch into the device volume and into the oracle's; the device's stats of the call."""
    kw = dict(pose=b['pose'], mask=None if b['mask'] is None else torch.as_tensor(b['mask'], device=DEV), min_depth=b['min_depth'],
              max_range=b['max_range'], carve_from=b['carve_from'])
    stats = vol.integrate(cloud_of(b, dtype), **kw)
    if dtype is not None:
        b = dict(b, vps=b['vps'].astype(dtype), dirs=b['dirs'].astype(dtype), depth=b['depth'].astype(dtype))
    R.integrate(want, **b)
    return stats


def assert_same_volume(vol, want, what=''):
    assert np.array_equal(vol.sums().cpu().numpy().ravel(), want.sum), what
    assert np.array_equal(vol.counts().cpu().numpy().ravel(), want.count), what
    assert list(vol.stats().values()) == want.stats.tolist(), what


def assert_same_mesh(vol, want, min_count, what=''):
    v, f = vol.extract(min_count)
    wv, wf = R.extract(want, min_count)
    assert v.dtype == torch.float64 and f.dtype == torch.int32
    assert tuple(v.shape) == wv.shape and tuple(f.shape) == wf.shape, (what, tuple(v.shape), wv.shape, tuple(f.shape), wf.shape)
    assert np.array_equal(v.cpu().numpy(), wv) and np.array_equal(f.cpu().numpy(), wf), what
    return wv, wf


INTEGRATION = {name: (vol, batches) for name, vol, batches in C.integration_cases()}
EXTRACTION = {name: rest for name, *rest in C.extraction_cases()}


@pytest.mark.parametrize('name', sorted(INTEGRATION))
def test_designed_integration_cases(name):
    volume, batches = INTEGRATION[name]
    vol, want = device_volume(volume), R.Volume(**volume)
    for b in batches:
        before = want.stats.copy()
        stats = integrate_both(vol, want, b)
        assert list(stats.values()) == (want.stats - before).tolist(), name
    assert_same_volume(vol, want, name)
    assert want.stats[0] > 0


@pytest.mark.parametrize('name', sorted(EXTRACTION))
def test_designed_extraction_cases(name):
    volume, s, c, min_count = EXTRACTION[name]
    vol, want = device_volume(volume), R.Volume(**volume)
    want.sum[:], want.count[:] = s.ravel(), c.ravel()
    vol.sums().copy_(torch.as_tensor(s, device=DEV))
    vol.counts().copy_(torch.as_tensor(c, device=DEV))
    wv, wf = assert_same_mesh(vol, want, min_count, name)
    assert len(wv) > 0


# ---- a random scene: 2 scans of 16 x 64 rays into 24 x 20 x 12 voxels ------------------------------------------------------------
RANDOM_VOLUME = dict(origin=(-1.2, -1.0, -0.6), dims=(24, 20, 12), voxel=0.1, trunc=0.3)


def _pose(yaw, t, roll=0.0, pitch=0.0):
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(roll, pitch, yaw)
    T[:3, 3] = t
    return np.asarray(T, dtype=np.float64)


def random_scans():
    """Organised 16 x 64 scans from inside the grid; depths from 0.2 to 1.6 m, so that some rays end (and some start) outside the 2.4 x
    2.0 x 1.2 m grid; one ray in 11 masked out, a few with a NaN or an infinite depth."""
    rng = np.random.default_rng(20)
    el = np.deg2rad(np.linspace(-40.0, 40.0, 16))[:, None]
    az = np.deg2rad(np.arange(64) * 360.0 / 64)[None, :]
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
    scans = []
    for s, pose in enumerate((_pose(0.3, (0.2, -0.1, 0.05), roll=0.05, pitch=-0.1), _pose(-1.1, (-0.7, 0.6, -0.2), roll=-0.2, pitch=0.15))):
        depth = 0.2 + 1.4 * rng.random(dirs.shape[0])
        depth[rng.integers(0, depth.size, 5)] = np.nan
        depth[rng.integers(0, depth.size, 3)] = np.inf
        d = dirs.copy()
        d[rng.integers(0, depth.size, 4), 1] = np.nan
        vps = np.tile(np.array([[0.01, -0.02, 0.03]]) * (s + 1), (dirs.shape[0], 1))
        mask = (np.arange(depth.size) % 11 != 3).astype(np.uint8)
        scans.append(C.batch(vps, d, depth, pose=pose, mask=mask, min_depth=0.25, max_range=1.5))
    return scans


@pytest.fixture(scope='module')
def random_scene():
    """{dtype: (device volume, oracle volume)} after both scans, computed once and left unchanged."""
    out = {}
    for dt in (np.float32, np.float64):
        vol, want = device_volume(RANDOM_VOLUME), R.Volume(**RANDOM_VOLUME)
        for b in random_scans():
            integrate_both(vol, want, b, dt)
        out[dt] = (vol, want)
    return out


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_random_scene_equals_oracle(random_scene, dt):
    vol, want = random_scene[dt]
    print('random scene %s: stats %s' % (dt.__name__, vol.stats()))
    assert want.stats[1] > 150 and want.stats[2] > 100 and want.stats[3] > 5000          # masked / NaN rays and samples outside exist
    assert_same_volume(vol, want)


@pytest.mark.parametrize('min_count', [1, 2])
def test_random_scene_extraction_equals_oracle(random_scene, min_count):
    vol, want = random_scene[np.float64]
    wv, wf = assert_same_mesh(vol, want, min_count)
    assert len(wv) > 100 and len(wf) > 50
    assert wf.min() >= 0 and wf.max() < len(wv)


def test_ray_order_and_repetition_do_not_change_a_bit(random_scene):
    vol, _ = random_scene[np.float64]
    for trial in range(2):
        again = device_volume(RANDOM_VOLUME)
        for s, b in enumerate(random_scans()):
            if trial:
                perm = np.random.default_rng(s).permutation(b['dirs'].shape[0])
                b = dict(b, vps=b['vps'][perm], dirs=b['dirs'][perm], depth=b['depth'][perm], mask=b['mask'][perm])
            again.integrate(cloud_of(b), pose=b['pose'], mask=torch.as_tensor(b['mask'], device=DEV), min_depth=b['min_depth'],
                            max_range=b['max_range'])
        assert torch.equal(again.sums(), vol.sums()) and torch.equal(again.counts(), vol.counts()), trial
        assert again.stats() == vol.stats()


def test_empty_and_masked_clouds_change_nothing():
    from depth_correction_amd.depth_cloud import DepthCloud
    vol = device_volume(RANDOM_VOLUME)
    empty = DepthCloud(torch.zeros((0, 3), dtype=torch.float64, device=DEV), torch.zeros((0, 3), dtype=torch.float64, device=DEV),
                       torch.zeros((0, 1), dtype=torch.float64, device=DEV))
    assert vol.integrate(empty) == dict(rays_used=0, rays_skipped=0, samples_outside=0, visits=0)
    b = random_scans()[0]
    cloud = cloud_of(b)
    cloud.mask = torch.zeros((len(cloud),), dtype=torch.bool, device=DEV)               # the cloud's own mask is used
    assert vol.integrate(cloud, pose=b['pose']) == dict(rays_used=0, rays_skipped=len(cloud), samples_outside=0, visits=0)
    assert int(vol.sums().abs().sum()) == 0 and int(vol.counts().sum()) == 0
    v, f = vol.extract()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    with pytest.raises(ValueError, match='no surface'):
        vol.extract_mesh()
    vol.integrate(cloud_of(b), pose=b['pose'])
    assert int(vol.counts().sum()) > 0
    vol.reset()
    assert int(vol.counts().sum()) == 0 and vol.stats()['rays_used'] == 0
    assert torch.isnan(vol.values()).all()


def test_arguments_are_checked():
    from depth_correction_amd import ops
    from depth_correction_amd.reconstruction import TsdfVolume
    with pytest.raises(ValueError, match='2\\^31'):
        TsdfVolume.from_bounds((0, 0, 0), (200.0, 200.0, 100.0), 0.05, device=DEV)
    with pytest.raises(ValueError):
        TsdfVolume((0, 0, 0), (1, 4, 4), 0.1, device=DEV)
    vol = device_volume(RANDOM_VOLUME)
    b = random_scans()[0]
    c = cloud_of(b)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.sums(), vol.counts(), vol._stats, vol.origin, vol.voxel_size, 0.0, c.vps, c.dirs, c.depth)
    with pytest.raises((ValueError, TypeError)):
        ops.tsdf_integrate(vol.sums(), vol.counts().long(), vol._stats, vol.origin, vol.voxel_size, 0.3, c.vps, c.dirs, c.depth)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(vol.sums(), vol.counts(), vol._stats, vol.origin, vol.voxel_size, 0.3, c.vps, c.dirs, c.depth[:-1])
    with pytest.raises(ValueError):
        ops.tsdf_extract(vol.sums(), vol.counts(), vol.origin, vol.voxel_size, min_count=0)
    assert int(vol.counts().sum()) == 0


# ---- end to end on a rendered pillared room --------------------------------------------------------------------------------------
ROOM_POSES = [(0.2 * i, (-2.0 + 1.3 * i, 0.3 * math.sin(i), 0.1 * i)) for i in range(4)]


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = tmp_path_factory.mktemp('recon') / 'pillared_room.ply'
    mesh.save_ply(str(path))
    return str(path), mesh


def _dataset(path, size):
    from depth_correction_amd.dataset import RenderedMeshDataset
    poses = np.stack([_pose(yaw, t) for yaw, t in ROOM_POSES])
    return RenderedMeshDataset(path, poses=poses, size=size, fov=(45.0, 360.0), num_segments=16, device=DEV)


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    base.update(kw)
    return Config(**base)


def test_rendered_room_end_to_end(room, tmp_path):
    from depth_correction_amd.dataset import RenderedMeshDataset
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.metrics import reconstruction_accuracy
    from depth_correction_amd.reconstruction import reconstruct
    path, gt = room
    ds = _dataset(path, (16, 256))
    clouds, poses = zip(*[(c, p) for c, p in ds])
    assert all(len(c) == 16 * 256 for c in clouds)
    mesh, vol = reconstruct(clouds, poses, 0.1, device=DEV)
    # the same rays through the oracle
    want = R.Volume(vol.origin, vol.dims, vol.voxel_size, vol.trunc)
    for c, p in zip(clouds, poses):
        dc = DepthCloud.from_structured_array(c, dtype=np.float64, device=DEV)
        R.integrate(want, dc.vps.cpu().numpy(), dc.dirs.cpu().numpy(), dc.depth.cpu().numpy(), pose=p)
    assert_same_volume(vol, want)
    assert want.stats[0] == 4 * 16 * 256 and want.stats[3] > 100000
    v, f = mesh.vertices, mesh.faces
    assert len(v) > 1000 and len(f) > 1000 and f.min() >= 0 and f.max() < len(v)
    wv, wf = R.extract(want)
    assert np.array_equal(v, wv) and np.array_equal(f, wf)
    acc = reconstruction_accuracy(mesh, gt, n_samples=50000, max_dist=0.2)
    print('room, 4 x 16 x 256 rays, voxel 0.1: %d vertices, %d faces; accuracy %s; completeness %s; coverage %.4f'
          % (len(v), len(f), acc['accuracy'], acc['completeness'], acc['coverage']))
    for part in ('accuracy', 'completeness'):
        assert acc[part]['n'] == 50000 and all(math.isfinite(acc[part][k]) for k in ('mean', 'rms', 'median', 'trimmed_mean', 'max'))
    assert 0.0 < acc['coverage'] <= 1.0
    # feed-back: the reconstruction is a scene to render from
    ply = str(tmp_path / 'recon.ply')
    mesh.save_ply(ply)
    back = RenderedMeshDataset(ply, poses=np.stack([_pose(0.0, (0.0, 0.0, 0.0))]), size=(16, 128), fov=(45.0, 360.0), num_segments=8, device=DEV)
    cloud, _ = back[0]
    print('feed-back: %d of %d rays hit the reconstruction' % (len(cloud), 16 * 128))
    assert len(cloud) > 16 * 128 // 4


def test_eval_recon_and_the_effect_of_the_correction(room, tmp_path):
    from depth_correction_amd.dataset import DepthBiasDataset
    from depth_correction_amd.eval import eval_recon
    from depth_correction_amd.mesh import read_ply
    from depth_correction_amd.model import ScaledPolynomial
    path, _ = room
    ds = _dataset(path, (32, 512))
    cfg = _cfg(recon_eval_csv=str(tmp_path / 'recon.csv'), recon_mesh_ply=str(tmp_path / 'recon.ply'), recon_eval_samples=50000,
               recon_eval_max_dist=0.2)
    w = 0.05
    biased = DepthBiasDataset(ds, ScaledPolynomial(w=[w], exponent=[2.0], device=DEV), cfg=cfg)
    raw = eval_recon(cfg, test_datasets=[biased], model=None)[0]
    fixed = eval_recon(cfg, test_datasets=[biased], model=ScaledPolynomial(w=[w], exponent=[2.0], device=DEV))[0]
    print('biased, no correction: accuracy %s completeness %s' % (raw['accuracy'], raw['completeness']))
    print('biased, true model:    accuracy %s completeness %s' % (fixed['accuracy'], fixed['completeness']))
    assert fixed['accuracy']['mean'] < raw['accuracy']['mean'], (fixed['accuracy'], raw['accuracy'])
    lines = open(cfg.recon_eval_csv).read().splitlines()
    assert len(lines) == 2 and all(len(line.split(' ')) == 12 and line.split(' ')[0] == str(ds) for line in lines)
    parts = lines[1].split(' ')
    mesh = fixed['mesh']
    assert int(parts[1]) == mesh.vertices.shape[0] and int(parts[2]) == len(mesh)
    assert float(parts[3]) == pytest.approx(fixed['accuracy']['mean'], abs=1e-9)
    vertices, faces = read_ply(cfg.recon_mesh_ply)
    assert len(vertices) == mesh.vertices.shape[0] and len(faces) == len(mesh)
    with pytest.raises(ValueError, match='recon_poses'):
        eval_recon(_cfg(recon_poses='odometry'), test_datasets=[ds], model=None)
