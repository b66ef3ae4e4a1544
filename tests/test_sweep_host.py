"""Moving-sweep lidar without a GPU: the sweep arithmetic of csrc/dc_sweepmath.h through its host build against numpy longdouble
(tests/sweep_reference.py), the per-ray sweep times, the identity behind de-skewing to a reference time, twists from poses, every
refusal, the defaults that keep existing behaviour, and the cast kernel's scratch size from the code object's notes."""
import math
import os
import re

import numpy as np
import pytest
import torch

import sweep_reference as R

PI_TWIST_AXES = ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.6, -0.64, 0.48))


@pytest.fixture(scope='module')
def host():
    return R.host_lib()


def _check(host, x, tau, tw):
    p, d = R.host_apply(host, x, tau, tw)
    rp, rd = R.apply(x, tau, tw)
    b = R.bound(x, tau, tw)
    ep, ed = np.abs(p.astype(R.LD) - rp).astype(np.float64), np.abs(d.astype(R.LD) - rd).astype(np.float64)
    print('max error / (2^-52 (|x| + |tau v|)): point %.2f, direction %.2f' % ((ep / (b / R.BOUND_ULPS)).max(), (ed / (b / R.BOUND_ULPS)).max()))
    assert (ep <= b).all() and (ed <= b).all()
    return p, d


# ---- 1. the sweep arithmetic ------------------------------------------------------------------------------------------------------------
def test_random_twists_against_longdouble(host):
    rng = np.random.default_rng(7)
    n = 4000
    x = rng.normal(scale=10.0, size=(n, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    tw = np.concatenate([rng.normal(scale=2.0, size=(n, 3)), axis * rng.uniform(0.0, math.pi, size=(n, 1))], axis=1)
    tau = rng.uniform(-1.0, 1.0, size=n)
    _check(host, x, tau, tw)


@pytest.mark.parametrize('theta', [0.0, 2.0 ** -26 * (1 - 2.0 ** -10), 2.0 ** -26 * (1 + 2.0 ** -10), 1e-4, 0.3, math.pi / 2,
                                   math.pi * (1 - 2.0 ** -40), math.pi])
def test_angles_at_the_edges(host, theta):
    """theta = 0 exactly, either side of the 2^-26 switch to A = 1, B = 1/2, and up to pi, with tau = 1 and tau < 0."""
    rng = np.random.default_rng(11)
    x = np.repeat(rng.normal(scale=5.0, size=(20, 3)), len(PI_TWIST_AXES) * 2, axis=0)
    axes = np.tile(np.asarray(PI_TWIST_AXES), (40, 1))
    tau = np.tile(np.repeat([1.0, -0.75], len(PI_TWIST_AXES)), 20)
    # |tau w| = theta: the axis is a unit vector up to rounding, so the angle the code sees is theta within an ulp or two
    tw = np.concatenate([rng.normal(size=(len(x), 3)), axes * (theta / np.abs(tau))[:, None]], axis=1)
    assert np.linalg.norm(tw[:, 3:], axis=1).max() <= math.pi * (4.0 / 3.0) + 1e-12        # |w| itself may exceed pi here: tau scales it
    _check(host, x, tau, tw)


def test_the_switch_is_at_two_to_the_minus_26(host):
    """Just below 2^-26 the rotation is x + a x x + (a x (a x x)) / 2 with A = 1 and B = 1/2 exactly: along a coordinate axis the
    cross products are exact, so the output can be predicted bit for bit."""
    th = 2.0 ** -27
    x = np.array([[1.0, 2.0, 4.0]])
    tw = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, th]])
    p, d = R.host_apply(host, x, [1.0], tw)
    want = np.array([[(1.0 + 1.0 * (-th * 2.0)) + 0.5 * (-th * th * 1.0), (2.0 + th * 1.0) + 0.5 * (-th * th * 2.0), 4.0]])
    assert np.array_equal(p, want) and np.array_equal(d, want)


def test_identities_are_exact(host):
    """tau = 0 with a non-zero twist, and a zero twist with any tau, return x itself; a NaN tau gives NaN."""
    rng = np.random.default_rng(3)
    x = rng.normal(scale=100.0, size=(64, 3))
    x[0] = 0.0
    tw = np.concatenate([rng.normal(size=(64, 3)), rng.normal(size=(64, 3))], axis=1)
    p, d = R.host_apply(host, x, np.zeros(64), tw)
    assert (p == x).all() and (d == x).all()
    tau = rng.uniform(-3.0, 3.0, size=64)
    tau[:4] = [0.0, 1.0, -1e300, 1e300]
    p, d = R.host_apply(host, x, tau, np.zeros((64, 6)))
    assert (p == x).all() and (d == x).all()
    for bad in (float('nan'), float('inf'), -float('inf')):
        p, d = R.host_apply(host, x, np.full(64, bad), tw)
        assert np.isnan(p).all() and np.isnan(d).all()
    p, d = R.host_apply(host, x[:4], np.full(4, float('nan')), np.zeros((4, 6)))
    assert np.isnan(p).all() and np.isnan(d).all()


def test_rigid(host):
    """|D x - D vp| = |x - vp| within 8 * 2^-52 (|x| + |vp|)."""
    rng = np.random.default_rng(5)
    n = 2000
    x, vp = rng.normal(scale=10.0, size=(n, 3)), rng.normal(scale=0.5, size=(n, 3))
    tw = np.concatenate([rng.normal(size=(n, 3)), rng.normal(scale=0.8, size=(n, 3))], axis=1)
    tau = rng.uniform(-1.0, 1.0, size=n)
    px, _ = R.host_apply(host, x, tau, tw)
    pv, _ = R.host_apply(host, vp, tau, tw)
    err = np.abs(np.linalg.norm(px - pv, axis=1) - np.linalg.norm(x - vp, axis=1))
    assert (err <= 8 * R.EPS * (np.linalg.norm(x, axis=1) + np.linalg.norm(vp, axis=1))).all()


# ---- 2. sweep times ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fov', [(45.0, 360.0), (30.0, 90.0)])
def test_sweep_times(fov):
    from depth_correction_amd.render import SweepModel, lidar_directions
    dirs, _ = lidar_directions(size=(4, 128), fov=fov, num_segments=16)
    tau = SweepModel.sweep_times(dirs, fov, 'ccw')
    assert tau.dtype == np.float64 and tau.shape == (len(dirs),)
    assert (tau >= 0.0).all() and (tau < 1.0).all()
    fh, a0 = math.radians(fov[1]), -math.radians(fov[1]) / 2 + 1e-3
    rel = np.mod(np.arctan2(dirs[:, 1], dirs[:, 0]) - a0, 2 * math.pi)          # the azimuth from the first segment's yaw
    order = np.argsort(rel, kind='stable')
    assert (np.diff(tau[order]) >= 0.0).all()                                   # monotone in azimuth
    inside = rel < fh
    assert inside.sum() >= 0.9 * len(dirs)
    np.testing.assert_allclose(tau[inside], rel[inside] / fh, rtol=0, atol=1e-15)
    assert (tau[~inside] == np.nextafter(1.0, 0.0)).all()                       # the half segment before the first yaw: clamped
    # rays of one column (one azimuth) share their time
    az = np.round(np.arctan2(dirs[:, 1], dirs[:, 0]), 9)
    for a in np.unique(az)[::7]:
        assert np.ptp(tau[az == a]) <= 1e-15
    cw = SweepModel.sweep_times(dirs, fov, 'cw')
    assert (cw >= 0.0).all() and (cw < 1.0).all()
    assert np.array_equal(cw, np.minimum(1.0 - tau, np.nextafter(1.0, 0.0)))
    assert np.array_equal(tau, SweepModel.sweep_times(dirs, fov, 'ccw'))        # deterministic
    with pytest.raises(ValueError):
        SweepModel.sweep_times(dirs, fov, 'up')


def test_sweep_times_at_the_atan2_seam():
    """With a 360 degree field of view the first yaw is -pi + 1e-3: the azimuths on either side of +-pi are late in the sweep and
    continue each other."""
    from depth_correction_amd.render import SweepModel
    az = np.array([math.pi - 1e-6, math.pi, -math.pi, -math.pi + 1e-6, -math.pi + 1e-3 - 1e-9, -math.pi + 1e-3, -math.pi + 1e-3 + 1e-9])
    dirs = np.stack([np.cos(az), np.sin(az), np.zeros_like(az)], axis=1)
    dirs[1], dirs[2] = (-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0)                      # atan2 = +pi and -pi exactly
    tau = SweepModel.sweep_times(dirs, (45.0, 360.0), 'ccw')
    assert (tau >= 0.0).all() and (tau < 1.0).all()
    assert (np.diff(tau[:5]) >= 0.0).all() and tau[1] == tau[2]
    np.testing.assert_allclose(tau[:5], 1.0 - (1e-3 - np.array([-1e-6, 0.0, 0.0, 1e-6, 1e-3 - 1e-9])) / (2 * math.pi), atol=1e-12)
    assert tau[5] <= 1e-12 or tau[5] >= 1 - 1e-12                               # the first yaw itself: either end, within rounding
    assert tau[6] < 1e-9


# ---- 3. the reference-time identity, twists from poses ----------------------------------------------------------------------------------
def test_ref_identity():
    """D(ref)^-1 D(tau) = D(tau - ref; (Exp(-ref w) v, w)) as 4 x 4 matrices, to 1e-14."""
    from depth_correction_amd.sweep import shifted_twist, sweep_matrix
    rng = np.random.default_rng(9)
    for _ in range(200):
        tw = np.concatenate([rng.normal(size=3), rng.normal(size=3) * rng.uniform(0, 1.5)])
        ref, tau = rng.uniform(0.0, 1.0), rng.uniform(-0.5, 1.5)
        lhs = np.linalg.inv(sweep_matrix(tw, ref)) @ sweep_matrix(tw, tau)
        assert np.abs(lhs - sweep_matrix(shifted_twist(tw, ref), tau - ref)).max() <= 1e-14
    tw = np.array([0.5, -0.2, 0.1, 0.0, 0.0, 0.0])
    assert np.array_equal(shifted_twist(tw, 0.7), tw) and np.array_equal(shifted_twist(np.arange(6.0), 0.0), np.arange(6.0))


def test_sweep_matrix_against_the_host_build(host):
    from depth_correction_amd.sweep import sweep_matrix
    rng = np.random.default_rng(13)
    x = rng.normal(size=(50, 3))
    tw = np.concatenate([rng.normal(size=(50, 3)), rng.normal(scale=0.7, size=(50, 3))], axis=1)
    tau = rng.uniform(-1, 1, size=50)
    p, d = R.host_apply(host, x, tau, tw)
    for i in range(50):
        D = sweep_matrix(tw[i], tau[i])
        assert np.abs(D[:3, :3] @ x[i] + D[:3, 3] - p[i]).max() <= 1e-14 and np.abs(D[:3, :3] @ x[i] - d[i]).max() <= 1e-14


def test_twists_from_poses():
    from depth_correction_amd.render import SweepModel
    from depth_correction_amd.sweep import twists_from_poses
    from helpers import slam_pose
    tw = np.array([0.5, 0.1, -0.05, 0.02, -0.03, 0.2])
    poses = R.constant_twist_poses(slam_pose(0.7, (1.0, -2.0, 0.3), roll=0.1, pitch=-0.2), tw, 5)
    got = twists_from_poses(poses)
    assert got.shape == (5, 6)
    np.testing.assert_allclose(got, np.tile(tw, (5, 1)), rtol=0, atol=1e-13)
    # the last scan repeats the previous twist
    bent = poses.copy()
    bent[4] = bent[3] @ R.twist_matrix([0.1, 0.0, 0.0, 0.0, 0.0, -0.3])
    got = twists_from_poses(bent)
    np.testing.assert_allclose(got[3], [0.1, 0.0, 0.0, 0.0, 0.0, -0.3], rtol=0, atol=1e-13)
    assert np.array_equal(got[4], got[3])
    assert np.array_equal(twists_from_poses(poses[:1]), np.zeros((1, 6))) and twists_from_poses(poses[:0]).shape == (0, 6)
    np.testing.assert_allclose(twists_from_poses(poses, 0.25), 0.25 * np.tile(tw, (5, 1)), rtol=0, atol=1e-13)
    # SweepModel: from the poses, or given; fraction scales both; the start pose is T D(ref)^-1
    np.testing.assert_allclose(SweepModel(fraction=0.5).scan_twists(poses), 0.5 * np.tile(tw, (5, 1)), rtol=0, atol=1e-13)
    given = SweepModel(twists=np.tile(tw, (5, 1)), fraction=0.5, ref=0.5)
    np.testing.assert_allclose(given.scan_twists(poses), 0.5 * np.tile(tw, (5, 1)), rtol=0, atol=0)
    start = given.start_poses(poses, given.scan_twists(poses))
    from depth_correction_amd.sweep import sweep_matrix
    for i in range(5):
        np.testing.assert_allclose(start[i] @ sweep_matrix(0.5 * tw, 0.5), poses[i], rtol=0, atol=1e-14)
    assert np.array_equal(SweepModel().start_poses(poses, got), poses)
    with pytest.raises(ValueError):
        given.scan_twists(poses[:3])


# ---- 4. refusals and defaults -----------------------------------------------------------------------------------------------------------
def _bvh():
    from depth_correction_amd.mesh import MeshBVH
    return MeshBVH(torch.zeros(1, dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                   torch.zeros((1, 6)), torch.zeros((1, 9), dtype=torch.float64))


def test_ops_refusals():
    """Every check of sweep_rays / raycast_sweep / deskew is a ValueError raised before anything is uploaded or launched: host tensors
    reach them, and only well-formed arguments get as far as the refusal to run without a GPU."""
    from depth_correction_amd import ops
    z = torch.zeros((4, 3), dtype=torch.float64)
    tau = torch.zeros(4, dtype=torch.float64)
    tw = np.zeros((2, 6))
    off = [0, 3, 4]
    poses = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    calls = {
        'sweep_rays': lambda vps=z, dirs=z, tau=tau, off=off, tw=tw: ops.sweep_rays(vps, dirs, tau, off, tw),
        'raycast_sweep': lambda vps=z, dirs=z, tau=tau, off=off, tw=tw, poses=poses: ops.raycast_sweep(_bvh(), vps, dirs, tau, off, poses, tw),
        'deskew': lambda vps=z, dirs=z, tau=tau, off=off, tw=tw: ops.deskew(dirs, tau, off, tw, vps=vps, normals=z),
    }
    nan_tw, inf_tw, big_tw = tw.copy(), tw.copy(), tw.copy()
    nan_tw[1, 4], inf_tw[0, 0] = float('nan'), float('inf')
    big_tw[1, 3:] = np.array([0.6, 0.0, 0.8]) * (math.pi * (1 + 1e-9))
    ok_tw = tw.copy()
    ok_tw[1, 3:] = np.array([0.6, 0.0, 0.8]) * (math.pi * (1 - 1e-9))
    bad = [dict(dirs=torch.zeros((4, 2), dtype=torch.float64)), dict(dirs=torch.zeros(12, dtype=torch.float64)),      # shapes
           dict(vps=torch.zeros((3, 3), dtype=torch.float64)),
           dict(tau=torch.zeros(3, dtype=torch.float64)), dict(tau=torch.zeros((4, 1), dtype=torch.float64)), dict(tau=np.zeros(4)),
           dict(tw=np.zeros((2, 5))), dict(tw=np.zeros(6)), dict(tw=nan_tw), dict(tw=inf_tw), dict(tw=big_tw),
           dict(off=[0, 4]), dict(off=[1, 3, 4]), dict(off=[0, 3, 5]), dict(off=[0, 4, 3]), dict(off=[0, 5, 4])]       # scan_offset
    for name, call in calls.items():
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
        for kw in (dict(), dict(tw=ok_tw)):
            with pytest.raises(RuntimeError, match='GPU'):
                call(**kw)
    with pytest.raises(ValueError):
        calls['raycast_sweep'](poses=torch.eye(4, dtype=torch.float64).repeat(3, 1, 1))
    with pytest.raises(ValueError):
        calls['raycast_sweep'](poses=torch.zeros((2, 3, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sweep_rays(z, z, tau, [0], np.zeros((0, 6)))                        # rays without a scan


def test_model_and_dataset_refusals(tmp_path):
    from depth_correction_amd.dataset import DeskewedDataset
    from depth_correction_amd.mesh import box_mesh
    from depth_correction_amd.preproc import deskew_cloud
    from depth_correction_amd.render import BeamModel, MovingObjectDataset, RenderedMeshDataset, SweepModel, render_lidar_clouds
    for kw in (dict(fraction=0.0), dict(fraction=1.5), dict(fraction=float('nan')), dict(ref=-0.1), dict(ref=1.1), dict(direction='up'),
               dict(twists=np.zeros((3, 5))), dict(twists=np.zeros(6)), dict(twists=np.full((1, 6), np.nan)),
               dict(twists=np.array([[0, 0, 0, 0, 0, 3.2]]))):
        with pytest.raises(ValueError):
            SweepModel(**kw)
    assert SweepModel(twists=np.array([[0, 0, 0, 0, 0, 3.2]]), fraction=0.5).fraction == 0.5         # the sweep turns by 1.6 rad
    mesh = box_mesh((0, 0, 0), (2, 2, 2), inward=True)
    path = str(tmp_path / 'box.ply')
    mesh.save_ply(path)
    poses = np.eye(4)[None]
    with pytest.raises(ValueError):
        render_lidar_clouds(mesh, poses, beam=BeamModel(samples=4), sweep=SweepModel())
    with pytest.raises(ValueError):
        RenderedMeshDataset(path, poses=poses, beam=BeamModel(samples=4), sweep=SweepModel())
    with pytest.raises(TypeError):
        RenderedMeshDataset(path, poses=poses, sweep='ccw')
    with pytest.raises(ValueError):
        MovingObjectDataset(mesh, [], poses, sweep=SweepModel())
    ds = RenderedMeshDataset(path, poses=poses, sweep=SweepModel())
    for kw in (dict(fraction=0.0), dict(ref=2.0), dict(twists=np.zeros((2, 6)))):
        with pytest.raises(ValueError):
            DeskewedDataset(ds, **kw)
    assert np.array_equal(DeskewedDataset(ds).twists, np.zeros((1, 6)))
    cloud = np.zeros(3, dtype=ds.cloud_dtype)
    for args in ((cloud, np.zeros(5)), (cloud, np.zeros(6), 1.5), (np.zeros(3, dtype=RenderedMeshDataset.cloud_dtype), np.zeros(6)),
                 (np.zeros((3, 3)), np.zeros(6)), ((np.zeros((3, 3)), np.zeros(2)), np.zeros(6))):
        with pytest.raises(ValueError):
            deskew_cloud(*args)


def test_defaults_keep_existing_behaviour(tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.mesh import box_mesh
    from depth_correction_amd.render import RenderedMeshDataset, SweepModel
    cfg = Config()
    assert cfg.slam_deskew is False and cfg.slam_sweep_fraction == 1.0
    path = str(tmp_path / 'box.ply')
    box_mesh((0, 0, 0), (2, 2, 2), inward=True).save_ply(path)
    kw = dict(poses=np.eye(4)[None], size=(16, 256), fov=(45.0, 360.0), num_segments=16, cache=True, cache_dir=str(tmp_path / 'gen'))
    thin = RenderedMeshDataset(path, **kw)
    names = ('x', 'y', 'z', 'vp_x', 'vp_y', 'vp_z', 'normal_x', 'normal_y', 'normal_z')
    want = os.path.join(str(tmp_path / 'gen'), 'rendered_mesh', 'box.ply', 'hash_%s_size_16_256_fov_45_360' % thin.hash_name,
                        'cloud_00000.bin')
    assert thin.sweep is None and thin.cloud_path(0) == want
    assert thin.cloud_dtype is RenderedMeshDataset.cloud_dtype and thin.cloud_dtype.names == names and thin.cloud_dtype.itemsize == 72
    sweep = SweepModel(fraction=0.5, ref=0.25, direction='cw')
    moving = RenderedMeshDataset(path, sweep=sweep, **kw)
    assert moving.sweep is sweep and moving[0:1].sweep is sweep
    assert moving.cloud_dtype.names == names + ('t',) and moving.cloud_dtype['t'] == np.float64
    assert RenderedMeshDataset.cloud_dtype.names == names                       # the class's dtype is untouched
    assert os.path.dirname(os.path.dirname(moving.cloud_path(0))) == os.path.dirname(want)
    assert os.path.basename(os.path.dirname(moving.cloud_path(0))) == sweep.cache_key() and moving.cloud_path(0) != want
    keys = {SweepModel(**k).cache_key() for k in (dict(), dict(fraction=0.5), dict(ref=0.5), dict(direction='cw'),
                                                  dict(twists=np.zeros((1, 6))), dict(twists=np.full((1, 6), 0.1)))}
    assert len(keys) == 6
    for token in ('0.5', '0.25', 'cw', 'poses'):
        assert token in sweep.cache_key()


# ---- 5. the code object -----------------------------------------------------------------------------------------------------------------
def test_sweep_cast_has_the_thin_cast_scratch():
    """raycast_sweep_kernel keeps what raycast_rays_kernel keeps in scratch memory (nothing): the sweep arithmetic, sincos included,
    stays in registers.  Metadata notes of the built library only."""
    from test_step_kernel_resources import _code_objects, _kernels
    import __graft_entry__ as ge
    ge.build()
    from depth_correction_amd import _native
    blob = open(_native.lib_path(), 'rb').read()
    found = {}
    for elf in _code_objects(blob):
        for k in _kernels(elf):
            m = re.search(r'\d+(raycast_rays_kernel|raycast_sweep_kernel|sweep_rays_kernel|deskew_kernel)I([fd])E', k['.name'])
            if m:
                found[m.groups()] = k
    assert len(found) == 8, sorted(found)
    for t in 'fd':
        thin, moving = found[('raycast_rays_kernel', t)], found[('raycast_sweep_kernel', t)]
        for name in ('raycast_rays_kernel', 'raycast_sweep_kernel', 'sweep_rays_kernel', 'deskew_kernel'):
            k = found[(name, t)]
            print('%s<%s>: vgpr %d sgpr %d scratch %d lds %d' % (name, t, k['.vgpr_count'], k['.sgpr_count'], k['.private_segment_fixed_size'],
                                                              k['.group_segment_fixed_size']))
        assert moving['.private_segment_fixed_size'] == thin['.private_segment_fixed_size']
        assert moving['.group_segment_fixed_size'] == thin['.group_segment_fixed_size']
        assert found[('sweep_rays_kernel', t)]['.private_segment_fixed_size'] == 0
        assert found[('deskew_kernel', t)]['.private_segment_fixed_size'] == 0


def test_deskewed_dataset_takes_a_slice_with_the_twists_it_was_rendered_with(tmp_path):
    """A slice of a RenderedMeshDataset keeps every pose and is rendered with the whole trajectory's twists; DeskewedDataset over it uses
    the same rows, by scan id -- from the poses, from the model's own twists, or from twists given for the whole trajectory."""
    from depth_correction_amd.dataset import DeskewedDataset
    from depth_correction_amd.mesh import box_mesh
    from depth_correction_amd.render import RenderedMeshDataset, SweepModel
    path = str(tmp_path / 'box.ply')
    box_mesh((0, 0, 0), (2, 2, 2), inward=True).save_ply(path)
    steps = np.array([[0.1, 0, 0, 0, 0, 0.1], [0.2, 0, 0, 0, 0, 0.05], [0.3, 0, 0, 0, 0, 0.0], [0.1, 0.1, 0, 0, 0, 0.2]])
    poses = [np.eye(4)]
    for tw in steps[:3]:
        poses.append(poses[-1] @ R.twist_matrix(tw))
    poses = np.stack(poses)
    whole = np.concatenate([steps[:3], steps[2:3]])                            # the last scan repeats the previous twist
    ds = RenderedMeshDataset(path, poses=poses, sweep=SweepModel(fraction=0.5))
    for index, ids in ((slice(1, 3), [1, 2]), (slice(None, None, 2), [0, 2]), ([3, 0], [3, 0]), (slice(None), [0, 1, 2, 3])):
        got = DeskewedDataset(ds[index], fraction=0.5)
        np.testing.assert_allclose(got.twists, 0.5 * whole[ids], rtol=0, atol=1e-13)
        np.testing.assert_allclose(got.twists, ds.sweep.scan_twists(ds.poses)[ids], rtol=0, atol=0)      # what the cast uses
    with pytest.raises(ValueError):
        DeskewedDataset(ds)                                                     # rendered with fraction 0.5, asked for 1.0
    with pytest.raises(ValueError):
        DeskewedDataset(ds, fraction=0.5, ref=0.5)
    given = RenderedMeshDataset(path, poses=poses, sweep=SweepModel(twists=steps))
    assert np.array_equal(DeskewedDataset(given[[3, 0]]).twists, steps[[3, 0]])
    plain = RenderedMeshDataset(path, poses=poses)
    assert np.array_equal(DeskewedDataset(plain[1:3], twists=steps).twists, steps[1:3])           # rows of the whole trajectory, by id
    assert np.array_equal(DeskewedDataset(plain[1:3], twists=steps[:2]).twists, steps[:2])        # one row per item
    with pytest.raises(ValueError):
        DeskewedDataset(plain[1:3], twists=steps[:3])
    # a cloud with sweep times but no item to name its scan is refused; one without sweep times passes
    wrapper = DeskewedDataset(given)
    with pytest.raises(ValueError):
        wrapper.transform_cloud(np.zeros(2, dtype=given.cloud_dtype))
    thin = np.zeros(2, dtype=RenderedMeshDataset.cloud_dtype)
    assert wrapper.transform_cloud(thin) is thin
