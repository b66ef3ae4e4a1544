"""SLAM evaluation on the MI355X (csrc/dc_slam.hip, slam.py, eval.eval_slam): the moved k-NN query against a kept grid, one ICP
iteration against a numpy + cKDTree restatement, registration and whole sequences of scans rendered from a room with pillars,
the correction's effect, the files eval_slam writes and the failure paths."""
import math
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _pose(yaw, t, roll=0.0, pitch=0.0):
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(roll, pitch, yaw)
    T[:3, 3] = t
    return T


def _moved(T, p):
    """x = ((T00 p0 + T01 p1) + T02 p2) + T03, the rounding order of dc_knn_grid_query."""
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = tmp_path_factory.mktemp('slam') / 'pillared_room.ply'
    mesh.save_ply(str(path))
    return str(path)


def _poses(n):
    return np.stack([_pose(0.04 * i, (-3.0 + 0.25 * i, 0.3 * math.sin(i / 3.0), 0.02 * math.sin(i / 2.0))) for i in range(n)])


def _dataset(room, n=24, size=(64, 512)):
    from depth_correction_amd.dataset import RenderedMeshDataset
    return RenderedMeshDataset(room, poses=_poses(n), size=size, fov=(45.0, 360.0), num_segments=16, device=DEV)


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    base.update(kw)
    return Config(**base)


def _err(A, B):
    D = np.linalg.solve(A, B)
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(D[:3, :3]) - 1) / 2)))), float(np.linalg.norm(D[:3, 3]))


def test_grid_query_moved_points_matches_ckdtree():
    from depth_correction_amd import ops
    rng = np.random.default_rng(5)
    pts = rng.uniform(-5, 5, size=(20000, 3))
    pts[:, 2] *= 0.2
    q = rng.uniform(-4, 4, size=(3000, 3))
    P = torch.as_tensor(pts, device=DEV)
    grid = ops.knn_grid_build(P, len(q), 3)
    Q = torch.as_tensor(q, device=DEV)
    tree = cKDTree(pts)
    for i, T in enumerate([_pose(0.3, (0.5, -0.2, 0.1), 0.05, -0.02), _pose(-1.2, (1.5, 0.7, 0.0))]):
        if i == 1:
            P.zero_()                                # the grid keeps its own copy: nothing is rebuilt from the points
        dist, idx = ops.knn_grid_query(grid, Q, torch.as_tensor(T, device=DEV), 3)
        rd, ri = tree.query(_moved(T, q), k=3)
        assert np.array_equal(idx.cpu().numpy(), ri), i
        np.testing.assert_allclose(dist.cpu().numpy(), rd, rtol=1e-15, atol=0)
    stop = torch.ones((4,), dtype=torch.int32, device=DEV)
    dist, idx = ops.knn_grid_query(grid, Q, torch.as_tensor(np.eye(4), device=DEV), 3, stop=stop)
    assert (idx.cpu().numpy() == -1).all() and np.isinf(dist.cpu().numpy()).all()


def test_one_iteration_matches_numpy(room):
    from depth_correction_amd import _native as nv, ops
    from depth_correction_amd.slam import IcpMapper, mapper_input
    cfg = _cfg()
    ds = _dataset(room, n=3)
    mapper = IcpMapper(cfg)
    s0 = mapper.prepare(mapper_input(ds[0][0], None, cfg))
    s1 = mapper.prepare(mapper_input(ds[2][0], None, cfg))
    mapper.update(s0, ds[0][1])
    prior = ds[2][1] @ _pose(0.03, (0.1, -0.05, 0.02))
    m, k = len(s1), 3
    mapper._ensure_grid(m)
    idx = torch.empty((m, k), dtype=torch.int32, device=DEV)
    dist = torch.empty((m, k), dtype=torch.float64, device=DEV)
    thr = torch.empty((1,), dtype=torch.float64, device=DEV)
    kept = torch.empty((m, k), dtype=torch.uint8, device=DEV)
    partials = torch.empty((ops.icp_blocks(m), nv.DC_ICP_PARTIALS), dtype=torch.float64, device=DEV)
    ops.icp_init(torch.as_tensor(prior, device=DEV), mapper.state, mapper.status)
    map_pts, map_nrm = mapper.map_points()
    pose_d = mapper.state[:16].view(4, 4)
    mapper.iteration(s1, pose_d, idx, dist, thr, partials, map_pts, map_nrm, math.cos(cfg.icp_max_normal_angle), kept=kept)
    torch.cuda.synchronize()
    # numpy + cKDTree
    mp, mn = map_pts.cpu().numpy(), map_nrm.cpu().numpy()
    p, pn = s1.points.cpu().numpy(), s1.normals.cpu().numpy()
    x = _moved(prior, p)
    rd, ri = cKDTree(mp).query(x, k=3, distance_upper_bound=cfg.icp_max_dist)
    assert np.array_equal(idx.cpu().numpy(), np.where(np.isfinite(rd), ri, -1))
    th = np.quantile(rd, cfg.icp_trim_ratio)
    assert abs(thr.item() - th) <= 1e-12 * th
    nr = pn @ prior[:3, :3].T
    keep = np.isfinite(rd) & (rd <= th)
    ric = np.where(keep, ri, 0)
    keep &= np.abs(np.einsum('ij,ikj->ik', nr, mn[ric])) >= math.cos(cfg.icp_max_normal_angle)
    assert np.array_equal(kept.cpu().numpy().astype(bool), keep)
    rows, cols = np.nonzero(keep)
    n, y, xx = mn[ri[rows, cols]], mp[ri[rows, cols]], x[rows]
    r = np.einsum('ij,ij->i', n, xx - y)
    J = np.concatenate([np.cross(xx, n), n], axis=1)
    A, b = J.T @ J, J.T @ r
    tot = partials.cpu().numpy().sum(axis=0)
    a21 = np.array([A[i, j] for i in range(6) for j in range(i, 6)])
    np.testing.assert_allclose(tot[:21], a21, rtol=1e-9, atol=1e-9 * np.abs(a21).max())
    np.testing.assert_allclose(tot[21:27], b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
    assert tot[27] == len(r) and abs(tot[28] - (r * r).sum()) <= 1e-9 * (r * r).sum()
    assert tot[29] == keep.any(axis=1).sum()
    st = mapper.state.cpu().numpy()
    assert st[nv.DC_ICP_STATE_PAIRS] == len(r)
    step = -np.linalg.solve(A, b)
    assert int(mapper.status[1].item()) == 1 and int(mapper.status[0].item()) == 0
    np.testing.assert_allclose(st[:3], (_rot(step[:3]) @ prior[:3, :3])[0], atol=1e-6)


def _rot(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K


def test_registration_recovers_perturbation(room):
    from depth_correction_amd.slam import IcpMapper, mapper_input
    cfg = _cfg(icp_min_diff_rot=1e-7, icp_min_diff_trans=1e-6)
    ds = _dataset(room, n=5)
    mapper = IcpMapper(cfg)
    mapper.update(mapper.prepare(mapper_input(ds[0][0], None, cfg)), ds[0][1])
    mapper.update(mapper.prepare(mapper_input(ds[1][0], None, cfg)), ds[1][1])
    gt = ds[4][1]
    prior = gt @ _pose(math.radians(4.0), (0.2, -0.15, 0.05), math.radians(1.0), math.radians(-1.5))
    pose, info = mapper.register(mapper_input(ds[4][0], None, cfg), prior)
    print(info, _err(pose, gt))
    assert info['status'] == 'converged'
    da, dt = _err(pose, gt)
    assert da <= 0.1 and dt <= 0.005, (da, dt)
    assert info['host_reads'] <= (info['iterations'] + mapper.status_every - 1) // mapper.status_every


def test_sequence_zero_noise_and_reproducible(room):
    from depth_correction_amd.slam import run_slam
    cfg = _cfg()
    ds = _dataset(room)
    res = run_slam(ds, None, cfg)
    errs = [_err(s, g) for s, g in zip(res['slam'], res['gt'])]
    print('max errors deg / m:', max(e[0] for e in errs), max(e[1] for e in errs))
    assert all(i['ok'] for i in res['info'])
    assert all(a <= 0.1 and t <= 0.005 for a, t in errs), errs


def test_sequence_odometry_noise(room):
    from depth_correction_amd.slam import run_slam, slam_errors
    cfg = _cfg(odom_cov=[1e-4] * 3 + [2.5e-3] * 3)
    ds = _dataset(room)
    res = run_slam(ds, None, cfg)
    e_slam = slam_errors(res['slam'], res['gt'], res['path_lengths'])
    e_odom = slam_errors(res['odom'], res['gt'], res['path_lengths'])
    print('slam', e_slam, 'odom', e_odom, [i['status'] for i in res['info']], [i['iterations'] for i in res['info']])
    assert e_slam[1] * 5.0 <= e_odom[1], (e_slam, e_odom)
    again = run_slam(ds, None, cfg)
    assert np.array_equal(res['slam'], again['slam'])


def test_correction_improves_slam(room, tmp_path):
    from depth_correction_amd.dataset import DepthBiasDataset
    from depth_correction_amd.eval import eval_slam
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.slam import run_slam, slam_errors
    cfg = _cfg(odom_cov=[1e-4] * 3 + [2.5e-3] * 3, slam_eval_csv=str(tmp_path / 'slam.csv'))
    ds = _dataset(room)
    w = 0.05
    biased = DepthBiasDataset(ds, ScaledPolynomial(w=[w], exponent=[2.0], device=DEV), cfg=cfg)
    plain = run_slam(biased, None, cfg)
    e_plain = slam_errors(plain['slam'], plain['gt'], plain['path_lengths'])
    res = eval_slam(cfg, test_datasets=[biased], model=ScaledPolynomial(w=[w], exponent=[2.0], device=DEV))
    e_corr = res[0]['errors']
    print('uncorrected', e_plain, 'corrected', e_corr)
    assert e_corr[0] < e_plain[0] and e_corr[1] < e_plain[1], (e_corr, e_plain)


def test_eval_slam_files(room, tmp_path):
    from depth_correction_amd.eval import eval_slam, eval_slam_all
    from depth_correction_amd.scan_io import read_poses_csv
    ds = _dataset(room, n=6)
    cfg = _cfg(slam_eval_csv=str(tmp_path / 'eval.csv'), slam_poses_csv=str(tmp_path / 'seq' / 'slam_poses_icp_mapper.csv'),
               slam_eval_bag=str(tmp_path / 'x.bag'))
    res = eval_slam(cfg, test_datasets=[ds], model=None)
    lines = open(cfg.slam_eval_csv).read().splitlines()
    assert len(lines) == 1
    parts = lines[0].split(' ')
    assert parts[0] == str(ds) and len(parts) == 5 and all(len(p.split('.')[1]) == 9 for p in parts[1:])
    ids, poses = read_poses_csv(cfg.slam_poses_csv)
    assert ids == list(range(6))
    np.testing.assert_allclose(np.stack(poses), res[0]['slam'], atol=1e-8)
    assert not os.path.exists(str(tmp_path / 'x.bag'))
    cfg2 = _cfg(log_dir=str(tmp_path / 'log'), test_names=['room'], min_depth=1.0, grid_res=0.2)
    eval_slam_all(cfg2)
    line = open(os.path.join(cfg2.log_dir, 'slam_eval_icp_mapper_test.csv')).read().splitlines()
    assert len(line) == 1 and line[0].startswith('room ')


def test_failure_paths_keep_prior_and_map(room):
    from depth_correction_amd.slam import IcpMapper, mapper_input
    cfg = _cfg()
    ds = _dataset(room, n=3)
    mapper = IcpMapper(cfg)
    mapper.update(mapper.prepare(mapper_input(ds[0][0], None, cfg)), ds[0][1])
    n0 = mapper.n_map
    before = mapper.map_points()[0].clone()
    prior = ds[1][1] @ _pose(0.01, (0.05, 0.0, 0.0))
    # empty scan
    pose, info = mapper.register(np.zeros((0, 3)), prior)
    assert info['status'] == 'empty' and not info['ok'] and np.array_equal(pose, prior)
    # near-empty scan
    scan = mapper_input(ds[1][0], None, cfg)
    few = scan.get_points()[:4].cpu().numpy()
    pose, info = mapper.register(few, prior)
    assert not info['ok'] and info['status'] in ('too_few_pairs', 'singular'), info
    assert np.array_equal(pose, prior)
    # a prior beyond the bound check
    tight = _cfg(icp_max_translation=0.01)
    mapper.cfg = tight
    pose, info = mapper.register(scan, ds[1][1] @ _pose(0.0, (0.3, 0.0, 0.0)))
    assert info['status'] == 'bound' and not info['ok'], info
    assert np.array_equal(pose, ds[1][1] @ _pose(0.0, (0.3, 0.0, 0.0)))
    assert mapper.n_map == n0 and torch.equal(mapper.map_points()[0], before)


def test_mapper_bookkeeping(room):
    """grid_builds rises exactly when the map changed or a larger reading arrives; update() with enough overlap, or of a scan that
    is already in the map, adds and builds nothing; a failed registration leaves the map, its rows and the grid as they were."""
    from depth_correction_amd.slam import IcpMapper, MapperScan, mapper_input
    cfg = _cfg()
    ds = _dataset(room, n=3)
    mapper = IcpMapper(cfg)
    s0 = mapper.prepare(mapper_input(ds[0][0], None, cfg))
    s1 = mapper.prepare(mapper_input(ds[1][0], None, cfg))
    pose, info = mapper.register(s1, ds[1][1])
    assert info['status'] == 'init' and info['ok'] and info['iterations'] == 0 and np.array_equal(pose, ds[1][1])
    assert mapper.grid_builds == 0 and mapper.n_map == 0
    assert mapper.update(s0, ds[0][1]) == len(s0) and mapper.grid_builds == 1
    small = MapperScan(s1.points[:1000].contiguous(), s1.normals[:1000].contiguous(), s1.depth[:1000].contiguous())
    prior = ds[1][1] @ _pose(0.01, (0.05, 0.0, 0.0))
    for _ in range(2):                                     # a repeated register() of a reading the grid already holds room for
        pose, info = mapper.register(small, prior)
        assert info['ok'] and mapper.grid_builds == 1
    n_query_max = mapper.grid.n_query_max
    larger = len(s1) > n_query_max
    pose, info = mapper.register(s1, prior)
    assert info['ok'] and mapper.grid_builds == (2 if larger else 1)
    pose2, info2 = mapper.register(s1, prior)
    assert mapper.grid_builds == (2 if larger else 1) and np.array_equal(pose, pose2) and info2['iterations'] == info['iterations']
    builds, n0 = mapper.grid_builds, mapper.n_map
    rows = mapper.map_points()[0].clone()
    assert mapper.update(s1, pose, overlap=cfg.slam_min_overlap) == 0          # overlap >= slam_min_overlap: nothing added, nothing built
    assert mapper.update(s1, pose, overlap=1.0) == 0
    assert mapper.update(s0, ds[0][1], overlap=0.0) == 0                       # every point is within min_dist of itself in the map
    assert mapper.grid_builds == builds and mapper.n_map == n0
    tight = _cfg(icp_max_translation=0.01)
    mapper.cfg = tight
    pose, info = mapper.register(s1, ds[1][1] @ _pose(0.0, (0.3, 0.0, 0.0)))
    assert info['status'] == 'bound' and mapper.grid_builds == builds and mapper.n_map == n0
    assert torch.equal(mapper.map_points()[0], rows)
    mapper.cfg = cfg
    added = mapper.update(s1, ds[1][1], overlap=0.0)
    assert added > 0 and mapper.grid_builds == builds + 1 and mapper.n_map == n0 + added
    assert torch.equal(mapper.map_points()[0][:n0], rows)
