"""Host-side logic of the reference-API layer on CPU tensors: container semantics of DepthCloud, models, loss
post-processing, filters, config, pose parametrisation.  The neighbourhood operators themselves must REFUSE CPU
tensors (there is no CPU implementation of the hot path)."""
import numpy as np
import pytest
import torch

import dc_oracle as O
from depth_correction_amd.config import Config, PoseCorrection
from depth_correction_amd.dataset import PlaneDataset, RoomBoxDataset, KittiLikeDataset
from depth_correction_amd.depth_cloud import DepthCloud
from depth_correction_amd.eval import create_corrected_poses, initialize_pose_corrections
from depth_correction_amd.filters import filter_depth, filter_grid, within_bounds
from depth_correction_amd.loss import Reduction, min_eigval_loss, reduce, trace_loss
from depth_correction_amd.model import Polynomial, ScaledPolynomial, load_model, model_by_name
from depth_correction_amd.transform import matrix_to_xyz_axis_angle, xyz_axis_angle_to_matrix
from depth_correction_amd.utils import covs, trace


def _cloud(n=50, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand((n, 3), generator=g, dtype=torch.float64) * 4 + 1
    return DepthCloud.from_points(pts, vps=torch.rand((n, 3), generator=g, dtype=torch.float64))


def test_from_points_and_to_points_roundtrip():
    pts = torch.tensor([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], dtype=torch.float64)
    dc = DepthCloud.from_points(pts)
    assert torch.allclose(dc.depth.flatten(), torch.tensor([5.0, 0.0, 3.0], dtype=torch.float64))
    assert torch.equal(dc.dirs[1], torch.zeros(3, dtype=torch.float64))       # zero-depth ray left un-normalised
    assert torch.allclose(dc.to_points(), pts)
    arr = dc.to_structured_array()
    assert arr.dtype.names[:6] == ('x', 'y', 'z', 'vp_x', 'vp_y', 'vp_z')
    back = DepthCloud.from_structured_array(arr)
    assert torch.allclose(back.to_points().double(), pts, atol=1e-6)


def test_container_semantics():
    dc = _cloud()
    dc.update_points()
    dc.mask = torch.arange(len(dc)) % 2 == 0
    dc.normals = torch.nn.functional.normalize(torch.rand(len(dc), 3, dtype=torch.float64), dim=-1)
    dc.neighbors = torch.zeros((len(dc), 3), dtype=torch.int64)
    snap = dc.copy()
    assert snap.points is dc.points and snap.neighbors is dc.neighbors        # shallow copy = snapshot
    sub = dc[dc.mask]
    assert len(sub) == 25 and sub.neighbors is None and sub.points.shape == (25, 3)   # only per-point fields sliced
    assert dc[['vps', 'dirs', 'depth']].points is None
    T = torch.eye(4, dtype=torch.float64)
    T[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    moved = dc.transform(T)
    assert moved.points is None and moved.neighbors is None and moved.mask is dc.mask and moved.normals is not None
    assert torch.allclose(moved.to_points(), dc.points + T[:3, 3])
    assert dc.float().type() == torch.float32 and dc.double().type() == torch.float64


def test_concatenate_shifts_neighbors_in_place():
    a, b = _cloud(4, 1), _cloud(3, 2)
    a.neighbors = torch.tensor([[0, 1], [1, 2], [2, 3], [3, 0]])
    b.neighbors = torch.tensor([[0, 1], [1, 2], [2, 0]])
    cat = DepthCloud.concatenate([a, b], dependent=True)
    assert len(cat) == 7 and torch.equal(cat.neighbors[4:], torch.tensor([[4, 5], [5, 6], [6, 4]]))
    assert torch.equal(b.neighbors, torch.tensor([[4, 5], [5, 6], [6, 4]]))    # reference quirk: shifted in place
    src = DepthCloud.concatenate([a, b])
    assert src.neighbors is None and len(src) == 7


def test_hot_path_refuses_cpu_tensors():
    dc = _cloud()
    dc.update_points()
    with pytest.raises(RuntimeError, match='GPU'):
        dc.update_neighbors(k=4)
    dc.neighbors = torch.zeros((len(dc), 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match='GPU'):
        dc.update_features()
    from depth_correction_amd.nearest_neighbors import nearest_neighbors
    with pytest.raises(RuntimeError, match='GPU'):
        nearest_neighbors(dc.points, dc.points, k=2)


@pytest.mark.parametrize('cls', [Polynomial, ScaledPolynomial])
def test_models_match_oracle_and_state_dict(cls):
    dc = _cloud(40)
    dc.inc_angles = torch.rand((40, 1), dtype=torch.float64)
    dc.mask = torch.arange(40) % 3 != 0
    m = cls(w=[-0.01, 0.02], exponent=[2.0, 4.0])
    out = m(dc)
    ref = O.model_apply(dc.depth, dc.inc_angles, dc.mask, m.w.detach(), m.exponent, cls.__name__)
    assert torch.allclose(out.depth, ref) and out.depth is not dc.depth
    assert torch.equal(out.depth[~dc.mask], dc.depth[~dc.mask])
    assert list(m.state_dict()) == ['w'] and m.w.shape == (1, 2) and m.w.dtype == torch.float64
    assert list(cls(w=[0.1], exponent=[1.0], learnable_exponents=True).state_dict()) == ['w', 'exponent']
    legacy = cls(p0=0.1, p1=0.2)
    assert legacy.exponent.tolist() == [[2.0, 4.0]] and legacy.w.tolist() == [[0.1, 0.2]]
    assert model_by_name(cls.__name__) is cls
    cfg = Config(model_class=cls.__name__, model_kwargs={'w': [0.0, 0.0], 'exponent': [2.0, 4.0]}, device='cpu')
    assert isinstance(load_model(cfg=cfg), cls)
    inv = m.inverse(out, dc.mask) if cls is ScaledPolynomial else None
    if inv is not None:
        assert torch.allclose(inv.depth, dc.depth)


def test_loss_postprocessing_matches_oracle():
    g = torch.Generator().manual_seed(3)
    dc = _cloud(200)
    ev = torch.sort(torch.rand((200, 3), generator=g, dtype=torch.float64), dim=1).values
    ev[::7, 0] = 0.0
    dc.eigvals = ev
    A = torch.rand((200, 3, 3), generator=g, dtype=torch.float64)
    dc.cov = A @ A.transpose(1, 2)
    mask = torch.rand(200, generator=g) > 0.3
    for norm in (False, True):
        for sq in (False, True):
            loss, lc = min_eigval_loss(dc, mask=mask, normalization=norm, sqrt=sq)
            ref = O.pointwise_loss(eigvals=ev, mask=mask, normalization=norm, sqrt=sq)
            assert torch.allclose(loss, ref.mean()) and torch.allclose(lc.loss, ref) and len(lc) == int(mask.sum())
    loss, _ = trace_loss(dc, mask=mask, reduction=Reduction.SUM)
    assert torch.allclose(loss, O.pointwise_loss(cov=dc.cov, kind='trace_loss', mask=mask).sum())
    # batch: pointwise losses concatenated then reduced once (loss.py:205-213)
    both, parts = min_eigval_loss([dc, dc], mask=[mask, None], normalization=True)
    ref = torch.cat([O.pointwise_loss(eigvals=ev, mask=mask, normalization=True), O.pointwise_loss(eigvals=ev, normalization=True)])
    assert torch.allclose(both, ref.mean()) and len(parts) == 2
    # quantile inliers
    loss, lc = min_eigval_loss(dc, inlier_ratio=0.5)
    assert len(lc) in (100, 101) and torch.allclose(loss, lc.loss.mean())
    x = torch.tensor([1.0, float('nan'), 3.0])
    assert reduce(x, skip_nans=True).item() == 2.0 and torch.isnan(reduce(x))


def test_covs_and_trace_match_oracle():
    g = torch.Generator().manual_seed(5)
    x = torch.rand((30, 8, 3), generator=g, dtype=torch.float64)
    w = (torch.rand((30, 8, 1), generator=g) > 0.2).double()
    assert torch.allclose(covs(x, weights=w), O.covs(x, weights=w))
    assert torch.allclose(covs(x), O.covs(x))
    assert torch.allclose(trace(covs(x)), O.trace(O.covs(x)))
    assert torch.allclose(covs(x[0]), torch.cov(x[0].T))


def test_filters_host():
    x = torch.tensor([0.0, 1.0, 2.0, float('nan'), 4.0])
    assert within_bounds(x, min=1.0, max=2.0).tolist() == [False, True, True, False, False]
    assert within_bounds(x, bounds=[-float('inf'), float('inf')]).all()
    assert within_bounds(x, min=None, max=None).all()
    dc = _cloud(100)
    kept = filter_depth(dc, min=2.0, max=5.0)
    assert ((kept.depth >= 2.0) & (kept.depth <= 5.0)).all()
    pts = np.random.default_rng(0).uniform(0, 1, size=(500, 3))
    ind = filter_grid(pts, 0.25, only_mask=True, keep='first')
    cells = np.floor(pts / 0.25).astype(int)
    assert len(ind) == len({tuple(c) for c in cells.tolist()})
    first = {}
    for i, c in enumerate(map(tuple, cells.tolist())):
        first.setdefault(c, i)
    assert sorted(ind) == sorted(first.values())
    a = filter_grid(pts, 0.25, only_mask=True, keep='random', rng=np.random.default_rng(135))
    b = filter_grid(pts, 0.25, only_mask=True, keep='random', rng=np.random.default_rng(135))
    assert a == b


def test_pose_parametrisation():
    pd = torch.tensor([[0.1, -0.2, 0.3, 0.02, -0.01, 0.03], [0, 0, 0, 0, 0, 0]], dtype=torch.float64, requires_grad=True)
    T = xyz_axis_angle_to_matrix(pd)
    assert torch.allclose(T, O.xyz_axis_angle_to_matrix(pd.detach()))
    R = T[:, :3, :3]
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(2, 3, 3), atol=1e-14)
    T.sum().backward()
    assert torch.isfinite(pd.grad).all()                                       # finite at the zero correction
    assert torch.allclose(matrix_to_xyz_axis_angle(T.detach()), pd.detach(), atol=1e-12)
    cfg = Config(pose_correction=PoseCorrection.pose, device='cpu')
    deltas = initialize_pose_corrections([range(3), range(2)], cfg)
    assert [d.shape for d in deltas] == [(3, 6), (2, 6)] and all(d.requires_grad for d in deltas)
    poses = [torch.eye(4, dtype=torch.float64).expand(3, 4, 4), torch.eye(4, dtype=torch.float64).expand(2, 4, 4)]
    upd = create_corrected_poses(poses, deltas, cfg)
    assert torch.allclose(upd[0], poses[0])
    cfg.pose_correction = PoseCorrection.common
    deltas = initialize_pose_corrections([range(3), range(2)], cfg)
    assert deltas[0] is deltas[1] and deltas[0].shape == (1, 6)


def test_config_roundtrip(tmp_path):
    cfg = Config(nn_k=10, nn_r=None, lr=1e-3)
    assert cfg.float_type == 'float64' and cfg.eigenvalue_ratio_bounds == [[0, 1, 0, 0.25], [1, 2, 0.25, 1.]]
    assert cfg.loss_kwargs['normalization'] is True and cfg.min_valid_neighbors == 5
    path = tmp_path / 'cfg.yaml'
    cfg.to_yaml(str(path))
    back = Config().from_yaml(str(path))
    assert back.nn_k == 10 and back.nn_r is None and back.lr == 1e-3 and back.vp_dispersion_bounds[0] == 0.36
    assert cfg.copy().diff(Config())['nn_k'] == 10


def test_synthetic_generators():
    ds = PlaneDataset(n_pts=1000, n_poses=2)
    cloud, pose = ds[0]
    assert len(ds) == 2 and len(cloud) == 500 and pose.shape == (4, 4) and 'normal_z' in cloud.dtype.names
    world_z = cloud['z'] + pose[2, 3]
    assert np.allclose(world_z, 0.0)                                           # points of the z = 0 plane
    room = RoomBoxDataset(n_pts=2000, n_poses=3)
    c, p = room[1]
    xyz = np.stack([c[f] for f in 'xyz'], 1) + p[:3, 3]
    on_wall = np.isclose(np.abs(xyz), RoomBoxDataset.half, rtol=5e-3).any(axis=1)
    assert on_wall.mean() > 0.99
    k = KittiLikeDataset(n_poses=2, n_rings=8, n_azimuth=64)
    c, p = k[1]
    assert 0 < len(c) <= 8 * 64 and np.isclose(p[0, 3], 1.0)


def test_install_as_reference_package():
    """Unmodified reference callers import `depth_correction.*`; the alias hands them this package."""
    import sys
    import depth_correction_amd
    assert 'depth_correction' not in sys.modules
    depth_correction_amd.install_as('depth_correction')
    try:
        from depth_correction.depth_cloud import DepthCloud as DC
        from depth_correction.loss import min_eigval_loss as f
        from depth_correction.preproc import local_feature_cloud, global_cloud, establish_neighborhoods  # noqa: F401
        from depth_correction.model import ScaledPolynomial as SP
        assert DC is DepthCloud and f is min_eigval_loss and SP is ScaledPolynomial
    finally:
        for k in [k for k in sys.modules if k == 'depth_correction' or k.startswith('depth_correction.')]:
            del sys.modules[k]


def test_filter_grid_host_matches_reference_golden(golden):
    g = golden('grid')
    for keep in ('first', 'last', 'random'):
        for po in (False, True):
            ind = filter_grid(g['points'], float(g['grid_res']), only_mask=True, keep=keep, preserve_order=po,
                              rng=np.random.default_rng(135))
            assert np.array_equal(np.asarray(ind), g['%s_%d' % (keep, po)]), (keep, po)


def test_scan_file_formats_roundtrip(tmp_path):
    from depth_correction_amd.scan_io import (ScanFolderDataset, read_kitti_bin, read_points_csv, read_points_npz,
                                              read_poses_csv, write_poses_csv)
    rng = np.random.default_rng(0)
    pts = rng.uniform(-5, 5, size=(200, 4)).astype(np.float32)
    pts[:10, :2] = rng.uniform(-0.9, 0.9, size=(10, 2))                  # inside the ego box
    d = tmp_path / 'velodyne'
    d.mkdir()
    pts.tofile(str(d / ('%010d.bin' % 7)))
    cloud = read_kitti_bin(str(d / ('%010d.bin' % 7)))
    keep = (np.abs(pts[:, 0]) > 1.0) | (np.abs(pts[:, 1]) > 1.0)
    assert cloud.dtype.names == ('x', 'y', 'z', 'i') and len(cloud) == keep.sum() and np.array_equal(cloud['x'], pts[keep, 0])
    assert len(read_kitti_bin(str(d / ('%010d.bin' % 7)), filter_ego_pts_depth=None)) == 200
    csv = tmp_path / 'scan.csv'
    np.savetxt(str(csv), np.concatenate([np.arange(5)[:, None], pts[:5, :3].astype(np.float64), np.ones((5, 2))], 1),
               delimiter=',', header='id,x,y,z,a,b')
    np.testing.assert_allclose(read_points_csv(str(csv)), pts[:5, :3], rtol=1e-12)
    np.savez(str(tmp_path / 'a.npz'), pts[:, :3])
    np.savez(str(tmp_path / 'b.npz'), cloud=pts[:, :3])
    assert np.array_equal(read_points_npz(str(tmp_path / 'a.npz')), pts[:, :3])
    assert np.array_equal(read_points_npz(str(tmp_path / 'b.npz')), pts[:, :3])
    poses = [np.eye(4), np.eye(4)]
    poses[1][:3, 3] = [1.5, -2.0, 0.25]
    write_poses_csv([7, 9], poses, str(tmp_path / 'poses.csv'))
    ids, back = read_poses_csv(str(tmp_path / 'poses.csv'))
    assert ids == [7, 9] and np.allclose(back[1], poses[1])
    ds = ScanFolderDataset(str(d), str(tmp_path / 'poses.csv'))
    assert len(ds) == 1 and ds.ids == [7]                               # scan 9 has no cloud file
    c, p = ds[0]
    assert len(c) == keep.sum() and np.allclose(p, np.eye(4))


def test_quantile_fallback_beyond_torch_limit_is_the_same_arithmetic():
    """plan._quantile: torch.quantile for inputs it accepts, the same interpolation on an explicit sort beyond its
    16 M-element limit (exercised here by calling the fallback branch directly on small inputs)."""
    import depth_correction_amd.plan as plan
    gen = torch.Generator().manual_seed(4)
    for dtype in (torch.float32, torch.float64):
        for n in (2, 3, 10, 1001, 4096):
            v = torch.rand(n, generator=gen, dtype=dtype) ** 3
            for q in (0.0, 0.3, 0.5, 0.7, 0.9, 1.0):
                want = torch.quantile(v, q, dim=0)
                s, _ = torch.sort(v)
                rank = torch.tensor(q, dtype=dtype) * (n - 1)
                lo = rank.floor().long()
                hi = torch.clamp(lo + 1, max=n - 1)
                got = torch.lerp(s[lo], s[hi], rank - lo.to(dtype))
                assert torch.equal(got, want), (dtype, n, q)
                assert torch.equal(plan._quantile(v, q), want)


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(bytes(bytearray(data.tolist())) if not isinstance(data, (bytes, bytearray)) else data)
    return str(p)


def test_scan_and_pose_readers_match_the_reference_readers(golden, tmp_path):
    """scan_io's host readers on the very files the LIVE reference read when tests/golden/io.npz was generated
    (oracle/gen_golden.py:gen_io): KITTI-360 .bin with the ego-box crop (datasets/kitti360.py:96-109), ASL-laser CSV and
    .npz (asl_laser.py:33-45), FEE-corridor structured .npz (fee_corridor.py:35-38), pose CSVs read (asl_laser.py:48-66,
    fee_corridor.py:41-49) and written (asl_laser.py:59-66: byte for byte)."""
    from numpy.lib.recfunctions import structured_to_unstructured
    from depth_correction_amd import scan_io
    g = golden('io')
    cloud = scan_io.read_kitti_bin(_write(tmp_path, '0000000003.bin', g['kitti_bin'].tobytes()))
    assert cloud.dtype.names == ('x', 'y', 'z', 'i')
    assert np.array_equal(structured_to_unstructured(cloud), g['kitti_xyzi'])
    pts = scan_io.read_points_csv(_write(tmp_path, 'PointCloud7.csv', g['asl_csv'].tobytes()))
    assert np.array_equal(pts, g['asl_csv_points'])
    assert np.array_equal(scan_io.read_points_npz(_write(tmp_path, 'cloud7.npz', g['asl_npz'].tobytes())), g['asl_csv_points'])
    fee = scan_io.read_points_npz(_write(tmp_path, 'scan.npz', g['fee_npz'].tobytes()))
    assert fee.dtype.names == ('x', 'y', 'z', 'vp_x', 'vp_y', 'vp_z') and len(fee) == len(g['fee_f64_depth'])
    ids, poses = scan_io.read_poses_csv(_write(tmp_path, 'poses.csv', g['poses_csv'].tobytes()))
    assert ids == g['poses_ids'].tolist() and np.array_equal(np.stack(poses), g['poses_T'])
    ids, poses = scan_io.read_poses_csv(_write(tmp_path, 'fee_poses.csv', g['fee_poses_csv'].tobytes()))
    assert ids == g['fee_poses_ids'].tolist() and np.array_equal(np.stack(poses), g['fee_poses_T'])
    out = str(tmp_path / 'written.csv')
    scan_io.write_poses_csv(g['poses_ids'].tolist(), list(g['poses_T']), out, ts=[10.5, 11.5, 12.5])
    # the reference wrote the fixture's file from the unrounded poses; what it READ BACK is what we are given, so the bytes
    # agree wherever nine decimals survive the round trip -- which is everywhere
    assert open(out, 'rb').read() == g['poses_csv'].tobytes()


def test_caller_script_helpers_match_the_reference(golden, capsys):
    """utils.delta_transform / rotation_angle / translation_norm / transform_inv and the NoisyPoseDataset / NoisyDepthDataset
    wrappers against the LIVE reference (tests/golden/helpers.npz; euler_matrix of ROS' tf substituted on both sides)."""
    from numpy.lib.recfunctions import structured_to_unstructured, unstructured_to_structured
    from depth_correction_amd import dataset as D, utils as U
    g = golden('helpers')
    Ts = g['poses']
    for k, T in enumerate(Ts):
        np.testing.assert_allclose(U.delta_transform(Ts[0], T), g['delta'][k], rtol=1e-12, atol=1e-14)
        assert abs(U.rotation_angle(T) - g['rotation_angle'][k]) < 1e-14
        assert abs(U.translation_norm(T) - g['translation_norm'][k]) < 1e-14
        np.testing.assert_allclose(U.transform_inv(T), g['transform_inv'][k], rtol=1e-14, atol=1e-16)
    cloud = unstructured_to_structured(g['cloud_xyz'], names=['x', 'y', 'z'])
    base = [(cloud.copy(), T) for T in Ts]
    for mode in ('pose', 'common'):
        ds = D.NoisyPoseDataset(base, noise=g['pose_noise'].tolist(), mode=mode)
        np.testing.assert_allclose(np.stack([p for _, p in ds]), g['noisy_pose_' + mode], rtol=1e-13, atol=1e-15)
    assert np.array_equal(g['noisy_pose_pose'][0], Ts[0]) and not np.allclose(g['noisy_pose_common'][0], Ts[0])
    ds = D.NoisyDepthDataset([(cloud.copy(), Ts[0])], noise=0.05)
    np.testing.assert_allclose(structured_to_unstructured(next(iter(ds))[0][['x', 'y', 'z']]), g['noisy_depth_xyz'], rtol=1e-13)
    capsys.readouterr()


CALLER_IMPORTS = {
    # the import lines of the reference's caller scripts that this package answers under install_as('depth_correction'):
    'scripts/train_demo': {'config': ['Config', 'Loss', 'Model', 'NeighborhoodType', 'PoseCorrection'],
                           'dataset': ['create_dataset', 'noisy_dataset', 'NoisyPoseDataset'], 'depth_cloud': ['DepthCloud'],
                           'model': ['load_model', 'model_by_name'], 'preproc': ['filtered_cloud', 'global_cloud', 'local_feature_cloud'],
                           'train': ['train', 'TrainCallbacks'], 'utils': ['delta_transform', 'rotation_angle', 'timing', 'translation_norm']},
    'scripts/model_poses_learning': {'depth_cloud': ['DepthCloud'], 'model': ['ScaledPolynomial'],
                                     'preproc': ['filtered_cloud', 'local_feature_cloud', 'establish_neighborhoods', 'compute_neighborhood_features'],
                                     'config': ['Config', 'PoseCorrection', 'Loss', 'NeighborhoodType'], 'loss': ['icp_loss', 'create_loss'],
                                     'eval': ['create_corrected_poses', 'global_cloud']},
    'scripts/model_poses_learning_icp': {'depth_cloud': ['DepthCloud'], 'model': ['ScaledPolynomial'], 'preproc': ['local_feature_cloud'],
                                         'config': ['Config', 'PoseCorrection'], 'loss': ['icp_loss'], 'eval': ['create_corrected_poses', 'global_cloud'],
                                         'io': ['write', 'append'], 'dataset': ['NoisyPoseDataset', 'FilteredDataset'],
                                         'transform': ['matrix_to_xyz_axis_angle', 'xyz_axis_angle_to_matrix']},
    'scripts/depth_correction': {'config': ['Config'], 'model': ['load_model'], 'preproc': ['local_feature_cloud']},
    'examples/optimization': {'dataset': ['create_dataset'], 'depth_cloud': ['DepthCloud'], 'model': ['ScaledPolynomial'],
                              'preproc': ['filtered_cloud', 'local_feature_cloud', 'establish_neighborhoods', 'compute_neighborhood_features'],
                              'config': ['Config', 'PoseCorrection', 'Loss', 'NeighborhoodType'], 'loss': ['create_loss'],
                              'eval': ['create_corrected_poses', 'global_cloud']},
    'examples/optimization_icp': {'dataset': ['create_dataset'], 'depth_cloud': ['DepthCloud'], 'model': ['ScaledPolynomial'],
                                  'preproc': ['filtered_cloud'], 'config': ['Config'], 'loss': ['point_to_plane_dist']},
}
# what those scripts import beyond it -- ROS / data-set / viewer glue that stays outside
NOT_PROVIDED = {'scripts/train_demo': ['point_cloud.PointCloud'],
                'scripts/model_poses_learning': ['datasets.fee_corridor.Dataset', 'datasets.fee_corridor.dataset_names'],
                'scripts/model_poses_learning_icp': ['datasets.fee_corridor.Dataset', 'datasets.fee_corridor.dataset_names',
                                                     'datasets.fee_corridor.seq_names'],
                'examples/optimization': ['visualization.visualize_dataset']}


def test_caller_script_imports_resolve_under_install_as():
    import importlib
    import sys
    import depth_correction_amd
    depth_correction_amd.install_as('depth_correction')
    try:
        for script, mods in CALLER_IMPORTS.items():
            for mod, names in mods.items():
                m = importlib.import_module('depth_correction.' + mod)
                for n in names:
                    assert hasattr(m, n), '%s: depth_correction.%s.%s does not resolve' % (script, mod, n)
        for script, names in NOT_PROVIDED.items():                    # stated as absent: make sure the statement stays true
            for dotted in names:
                mod = dotted.rsplit('.', 1)[0]
                with pytest.raises(ImportError):
                    importlib.import_module('depth_correction.' + mod)
    finally:
        for k in [k for k in sys.modules if k == 'depth_correction' or k.startswith('depth_correction.')]:
            del sys.modules[k]


def test_cat_rows_views_consecutive_slices_and_copies_the_rest():
    """ops.cat_rows (the plan's concatenation of per-scan arrays): consecutive row ranges of one contiguous tensor come back as a
    view of it -- no copy, same storage -- anything else as torch.cat."""
    import torch
    from depth_correction_amd import ops
    base = torch.arange(60, dtype=torch.float32).reshape(20, 3)
    parts = [base[0:7], base[7:12], base[12:20]]
    out = ops.cat_rows(parts)
    assert out.data_ptr() == base.data_ptr() and out.shape == (20, 3) and torch.equal(out, base)
    mid = ops.cat_rows([base[7:12], base[12:20]])
    assert mid.data_ptr() == base[7:].data_ptr() and torch.equal(mid, base[7:])
    col = torch.arange(20, dtype=torch.float32).reshape(20, 1)
    assert ops.cat_rows([col[:5], col[5:]]).reshape(-1).data_ptr() == col.data_ptr()
    flat = torch.arange(20)
    assert ops.cat_rows([flat[:5], flat[5:]]).data_ptr() == flat.data_ptr()
    # not consecutive, different bases, a gap, a single part, a non-contiguous part: copies with the right content
    for bad in ([base[7:12], base[0:7]], [base[0:7], base.clone()[7:12]], [base[0:7], base[8:12]], [base[3:9]], [base[:, :2][0:4], base[:, :2][4:8]]):
        got = ops.cat_rows(bad)
        assert torch.equal(got, torch.cat(bad)) and (len(bad) == 1 or got.data_ptr() not in [b.data_ptr() for b in bad])


def test_filter_grid_host_at_voxel_faces(golden):
    """filter_grid on host arrays that sit on the voxel faces (fp32 and fp64, resolutions whose division rounds) and on a
    clustered cloud with negative coordinates, against the live reference's survivors."""
    g = golden('filters_edge')
    for name in g['grid_names'].tolist():
        pts, res = g[name + '_points'], float(g[name + '_res'])
        for keep in ('first', 'last', 'random'):
            for po in (False, True):
                ind = filter_grid(pts, res, only_mask=True, keep=keep, preserve_order=po, rng=np.random.default_rng(135))
                assert np.array_equal(np.asarray(ind), g['%s_%s_%d' % (name, keep, po)]), (name, keep, po)


@pytest.mark.parametrize('tag', ['f32', 'f64'])
def test_within_bounds_uses_the_float32_bound(golden, tag):
    """within_bounds on CPU tensors against the reference's masks on values and ratios that equal float32(bound), its
    neighbouring floats and the unrounded bound: the reference compares with torch.tensor(bound), a float32 scalar."""
    g = golden('filters_edge')
    ev = torch.as_tensor(g[tag + '_eigvals'])
    cloud = DepthCloud(torch.zeros_like(ev), torch.zeros_like(ev), torch.zeros_like(ev[:, :1]))
    cloud.eigvals = ev
    from depth_correction_amd.filters import (filter_eigenvalue, filter_eigenvalue_ratio, filter_eigenvalue_ratios,
                                              filter_eigenvalues)
    nn = lambda b: None if b != b else b
    for (e, lo, hi), want in zip(g['value_cases'].tolist(), g[tag + '_value_masks']):
        assert np.array_equal(within_bounds(ev[:, int(e)], min=nn(lo), max=nn(hi)).numpy(), want), (e, lo, hi)
        assert np.array_equal(within_bounds(ev[:, int(e)], bounds=[lo, hi]).numpy(), want), (e, lo, hi)
        assert np.array_equal(filter_eigenvalue(cloud, int(e), min=nn(lo), max=nn(hi), only_mask=True).numpy(), want)
    for (i, j, lo, hi), want in zip(g['ratio_cases'].tolist(), g[tag + '_ratio_masks']):
        got = filter_eigenvalue_ratio(cloud, (int(i), int(j)), min=nn(lo), max=nn(hi), only_mask=True)
        assert np.array_equal(got.numpy(), want), (i, j, lo, hi)
    vb = [[int(e), lo, hi] for e, lo, hi in g['value_cases'][:3].tolist()]
    rb = [[int(i), int(j), lo, hi] for i, j, lo, hi in g['ratio_cases'][:3].tolist()]
    assert np.array_equal(filter_eigenvalues(cloud, vb, only_mask=True).numpy(), g[tag + '_values_all'])
    assert np.array_equal(filter_eigenvalue_ratios(cloud, rb, only_mask=True).numpy(), g[tag + '_ratios_all'])
    x = torch.tensor([float(np.float32(0.0004)), float(np.float32(0.1))], dtype=ev.dtype)
    assert within_bounds(x, min=0.0004, max=0.1).tolist() == [True, True]


def test_device_bounds_are_rounded_like_the_reference():
    """What the mask kernels and the depth bounds of cloud_from_points receive: the widened float32 value of the bound
    (torch.tensor(bound)); None and NaN mean unbounded, infinities stay."""
    from depth_correction_amd.ops import _bound
    inf = float('inf')
    assert _bound(0.0004, -inf) == float(np.float32(0.0004)) < 0.0004 and _bound(0.1, inf) == float(np.float32(0.1)) > 0.1
    assert _bound(0.25, inf) == 0.25 and _bound(5, -inf) == 5.0
    assert _bound(None, -inf) == -inf and _bound(float('nan'), inf) == inf and _bound(inf, inf) == inf and _bound(-inf, 0.0) == -inf
