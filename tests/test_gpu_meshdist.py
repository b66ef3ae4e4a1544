"""Map accuracy on the MI355X (csrc/dc_meshdist.hip, metrics.point_to_mesh_distance / map_accuracy, eval.eval_map, MeshDataset):
the closest-point query against a numpy brute force over every (point, face) pair (tests/mesh_reference.py, itself held to
analytic cases by tests/test_meshdist_host.py), its tie rule against the host build of the kernel's own arithmetic, the edges of
its contract, the sampler against its numpy restatement, the new metric against the chamfer distance, and the evaluation end to
end on the pillared room of the SLAM tests.

Bars.  Distances: 2^-40 x scene extent (3.6e-11 m at 40 m).  The arithmetic is some tens of fp64 roundings of coordinates of
that size (~1e-14 m), so the bar has three orders of headroom and sits seven below a millimetre.  Faces are compared where the
reference's second-best distance exceeds its best by more than 1e-9 x extent; the rows left out are capped (1 % on the soup, 5 %
on the watertight room, where a point nearest to an edge is equally near two faces)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mesh_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')


def _soup(n_faces=5000, shift=0.0):
    """The triangle soup of test_gpu_raycast.test_cast_matches_brute_force: centres uniform in +-20 m, vertices N(0, 0.4 m)."""
    from depth_correction_amd.mesh import TriangleMesh
    rng = np.random.default_rng(7)
    c = rng.uniform(-20, 20, size=(n_faces, 1, 3))
    v = (c + rng.normal(scale=0.4, size=(n_faces, 3, 3))).reshape(-1, 3) + shift
    return TriangleMesh(v, np.arange(3 * n_faces).reshape(-1, 3))


def _room():
    from depth_correction_amd.mesh import room_mesh
    return room_mesh((8, 5, 2), cell=1.0, pillars=[((2, 1, 0), (0.5, 0.5, 2)), ((-3, -2, 0), (0.4, 0.6, 2))])


def _closest(mesh, pts, **kw):
    from depth_correction_amd.ops import mesh_closest
    bvh = mesh.on_device(DEV)[3]
    t = pts if isinstance(pts, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(pts), device=DEV)
    face, dist, closest = mesh_closest(bvh, t, **kw)
    torch.cuda.synchronize()
    return face.cpu().numpy(), dist.cpu().numpy(), None if closest is None else closest.cpu().numpy()


def _host():
    lib = ctypes.CDLL(HOSTLIB)
    lib.dc_host_closest_on_triangle.restype = ctypes.c_double
    lib.dc_host_closest_on_triangle.argtypes = [ctypes.c_void_p] * 4
    return lib


def _host_d2(lib, tri, p):
    tri, p, q = np.ascontiguousarray(tri, np.float64).reshape(9), np.ascontiguousarray(p, np.float64), np.zeros(3)
    return lib.dc_host_closest_on_triangle(tri.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p),
                                           q.ctypes.data_as(ctypes.c_void_p), None)


def _check_against_brute_force(mesh, pts, extent, cap, what, tie_rule=False):
    """The device's answer for ``pts`` against the brute force: distances within the bar on every row, faces on the rows the
    reference decides clearly (at most ``cap`` of the rows left out), the returned face and point consistent on every row; with
    ``tie_rule`` the rows left out are decided by the host build of the kernel's arithmetic.  Returns the largest deviation."""
    bar, gap = 2.0 ** -40 * extent, 1e-9 * extent
    face, dist, closest = _closest(mesh, pts)
    ref_f, ref_d, second = R.brute_force(mesh.vertices, mesh.faces, pts)
    dev = np.abs(dist - ref_d)
    print('%s: %d queries, largest |dist - reference| = %.3g m (bar %.3g m), distances %.3g .. %.3g m'
          % (what, len(pts), dev.max(), bar, ref_d.min(), ref_d.max()))
    assert (face >= 0).all() and np.isfinite(dist).all()
    assert dev.max() <= bar, (what, dev.max(), bar, int(dev.argmax()))
    clear = second - ref_d > gap
    left_out = 1.0 - clear.mean()
    print('%s: %.2f %% of the rows left out of the face comparison (cap %.0f %%)' % (what, 100 * left_out, 100 * cap))
    assert left_out <= cap, (what, left_out)
    assert np.array_equal(face[clear], ref_f[clear]), (what, np.flatnonzero(clear & (face != ref_f))[:10])
    # every row: the distance from the query to the RETURNED face equals dist, and closest lies on that face, at that distance
    d_own, _ = R.distance_to_faces(mesh.vertices, mesh.faces, pts, face)
    assert np.abs(d_own - dist).max() <= bar, (what, np.abs(d_own - dist).max())
    on_face, _ = R.distance_to_faces(mesh.vertices, mesh.faces, closest, face)
    assert on_face.max() <= bar, (what, on_face.max())
    assert np.abs(np.linalg.norm(pts - closest, axis=1) - dist).max() <= bar
    if tie_rule:
        lib = _host()
        rows = np.flatnonzero(~clear)
        all_d = R.all_distances(mesh.vertices, mesh.faces, pts[rows])
        tri = mesh.vertices[mesh.faces]
        for r, d_row in zip(rows, all_d):
            cand = np.flatnonzero(d_row - d_row.min() <= gap)            # the reference's best faces (two at an edge, more at a corner)
            assert len(cand) >= 2 and face[r] in cand, (what, r, face[r], cand)
            keyed = sorted((_host_d2(lib, tri[f], pts[r]), int(f)) for f in cand)
            assert face[r] == keyed[0][1], (what, r, face[r], keyed[:3])
            assert dist[r] == math.sqrt(keyed[0][0]), (what, r)
        print('%s: tie rule checked on %d rows' % (what, len(rows)))
    return dev.max()


def test_soup_matches_brute_force():
    mesh = _soup()
    rng = np.random.default_rng(21)
    near, _ = R.sample(mesh.vertices, mesh.faces, 2000, 3)
    pts = np.concatenate([rng.uniform(-22, 22, size=(2000, 3)), near + rng.normal(scale=0.02, size=near.shape)])
    _check_against_brute_force(mesh, pts, 40.0, 0.01, 'soup')


def test_room_matches_brute_force_and_tie_rule():
    mesh = _room()
    assert len(mesh) == 1148
    rng = np.random.default_rng(22)
    surf, _ = R.sample(mesh.vertices, mesh.faces, 4000, 5)
    _check_against_brute_force(mesh, surf + rng.normal(scale=0.02, size=surf.shape), 16.0, 0.05, 'room', tie_rule=True)


def test_exact_ties_go_to_the_lower_face():
    """Queries EXACTLY as near to several faces (on the bisector plane of a pillar's edge, off a corner, over a shared diagonal:
    small binary fractions, so every d^2 is exact): the lowest face index among the exactly equal ones, in any query order."""
    mesh = _room()
    pts = np.array([[2.75, 1.75, 0.25], [2.75, 1.75, 0.5], [1.25, 0.25, -0.5], [2.0, 1.75, 0.5], [3.0, 1.0, 0.5], [0.5, 0.5, -1.75],
                    [0.25, 0.25, -1.5], [6.5, -3.5, 1.0]])
    face, dist, _ = _closest(mesh, pts)
    all_d = R.all_distances(mesh.vertices, mesh.faces, pts)
    ties = 0
    for r in range(len(pts)):
        equal = np.flatnonzero(all_d[r] == all_d[r].min())
        ties += len(equal) > 1
        assert face[r] == equal[0] and dist[r] == all_d[r].min(), (r, face[r], equal)
    assert ties >= 4
    perm = np.random.default_rng(0).permutation(len(pts))
    f2, d2, _ = _closest(mesh, pts[perm])
    assert np.array_equal(f2, face[perm]) and np.array_equal(d2, dist[perm])


def test_order_independence_and_determinism():
    mesh = _soup()
    rng = np.random.default_rng(23)
    pts = rng.uniform(-22, 22, size=(50000, 3))
    a = _closest(mesh, pts)
    b = _closest(mesh, pts)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    perm = rng.permutation(len(pts))
    c = _closest(mesh, pts[perm])
    for x, y in zip(a, c):
        assert np.array_equal(x[perm], y)
    p32 = pts.astype(np.float32)
    d = _closest(mesh, torch.as_tensor(p32, device=DEV))
    e = _closest(mesh, p32.astype(np.float64))
    for x, y in zip(d, e):
        assert np.array_equal(x, y)
    # without the closest points: the same faces and distances
    f = _closest(mesh, pts, want_closest=False)
    assert f[2] is None and np.array_equal(f[0], a[0]) and np.array_equal(f[1], a[1])


def test_contract_edges():
    from depth_correction_amd.mesh import TriangleMesh
    rng = np.random.default_rng(24)
    # one face: the root is a leaf
    one = TriangleMesh([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]], [[0, 1, 2]])
    pts = rng.uniform(-6, 6, size=(500, 3))
    face, dist, closest = _closest(one, pts)
    ref_f, ref_d, _ = R.brute_force(one.vertices, one.faces, pts)
    assert (face == 0).all() and np.abs(dist - ref_d).max() <= 2.0 ** -40 * 12.0
    # no points
    face, dist, closest = _closest(one, np.zeros((0, 3)))
    assert face.shape == (0,) and dist.shape == (0,) and closest.shape == (0, 3)
    # max_dist: found exactly at the bound, not beyond it
    over = np.array([[1.0, 1.0, 3.0], [1.0, 1.0, 3.0 + 2.0 ** -40], [-3.0, -4.0, 0.0], [1.0, 1.0, -0.5]])
    face, dist, closest = _closest(one, over, max_dist=3.0)
    assert np.array_equal(face, [0, -1, -1, 0]) and np.array_equal(dist[[0, 3]], [3.0, 0.5]) and np.isinf(dist[[1, 2]]).all()
    assert np.isnan(closest[[1, 2]]).all() and np.array_equal(closest[0], [1.0, 1.0, 0.0])
    face, dist, _ = _closest(one, over, max_dist=5.0)
    assert np.array_equal(face, [0, 0, 0, 0]) and dist[2] == 5.0
    for unbounded in (None, 0.0, -1.0, float('inf')):
        assert (_closest(one, over, max_dist=unbounded)[0] == 0).all()
    soup = _soup()
    pts = rng.uniform(-22, 22, size=(20000, 3))
    free = _closest(soup, pts)
    for bound in (0.3, 1.0):
        got = _closest(soup, pts, max_dist=bound)
        found = free[1] <= bound
        assert 0.02 < found.mean() < 0.98
        assert np.array_equal(got[0] >= 0, found)
        for x, y in zip(got, free):
            assert np.array_equal(x[found], y[found])                 # bit-equal to the unbounded call's
        assert (got[0][~found] == -1).all() and np.isinf(got[1][~found]).all() and np.isnan(got[2][~found]).all()
    # NaN and infinite query rows disturb no other row
    bad = pts[:1000].copy()
    rows = np.arange(0, 1000, 7)
    bad[rows[0::3], 0] = np.nan
    bad[rows[1::3], 1] = np.inf
    bad[rows[2::3], 2] = -np.inf
    got = _closest(soup, bad)
    good = np.ones(1000, dtype=bool)
    good[rows] = False
    assert (got[0][rows] == -1).all() and np.isinf(got[1][rows]).all() and np.isnan(got[2][rows]).all()
    for x, y in zip(got, free):
        assert np.array_equal(x[good], y[:1000][good])
    # more than one trip of any grid-stride loop
    many = rng.uniform(-22, 22, size=(300001, 3))
    face, dist, closest = _closest(soup, many)
    spot = np.concatenate([rng.choice(300001, size=1998, replace=False), [0, 300000]])
    ref_f, ref_d, second = R.brute_force(soup.vertices, soup.faces, many[spot])
    assert np.abs(dist[spot] - ref_d).max() <= 2.0 ** -40 * 40.0
    clear = second - ref_d > 4e-8
    assert clear.mean() >= 0.99 and np.array_equal(face[spot][clear], ref_f[clear])


def test_degenerate_faces_next_to_proper_ones():
    from depth_correction_amd.mesh import TriangleMesh
    rng = np.random.default_rng(25)
    base = _soup(400)
    v, f = [base.vertices], [base.faces]
    off = len(base.vertices)
    centres = []
    for k in range(60):                                               # exactly representable: collinear, two equal, three equal
        a = np.round(rng.uniform(-20, 20, size=3) * 4) / 4
        d = np.round(rng.normal(size=3) * 4) / 8 + np.array([0.125, 0.0, 0.0])
        tri = [(a, a + d, a + 2 * d), (a, a + 2 * d, a + d), (a, a, a + d), (a, a + d, a + d), (a, a, a)][k % 5]
        v.append(np.stack(tri))
        f.append(np.array([[off, off + 1, off + 2]]))
        off += 3
        centres.append(a + d)
    mesh = TriangleMesh(np.concatenate(v), np.concatenate(f))
    centres = np.stack(centres)
    pts = np.concatenate([centres[rng.integers(0, len(centres), size=1500)] + rng.normal(scale=0.3, size=(1500, 3)),
                          centres, rng.uniform(-22, 22, size=(1000, 3))])
    face, dist, closest = _closest(mesh, pts)
    assert np.isfinite(dist).all() and np.isfinite(closest).all()
    assert (face >= len(base)).mean() > 0.3                           # the degenerate faces do win where they are nearest
    _check_against_brute_force(mesh, pts, 40.0, 0.05, 'degenerate')


def test_pruning_is_conservative_at_large_coordinates():
    """The soup shifted by 1e4 m, where fp32 boxes are coarse (ulp 1e-3 m), queries from 1e-9 m to 1e3 m off the surface: a margin
    that is too small shows as a distance above the brute force's."""
    shift = 1.0e4
    mesh = _soup(shift=shift)
    rng = np.random.default_rng(26)
    surf, _ = R.sample(mesh.vertices, mesh.faces, 2000, 9)
    d = rng.normal(size=surf.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = surf + d * (10.0 ** rng.uniform(-9, 3, size=(len(surf), 1)))
    extent = shift + 20.0
    _check_against_brute_force(mesh, pts, extent, 0.01, 'shifted soup')


def test_sampler():
    from depth_correction_amd.mesh import TriangleMesh
    from depth_correction_amd.metrics import point_to_mesh_distance
    mesh = _room()
    pts, nrm, face = mesh.sample(200000, seed=135, device=DEV)
    assert pts.dtype == torch.float64 and face.dtype == torch.int32 and pts.shape == (200000, 3) and nrm.shape == (200000, 3)
    ref_p, ref_f = R.sample(mesh.vertices, mesh.faces, 200000, 135)
    assert np.array_equal(face.cpu().numpy(), ref_f) and np.array_equal(pts.cpu().numpy(), ref_p)
    assert np.array_equal(nrm.cpu().numpy(), mesh.face_normals()[ref_f])
    again = mesh.sample(200000, seed=135, device=DEV)
    assert torch.equal(again[0], pts) and torch.equal(again[2], face)
    other = mesh.sample(200000, seed=136, device=DEV)
    assert not torch.equal(other[0], pts)
    assert np.array_equal(other[0].cpu().numpy(), R.sample(mesh.vertices, mesh.faces, 200000, 136)[0])
    # a prefix of a longer draw is the shorter draw (a pure function of (mesh, seed, i)), and n = 0 is empty
    assert torch.equal(mesh.sample(1000, seed=135, device=DEV)[0], pts[:1000])
    assert mesh.sample(0, device=DEV)[0].shape == (0, 3)
    # the two kernels against each other: every sample lies on its own mesh
    d = point_to_mesh_distance(pts, mesh)
    print('largest distance of a sample from its mesh: %.3g m' % d.max().item())
    assert d.max().item() <= 2.0 ** -40 * 16.0
    # areas 1 : 3
    two = TriangleMesh([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 0, 0], [0, 0, 5]], [[0, 1, 2], [0, 3, 2]])
    np.testing.assert_allclose(two.face_areas(), [1.0, 3.0])
    n = 200000
    f = two.sample(n, seed=7, device=DEV)[2].cpu().numpy()
    share = (f == 0).mean()
    assert abs(share - 0.25) <= 5 * math.sqrt(0.25 * 0.75 / n), share
    with pytest.raises(ValueError):
        TriangleMesh([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0, 1, 2]]).sample(10, device=DEV)


def test_metric_against_chamfer():
    """Distance to a surface is never above the distance to points sampled on it, and denser samples close the gap."""
    from depth_correction_amd.metrics import chamfer_distance, map_accuracy, point_to_mesh_distance
    mesh = _room()
    rng = np.random.default_rng(27)
    surf, _ = R.sample(mesh.vertices, mesh.faces, 30000, 11)
    noisy = torch.as_tensor(surf + rng.normal(scale=0.02, size=surf.shape), device=DEV)
    d_mesh = point_to_mesh_distance(noisy, mesh)
    assert d_mesh.dtype == torch.float64 and d_mesh.shape == (30000,)
    bar = 2.0 ** -40 * 16.0
    gaps = {}
    for n in (200000, 20000):
        cloud = mesh.sample(n, seed=135, device=DEV)[0]
        d_cloud = chamfer_distance(noisy, cloud, apply_point_reduction=False)
        assert (d_mesh <= d_cloud + bar).all(), (n, (d_mesh - d_cloud).max().item())
        gaps[n] = (d_cloud - d_mesh).mean().item()
    print('mean gap chamfer - mesh distance: %s' % gaps)
    assert gaps[200000] < gaps[20000]
    # float32 points give float32 distances; a DepthCloud's points are used
    from depth_correction_amd.depth_cloud import DepthCloud
    d32 = point_to_mesh_distance(noisy.float(), mesh)
    assert d32.dtype == torch.float32 and (d32.double() - d_mesh).abs().max().item() < 1e-5
    dc = DepthCloud.from_points(noisy, dtype=torch.float64, device=DEV)
    assert (point_to_mesh_distance(dc, mesh) - d_mesh).abs().max().item() < 1e-12
    acc = map_accuracy(noisy, mesh, n_samples=20000)
    dn = d_mesh.cpu().numpy()
    assert acc['n'] == 30000 and abs(acc['mean'] - dn.mean()) < 1e-15 and abs(acc['median'] - np.median(dn)) < 1e-15
    assert abs(acc['trimmed_mean'] - dn[dn <= np.quantile(dn, 0.8)].mean()) < 1e-15 and abs(acc['rms'] - np.sqrt((dn ** 2).mean())) < 1e-15
    assert abs(acc['signed_mean']) < acc['mean'] and 0.0 < acc['completeness_mean'] < 0.2
    with pytest.raises(RuntimeError):
        point_to_mesh_distance(noisy.cpu(), mesh)


# ---- end to end: the 24-pose pillared room of tests/test_gpu_slam.py, built the same way ---------------------------------------
def _pose(yaw, t):
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(0.0, 0.0, yaw)
    T[:3, 3] = t
    return T


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = tmp_path_factory.mktemp('map') / 'pillared_room.ply'
    mesh.save_ply(str(path))
    return str(path)


def _dataset(room, n=24, size=(64, 512)):
    from depth_correction_amd.dataset import RenderedMeshDataset
    poses = np.stack([_pose(0.04 * i, (-3.0 + 0.25 * i, 0.3 * math.sin(i / 3.0), 0.02 * math.sin(i / 2.0))) for i in range(n)])
    return RenderedMeshDataset(room, poses=poses, size=size, fov=(45.0, 360.0), num_segments=16, device=DEV)


def _cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    base.update(kw)
    return Config(**base)


def test_eval_map_end_to_end(room, tmp_path):
    from depth_correction_amd.dataset import DepthBiasDataset, RoomBoxDataset
    from depth_correction_amd.eval import eval_map
    from depth_correction_amd.model import ScaledPolynomial
    ds = _dataset(room)
    # (a) unbiased scans at the poses they were rendered from: every map point lies on the mesh
    cfg = _cfg(map_eval_csv=str(tmp_path / 'map.csv'))
    plain = eval_map(cfg, test_datasets=[ds], model=None)[0]      # None: the configuration's model, whose default weights are zero
    print('(a) unbiased: %s' % plain)
    assert plain['n'] > 10000 and plain['max'] <= 1e-10, plain
    # (b) a known bias, with and without the model that removes it
    w = 0.05
    biased = DepthBiasDataset(ds, ScaledPolynomial(w=[w], exponent=[2.0], device=DEV), cfg=cfg)
    raw = eval_map(cfg, test_datasets=[biased], model=None)[0]
    fixed = eval_map(cfg, test_datasets=[biased], model=ScaledPolynomial(w=[w], exponent=[2.0], device=DEV))[0]
    print('(b) biased, no correction: %s' % raw)
    print('(b) biased, true model:    %s' % fixed)
    assert fixed['mean'] < raw['mean'] and fixed['trimmed_mean'] < raw['trimmed_mean'], (fixed, raw)
    lines = open(cfg.map_eval_csv).read().splitlines()
    assert len(lines) == 3 and all(len(line.split(' ')) == 7 and line.split(' ')[0] == str(ds) for line in lines)
    # (c) the map the mapper would have built: the poses of run_slam
    cfg_slam = _cfg(map_eval_poses='slam', map_eval_csv=str(tmp_path / 'slam_map.csv'), odom_cov=[1e-4] * 3 + [2.5e-3] * 3)
    slam = eval_map(cfg_slam, test_datasets=[biased], model=ScaledPolynomial(w=[w], exponent=[2.0], device=DEV))[0]
    print('(c) biased, true model, SLAM poses: %s' % slam)
    assert slam['n'] > 0 and all(math.isfinite(slam[k]) for k in ('mean', 'rms', 'median', 'trimmed_mean', 'signed_mean'))
    parts = open(cfg_slam.map_eval_csv).read().splitlines()[0].split(' ')
    assert len(parts) == 7 and parts[0] == str(ds) and int(parts[1]) == slam['n'] and all(len(p.split('.')[1]) == 9 for p in parts[2:])
    # a dataset without a mesh is refused by name
    with pytest.raises(ValueError, match='room'):
        eval_map(_cfg(), test_datasets=[RoomBoxDataset(n_pts=1000, n_poses=2)], model=ScaledPolynomial(w=[0.0], exponent=[2.0], device=DEV))
    with pytest.raises(ValueError, match='map_eval_poses'):
        eval_map(_cfg(map_eval_poses='odometry'), test_datasets=[ds], model=ScaledPolynomial(w=[0.0], exponent=[2.0], device=DEV))


def test_mesh_dataset(tmp_path):
    from depth_correction_amd.dataset import MeshDataset, create_dataset
    from depth_correction_amd.metrics import point_to_mesh_distance
    mesh = _room()
    path = str(tmp_path / 'room.ply')
    mesh.save_ply(path)
    ds = MeshDataset(path, n_poses=5, n_pts_to_sample=200000, device=DEV)
    assert len(ds) == 5 and ds.n_pts == 200000 and str(ds) == path and len(ds.get_mesh()) == len(mesh)
    assert np.array_equal(ds.pts, R.sample(mesh.vertices, mesh.faces, 200000, 135)[0])
    assert len(ds[[0, 2]]) == 2 and len(ds[1:4]) == 3 and list(ds[1:4].ids) == [1, 2, 3] and ds[[4, 0]].ids == [4, 0]
    cloud, pose = ds[[0, 2]][1]
    assert np.array_equal(pose, ds.cloud_pose(2)) and np.array_equal(cloud, ds.local_cloud(2))
    bar = 2.0 ** -40 * 16.0
    normals = mesh.face_normals()
    for i, (cloud, pose) in enumerate(ds):
        assert len(cloud) == 200000 // 5 and pose.shape == (4, 4)
        x = np.stack([cloud[f] for f in 'xyz'], axis=1) @ pose[:3, :3].T + pose[:3, 3]
        n = np.stack([cloud[f] for f in ('normal_x', 'normal_y', 'normal_z')], axis=1) @ pose[:3, :3].T
        d, face, _ = point_to_mesh_distance(torch.as_tensor(x, device=DEV), mesh, return_closest=True)
        assert d.max().item() <= bar, (i, d.max().item())
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
        rows = np.arange(0, len(x), 40)[:1000]
        ref_f, ref_d, second = R.brute_force(mesh.vertices, mesh.faces, x[rows])
        clear = second - ref_d > 1e-9 * 16.0
        assert clear.mean() > 0.9 and np.array_equal(face.cpu().numpy()[rows][clear], ref_f[clear])
        assert np.array_equal(n[rows][clear], normals[ref_f[clear]])
    # a crop smaller than the room drops the samples outside
    small = MeshDataset(path, n_poses=2, n_pts_to_sample=20000, size=([-4.0, 4.0], [-10.0, 10.0], [-10.0, 10.0]), device=DEV)
    assert 0 < small.n_pts < 20000 and np.abs(small.pts[:, 0]).max() <= 4.0
    made = create_dataset('mesh/' + path, n_pts_to_sample=1000, n_poses=2)
    assert isinstance(made, MeshDataset) and len(made) == 2 and made.n_pts == 1000
