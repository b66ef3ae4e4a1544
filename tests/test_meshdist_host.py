"""Map accuracy on the host (no GPU): the reference of the GPU tests (tests/mesh_reference.py) against analytic cases, the
kernel's per-triangle arithmetic and the sampler's three lines through their host build (libdc_hostcheck.so, the header the
kernels include) against that reference, the statistics of map_accuracy against numpy, the new Config fields and file names."""
import ctypes
import os

import numpy as np
import pytest

import mesh_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')
REGIONS = {0: 'vertex a', 1: 'vertex b', 2: 'vertex c', 3: 'edge ab', 4: 'edge ca', 5: 'edge bc', 6: 'interior', 7: 'thin'}


@pytest.fixture(scope='module')
def host():
    if not os.path.exists(LIB) or not hasattr(ctypes.CDLL(LIB), 'dc_host_closest_on_triangle'):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    lib.dc_host_closest_on_triangle.restype = ctypes.c_double
    lib.dc_host_closest_on_triangle.argtypes = [ctypes.c_void_p] * 4
    lib.dc_host_mesh_sample_point.restype = None
    lib.dc_host_mesh_sample_point.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.dc_host_mesh_sample_face.restype = ctypes.c_int64
    lib.dc_host_mesh_sample_face.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _closest(host, tri, p):
    """(d2, closest [3], region) of dc_host_closest_on_triangle for one triangle [3,3] and one point [3]."""
    tri, p = np.ascontiguousarray(tri, dtype=np.float64).reshape(9), np.ascontiguousarray(p, dtype=np.float64)
    q = np.zeros(3)
    reg = ctypes.c_int(-1)
    d2 = host.dc_host_closest_on_triangle(_p(tri), _p(p), _p(q), ctypes.byref(reg))
    return d2, q, reg.value


# ---- the reference against analytic cases ---------------------------------------------------------------------------------------
def test_reference_analytic_triangle():
    a, b, c = np.array([0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0]), np.array([0.0, 3.0, 0.0])
    cases = [((1.0, 1.0, 2.5), 2.5, (1.0, 1.0, 0.0)),                  # over the interior: the plane distance
             ((2.0, -1.5, 2.0), 2.5, (2.0, 0.0, 0.0)),                 # beyond the edge ab: point-segment
             ((-3.0, -4.0, 12.0), 13.0, (0.0, 0.0, 0.0)),              # beyond the vertex a
             ((7.0, -4.0, 0.0), 5.0, (4.0, 0.0, 0.0)),                 # beyond the vertex b, in the plane
             ((4.0, 3.0, 0.0), 2.4, (4.0 - 2.4 * 0.6, 3.0 - 2.4 * 0.8, 0.0))]   # beyond the hypotenuse: 12 / 5 from 4 x + 3 y = 12... scaled
    for p, want, q_want in cases:
        d2, q = R.closest_on_triangles(np.array(p), a, b, c)
        assert abs(np.sqrt(d2) - want) < 1e-14, (p, np.sqrt(d2), want)
        np.testing.assert_allclose(q, q_want, atol=1e-14)
    # a permutation of the vertices changes nothing
    for perm in ((b, c, a), (c, a, b), (a, c, b)):
        for p, want, _ in cases:
            assert abs(np.sqrt(R.closest_on_triangles(np.array(p), *perm)[0]) - want) < 1e-14


def _box(lo, hi):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    return v, f


def test_reference_box_offsets():
    """The 27 offsets of a point around an axis-aligned box against the closed-form box distance (inside: to the nearest side)."""
    lo, hi = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 3.5, 4.0])
    v, f = _box(lo, hi)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    pts = np.array([mid + np.array([sx, sy, sz]) * (half + 0.7) * np.array([1.0, 1.3, 1.1])
                    for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)])
    pts[13] += (0.3, 0.1, -0.4)                                       # the centre one: inside, off-centre
    face, dist, second = R.brute_force(v, f, pts)
    gap = np.maximum(np.maximum(lo - pts, pts - hi), 0.0)
    want = np.linalg.norm(gap, axis=1)
    inside = (gap == 0).all(axis=1)
    want[inside] = np.minimum(pts - lo, hi - pts).min(axis=1)[inside]
    np.testing.assert_allclose(dist, want, atol=1e-14)
    assert inside.sum() == 1 and (second >= dist).all()
    d, q = R.distance_to_faces(v, f, pts, face)
    assert np.array_equal(d, dist) and np.abs(np.linalg.norm(pts - q, axis=1) - dist).max() < 1e-14


# ---- the kernel's triangle arithmetic ---------------------------------------------------------------------------------------------
def _random_cases(rng, n, extent=20.0):
    """Triangles of all shapes in +-extent (every fourth a sliver with an aspect down to 1e-3) and queries around them."""
    tris, pts = [], []
    for i in range(n):
        a = rng.uniform(-extent, extent, size=3)
        if i % 4 == 3:
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            w = np.cross(u, rng.normal(size=3))
            w /= np.linalg.norm(w)
            L = rng.uniform(0.5, 5.0)
            b, c = a + L * u, a + rng.uniform(-0.5, 1.5) * L * u + L * 10.0 ** rng.uniform(-3, -1) * w
        else:
            b, c = a + rng.normal(scale=2.0, size=3), a + rng.normal(scale=2.0, size=3)
        tri = np.stack([a, b, c])
        k = i % 3
        if k == 0:                                                    # anywhere around
            p = tri.mean(axis=0) + rng.normal(scale=3.0, size=3)
        elif k == 1:                                                  # near the surface: a point of the triangle + 2 cm
            w = rng.dirichlet(np.ones(3))
            p = w @ tri + rng.normal(scale=0.02, size=3)
        else:                                                         # in the plane, outside or inside
            w = rng.normal(scale=1.0, size=3)
            w /= w.sum() if abs(w.sum()) > 0.1 else 1.0
            p = w @ tri
        tris.append(tri)
        pts.append(p)
    return np.stack(tris), np.stack(pts)


def test_closest_on_triangle_all_regions(host):
    rng = np.random.default_rng(11)
    extent = 40.0
    bar = 2.0 ** -40 * extent
    tris, pts = _random_cases(rng, 6000)
    d2_ref, _ = R.closest_on_triangles(pts, tris[:, 0], tris[:, 1], tris[:, 2])
    seen = set()
    worst = 0.0
    for tri, p, want in zip(tris, pts, np.sqrt(d2_ref)):
        d2, q, reg = _closest(host, tri, p)
        seen.add(reg)
        assert np.isfinite(d2) and np.isfinite(q).all()
        worst = max(worst, abs(np.sqrt(d2) - want))
        assert abs(np.sqrt(d2) - want) <= bar, (tri, p, REGIONS[reg], np.sqrt(d2), want)
        assert abs(np.linalg.norm(p - q) - np.sqrt(d2)) <= bar
        # the returned point lies inside its triangle and in its plane: its own distance to the triangle is within the bar
        assert np.sqrt(R.closest_on_triangles(q, *tri)[0]) <= bar, (tri, p, REGIONS[reg])
    print('largest deviation from the reference: %.3g m (bar %.3g m)' % (worst, bar))
    assert seen >= set(range(7)), sorted(REGIONS[r] for r in seen)


def test_query_over_an_edge_or_vertex_gives_one_point(host):
    """A query exactly over a vertex or an edge is on the border of several regions: whichever branch takes it, the point is the
    same (exactly representable cases: small integers)."""
    tri = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    cases = [((0.0, 0.0, 3.0), (0.0, 0.0, 0.0)), ((4.0, 0.0, -2.0), (4.0, 0.0, 0.0)), ((0.0, 4.0, 1.0), (0.0, 4.0, 0.0)),
             ((2.0, 0.0, 5.0), (2.0, 0.0, 0.0)), ((0.0, 1.0, 5.0), (0.0, 1.0, 0.0)), ((2.0, 2.0, 1.0), (2.0, 2.0, 0.0)),
             ((-1.0, -1.0, 0.0), (0.0, 0.0, 0.0)), ((2.0, -3.0, 0.0), (2.0, 0.0, 0.0)), ((1.0, 1.0, 7.0), (1.0, 1.0, 0.0))]
    for p, want in cases:
        regs = set()
        for perm in perms:
            d2, q, reg = _closest(host, tri[list(perm)], np.array(p))
            regs.add(reg)
            assert np.array_equal(q, np.array(want)), (p, perm, REGIONS[reg], q)
            assert d2 == float(np.sum((np.array(p) - np.array(want)) ** 2))
        print(p, sorted(REGIONS[r] for r in regs))


def test_degenerate_triangles(host):
    """Collinear, two equal and three equal vertices, with queries on, beside and beyond them: the finite point-segment /
    point-point answer."""
    a, d = np.array([1.0, 2.0, 3.0]), np.array([2.0, -1.0, 2.0])
    queries = [a + 0.5 * d, a + 0.25 * d + np.array([0.5, 1.0, 0.0]), a - 2.0 * d + np.array([0.0, 0.0, 1.0]), a + 3.0 * d,
               np.array([10.0, -7.0, 0.5])]
    shapes = {'collinear': (a, a + d, a + 2.0 * d), 'collinear, middle last': (a, a + 2.0 * d, a + d),
              'two equal': (a, a, a + 2.0 * d), 'two equal (b = c)': (a, a + 2.0 * d, a + 2.0 * d), 'three equal': (a, a, a)}
    for name, tri in shapes.items():
        lo, hi = (a, a) if name == 'three equal' else (a, a + 2.0 * d)
        for p in queries:
            d2, q, reg = _closest(host, np.stack(tri), p)
            want2, q_want = R._segment(p, lo, hi)
            assert reg == 7 and np.isfinite(d2) and np.isfinite(q).all(), (name, p, REGIONS[reg])
            assert abs(np.sqrt(d2) - np.sqrt(want2)) <= 1e-14 and np.abs(q - q_want).max() <= 1e-14, (name, p, d2, want2)
    # vertices that are collinear only up to their rounding: still the segment answer, within the triangle's width
    rng = np.random.default_rng(2)
    for _ in range(200):
        a, d = rng.uniform(-20, 20, size=3), rng.normal(size=3)
        tri = np.stack([a, a + 0.37 * d, a + d])
        p = a + rng.uniform(-0.5, 1.5) * d + rng.normal(scale=0.3, size=3)
        d2, q, reg = _closest(host, tri, p)
        assert np.isfinite(d2) and abs(np.sqrt(d2) - np.sqrt(R._segment(p, a, a + d)[0])) <= 1e-13, (tri, p, REGIONS[reg])


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def test_sampler_lines_bit_equal(host):
    rng = np.random.default_rng(4)
    n = 100000
    seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, size=n, dtype=np.int64)
    seeds[:4] = (0, 135, -1, 2 ** 63 - 1)
    idx = rng.integers(0, 2 ** 40, size=n, dtype=np.int64)
    idx[:3] = (0, 1, 2 ** 62)
    tris = rng.uniform(-50, 50, size=(n, 3, 3))
    u_ref = np.stack([R.sample_uniforms(int(s), [int(i)])[0] for s, i in zip(seeds[:2000], idx[:2000])])
    # the restatement vectorises over i for one seed: check the per-pair calls above against a vectorised call too
    assert np.array_equal(R.sample_uniforms(135, idx[:2000]), np.stack([R.sample_uniforms(135, [int(i)])[0] for i in idx[:2000]]))
    u, p = np.zeros(3), np.zeros(3)
    us, ps = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n):
        host.dc_host_mesh_sample_point(_p(tris[k]), int(seeds[k]), int(idx[k]), _p(u), _p(p))
        us[k], ps[k] = u, p
    assert np.array_equal(us[:2000], u_ref)
    # every pair against the restatement: group by seed is not possible (all differ), so restate the uniforms from the host's base
    # formula for all of them in one vectorised pass
    with np.errstate(over='ignore'):
        base = R.splitmix64(seeds.astype(np.uint64)) + np.uint64(4) * idx.astype(np.uint64)
        u_all = np.stack([(R.splitmix64(base + np.uint64(t)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for t in range(3)], axis=1)
    assert np.array_equal(us, u_all)
    assert (us >= 0).all() and (us < 1).all()
    assert np.array_equal(ps, R.sample_points(tris, us[:, 1], us[:, 2]))
    # the point lies inside its triangle: weights >= 0, sum 1 within 4 ulp
    s = np.sqrt(us[:, 1])
    w = np.stack([1.0 - s, s * (1.0 - us[:, 2]), s * us[:, 2]], axis=1)
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps


def test_sampler_face_pick(host):
    areas = np.array([0.0, 1.0, 0.0, 0.0, 3.0, 0.5, 0.0, 4.0, 0.0, 0.0])          # zero-area faces in front, inside, at the end
    cdf = np.cumsum(areas)
    total = cdf[-1]
    pick = lambda u0: host.dc_host_mesh_sample_face(_p(cdf), len(cdf), float(u0))
    # exactly on a step: the next face (u0 total == cdf[f] is not < cdf[f]); 1.0 / 8.5 etc. are not exact, so use u0 = k / 8.5 only
    # where the product is exact: rebuild with a total that is a power of two
    areas2 = np.array([0.0, 1.0, 0.0, 3.0, 0.0, 4.0, 0.0])
    cdf2 = np.cumsum(areas2)                                                       # total 8
    pick2 = lambda u0: host.dc_host_mesh_sample_face(_p(cdf2), len(cdf2), float(u0))
    assert pick2(0.0) == 1 and pick2(0.124) == 1 and pick2(0.125) == 3 and pick2(0.4999) == 3 and pick2(0.5) == 5
    assert pick2(1.0 - 2.0 ** -53) == 5
    assert pick2(1.0) == 5                                                         # off the end (cannot happen for u0 < 1): guarded
    u0 = np.random.default_rng(9).uniform(size=20000)
    got = np.array([pick(u) for u in u0])
    assert np.array_equal(got, R.sample_faces(cdf, u0))
    assert set(np.unique(got)) == {1, 4, 5, 7}                                     # faces of zero area get none
    share = np.array([(got == f).mean() for f in (1, 4, 5, 7)])
    np.testing.assert_allclose(share, areas[[1, 4, 5, 7]] / total, atol=5 * np.sqrt(0.25 / len(u0)))


# ---- configuration, file names, statistics ------------------------------------------------------------------------------------
def test_config_and_file_names():
    from depth_correction_amd.config import Config, map_eval_csv, slam_eval_csv
    cfg = Config()
    assert cfg.map_eval_csv is None and cfg.map_eval_poses == 'dataset' and cfg.map_eval_inlier_ratio == 0.8 and cfg.map_eval_samples == 0
    assert Config(map_eval_poses='slam').copy().map_eval_poses == 'slam'
    assert map_eval_csv('/tmp/log', 'val') == '/tmp/log/map_eval_val.csv' and map_eval_csv('', None) == 'map_eval.csv'
    assert map_eval_csv('log', 'test') == 'log/map_eval_test.csv' and map_eval_csv(None, 'train') == 'map_eval_train.csv'
    # the same rule as slam_eval_csv's names
    assert os.path.dirname(map_eval_csv('/x/y', 'test')) == os.path.dirname(slam_eval_csv('/x/y', 'icp_mapper', 'test'))


def test_map_statistics_equal_numpy():
    import torch
    from depth_correction_amd.metrics import map_statistics
    rng = np.random.default_rng(3)
    d = np.abs(rng.normal(scale=0.05, size=1001))
    d[::50] += 1.0                                                                 # outliers the trimmed mean must drop
    sgn = d * rng.choice([-1.0, 1.0], size=d.shape)
    for ratio in (0.8, 0.5, 1.0):
        got = map_statistics(torch.as_tensor(d), torch.as_tensor(sgn), inlier_ratio=ratio)
        thr = np.quantile(d, ratio)
        want = dict(n=float(len(d)), mean=d.mean(), rms=np.sqrt((d ** 2).mean()), median=np.median(d), trimmed_mean=d[d <= thr].mean(),
                    signed_mean=sgn.mean(), max=d.max())
        assert set(got) == set(want)
        for k in want:
            assert isinstance(got[k], float) and abs(got[k] - want[k]) <= 1e-15 + 1e-13 * abs(want[k]), (ratio, k, got[k], want[k])
    # non-finite rows (queries that were NaN, or beyond max_dist) are not counted
    d2 = np.concatenate([d, [np.inf, np.nan]])
    got = map_statistics(torch.as_tensor(d2), torch.as_tensor(np.concatenate([sgn, [0.0, 0.0]])))
    assert got['n'] == len(d) and abs(got['mean'] - d.mean()) < 1e-15
    empty = map_statistics(torch.zeros((0,), dtype=torch.float64))
    assert empty['n'] == 0 and np.isnan(empty['mean'])


def test_mesh_sampling_host_parts():
    """TriangleMesh.face_areas / area_cdf (host side of the sampler) and MeshDataset's argument checks need no GPU."""
    from depth_correction_amd.mesh import TriangleMesh, box_mesh
    m = box_mesh((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    assert abs(m.face_areas().sum() - 2 * (2 * 4 + 2 * 6 + 4 * 6)) < 1e-12
    assert np.array_equal(m.area_cdf(), np.cumsum(m.face_areas()))
    t = TriangleMesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 3, 0]], [[0, 1, 2], [0, 1, 3], [0, 0, 1]])
    np.testing.assert_allclose(t.face_areas(), [0.5, 1.5, 0.0])
    from depth_correction_amd.dataset import MeshDataset
    with pytest.raises(FileNotFoundError):
        MeshDataset('mesh/no_such_mesh.ply')
