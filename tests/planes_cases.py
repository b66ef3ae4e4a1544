"""The inputs the plane tests share between the host oracle (test_planes_host.py) and the kernels (test_gpu_planes_edge.py):
RANSAC clouds and cases, DBSCAN clouds, fit_planes scenes and synthetic planes for the plane moments (test infrastructure)."""
import numpy as np

THRESH = 0.03
OFFSET = np.array([4e5, 5e6, 300.0])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- RANSAC ---------------------------------------------------------------------------------------------------------------------
def ransac_cloud(n_total, n_rem, seed, dtype=np.float64, offset=False):
    """(x [n_total,3], remaining int32 [n_rem]): a noisy plane (60 %), a second one (20 %) and clutter, in shuffled order; `remaining`
    is a shuffled strict subset of the rows (n_total > n_rem)."""
    assert n_total > n_rem
    rng = np.random.default_rng(seed)
    a, b = (6 * n_total) // 10, (2 * n_total) // 10
    p1 = np.c_[rng.uniform(-4, 4, (a, 2)), 0.5 + 0.01 * rng.normal(size=a)]
    q = rng.uniform(-3, 3, (b, 2))
    p2 = np.c_[2.0 + 0.01 * rng.normal(size=b), q[:, 0], 1.5 + q[:, 1]]
    x = np.concatenate([p1, p2, rng.uniform(-4, 4, (n_total - a - b, 3))])
    x = x[rng.permutation(n_total)]
    if offset:
        x = x + OFFSET
    rem = rng.permutation(n_total)[:n_rem].astype(np.int32)
    return np.ascontiguousarray(x.astype(dtype)), rem


# (n_rem, H, dtype, round, seed): every n_rem and H the issue names at least once, both dtypes, every round and seed
RANSAC_CASES = [(3, 1, np.float64, 0, 0), (3, 257, np.float32, 1, 135), (4, 2, np.float64, 4097, 2 ** 63 + 5),
                (255, 255, np.float32, 0, 2 ** 64 - 1), (255, 1024, np.float64, 1, 0), (1023, 256, np.float64, 4097, 135),
                (1024, 257, np.float32, 0, 2 ** 63 + 5), (1024, 1, np.float64, 1, 2 ** 64 - 1), (1025, 2, np.float32, 4097, 0),
                (1025, 1024, np.float64, 0, 135), (4097, 256, np.float32, 1, 2 ** 63 + 5), (4097, 1024, np.float64, 4097, 2 ** 64 - 1),
                (4097, 255, np.float64, 0, 135)]


def lattice_cloud():
    """The exact case, 320 points with coordinates that are multiples of 2^-6: rows 0..63 an 8 x 8 lattice at z = 0, then copies of
    it at z = +-2^-5 (inliers of the plane z = 0 at thresh = 2^-5, exactly on the border) and z = +-(2^-5 + 2^-6) (outliers).  A
    hypothesis through three non-collinear rows below 64 is n = (0, 0, +-1), d = 0 exactly and has exactly 192 inliers."""
    g = np.arange(8) * 2.0 ** -6 * 5
    xy = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    layers = [0.0, 2.0 ** -5, -2.0 ** -5, 2.0 ** -5 + 2.0 ** -6, -(2.0 ** -5 + 2.0 ** -6)]
    return np.concatenate([np.c_[xy, np.full(64, z)] for z in layers])


def flat_lattice():
    """64 points of the plane z = 0 on an 8 x 8 lattice: every non-degenerate hypothesis has all 64 as inliers (the tie case)."""
    return lattice_cloud()[:64].copy()


# (seed, round, lowest proper h) on flat_lattice(): the hypotheses below it repeat a position or are collinear
# (seed 88: (35, 6, 6) and the collinear (47, 55, 39); seed 113: three repeats; seed 322: a repeat and a collinear triple)
TIE_SEEDS = [(88, 0, 2), (113, 1, 3), (322, 4097, 2)]


def collinear_cloud(n=200):
    """Every point on one line (exactly: multiples of one direction with small integer factors)."""
    t = np.arange(n, dtype=np.float64)
    return np.c_[0.25 * t, -0.5 * t, 0.125 * t]


def big_refit_case(seed=31):
    """(x f64 [n,3], remaining int32 [n], hypothesis [4], anchor [3]) with n = 262144 + 257: more points than the refit's 1024 blocks
    of 256 threads hold, so the moments kernel strides.  8000 points of a tilted noisy plane among clutter (about 2000 more inliers)."""
    n = 262144 + 257
    rng = np.random.default_rng(seed)
    n0 = np.array([0.2, -0.3, 0.9])
    n0 /= np.linalg.norm(n0)
    t1 = _unit(np.cross(n0, [1.0, 0.0, 0.0]))
    t2 = np.cross(n0, t1)
    x = rng.uniform(-4, 4, (n, 3))
    uv = rng.uniform(-3, 3, (8000, 2))
    x[:8000] = uv[:, :1] * t1 + uv[:, 1:] * t2 + (0.5 + 0.01 * rng.normal(size=(8000, 1))) * n0
    anchor = x[17].copy()
    x = np.ascontiguousarray(x[rng.permutation(n)])
    return x, rng.permutation(n).astype(np.int32), np.concatenate([n0, [-0.5]]), anchor


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------------------
def dbscan_cases():
    """name -> (points f64 [m,3], eps, min_points)."""
    rng = np.random.default_rng(11)
    out = {}
    g = np.arange(12) * 0.125
    out['lattice'] = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3), 0.125, 7)
    chain = np.c_[0.09 * np.arange(4096), np.zeros(4096), np.zeros(4096)]
    out['chain'] = (chain[rng.permutation(4096)], 0.1, 3)
    blob = lambda c, k: np.asarray(c) + 0.01 * rng.uniform(-1, 1, (k, 3)) / np.sqrt(3.0)
    # a non-core point (row 0: three neighbours with itself) within eps of one core point of each blob
    out['bridge'] = (np.concatenate([[[0.15, 0, 0]], blob([0.3, 0, 0], 30), [[0.25, 0, 0]], blob([0, 0, 0], 30), [[0.05, 0, 0]]]), 0.11, 10)
    b = blob([0, 0, 0], 40)
    out['equal'] = (np.concatenate([rng.uniform(5, 9, (5, 3)), b + [2.0, 0, 0], b]), 0.1, 10)
    g = np.arange(50, dtype=np.float64)
    out['noise'] = (np.c_[g, 0 * g, 0 * g], 0.1, 10)
    out['single'] = (np.array([[0.5, -1.0, 2.0]]), 0.1, 10)
    out['single_core'] = (np.array([[0.5, -1.0, 2.0]]), 0.1, 1)
    out['copies'] = (np.tile([[0.25, 0.5, -0.75]], (25, 1)), 0.1, 10)
    c3 = np.concatenate([rng.normal(0, 0.3, (1400, 3)), [3.0, 0, 0] + rng.normal(0, 0.25, (1200, 3)), rng.uniform(-3, 6, (400, 3))])
    out['random3d'] = (c3[rng.permutation(len(c3))], 0.12, 10)
    return out


# ---- fit_planes scenes -----------------------------------------------------------------------------------------------------------
def scene_three_planes(seed=5):
    """Three noisy planes (2000, 1500 and 1000 points) and 500 points of clutter, shuffled."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2, 2, (2000, 2))
    b = rng.uniform(-2, 2, (1500, 2))
    c = rng.uniform(-2, 2, (1000, 2))
    x = np.concatenate([np.c_[a, 0.005 * rng.normal(size=2000)], np.c_[2.5 + 0.005 * rng.normal(size=1500), b[:, 0], 2.5 + b[:, 1]],
                        np.c_[c[:, 0], -2.5 + 0.005 * rng.normal(size=1000), 2.5 + c[:, 1]], rng.uniform(-3, 5, (500, 3))])
    return x[rng.permutation(len(x))]


def scene_sparse_plane(seed=9):
    """A large plane sampled on a 0.5 m lattice (1600 points at z = 3: no two within eps = 0.3 of each other, so it has no cluster)
    beside two dense smaller planes (1300 and 900 points) and 300 points of clutter, shuffled."""
    rng = np.random.default_rng(seed)
    g = (np.arange(40) - 20) * 0.5
    sp = np.c_[np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2), 3.0 + 0.005 * rng.normal(size=1600)]
    a = rng.uniform(0, 2, (1300, 2))
    b = rng.uniform(0, 2, (900, 2))
    x = np.concatenate([sp, np.c_[0.005 * rng.normal(size=1300), a[:, 0], a[:, 1]], np.c_[4.0 + b[:, 0], 5.0 + 0.005 * rng.normal(size=900), b[:, 1]],
                        np.c_[rng.uniform(-10, 10, (300, 2)), rng.uniform(-2, 2.5, 300)]])
    return x[rng.permutation(len(x))]


SCENE_ARGS = dict(distance_threshold=THRESH, min_support=50, max_iterations=96, max_models=10, seed=135)
SCENE_EPS = 0.3


# ---- plane moments ---------------------------------------------------------------------------------------------------------------
PLANE_SIZES = (2, 3, 2047, 2048, 2049, 4097)
MODELS = {None: (None, None), 'Polynomial': ([2e-3, -1e-3], [2.0, 4.0]), 'ScaledPolynomial': ([2e-3, -1e-3], [2.0, 4.0]),
          'Linear': ([0.998, 3e-3, -2e-3], None), 'InvCos': ([2e-3], None), 'ScaledInvCos': ([1.5e-3], None)}
PERP_KINDS = (None, 'Polynomial', 'ScaledPolynomial', 'Linear')      # the InvCos kinds divide by cos(gamma) = 0 at dir perpendicular to n


def moments_cloud(kind, dtype=np.float64, offset=False, sizes=PLANE_SIZES, seed=21):
    """Synthetic planes for the plane moments: dict(vps, dirs [N,3], depth [N,1], indices (list of int64 arrays, shuffled rows of the
    cloud), normals [P,3]).  One sensor at `centre`; every plane is a noisy patch some metres away with its own unit normal.  Every
    plane of at least 2047 points holds a point seen along +n (cos = 1), one along -n and, for the kinds in PERP_KINDS, one seen
    along a direction perpendicular to n.  The directions are unit vectors rounded to `dtype`."""
    rng = np.random.default_rng(seed)
    centre = OFFSET.copy() if offset else np.zeros(3)
    # the two small planes are tilted; the large ones, which hold the special points, have axis-aligned normals, so that
    # dir . n is exactly +-1 or 0 in either dtype (with a tilted n the rounded dot product lands an ulp beside 1, where
    # d gamma / d dir ~ 1 / sqrt(1 - c^2) amplifies that ulp without bound: a property of the formula, not of a kernel)
    normals = np.array([[0.6, 0.0, 0.8], [0.0, -0.6, 0.8], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])[:len(sizes)]
    perp = np.array([[0.8, 0.0, -0.6], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])[:len(sizes)]
    vps, dirs, depth, sizes_out = [], [], [], []
    for n, s, pp in zip(normals, sizes, perp):
        t1 = _unit(np.cross(n, [0.3, -0.5, 0.8]))
        t2 = np.cross(n, t1)
        uv = rng.uniform(0.5, 3, (s, 2)) * rng.choice([-1.0, 1.0], (s, 2))       # no other point is seen face-on
        pts = 6.0 * n + uv[:, :1] * t1 + uv[:, 1:] * t2 + 0.01 * rng.normal(size=(s, 1)) * n        # relative to the sensor
        d = np.linalg.norm(pts, axis=1)
        dr = pts / d[:, None]
        if s >= 2047:
            dr[5], d[5] = n, 6.0
            dr[6], d[6] = -n, 6.0
            if kind in PERP_KINDS:
                dr[7], d[7] = pp, 4.0
        vps.append(np.tile(centre, (s, 1)))
        dirs.append(dr)
        depth.append(d)
        sizes_out.append(s)
    vps, dirs, depth = np.concatenate(vps), np.concatenate(dirs), np.concatenate(depth)
    order = rng.permutation(len(dirs))                       # the cloud's rows are shuffled: the planes index all over it
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    starts = np.concatenate([[0], np.cumsum(sizes_out)])
    indices = [inv[a:b].astype(np.int64) for a, b in zip(starts[:-1], starts[1:])]
    return dict(vps=np.ascontiguousarray(vps[order].astype(dtype)), dirs=np.ascontiguousarray(dirs[order].astype(dtype)),
                depth=np.ascontiguousarray(depth[order].astype(dtype).reshape(-1, 1)), indices=indices, normals=normals)


MOMENT_CASES = [(k, np.float64, False) for k in MODELS] + [(k, np.float32, False) for k in MODELS] + [(k, np.float64, True) for k in MODELS]
GOLDEN = 'golden/planes_moments_mp.npz'


def moments_key(kind, dtype, offset):
    return '%s_%s_%s' % (kind, np.dtype(dtype).name, 'offset' if offset else 'origin')


def moments_digest(c):
    import hashlib
    h = hashlib.sha256()
    for a in [c['vps'], c['dirs'], c['depth'], c['normals']] + list(c['indices']):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def moments_cov_mp(kind, dtype, offset, c):
    """The 50-digit covariances [P,3,3] of the case (planes_reference.plane_mp): read from tests/golden when the fixture was made
    from these very inputs (it stores their digest), computed otherwise (a few seconds)."""
    import os
    import planes_reference as R
    key = moments_key(kind, dtype, offset)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), GOLDEN)
    if os.path.exists(path):
        g = np.load(path)
        if key in g and str(g[key + '_digest']) == moments_digest(c):
            return g[key]
    w, e = MODELS[kind]
    return np.stack([R.plane_mp(c['vps'], c['dirs'], c['depth'], i, n, kind, w, e)['cov'] for i, n in zip(c['indices'], c['normals'])])


if __name__ == '__main__':
    # regenerates tests/golden/planes_moments_mp.npz (python tests/planes_cases.py)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import planes_reference as R
    out = {}
    for kind, dtype, offset in MOMENT_CASES:
        c = moments_cloud(kind, dtype, offset)
        w, e = MODELS[kind]
        key = moments_key(kind, dtype, offset)
        out[key] = np.stack([R.plane_mp(c['vps'], c['dirs'], c['depth'], i, n, kind, w, e)['cov'] for i, n in zip(c['indices'], c['normals'])])
        out[key + '_digest'] = np.array(moments_digest(c))
        print(key, flush=True)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), GOLDEN), **out)


def random_plane(seed, n=300):
    """n points of a noisy plane with a random unit normal (seeded); for the refit's sign rule."""
    rng = np.random.default_rng(seed)
    n0 = _unit(rng.normal(size=3))
    t1 = _unit(np.cross(n0, [0.0, 0.0, 1.0]) if abs(n0[2]) < 0.9 else np.cross(n0, [1.0, 0.0, 0.0]))
    t2 = np.cross(n0, t1)
    uv = rng.uniform(-2, 2, (n, 2))
    return 1.5 * n0 + uv[:, :1] * t1 + uv[:, 1:] * t2 + 0.003 * rng.normal(size=(n, 1)) * n0


def moments_about(pts, anchor):
    """The ten moments [count, s (3), S (6: xx xy xz yy yz zz)] of pts about anchor, in numpy float64."""
    d = pts - anchor
    return np.concatenate([[len(pts)], d.sum(0), [(d[:, i] * d[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]])


def cov6_of_moments(v):
    n, m = v[0], v[1:4] / v[0]
    return np.array([v[4] / n - m[0] * m[0], v[5] / n - m[0] * m[1], v[6] / n - m[0] * m[2], v[7] / n - m[1] * m[1],
                     v[8] / n - m[1] * m[2], v[9] / n - m[2] * m[2]])
