"""Reference of the survey registration tests (test_align_host.py, test_gpu_align.py): numpy, scipy's cKDTree and math.fsum only --
nothing here calls depth_correction_amd.

Two independent fp64 routes to the rigid fit y ~ R p + t of paired points:
  (A) ``fit_svd``    plain means, the 3 x 3 cross-covariance, np.linalg.svd with the determinant fix (Kabsch / Umeyama);
  (B) ``fit_horn``   math.fsum moments about two fixed origins, Horn's symmetric 4 x 4 matrix, np.linalg.eigh.
Their disagreement along the reference trajectory is the yardstick of the tests (``bars``): what two correct fp64 implementations
of the same closed form differ by on this data.

``icp`` is the trimmed ICP on route A with the rules of DESIGN "Survey registration" restated: the nearest survey point strictly
within max_dist of T_k p, tau = np.quantile of the matched distances at the inlier ratio, kept = matched and d <= tau, T_{k+1}
fitted from the ORIGINAL p, the increment by atan2 of the axial vector and by the motion of the query's origin, the status order
pairs / degenerate / non-finite / converged / max iterations.

The scene is a hand-written room: 8 x 6 x 3 m with two box pillars of different footprint and height (no symmetry leaves the
alignment ambiguous), sampled area-weighted.
"""
import functools
import math

import numpy as np
from scipy.spatial import cKDTree

SEED = 135
N_SURVEY = 20000
ROOM = (8.0, 6.0, 3.0)
# (x0, y0, x1, y1, height): the second pillar reaches the ceiling
PILLARS = ((1.7, 1.1, 2.3, 1.9, 2.0), (5.0, 3.75, 6.0, 4.25, 3.0))
EXTENT = 8.0
BAR_PT = 2.0 ** -40 * EXTENT                       # the project's bar for a point (test_gpu_meshdist.py)
MAX_DIST = 0.5
RATIO = 0.8
SIZES = (257, 4099)
SIGMA = 0.01
SHIFT = np.array([1e5, -2e5, 3e4])
STEPS = (0, 1, 5, 15)
EPS = np.finfo(np.float64).eps
STATUS = {0: 'running', 1: 'converged', 2: 'max_iterations', -1: 'too_few_pairs', -2: 'degenerate', -3: 'not_finite'}
REL_EPS = 1e-12


def axis_angle(axis, angle):
    """Rodrigues' rotation matrix."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


T_TRUE = rigid(axis_angle((0.3, -0.2, 1.0), math.radians(3.0)), (0.12, -0.08, 0.05))


def move(T, p):
    """x = ((T00 p0 + T01 p1) + T02 p2) + T03, the order dc_knn_grid_query moves its queries in."""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def _rectangles():
    """(origin, edge u, edge v, normal) of every surface rectangle of the room."""
    X, Y, Z = ROOM
    rect = [((0, 0, 0), (X, 0, 0), (0, Y, 0), (0, 0, 1)), ((0, 0, Z), (X, 0, 0), (0, Y, 0), (0, 0, -1)),
            ((0, 0, 0), (X, 0, 0), (0, 0, Z), (0, 1, 0)), ((0, Y, 0), (X, 0, 0), (0, 0, Z), (0, -1, 0)),
            ((0, 0, 0), (0, Y, 0), (0, 0, Z), (1, 0, 0)), ((X, 0, 0), (0, Y, 0), (0, 0, Z), (-1, 0, 0))]
    for x0, y0, x1, y1, h in PILLARS:
        rect += [((x0, y0, 0), (x1 - x0, 0, 0), (0, 0, h), (0, -1, 0)), ((x0, y1, 0), (x1 - x0, 0, 0), (0, 0, h), (0, 1, 0)),
                 ((x0, y0, 0), (0, y1 - y0, 0), (0, 0, h), (-1, 0, 0)), ((x1, y0, 0), (0, y1 - y0, 0), (0, 0, h), (1, 0, 0))]
        if h < Z:
            rect.append(((x0, y0, h), (x1 - x0, 0, 0), (0, y1 - y0, 0), (0, 0, 1)))
    return [tuple(np.array(v, dtype=np.float64) for v in r) for r in rect]


@functools.lru_cache(maxsize=None)
def survey(shifted=False, n=N_SURVEY, seed=SEED):
    """(points [n,3], unit normals [n,3]) of the room, area-weighted, seeded; ``shifted``: the whole scene moved by SHIFT."""
    rng = np.random.default_rng(seed)
    rect = _rectangles()
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v, _ in rect])
    which = rng.choice(len(rect), size=n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    o = np.stack([rect[k][0] for k in which])
    u = np.stack([rect[k][1] for k in which])
    v = np.stack([rect[k][2] for k in which])
    nrm = np.stack([rect[k][3] for k in which])
    pts = o + a[:, None] * u + b[:, None] * v
    if shifted:
        pts = pts + SHIFT
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm


def true_transform(shifted=False):
    """T with T p = y for the inliers: T_TRUE, conjugated by the shift for the shifted scene."""
    if not shifted:
        return T_TRUE.copy()
    S, Si = rigid(np.eye(3), SHIFT), rigid(np.eye(3), -SHIFT)
    return S @ T_TRUE @ Si


@functools.lru_cache(maxsize=None)
def scene(n, sigma=0.0, shifted=False, seed=SEED):
    """dict(survey, normals, query [n + n // 10, 3], inlier_idx [n] (the survey row every inlier came from), n_inliers, T_true): the
    first n query rows are survey points moved by the inverse of the true transform (plus N(0, sigma) noise), the rest clutter."""
    pts, nrm = survey(shifted)
    rng = np.random.default_rng(seed + 1000 + n)
    rows = rng.choice(len(pts), size=n, replace=False)
    T = true_transform(shifted)
    Ti = np.linalg.inv(T)
    q = move(Ti, pts[rows])
    if sigma:
        q = q + rng.normal(0.0, sigma, size=q.shape)
    clutter = rng.uniform((1.0, 1.0, 0.8), (7.0, 5.0, 2.2), size=(n // 10, 3))
    if shifted:
        clutter = clutter + SHIFT
    query = np.ascontiguousarray(np.concatenate([q, clutter]))
    query.setflags(write=False)
    return dict(survey=pts, normals=nrm, query=query, inlier_idx=rows, n_inliers=n, T_true=T, shifted=shifted)


def origins(query, survey_pts):
    """[o_p, o_y]: the centre of the bounding box of the finite query rows and the centre of the survey's bounds."""
    q = query[np.isfinite(query).all(axis=1)]
    o_p = 0.5 * (q.min(axis=0) + q.max(axis=0)) if len(q) else np.zeros(3)
    return np.concatenate([o_p, 0.5 * (survey_pts.min(axis=0) + survey_pts.max(axis=0))])


# ---- route A ------------------------------------------------------------------------------------------------------------------------
def fit_svd(p, y):
    """(T [4,4], s [3] singular values, d = the determinant sign): the least-squares proper rotation and translation with y ~ R p + t."""
    p, y = np.asarray(p, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mp, my = p.mean(axis=0), y.mean(axis=0)
    H = (y - my).T @ (p - mp)                       # sum (y - my)(p - mp)^T
    U, s, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    return rigid(R, my - R @ mp), s, d


def svd_gap(s, d):
    """(lam1 - lam2, max |lam|) of Horn's matrix from the singular values: its eigenvalues are s1 + s2 + d s3, s1 - s2 - d s3,
    -s1 + s2 - d s3, -s1 - s2 + d s3."""
    return 2.0 * (s[1] + d * s[2]), s[0] + s[1] + s[2]


# ---- route B ------------------------------------------------------------------------------------------------------------------------
def moments(p, y, d, o):
    """The 17 moments [W, a, b, S row-major, E] of the pairs about the origins o [6], each by math.fsum (exactly rounded sums)."""
    p, y = np.asarray(p, dtype=np.float64) - o[:3], np.asarray(y, dtype=np.float64) - o[3:]
    out = [float(len(p))]
    out += [math.fsum(p[:, i]) for i in range(3)]
    out += [math.fsum(y[:, i]) for i in range(3)]
    out += [math.fsum(p[:, i] * y[:, j]) for i in range(3) for j in range(3)]
    out.append(math.fsum(np.asarray(d, dtype=np.float64) ** 2))
    return np.array(out)


def horn(C):
    xx, xy, xz, yx, yy, yz, zx, zy, zz = C.reshape(-1)
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                     [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, yy - xx - zz, yz + zy],
                     [xy - yx, zx + xz, yz + zy, zz - xx - yy]])


def quat_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def fit_moments(m, o):
    """(T, lam descending) from the 17 moments about o."""
    W, a, b, S = m[0], m[1:4], m[4:7], m[7:16].reshape(3, 3)
    lam, V = np.linalg.eigh(horn(S - np.outer(a, b) / W))
    q = V[:, -1] * (1.0 if V[0, -1] >= 0 else -1.0)
    R = quat_matrix(q)
    return rigid(R, (o[3:] + b / W) - R @ (o[:3] + a / W)), lam[::-1]


def fit_horn(p, y, o):
    return fit_moments(moments(p, y, np.zeros(len(p)), o), o)


# ---- increments -------------------------------------------------------------------------------------------------------------------
def rotation_angle(Ra, Rb):
    """Angle of Ra Rb^T by atan2(|axial vector|, (trace - 1) / 2)."""
    D = Ra[:3, :3] @ Rb[:3, :3].T
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return math.atan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0))


def increment(Tn, Tk, o_p):
    return rotation_angle(Tn, Tk), float(np.linalg.norm((Tn[:3, :3] @ o_p + Tn[:3, 3]) - (Tk[:3, :3] @ o_p + Tk[:3, 3])))


# ---- the trimmed ICP ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tree(shifted):
    return cKDTree(survey(shifted)[0])


def match(sc, T, max_dist=MAX_DIST):
    """(idx [n] int64 or -1, d [n] or inf) of the nearest survey point strictly within max_dist of T p."""
    x = move(T, sc['query'])
    ok = np.isfinite(x).all(axis=1)
    idx, d = np.full(len(x), -1, np.int64), np.full(len(x), np.inf)
    dd, ii = _tree(sc['shifted']).query(x[ok])
    hit = dd < max_dist
    rows = np.flatnonzero(ok)
    idx[rows[hit]], d[rows[hit]] = ii[hit], dd[hit]
    return idx, d


def step(sc, T, ratio=RATIO, max_dist=MAX_DIST, o=None):
    """One iteration from T: dict(idx, d, tau, kept, W, rms, T_a (route A), T_b (route B), gap, lam_max)."""
    o = origins(sc['query'], sc['survey']) if o is None else o
    idx, d = match(sc, T, max_dist)
    matched = idx >= 0
    tau = (float(np.quantile(d[matched], ratio)) if matched.any() else float('nan')) if ratio < 1.0 else float('inf')
    kept = matched & (d <= tau)
    out = dict(idx=idx, d=d, tau=tau, kept=kept, W=int(kept.sum()), o=o)
    out['rms'] = math.sqrt(np.mean(d[kept] ** 2)) if kept.any() else float('nan')
    if out['W'] >= 3:
        p, y = sc['query'][kept], sc['survey'][idx[kept]]
        out['T_a'], s, dsign = fit_svd(p, y)
        out['gap'], out['lam_max'] = svd_gap(s, dsign)
        out['T_b'], _ = fit_moments(moments(p, y, d[kept], o), o)
    return out


def icp(sc, init=None, ratio=RATIO, max_dist=MAX_DIST, n_iters=100, min_rot=0.0, min_trans=0.0, min_pairs=3):
    """The whole run on route A: dict(T, status, iterations, history [n_iters,5] (NaN rows never reached), poses [T_0 .. T_last],
    dR, dt (the largest route A / route B disagreement of any T_{k+1}))."""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    o = origins(sc['query'], sc['survey'])
    hist = np.full((n_iters, 5), np.nan)
    poses, status, dR, dt, it = [T.copy()], 0, 0.0, 0.0, 0
    while status == 0:
        s = step(sc, T, ratio, max_dist, o)
        hist[it, :3] = s['W'], s['rms'], s['tau']
        it += 1
        if s['W'] < min_pairs:
            status = -1
        elif s['gap'] <= REL_EPS * s['lam_max']:
            status = -2
        elif not np.isfinite(s['T_a']).all():
            status = -3
        else:
            dR = max(dR, np.abs(s['T_a'][:3, :3] - s['T_b'][:3, :3]).max())
            dt = max(dt, np.abs(s['T_a'][:3, 3] - s['T_b'][:3, 3]).max())
            d_rot, d_trans = increment(s['T_a'], T, o[:3])
            hist[it - 1, 3:] = d_rot, d_trans
            T = s['T_a']
            poses.append(T.copy())
            if d_rot < min_rot and d_trans < min_trans:
                status = 1
            elif it >= n_iters:
                status = 2
    return dict(T=T, status=STATUS[status], iterations=it, history=hist, poses=poses, dR=dR, dt=dt, o=o)


@functools.lru_cache(maxsize=None)
def trajectory(n, sigma=SIGMA, shifted=False, n_iters=25):
    """icp of scene(n, sigma, shifted) from the identity for n_iters iterations with the checks off."""
    return icp(scene(n, sigma, shifted), n_iters=n_iters)


def bars(traj, coord_max):
    """(bar_R, bar_t): 16 x the largest route A / route B disagreement along the trajectory; floors 16 eps and 16 ulp of the largest
    coordinate.  The margin covers a third summation order (the device's blocks) and FMA contraction."""
    return 16.0 * max(traj['dR'], EPS), 16.0 * max(traj['dt'], float(np.spacing(coord_max)))


def scene_bars(n, sigma=SIGMA, shifted=False):
    sc = scene(n, sigma, shifted)
    return bars(trajectory(n, sigma, shifted), float(np.abs(sc['survey']).max()))


# ---- brute force ------------------------------------------------------------------------------------------------------------------
def nearest(survey_pts, x, chunk=128):
    """(idx [n], d2 [n], second d2 [n]) of the brute-force 1-NN, d2 = (dx^2 + dy^2) + dz^2 of survey - x, the lowest index among equal
    d2; rows of x that are not finite get -1 / inf / inf."""
    n = len(x)
    idx, best, second = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    ok = np.flatnonzero(np.isfinite(x).all(axis=1))
    for a in range(0, len(ok), chunk):
        rows = ok[a:a + chunk]
        d = survey_pts[None, :, :] - x[rows][:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = np.argmin(d2, axis=1)
        idx[rows], best[rows] = j, d2[np.arange(len(rows)), j]
        d2[np.arange(len(rows)), j] = np.inf
        second[rows] = d2.min(axis=1)
    return idx, best, second


# ---- designed pair sets of the solver tests ---------------------------------------------------------------------------------------
def pair_sets():
    """{name: (p [m,3], y [m,3])} whose fit is unique: generic, identity, a half turn, planar pairs, mirrored data (the unconstrained
    optimum is a reflection), large world coordinates."""
    rng = np.random.default_rng(SEED + 7)
    p = rng.uniform(-2.0, 2.0, size=(40, 3)) * (1.0, 0.7, 0.4)
    R = axis_angle((0.5, 0.4, -0.3), 0.7)
    t = np.array([0.3, -1.2, 0.8])
    out = {'generic': (p, p @ R.T + t + rng.normal(0, 1e-3, p.shape)),
           'identity': (p, p.copy()),
           'half_turn': (p, p @ axis_angle((0.2, 1.0, -0.4), math.pi).T + t)}
    flat = p * (1.0, 1.0, 0.0)
    out['planar'] = (flat, flat @ R.T + t)
    mirror = p * (1.0, 1.0, -1.0)
    out['mirrored'] = (p, mirror @ R.T + t + rng.normal(0, 1e-3, p.shape))
    out['shifted'] = (p + SHIFT, (p + SHIFT) @ R.T + t)
    return out


def degenerate_sets():
    """{name: (p, y)} without a unique rotation: collinear pairs, coincident pairs."""
    s = np.linspace(-1.0, 1.0, 9)[:, None]
    line = s * np.array([0.6, -0.3, 0.2]) + (0.4, 0.1, -0.2)
    R = axis_angle((0.1, 0.2, 1.0), 0.3)
    one = np.tile([0.7, -0.4, 1.3], (6, 1))
    return {'collinear': (line, line @ R.T + (0.1, 0.2, 0.3)), 'coincident': (one, one + (0.25, 0.5, -0.125))}
