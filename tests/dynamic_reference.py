"""The reference of the dynamic-point tests: the rule of DESIGN "Dynamic points in the map" restated in plain numpy + cKDTree, fp64,
every sum and product written out in the stated order (numpy rounds each elementwise operation on its own: nothing is fused).
Nothing here calls depth_correction_amd; the host tests hold csrc/dc_dynmath.h (through libdc_hostcheck.so) and the GPU tests hold
the kernels of csrc/dc_dynamic.hip against it, bit for bit.

Every discrete decision is returned with its *margin*, the relative distance of the deciding quantity from its threshold, so that
a comparison can assert that it does not rest on a rounding; ``branch`` names the branch every row took.
"""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

EPS = 1e-4
ONE = 1.0 - EPS
OCCLUDED, UPDATED = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DEFAULTS = dict(prior=0.6, threshold=0.9, beam_half_angle=0.01, epsilon_a=0.01, epsilon_d=0.01, alpha=0.8, beta=0.99, max_range=25.0)


def params(cfg=None, **kw):
    """The rule's parameters with the slam.launch values; ``cfg`` (attributes slam_prior_dynamic, ... slam_sensor_max_range) and ``kw``
    override.  chord_max = 2 sin(beam_half_angle) unless given."""
    d = dict(_DEFAULTS)
    names = dict(prior='slam_prior_dynamic', threshold='slam_threshold_dynamic', beam_half_angle='slam_beam_half_angle',
                 epsilon_a='slam_epsilon_a', epsilon_d='slam_epsilon_d', alpha='slam_alpha', beta='slam_beta', max_range='slam_sensor_max_range')
    for k, attr in names.items():
        if cfg is not None and hasattr(cfg, attr):
            d[k] = float(getattr(cfg, attr))
    d.update(kw)
    d.setdefault('chord_max', 2.0 * math.sin(d['beam_half_angle']))
    return SimpleNamespace(**d)


def _norm3(a0, a1, a2):
    return np.sqrt((a0 * a0 + a1 * a1) + a2 * a2)


def direction(points, pose=None, max_range=0.0):
    """d = q - t, x_r = (R[0][r] d0 + R[1][r] d1) + R[2][r] d2, rho, u = x / rho and the valid mask (rho finite, > 0, <= max_range
    when that is > 0 and finite); pose None: the reading form (x = d = q).  u is zero on invalid rows."""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        if pose is not None:
            T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
            d = np.stack([q[:, 0] - T[0, 3], q[:, 1] - T[1, 3], q[:, 2] - T[2, 3]], axis=1)
            x = np.stack([(T[0, r] * d[:, 0] + T[1, r] * d[:, 1]) + T[2, r] * d[:, 2] for r in range(3)], axis=1)
        else:
            d, x = q.copy(), q.copy()
        rho = _norm3(x[:, 0], x[:, 1], x[:, 2])
        valid = np.isfinite(rho) & (rho > 0.0)
        bounded = max_range > 0.0 and math.isfinite(max_range)
        if bounded:
            valid &= rho <= max_range
        u = np.zeros_like(x)
        u[valid] = x[valid] / rho[valid][:, None]
        margin = np.abs(rho - max_range) / max_range if bounded else np.full(rho.shape, np.inf)
    return SimpleNamespace(d=d, x=x, rho=rho, u=u, valid=valid, range_margin=margin)


def _rel(a, b):
    with np.errstate(all='ignore'):
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def update_rows(map_points, map_normals, pose, reading, rows, match_idx, match_chord, prm, prob):
    """dc_dyn_update's contract on host arrays: entry i pairs the map row rows[i] with the reading row match_idx[i] at the chord
    match_chord[i].  Returns SimpleNamespace(prob [N] (a copy, updated), seen uint8 [N], branch {name: bool [R]}, margin {name:
    float [R]}); the margins are inf where the decision was not taken."""
    q = np.asarray(map_points, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(map_normals, dtype=np.float64).reshape(-1, 3)
    p_all = np.asarray(reading, dtype=np.float64).reshape(-1, 3)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    j = np.asarray(match_idx, dtype=np.int64).reshape(-1)
    c = np.asarray(match_chord, dtype=np.float64).reshape(-1)
    P_out = np.array(prob, dtype=np.float64).reshape(-1).copy()
    seen = np.zeros(q.shape[0], dtype=np.uint8)
    R = rows.shape[0]
    inf = np.full(R, np.inf)
    branch = {k: np.zeros(R, dtype=bool) for k in ('unmatched', 'chord_refused', 'map_invalid', 'reading_invalid', 'occluded', 'updated',
                                                   'wd2_eps', 'wd2_ramp', 'wd2_one', 'wp2_one', 'wp2_ramp', 'wp2_eps', 'below_threshold',
                                                   'dynamic')}
    margin = {k: inf.copy() for k in ('chord', 'range', 'occlusion', 'delta', 'offset', 'behind', 'threshold')}
    ok = (rows >= 0) & (rows < q.shape[0])
    branch['unmatched'] = ok & ((j < 0) | (j >= p_all.shape[0]))
    ok &= ~branch['unmatched']
    with np.errstate(all='ignore'):
        refused = ok & ~(c < prm.chord_max)
    branch['chord_refused'] = refused
    margin['chord'] = np.where(ok, _rel(c, prm.chord_max), np.inf)
    ok &= ~refused
    rs = np.where(ok, rows, 0)
    js = np.where(ok, j, 0)
    dm = direction(q[rs], pose, prm.max_range)
    margin['range'] = np.where(ok, dm.range_margin, np.inf)
    branch['map_invalid'] = ok & ~dm.valid
    ok &= dm.valid
    p = p_all[js]
    with np.errstate(all='ignore'):
        r = _norm3(p[:, 0], p[:, 1], p[:, 2])
        r_ok = np.isfinite(r) & (r > 0.0)
        branch['reading_invalid'] = ok & ~r_ok
        ok &= r_ok
        x, rho, d, n = dm.x, dm.rho, dm.d, nrm[rs]
        delta = _norm3(p[:, 0] - x[:, 0], p[:, 1] - x[:, 1], p[:, 2] - x[:, 2])
        d_max = prm.epsilon_a * r
        reach = (r + prm.epsilon_d) + d_max
        occluded = ok & ~(reach >= rho)
        margin['occlusion'] = np.where(ok, _rel(reach, rho), np.inf)
        upd = ok & ~occluded
        w_v = EPS + ONE * np.abs((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) / rho
        w_d1 = EPS + ONE * (1.0 - c / prm.chord_max)
        offset = delta - prm.epsilon_d
        near = delta < prm.epsilon_d
        behind = rho > r
        ramp = offset < d_max
        wd2_eps = near | behind
        w_d2 = np.where(wd2_eps, EPS, np.where(ramp, EPS + ONE * offset / d_max, 1.0))
        w_p2 = np.where(near, 1.0, np.where(ramp, EPS + ONE * (1.0 - offset / d_max), EPS))
        c2 = w_v * w_d1
        c1 = 1.0 - c2
        P = P_out[rs]
        below = P < prm.threshold
        pd = np.where(below, c1 * P + (c2 * w_d2) * ((1.0 - prm.alpha) * (1.0 - P) + prm.beta * P), ONE)
        ps = np.where(below, c1 * (1.0 - P) + (c2 * w_p2) * (prm.alpha * (1.0 - P) + (1.0 - prm.beta) * P), EPS)
        P_new = pd / (pd + ps)
    P_out[rs[upd]] = P_new[upd]
    seen[rs[occluded]] = OCCLUDED
    seen[rs[upd]] = UPDATED
    branch['occluded'], branch['updated'] = occluded, upd
    branch['wd2_eps'], branch['wd2_ramp'], branch['wd2_one'] = upd & wd2_eps, upd & ~wd2_eps & ramp, upd & ~wd2_eps & ~ramp
    branch['wp2_one'], branch['wp2_ramp'], branch['wp2_eps'] = upd & near, upd & ~near & ramp, upd & ~near & ~ramp
    branch['below_threshold'], branch['dynamic'] = upd & below, upd & ~below
    margin['delta'] = np.where(upd, _rel(delta, prm.epsilon_d), np.inf)
    margin['offset'] = np.where(upd & ~near, _rel(offset, d_max), np.inf)
    margin['behind'] = np.where(upd & ~near, _rel(rho, r), np.inf)
    margin['threshold'] = np.where(upd, _rel(P, prm.threshold), np.inf)
    return SimpleNamespace(prob=P_out, seen=seen, branch=branch, margin=margin)


def match_table(map_points, pose, reading, prm):
    """The angular search: every valid map direction's two nearest valid reading directions within chord_max (strict <, cKDTree's
    distance_upper_bound).  Returns SimpleNamespace(rows [R] (valid map rows, ascending), idx [R] (reading row of the nearest, -1
    without one), chord [R] (inf without one), idx2 / chord2 (the second nearest), map / reading (direction() of both))."""
    dm = direction(map_points, pose, prm.max_range)
    dr = direction(reading, None, 0.0)
    rows = np.flatnonzero(dm.valid)
    vrows = np.flatnonzero(dr.valid)
    R = rows.shape[0]
    idx = np.full((R, 2), -1, dtype=np.int64)
    chord = np.full((R, 2), np.inf)
    if R and vrows.shape[0]:
        dist, ind = cKDTree(dr.u[vrows]).query(dm.u[rows], k=2, distance_upper_bound=prm.chord_max)
        found = np.isfinite(dist)
        chord = np.where(found, dist, np.inf)
        idx = np.where(found, vrows[np.minimum(ind, vrows.shape[0] - 1)], -1)
    return SimpleNamespace(rows=rows, idx=idx[:, 0], chord=chord[:, 0], idx2=idx[:, 1], chord2=chord[:, 1], map=dm, reading=dr)


def update_map(map_points, map_normals, pose, reading, prm, prob):
    """One whole update of the map against a registered reading: match_table, then update_rows.  Returns update_rows' result with
    ``table`` and ``counts`` = dict(in_range, matched, occluded, updated, dynamic)."""
    tab = match_table(map_points, pose, reading, prm)
    out = update_rows(map_points, map_normals, pose, reading, tab.rows, tab.idx, tab.chord, prm, prob)
    out.table = tab
    out.counts = dict(in_range=int(tab.rows.shape[0]), matched=int((tab.idx >= 0).sum()), occluded=int((out.seen == OCCLUDED).sum()),
                      updated=int((out.seen == UPDATED).sum()), dynamic=int((out.prob >= prm.threshold).sum()))
    return out


# ---- the host build of csrc/dc_dynmath.h ----------------------------------------------------------------------------------------------
def host_lib():
    """libdc_hostcheck.so with the dynamic-point exports, rebuilt with ``make hostcheck`` when it is missing or predates them."""
    path = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), 'dc_host_dyn_update'):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'depth_correction_amd', 'csrc'), '-B', 'hostcheck'], check=True, capture_output=True)
    lib = ctypes.CDLL(path)
    vp, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    lib.dc_host_dyn_directions.restype = None
    lib.dc_host_dyn_directions.argtypes = [vp, i64, vp, f64, vp, vp, vp]
    lib.dc_host_dyn_update.restype = ctypes.c_int
    lib.dc_host_dyn_update.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, vp, i64] + 7 * [f64] + [vp, vp]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_directions(lib, points, pose=None, max_range=0.0):
    """dc_host_dyn_directions -> (dirs [n,3], depth [n], valid bool [n])."""
    q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    T = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(16)
    n = q.shape[0]
    dirs, depth, valid = np.full((n, 3), np.nan), np.full(n, np.nan), np.full(n, 7, dtype=np.uint8)
    lib.dc_host_dyn_directions(_ptr(q), n, _ptr(T), float(max_range), _ptr(dirs), _ptr(depth), _ptr(valid))
    return dirs, depth, valid.astype(bool)


def host_update(lib, map_points, map_normals, pose, reading, rows, match_idx, match_chord, prm, prob):
    """dc_host_dyn_update -> (status, prob [N] (a copy, updated), seen uint8 [N])."""
    q = np.ascontiguousarray(map_points, dtype=np.float64).reshape(-1, 3)
    nrm = np.ascontiguousarray(map_normals, dtype=np.float64).reshape(-1, 3)
    T = np.ascontiguousarray(pose, dtype=np.float64).reshape(16)
    p = np.ascontiguousarray(reading, dtype=np.float64).reshape(-1, 3)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    j = np.ascontiguousarray(match_idx, dtype=np.int32)
    c = np.ascontiguousarray(match_chord, dtype=np.float64)
    P = np.array(prob, dtype=np.float64).reshape(-1).copy()
    seen = np.zeros(q.shape[0], dtype=np.uint8)
    rc = lib.dc_host_dyn_update(_ptr(q), _ptr(nrm), q.shape[0], _ptr(T), _ptr(p), p.shape[0], _ptr(rows), _ptr(j), _ptr(c), rows.shape[0],
                                prm.chord_max, prm.epsilon_a, prm.epsilon_d, prm.alpha, prm.beta, prm.threshold, prm.max_range, _ptr(P),
                                _ptr(seen))
    return rc, P, seen


def same_bits(a, b):
    """Elementwise: the same fp64 bit pattern, or both NaN (a NaN's sign and payload are not part of any contract here)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ---- inputs the host and the GPU tests share ------------------------------------------------------------------------------------------
TABLE_PRM = dict(epsilon_d=2.0 ** -7, epsilon_a=2.0 ** -6, threshold=0.9, alpha=0.8, beta=0.99, max_range=8.0, beam_half_angle=0.01)


def hand_table():
    """The hand-made table: points on the x axis seen from the identity pose, constants that are powers of two (epsilon_d = 2^-7,
    epsilon_a = 2^-6, r = 4, so d_max = 2^-4 and the reach (r + epsilon_d) + d_max are exact), one row for every branch and both sides
    of every boundary.  Returns SimpleNamespace(prm, pose, map_points, map_normals, reading, rows, match_idx, match_chord, prob,
    names, expect {name: seen code}).  Reading rows: 0 = (4, 0, 0), 1 = (8, 0, 0), 2 = the origin."""
    prm = params(**TABLE_PRM)
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    e_d, d_max, r = prm.epsilon_d, prm.epsilon_a * 4.0, 4.0
    reach = (r + e_d) + d_max
    X, Y, Z0 = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)
    cm = prm.chord_max
    # name, rho (map point (rho, 0, 0)), normal, reading row, chord, P, expected seen
    spec = [
        ('delta_below_eps_d', r - 2.0 ** -8, X, 0, 0.0, 0.6, 2),
        ('delta_equals_eps_d', r - e_d, X, 0, 0.0, 0.6, 2),
        ('delta_above_eps_d', r - 2.0 ** -6, X, 0, 0.0, 0.6, 2),
        ('offset_below_d_max', r - (e_d + 2.0 ** -5), X, 0, 0.0, 0.6, 2),
        ('offset_equals_d_max', r - (e_d + d_max), X, 0, 0.0, 0.6, 2),
        ('offset_above_d_max', r - 0.5, X, 0, 0.0, 0.6, 2),
        ('rho_far_in_front', 1.0, X, 0, 0.0, 0.6, 2),
        ('rho_equals_r', r, X, 0, 0.0, 0.6, 2),
        ('rho_above_r_near', r + 2.0 ** -8, X, 0, 0.0, 0.6, 2),
        ('rho_above_r_ramp', r + 2.0 ** -6, X, 0, 0.0, 0.6, 2),
        ('rho_one_ulp_above_r', up(r), X, 0, 0.0, 0.6, 2),
        ('rho_one_ulp_below_r', dn(r), X, 0, 0.0, 0.6, 2),
        ('reach_exact', reach, X, 0, 0.0, 0.6, 2),
        ('reach_one_ulp_inside', dn(reach), X, 0, 0.0, 0.6, 2),
        ('reach_one_ulp_behind', up(reach), X, 0, 0.0, 0.6, 1),
        ('far_behind', 6.0, X, 0, 0.0, 0.6, 1),
        ('P_one_ulp_below_threshold', r - 0.5, X, 0, 0.0, dn(prm.threshold), 2),
        ('P_at_threshold', r - 0.5, X, 0, 0.0, prm.threshold, 2),
        ('P_one_ulp_above_threshold', r - 0.5, X, 0, 0.0, up(prm.threshold), 2),
        ('P_dynamic_static_evidence', r, X, 0, 0.0, 0.95, 2),
        ('P_zero', r - 0.5, X, 0, 0.0, 0.0, 2),
        ('P_one', r, X, 0, 0.0, 1.0, 2),
        ('rho_equals_max_range', 8.0, X, 1, 0.0, 0.6, 2),
        ('rho_one_ulp_above_max_range', up(8.0), X, 1, 0.0, 0.6, 0),
        ('chord_zero', r - 2.0 ** -5, X, 0, 0.0, 0.3, 2),
        ('chord_one_ulp_below_max', r - 2.0 ** -5, X, 0, dn(cm), 0.3, 2),
        ('chord_equals_max', r - 2.0 ** -5, X, 0, cm, 0.3, 0),
        ('chord_above_max', r - 2.0 ** -5, X, 0, 2.0 * cm, 0.3, 0),
        ('chord_half', r - 0.5, X, 0, 0.5 * cm, 0.6, 2),
        ('normal_perpendicular', r - 0.5, Y, 0, 0.0, 0.6, 2),
        ('normal_zero', r - 0.5, Z0, 0, 0.0, 0.6, 2),
        ('normal_opposed', r - 0.5, (-1.0, 0.0, 0.0), 0, 0.0, 0.6, 2),
        ('unmatched', r - 0.5, X, -1, np.inf, 0.6, 0),
        ('reading_at_origin', r - 0.5, X, 2, 0.0, 0.6, 0),
        ('map_point_at_sensor', 0.0, X, 0, 0.0, 0.6, 0),
        ('map_point_behind_sensor', -3.0, X, 0, 0.0, 0.6, 2),
    ]
    n = len(spec)
    t = SimpleNamespace(prm=prm, pose=np.eye(4), names=[s[0] for s in spec], expect={s[0]: s[6] for s in spec})
    t.map_points = np.array([[s[1], 0.0, 0.0] for s in spec])
    t.map_normals = np.array([s[2] for s in spec], dtype=np.float64)
    t.reading = np.array([[4.0, 0.0, 0.0], [8.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    t.rows = np.arange(n, dtype=np.int32)
    t.match_idx = np.array([s[3] for s in spec], dtype=np.int32)
    t.match_chord = np.array([s[4] for s in spec], dtype=np.float64)
    t.prob = np.array([s[5] for s in spec], dtype=np.float64)
    return t


def random_pose(rng):
    """A rigid pose with a generic rotation (QR of a Gaussian matrix, determinant +1) and a translation of a few metres."""
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3] = Q
    T[:3, 3] = rng.uniform(-3.0, 3.0, size=3)
    return T


def random_rows(n, m, seed, skip=False):
    """n map rows against m reading points built so that every branch of the rule is taken often: a map point is its reading point
    moved along the ray (a hair, into the ramp, far in front, just behind, far behind) and turned by a fraction of the beam; some
    rows are unmatched, out of range (max_range = 8 with depths up to 10), beyond the chord, or dynamic already.  The chord handed
    in is that of the two unit vectors.  ``skip``: the rows handed in leave map rows out (every third row of a larger map).
    Returns the fields of hand_table()."""
    rng = np.random.default_rng(seed)
    prm = params(max_range=8.0)
    pose = random_pose(rng)
    v = rng.normal(size=(m, 3))
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    depth = rng.uniform(1.0, 10.0, size=m)
    reading = v * depth[:, None]
    j = rng.integers(0, m, size=n)
    r = depth[j]
    kind = rng.integers(0, 6, size=n)
    d_max = prm.epsilon_a * r
    along = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                      [rng.uniform(-0.9, 0.9, n) * prm.epsilon_d, -(prm.epsilon_d + rng.uniform(0.05, 0.95, n) * d_max),
                       -rng.uniform(0.2, 0.8, n) * r, rng.uniform(0.05, 0.95, n) * (prm.epsilon_d + d_max),
                       prm.epsilon_d + d_max + rng.uniform(0.05, 2.0, n)], prm.epsilon_d + rng.uniform(0.05, 0.95, n) * d_max * 0.5)
    side = rng.normal(size=(n, 3))
    side -= (side * v[j]).sum(axis=1, keepdims=True) * v[j]
    side /= np.sqrt((side * side).sum(axis=1, keepdims=True))
    wide = rng.random(n) < 0.1
    ang = np.where(wide, rng.uniform(1.05, 3.0, n), np.where(kind == 0, rng.uniform(0.0, 0.05, n), rng.uniform(0.0, 0.95, n))) * prm.chord_max
    x = (v[j] * np.cos(ang)[:, None] + side * np.sin(ang)[:, None]) * (r + along)[:, None]
    q = x @ pose[:3, :3].T + pose[:3, 3]
    nrm = rng.normal(size=(n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    prob = np.where(rng.random(n) < 0.15, rng.uniform(0.9, 1.0, n), rng.uniform(0.0, 0.9, n))
    dm, dr = direction(q, pose, 0.0), direction(reading, None, 0.0)
    e = dr.u[j] - dm.u
    chord = _norm3(e[:, 0], e[:, 1], e[:, 2])
    j = np.where(rng.random(n) < 0.08, -1, j)
    t = SimpleNamespace(prm=prm, pose=pose, map_points=q, map_normals=nrm, reading=reading, prob=prob)
    keep = np.arange(0, n, 3) if skip else np.arange(n)
    t.rows, t.match_idx, t.match_chord = keep.astype(np.int32), j[keep].astype(np.int32), chord[keep]
    return t
