"""The reference of the sweep-aware (12-dof) registration: DESIGN "Sweep-aware registration" restated in plain numpy + cKDTree, fp64 on
the CPU, sums in extended precision.  Nothing here calls depth_correction_amd; the plain helpers (moved points, matching, the trimmed
threshold, the rotation of a step) are those of tests/slam_reference.py, which the 6-dof kernels are held to.

Model: reading point p measured at the sweep time tau, pose T = [R | t] of the sweep's start, twist (v, w):
    q = Exp(tau w) p + tau v,   x = R q + t,   r = n_map . (x - y)
Unknown (d theta, d t, d v, d w): d theta, d t left-multiplied onto T, v += d v, w += d w.  Row of the Jacobian, n_s = R^T n_map,
a = tau w, u = Exp(a) p:   [x x n_map, n_map, tau n_s, tau J_l(a)^T (u x n_s)].
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree

import slam_reference as R

LD = np.longdouble
N_TOT = 93
# The largest change of this reference's own poses and twists, per iteration, when the order of its extended-precision sums is permuted:
# 200 random orders on the host-cast parity scene of tests/test_slam_ct_host.py (which recomputes it over a few orders).  The GPU
# parity test allows the device 2 000 x this, the factor DESIGN "SLAM evaluation" gives for the 6-dof bar.  The figure depends on where
# roundings fall: a copy of the scene whose rays were formed in another operation order gave 2.2e-16.
REF_SENSITIVITY = 3.61e-16
CT_DEFAULTS = dict(slam_ct_prior=(1e-4, 1e-4), slam_ct_max_twist=None)


def params(cfg=None, **kw):
    """slam_reference.params plus slam_ct_prior = (beta_v, beta_w) and slam_ct_max_twist = (trans, rot) (None: the pose bounds)."""
    ct = dict(CT_DEFAULTS)
    for name in ct:
        if cfg is not None and hasattr(cfg, name):
            ct[name] = getattr(cfg, name)
        if name in kw:
            ct[name] = kw.pop(name)
    prm = R.params(cfg, **kw)
    prm.slam_ct_prior = tuple(float(b) for b in ct['slam_ct_prior'])
    mt = ct['slam_ct_max_twist']
    prm.slam_ct_max_twist = (prm.icp_max_translation, prm.icp_max_rotation) if mt is None else tuple(float(b) for b in mt)
    return prm


def hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=np.asarray(a).dtype)


def _series(x, first, n_terms=14):
    """sum_k (-x)^k / (first + 2 k)! in the dtype of x."""
    s, term = type(x)(0), type(x)(1) / type(x)(math.factorial(first))
    for k in range(n_terms):
        s += term
        term = -term * x / type(x)((first + 2 * k + 1) * (first + 2 * k + 2))
    return s


def coefficients(th):
    """(A, C1, C2) = (sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3) in the dtype of th; series below 1/2."""
    if abs(th) < 0.5:
        x = th * th
        return _series(x, 1), _series(x, 2), _series(x, 3)
    h = th / 2
    q = np.sin(h) / h
    return np.sin(th) / th, q * q / 2, (th - np.sin(th)) / (th * th * th)


def left_jacobian(a, dtype=np.float64):
    """J_l(a) = I + C1 [a]x + C2 [a]x^2 (dtype longdouble: the exact matrix the header's count is measured against)."""
    a = np.asarray(a, dtype=dtype)
    th = np.sqrt(a @ a)
    _, c1, c2 = coefficients(th)
    K = hat(a)
    return np.eye(3, dtype=dtype) + c1 * K + c2 * (K @ K)


def sweep_rotation(a, dtype=np.float64):
    a = np.asarray(a, dtype=dtype)
    th = np.sqrt(a @ a)
    A, c1, _ = coefficients(th)
    K = hat(a)
    return np.eye(3, dtype=dtype) + A * K + c1 * (K @ K)


def deskew(p, pn, tau, twist):
    """(q [M,3], nq [M,3], u [M,3]): q = Exp(tau w) p + tau v, nq = Exp(tau w) pn, u = Exp(tau w) p, with the operation order of
    csrc/dc_sweepmath.h: ((x + A (a x x)) + B (a x (a x x))) + tau v, A = (sin h / h) cos h, B = (sin h / h)^2 / 2 at h = |a| / 2."""
    p, pn, tau = np.asarray(p, dtype=np.float64), np.asarray(pn, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    v, w = np.asarray(twist[:3], dtype=np.float64), np.asarray(twist[3:], dtype=np.float64)
    a = tau[:, None] * w[None, :]
    th = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    small = th < 2.0 ** -26
    h = np.where(small, 1.0, 0.5 * th)
    qq = np.sin(h) / h
    A = np.where(small, 1.0, qq * np.cos(h))[:, None]
    B = np.where(small, 0.5, 0.5 * (qq * qq))[:, None]

    def rot(x):
        c = np.cross(a, x)
        e = np.cross(a, c)
        return (x + A * c) + B * e
    u = rot(p)
    return u + tau[:, None] * v[None, :], rot(pn), u


def coefficient_rows(th):
    """(C1, C2) of the rows th [n] in th's dtype: series below 1/2, the closed forms above."""
    th = np.asarray(th)
    x = th * th
    one = th.dtype.type(1)
    s2, s3 = np.zeros_like(th), np.zeros_like(th)
    t2, t3 = np.full_like(th, one / 2), np.full_like(th, one / 6)
    for k in range(14):
        s2, s3 = s2 + t2, s3 + t3
        t2 = -t2 * x / ((2 * k + 3) * (2 * k + 4))
        t3 = -t3 * x / ((2 * k + 4) * (2 * k + 5))
    big = th >= 0.5
    safe = np.where(big, th, one)
    q = np.sin(safe / 2) / (safe / 2)
    return np.where(big, q * q / 2, s2), np.where(big, (safe - np.sin(safe)) / (safe * safe * safe), s3)


def jl_transposed_rows(a, c):
    """J_l(a_i)^T c_i of the rows a, c [n,3] (their dtype): c - C1 (a x c) + C2 (a x (a x c))."""
    c1, c2 = coefficient_rows(np.sqrt((a * a).sum(axis=1)))
    ac = np.cross(a, c)
    return c - c1[:, None] * ac + c2[:, None] * np.cross(a, ac)


def rotate_rows(a, x):
    """Exp(a_i) x_i of the rows a, x [n,3] in longdouble (x + A (a x x) + C1 (a x (a x x)))."""
    a, x = np.asarray(a, dtype=LD), np.asarray(x, dtype=LD)
    th = np.sqrt((a * a).sum(axis=1))
    c1, _ = coefficient_rows(th)
    sA, tA = np.zeros_like(th), np.ones_like(th)
    for k in range(14):
        sA = sA + tA
        tA = -tA * th * th / ((2 * k + 2) * (2 * k + 3))
    safe = np.where(th >= 0.5, th, LD(1))
    A = np.where(th >= 0.5, np.sin(safe) / safe, sA)
    ax = np.cross(a, x)
    return x + A[:, None] * ax + c1[:, None] * np.cross(a, ax)


def residual(p, tau, T, twist, n, y):
    """r = n . (R (Exp(tau w) p + tau v) + t - y) of single pairs [n_pairs], plain fp64 (the function the Jacobian is checked against)."""
    q, _, _ = deskew(p, p, tau, twist)
    x = q @ T[:3, :3].T + T[:3, 3]
    return np.einsum('ij,ij->i', n, x - y)


def jacobian_rows(p, tau, T, twist, n, x=None, dtype=np.float64):
    """J [n_pairs, 12] of single pairs (p, tau, n one row per pair) in ``dtype``; x [n_pairs, 3] are the moved points (computed from
    the reference's own de-skew when not given).  With dtype longdouble u = Exp(tau w) p and J_l are formed in extended precision
    from the fp64 inputs: the exact row the device's fp64 row is an approximation of."""
    tau = np.asarray(tau, dtype=np.float64)
    w = np.asarray(twist[3:], dtype=np.float64)
    if x is None:
        x = R.moved(T, deskew(p, p, tau, twist)[0])
    a = tau.astype(dtype)[:, None] * w.astype(dtype)[None, :]
    u = rotate_rows(a, p).astype(dtype)
    n, x = np.asarray(n, dtype=dtype), np.asarray(x, dtype=dtype)
    ns = n @ np.asarray(T[:3, :3], dtype=dtype)            # rows R^T n
    jw = jl_transposed_rows(a, np.cross(u, ns))
    tt = tau.astype(dtype)[:, None]
    return np.concatenate([np.cross(x, n), n, tt * ns, tt * jw], axis=1)


def pair_terms(map_pts, map_nrm, p, tau, T, twist, x, rows, ids):
    """The 93 summands of every kept pair [n, 93] in longdouble (JtJ upper triangle 78, Jtr 12, 1, r^2, 0): pair (rows[i], ids[i]);
    x [M,3] the moved de-skewed points."""
    if len(rows) == 0:
        return np.zeros((0, N_TOT), dtype=LD)
    n, y, xx = map_nrm[ids].astype(LD), map_pts[ids].astype(LD), x[rows].astype(LD)
    J = jacobian_rows(p[rows], tau[rows], T, twist, n, x=xx, dtype=LD)
    r = (n * (xx - y)).sum(axis=1)
    cols = [J[:, a] * J[:, b] for a in range(12) for b in range(a, 12)] + [J[:, a] * r for a in range(12)]
    cols += [np.ones_like(r), r * r, np.zeros_like(r)]
    return np.stack(cols, axis=1)


def totals(map_pts, map_nrm, p, pn, tau, T, twist, idx, dist, thr, cos_min, order=None, q=None, nq=None):
    """slam_reference.totals for the sweep-aware row: both pair filters (on the de-skewed normals, rotated by R) and the 93 totals;
    q / nq: the de-skewed points and normals to use (the device's own; the reference's deskew when not given).
    Returns dict(kept, totals [93], abs_totals [93], n_pairs, normal_margin)."""
    if q is None or nq is None:
        q, nq, _ = deskew(p, pn, tau, twist)
    x = R.moved(T, q)
    nr = nq @ T[:3, :3].T
    with np.errstate(invalid='ignore'):
        near = (idx >= 0) & (dist <= thr)
    rows, cols = np.nonzero(near)
    dots = np.abs(np.einsum('ij,ij->i', nr[rows], map_nrm[idx[rows, cols]]))
    kept = np.zeros(idx.shape, dtype=bool)
    kept[rows, cols] = dots >= cos_min
    rows, cols = np.nonzero(kept)
    if order is not None:
        rows, cols = rows[order], cols[order]
    tot, abs_tot = np.zeros(N_TOT, dtype=LD), np.zeros(N_TOT, dtype=LD)
    for a in range(0, len(rows), 1 << 16):
        sl = slice(a, a + (1 << 16))
        terms = pair_terms(map_pts, map_nrm, p, tau, T, twist, x, rows[sl], idx[rows[sl], cols[sl]])
        tot += terms.sum(axis=0)
        abs_tot += np.abs(terms).sum(axis=0)
    tot, abs_tot = np.asarray(tot, dtype=np.float64), np.asarray(abs_tot, dtype=np.float64)
    tot[92] = float(kept.any(axis=1).sum())
    normal_margin = float(np.abs(dots - cos_min).min()) if len(dots) else float('inf')
    return dict(kept=kept, totals=tot, abs_totals=abs_tot, n_pairs=len(rows), normal_margin=normal_margin)


def pack78(A):
    return np.array([A[r, c] for r in range(12) for c in range(r, 12)])


def unpack78(a78, dtype=LD):
    A = np.zeros((12, 12), dtype=dtype)
    q = 0
    for r in range(12):
        for c in range(r, 12):
            A[r, c] = A[c, r] = a78[q]
            q += 1
    return A


def solve12(A, b, rel_eps=1e-12):
    """x = -A^-1 b by Cholesky in extended precision (A [12,12] longdouble), None when a pivot is <= rel_eps x the largest diagonal
    entry or not finite."""
    dmax = np.abs(np.diag(A)).max()
    if not (dmax > 0) or not np.isfinite(dmax):
        return None
    L = np.zeros((12, 12), dtype=LD)
    for j in range(12):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (s > rel_eps * dmax) or not np.isfinite(s):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 12):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y, x = np.zeros(12, dtype=LD), np.zeros(12, dtype=LD)
    with np.errstate(invalid='ignore'):
        for i in range(12):
            y[i] = (-b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
        for i in range(11, -1, -1):
            x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x.astype(np.float64)


def new_state(prior, twist0=None):
    st = R.new_state(prior)
    tw = np.zeros(6) if twist0 is None else np.asarray(twist0, dtype=np.float64).reshape(6)
    st.twist, st.twist0 = tw.copy(), tw.copy()
    return st


def _norm(a):
    return math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))


def finish(tot, m, prm, st):
    """The end of a sweep-aware iteration from its 93 totals, in dc_icp_ct_finish's documented order.  Returns (x or None, margins)."""
    st.iters += 1
    st.pairs, st.sse = float(tot[90]), float(tot[91])
    st.overlap = float(tot[92]) / m if m > 0 else 0.0
    margins = {}
    if tot[90] < prm.min_pairs:
        st.code = R.FAIL_PAIRS
        return None, margins
    A, b = unpack78(tot[:78]), np.asarray(tot[78:90], dtype=LD).copy()
    bv, bw = prm.slam_ct_prior
    for q in range(6):
        wgt = LD(st.pairs) * LD(bv if q < 3 else bw)
        A[6 + q, 6 + q] += wgt
        b[6 + q] += wgt * (LD(st.twist[q]) - LD(st.twist0[q]))
    x = solve12(A, b)
    if x is None:
        st.code = R.FAIL_SINGULAR
        return None, margins
    D = np.eye(4)
    with np.errstate(all='ignore'):
        D[:3, :3], D[:3, 3] = R.rotation(x[:3]), x[3:6]
        Tn = D @ st.pose
        twn = st.twist + x[6:]
    if not (np.isfinite(x).all() and np.isfinite(Tn).all() and np.isfinite(twn).all()):
        st.code = R.FAIL_NONFINITE
        return x, margins
    C = Tn @ R.rigid_inv(st.prior)
    c_rot, c_trans = R.rotation_angle(C), float(np.linalg.norm(C[:3, 3]))
    max_tt, max_tr = prm.slam_ct_max_twist
    dv, dw, wn = _norm(twn[:3] - st.twist0[:3]), _norm(twn[3:] - st.twist0[3:]), _norm(twn[3:])
    margins['bound_rot'], margins['bound_trans'] = abs(c_rot - prm.icp_max_rotation), abs(c_trans - prm.icp_max_translation)
    margins['bound_twist'] = min(abs(dv - max_tt), abs(dw - max_tr), abs(wn - math.pi))
    if not (c_rot <= prm.icp_max_rotation) or not (c_trans <= prm.icp_max_translation) or not (wn <= math.pi) or not (dv <= max_tt) \
            or not (dw <= max_tr):
        st.code = R.FAIL_BOUND
        return x, margins
    st.pose, st.twist = Tn, twn
    slot = (st.iters - 1) % R.MAX_SMOOTH
    st.hist_rot[slot] = max(_norm(x[0:3]), _norm(x[9:12]))
    st.hist_trans[slot] = max(_norm(x[3:6]), _norm(x[6:9]))
    smooth = int(prm.icp_smooth_length)
    if st.iters >= smooth:
        slots = [(st.iters - 1 - h) % R.MAX_SMOOTH for h in range(smooth)]
        mr, mt = st.hist_rot[slots].sum() / smooth, st.hist_trans[slots].sum() / smooth
        margins['conv_rot'] = abs(mr - prm.icp_min_diff_rot) / prm.icp_min_diff_rot
        margins['conv_trans'] = abs(mt - prm.icp_min_diff_trans) / prm.icp_min_diff_trans
        margins['mean_rot'], margins['mean_trans'] = mr, mt
        if mr < prm.icp_min_diff_rot and mt < prm.icp_min_diff_trans:
            st.code = R.CONVERGED
            return x, margins
    if st.iters >= prm.icp_max_iters:
        st.code = R.MAX_ITERS
    return x, margins


def iteration(map_pts, map_nrm, p, pn, tau, st, prm, tree=None, order_seed=None):
    """One sweep-aware iteration on ``st`` (new_state): de-skew by the twist, match, threshold, totals, finish.  A record like
    slam_reference.iteration's, with twist and q."""
    tree = tree if tree is not None else cKDTree(map_pts)
    T, twist = st.pose.copy(), st.twist.copy()
    q, _, _ = deskew(p, pn, tau, twist)
    idx, dist = R.match(tree, len(map_pts), R.moved(T, q), int(prm.icp_knn), prm.icp_max_dist)
    thr = R.quantile_finite(dist, prm.icp_trim_ratio)
    cos_min = math.cos(prm.icp_max_normal_angle)
    t = totals(map_pts, map_nrm, p, pn, tau, T, twist, idx, dist, thr, cos_min)
    if order_seed is not None and t['n_pairs']:
        order = np.random.default_rng(order_seed).permutation(t['n_pairs'])
        t = totals(map_pts, map_nrm, p, pn, tau, T, twist, idx, dist, thr, cos_min, order=order)
    x, margins = finish(t['totals'], len(p), prm, st)
    fin = dist[np.isfinite(dist)]
    off = fin[fin != thr] if ((fin.size - 1) * prm.icp_trim_ratio) % 1.0 == 0.0 else fin
    margins['thr'] = float(np.abs(off - thr).min() / thr) if off.size and thr > 0 else float('inf')
    margins['normal'] = t['normal_margin']
    return SimpleNamespace(idx=idx, dist=dist, thr=thr, kept=t['kept'], totals=t['totals'], abs_totals=t['abs_totals'], x=x,
                           pose_before=T, twist_before=twist, pose=st.pose.copy(), twist=st.twist.copy(), code=st.code, iters=st.iters,
                           pairs=st.pairs, sse=st.sse, overlap=st.overlap, hist_rot=st.hist_rot.copy(), hist_trans=st.hist_trans.copy(),
                           margins=margins)


Registration = namedtuple('Registration', 'pose twist status iterations overlap pairs sse records')


def register(map_pts, map_nrm, p, pn, tau, prior, twist0, prm, tree=None, order_seed=None):
    """A sweep-aware registration from ``prior`` and the prior twist ``twist0``; a failed one returns the prior and twist0."""
    prior = np.asarray(prior, dtype=np.float64).reshape(4, 4)
    tree = tree if tree is not None else cKDTree(map_pts)
    st = new_state(prior, twist0)
    recs = []
    while st.code == R.RUNNING:
        recs.append(iteration(map_pts, map_nrm, p, pn, tau, st, prm, tree, None if order_seed is None else order_seed + len(recs)))
    status = R.STATUS[st.code]
    failed = status in R.FAILED
    return Registration(prior.copy() if failed else st.pose.copy(), st.twist0.copy() if failed else st.twist.copy(), status, st.iters,
                        st.overlap, int(st.pairs), st.sse, recs)


# ---- dc_icp_ct_finish as a state machine: scripted registrations -------------------------------------------------------------------
# As in slam_reference: JtJ = I, beta = 0 and Jtr = -x make the solved step exactly x.  A step is (rot, trans, dv, dw) magnitudes on
# one axis per part, powers of two, so every norm, maximum and mean of the history is exact.
D_ROT, D_TRANS = R.D_ROT, R.D_TRANS


def _x(rot=0.0, trans=0.0, dv=0.0, dw=0.0, axis=2):
    x = np.zeros(12)
    x[axis], x[3 + (axis + 1) % 3], x[6 + (axis + 2) % 3], x[9 + axis] = rot, trans, dv, dw
    return x


def finish_cases():
    """[(name, parameter overrides, steps, expected status after every step)]; a step is an increment x [12] or a dict(x, pairs, sse,
    used, m, A (12 x 12), b [12])."""
    big, small = _x(8 * D_ROT, 8 * D_TRANS, 4 * D_TRANS, 4 * D_ROT), _x(D_ROT / 2, D_TRANS / 2, D_TRANS / 4, D_ROT / 4)
    tw_big = _x(D_ROT / 2, D_TRANS / 2, 8 * D_TRANS, 8 * D_ROT)            # the pose is still, the twist is not
    equal_times = np.eye(12)                                               # all tau equal: the columns of v are tau x those of t
    equal_times[6:9, 6:9] = 0.25 * np.eye(3)
    equal_times[3:6, 6:9] = equal_times[6:9, 3:6] = 0.5 * np.eye(3)
    b_nan, b_inf = np.zeros(12), np.zeros(12)
    b_nan[7], b_inf[10] = np.nan, np.inf
    loose = dict(icp_min_diff_rot=2.0 ** -30, icp_min_diff_trans=2.0 ** -30)
    return [
        ('smooth1_crosses_at_3', dict(icp_smooth_length=1), [_x(4 * D_ROT, 4 * D_TRANS), _x(2 * D_ROT, 2 * D_TRANS), small], [0, 0, 1]),
        ('smooth1_twist_keeps_it_running', dict(icp_smooth_length=1), [tw_big, _x(dv=2 * D_TRANS), _x(dw=2 * D_ROT), small], [0, 0, 0, 1]),
        ('smooth1_norm_equal_is_not_below', dict(icp_smooth_length=1), [_x(D_ROT, 0.0), _x(0.0, D_TRANS), _x(dv=D_TRANS), _x(dw=D_ROT),
                                                                        small], [0, 0, 0, 0, 1]),
        ('smooth2_mean', dict(icp_smooth_length=2), [big, small, small], [0, 0, 1]),
        ('smooth2_mean_equal_is_not_below', dict(icp_smooth_length=2), [_x(dw=1.5 * D_ROT), _x(dw=0.5 * D_ROT), small], [0, 0, 1]),
        ('smooth8_needs_eight_iterations', dict(icp_smooth_length=8), 8 * [small], 7 * [0] + [1]),
        ('smooth8_ring_wraps', dict(icp_smooth_length=8), 3 * [big] + 8 * [small], 10 * [0] + [1]),
        ('max_iters_keeps_the_update', dict(icp_max_iters=3), 3 * [big], [0, 0, 2]),
        ('converged_wins_over_max_iters', dict(icp_smooth_length=1, icp_max_iters=2), [big, small], [0, 1]),
        ('bound_rotation_total_from_prior', dict(icp_max_rotation=0.85, **loose), 10 * [_x(0.1, 0.0)], 8 * [0] + [-4]),
        ('bound_translation_total_from_prior', dict(icp_max_translation=0.85, **loose), 10 * [_x(0.0, 0.1)], 8 * [0] + [-4]),
        ('bound_twist_translation', dict(slam_ct_max_twist=(0.4375, 3.0), **loose), 5 * [_x(dv=0.125)], 3 * [0] + [-4]),
        ('bound_twist_translation_equal_is_inside', dict(slam_ct_max_twist=(0.375, 3.0), **loose), 5 * [_x(dv=0.125)], 3 * [0] + [-4]),
        ('bound_twist_rotation', dict(slam_ct_max_twist=(30.0, 0.4375), **loose), 5 * [_x(dw=0.125)], 3 * [0] + [-4]),
        ('bound_twist_nan_fails_at_once', dict(slam_ct_max_twist=(float('nan'), 3.0)), [small], [-4]),
        ('w_above_pi', dict(slam_ct_max_twist=(30.0, 30.0), **loose), 8 * [_x(dw=0.5)], 6 * [0] + [-4]),
        ('pairs_equal_min_pairs_runs', dict(min_pairs=6), [dict(x=big, pairs=6.0), dict(x=big, pairs=5.0, sse=0.25, used=3.0)], [0, -1]),
        ('no_points', dict(min_pairs=6), [dict(x=big, pairs=0.0, sse=0.0, used=0.0, m=0)], [-1]),
        ('equal_times_beta0_is_singular', dict(), [big, dict(x=big, A=equal_times)], [0, -2]),
        ('nan_in_jtr', dict(), [big, dict(x=big, b=b_nan)], [0, -3]),
        ('inf_in_jtr', dict(), [big, dict(x=big, b=b_inf)], [0, -3]),
    ]


SCRIPT_TWIST = np.array([0.25, -0.125, 0.0625, 0.03125, 0.0, -0.0625])


def script_params(over):
    kw = dict(icp_min_diff_rot=D_ROT, icp_min_diff_trans=D_TRANS, icp_smooth_length=2, icp_max_iters=100, icp_max_rotation=3.0,
              icp_max_translation=30.0, min_pairs=6, slam_ct_prior=(0.0, 0.0), slam_ct_max_twist=(30.0, 3.0))
    kw.update(over)
    return params(**kw)


def script_totals(step):
    """(totals [93], m) of a script step."""
    step = step if isinstance(step, dict) else dict(x=step)
    x = np.asarray(step['x'], dtype=np.float64)
    tot = np.zeros(N_TOT)
    tot[:78] = pack78(np.asarray(step.get('A', np.eye(12)), dtype=np.float64))
    tot[78:90] = step.get('b', -x)
    tot[90], tot[91], tot[92] = step.get('pairs', 100.0), step.get('sse', 0.5), step.get('used', 40.0)
    return tot, int(step.get('m', 50))


def state_vectors(st):
    """(the 64 doubles of the 6-dof state, the 16 of the twist state) of a reference state."""
    ct = np.zeros(16)
    ct[0:6], ct[6:12] = st.twist, st.twist0
    return R.state_vector(st), ct


def block_sum(partials):
    return R.block_sum(partials)
