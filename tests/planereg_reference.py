"""Reference of the plane registration tests (test_planereg_host.py, test_gpu_planereg.py): numpy and scipy's cKDTree only, a
restatement of DESIGN "Plane registration" -- nothing here calls depth_correction_amd except planes_reference's sampler.  The fit is
by SVD on the normals (``align_reference.fit_svd`` style, no means: normals are directions) with the translation by numpy's LU
solve; a second route, Horn's matrix + ``numpy.linalg.eigh`` with the translation by Cramer's rule, is the yardstick of the bar on T.

Every discrete decision the tests compare is taken here with a margin, asserted on every input they use:
  the cloud triples  | |det[n_a n_b n_c]| - min_det | >= 1e-9
  rule 2             | |det[m_i m_j m_k]| - min_det | >= 1e-9 for every distinct (i, j, k)
  rule 3             every comparison a hypothesis REACHES (rules are checked in order) is decided by >= 1e-9
  rule 4             |det product| >= 1e-6 where it is reached
  plane agreement    | |n'.m| - cos_tol | >= 1e-9 for every (valid hypothesis, q, r); | |sgn d' - e| - tol_d | >= 1e-9 where the first holds
  suppression        |angle - dedupe_rot| >= 1e-9 and |distance - dedupe_trans| >= 1e-9 for every hypothesis alive in a round
  fitness            1e-9 m (globalreg_reference.fitness)
  plane fits         ``border`` == 0 (planes_reference.fit_planes_restated)
Score and fitness ties are integer ties decided by stated rules (the lower h, the earlier candidate): counted, their order checked.

Scenes: the five placements of globalreg_reference and 'last60', the LAST 60 % of the room's length (x > 3.2 m) turned by 180 deg
about z -- the partial cloud the descriptor method cannot place (DESIGN "Global registration").

The bar on T: the two routes differ by at most 1.07e-14 over every valid hypothesis of every input the tests use (the largest figure
is 'turn75' on the restated planes; 5.3e-15 to 7.1e-15 on the other scenes and on the device's planes, 6.7e-16 to 4e-15 on the
designed inputs: min_det = 0.5 keeps the triples fat).  ``T_ROUTES`` = 1.07e-14 is that figure (1.0658e-14 written with three
digits), ``hypotheses`` asserts that every input stays below it, and the bar is ``T_BAR`` = 16 x T_ROUTES = 1.71e-13.  (The host build
and the kernels differ from route A by at most 4e-15 on these inputs, and from each other by nothing: asserted.)
"""
import functools
import math

import numpy as np
from scipy.spatial import cKDTree

import align_reference as A
import globalreg_reference as G
import planes_reference as PR

# the parameters of the issue's prototype
THRESH = 0.03
RANSAC_ITERS = 500
CLUSTER_EPS = 0.4
MIN_SUPPORT = 40
SURVEY_MIN_SUPPORT = 100
MAX_PLANES = 32
MIN_DET = 0.5
TOL_DOT = 0.05
ANGLE_TOL = math.radians(3.0)
COS_TOL = math.cos(ANGLE_TOL)
OFFSET_TOL = 0.05
VOXEL = 0.25
EPS = 0.6 * VOXEL
N_CANDIDATES = 64
DEDUPE_ROT = math.radians(5.0)
DEDUPE_TRANS = 0.25
MARGIN = 1e-9
MARGIN_DET = 1e-6
T_ROUTES = 1.07e-14                                # the measured disagreement of the two routes: see the module docstring
T_BAR = 16 * T_ROUTES                              # 1.71e-13
SCENES = G.PLACEMENTS + ('last60',)
PARAMS = dict(min_det=MIN_DET, tol_dot=TOL_DOT, cos_tol=COS_TOL, tol_d=OFFSET_TOL)


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def det3(a, b, c):
    m0 = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
    m1 = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
    m2 = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
    return (a[..., 0] * m0 + a[..., 1] * m1) + a[..., 2] * m2


def _near(values, bar):
    """The smallest |values - bar| (inf for none; NaN values decide nothing: a comparison with NaN is false on every route)."""
    v = np.abs(np.asarray(values, dtype=np.float64) - bar).reshape(-1)
    v = v[~np.isnan(v)]
    return float(v.min()) if v.size else float('inf')


def triples(cp, min_det=MIN_DET, check=True):
    """(int32 [U,3], margin): the cloud triples a < b < c with |det| >= min_det, lexicographic."""
    cp = np.asarray(cp, dtype=np.float64)
    P = len(cp)
    a, b, c = np.meshgrid(np.arange(P), np.arange(P), np.arange(P), indexing='ij')
    sel = (a < b) & (b < c)
    a, b, c = a[sel], b[sel], c[sel]                # C order of the mask: lexicographic
    with np.errstate(invalid='ignore'):
        d = np.abs(det3(cp[a, :3], cp[b, :3], cp[c, :3]))
        margin = _near(d, min_det)
        keep = d >= min_det
    if check:
        assert margin >= MARGIN, 'a cloud triple is decided by %.3g' % margin
    return np.stack([a[keep], b[keep], c[keep]], axis=1).astype(np.int32), margin


SIGNS = np.array([[1.0 if not (s >> b) & 1 else -1.0 for b in range(3)] for s in range(8)])      # [8, 3]: sigma_a, sigma_b, sigma_c


def decode(h, ps):
    h = np.asarray(h, dtype=np.int64)
    s, r = h & 7, h >> 3
    k, r = r % ps, r // ps
    j, r = r % ps, r // ps
    return r // ps, r % ps, j, k, s


def fit_svd(n, m, b):
    """Route A: R [V,3,3] the proper rotation with R n_t ~ m_t (n, m [V,3,3]: rows t), t [V,3] with m_t . t = b_t by LU."""
    H = np.einsum('vti,vtj->vij', m, n)             # sum m_t n_t^T
    U, _, Vt = np.linalg.svd(H)
    d = np.where(np.linalg.det(U) * np.linalg.det(Vt) >= 0.0, 1.0, -1.0)
    Us = U.copy()
    Us[:, :, 2] *= d[:, None]
    return Us @ Vt, np.linalg.solve(m, b[..., None])[..., 0]


def fit_horn(n, m, b):
    """Route B: Horn's matrix of C = sum n_t m_t^T, numpy.linalg.eigh, the quaternion's matrix; t by Cramer's rule."""
    C = np.einsum('vti,vtj->vij', n, m)
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (C[:, i, j] for i in range(3) for j in range(3))
    N = np.stack([np.stack([xx + yy + zz, yz - zy, zx - xz, xy - yx], -1), np.stack([yz - zy, xx - yy - zz, xy + yx, zx + xz], -1),
                  np.stack([zx - xz, xy + yx, yy - xx - zz, yz + zy], -1), np.stack([xy - yx, zx + xz, yz + zy, zz - xx - yy], -1)], -2)
    _, V = np.linalg.eigh(N)
    q = V[:, :, -1]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    c0, c1, c2 = m[:, :, 0], m[:, :, 1], m[:, :, 2]
    D = det3(c0, c1, c2)
    t = np.stack([det3(b, c1, c2), det3(c0, b, c2), det3(c0, c1, b)], -1) / D[:, None]
    return R, t


def rigid_stack(R, t):
    T = np.zeros((len(R), 4, 4))
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1.0
    return T


def score(T, cp, cs, sp, cos_tol=COS_TOL, tol_d=OFFSET_TOL, check=True, chunk=20000):
    """(score int64 [V], margins (cos, offset))."""
    cp, sp, cs = np.asarray(cp, dtype=np.float64), np.asarray(sp, dtype=np.float64), np.asarray(cs, dtype=np.int64)
    out, mc, mo = np.zeros(len(T), np.int64), float('inf'), float('inf')
    for a in range(0, len(T), chunk):
        R, t = T[a:a + chunk, :3, :3], T[a:a + chunk, :3, 3]
        with np.errstate(invalid='ignore'):
            n1 = np.einsum('vij,qj->vqi', R, cp[:, :3])
            d1 = cp[None, :, 3] - np.einsum('vqi,vi->vq', n1, t)
            c = np.einsum('vqi,ri->vqr', n1, sp[:, :3])
            first = np.abs(c) >= cos_tol
            off = np.abs(np.where(c >= 0.0, 1.0, -1.0) * d1[:, :, None] - sp[None, None, :, 3])
            agree = first & (off <= tol_d)
        mc, mo = min(mc, _near(np.abs(c), cos_tol)), min(mo, _near(off[first], tol_d))
        out[a:a + chunk] = (agree.any(axis=2) * cs[None, :]).sum(axis=1)
    if check:
        assert mc >= MARGIN and mo >= MARGIN, 'a plane agreement is decided by %.3g (cosine) / %.3g m (offset)' % (mc, mo)
    return out, (mc, mo)


def hypotheses(cp, cs, sp, min_det=MIN_DET, tol_dot=TOL_DOT, cos_tol=COS_TOL, tol_d=OFFSET_TOL, h_begin=0, h_end=None, check=True,
               tri=None):
    """dict(tri, h int64 [V] ascending, T [V,4,4] (route A), score int64 [V], routes (the largest |route A - route B| entry), margins,
    n_enumerated) of the hypotheses h_begin <= h < h_end (default: all of them)."""
    cp, sp = np.ascontiguousarray(cp, dtype=np.float64), np.ascontiguousarray(sp, dtype=np.float64)
    pc, ps = len(cp), len(sp)
    margins = {}
    if tri is None:
        tri, margins['triple'] = triples(cp, min_det, check)
    U = len(tri)
    total = U * ps ** 3 * 8
    h_end = total if h_end is None else h_end
    assert 0 <= h_begin <= h_end <= total
    n, m = cp[:, :3], sp[:, :3]
    with np.errstate(invalid='ignore'):
        mm = dot3(m[:, None, :], m[None, :, :])
        detm = det3(m[:, None, None, :], m[None, :, None, :], m[None, None, :, :])
        ii, jj, kk = np.meshgrid(np.arange(ps), np.arange(ps), np.arange(ps), indexing='ij')
        rule1 = (ii != jj) & (ii != kk) & (jj != kk)
        margins['rule2'] = _near(np.abs(detm[rule1]), min_det)
        pass2 = rule1 & (np.abs(detm) >= min_det)                   # [ps, ps, ps]
    sa, sb, sc = SIGNS[:, 0], SIGNS[:, 1], SIGNS[:, 2]
    m3, m4 = float('inf'), float('inf')
    hs = []
    per_u = ps ** 3 * 8
    for u in range(h_begin // per_u if per_u else 0, -(-h_end // per_u) if h_end > h_begin else 0):
        a, b, c = tri[u]
        with np.errstate(invalid='ignore'):
            nab, nac, nbc = dot3(n[a], n[b]), dot3(n[a], n[c]), dot3(n[b], n[c])
            detn = ((sa * sb) * sc) * det3(n[a], n[b], n[c])        # [8]
            e1 = np.abs((sa * sb)[None, None, None, :] * nab - mm[:, :, None, None])            # [ps, ps, 1, 8]
            e2 = np.abs((sa * sc)[None, None, None, :] * nac - mm[:, None, :, None])            # [ps, 1, ps, 8]
            e3 = np.abs((sb * sc)[None, None, None, :] * nbc - mm[None, :, :, None])            # [1, ps, ps, 8]
            r0 = np.broadcast_to(pass2[..., None], (ps, ps, ps, 8))
            r1 = r0 & (e1 <= tol_dot)
            r2 = r1 & (e2 <= tol_dot)
            r3 = r2 & (e3 <= tol_dot)
            prod = detn[None, None, None, :] * detm[..., None]
            ok = r3 & (prod > 0.0)
        hh = (u * per_u + np.arange(per_u, dtype=np.int64)).reshape(ps, ps, ps, 8)
        inr = (hh >= h_begin) & (hh < h_end)
        for reached, e in ((r0, e1), (r1, e2), (r2, e3)):
            m3 = min(m3, _near(np.broadcast_to(e, (ps, ps, ps, 8))[reached & inr], tol_dot))
        m4 = min(m4, _near(np.abs(prod[r3 & inr]), 0.0))
        hs.append(hh[ok & inr])
    margins['rule3'], margins['rule4'] = m3, m4
    h = np.concatenate(hs) if hs else np.zeros(0, np.int64)         # C order within u, u ascending: ascending h
    if check:
        assert margins['rule2'] >= MARGIN and m3 >= MARGIN, 'rules 2 / 3 are decided by %.3g / %.3g' % (margins['rule2'], m3)
        assert m4 >= MARGIN_DET, 'rule 4 is decided by %.3g' % m4
    u, i, j, k, s = decode(h, ps)
    sg = SIGNS[s]                                                   # [V, 3]
    rows = np.stack([tri[u, 0], tri[u, 1], tri[u, 2]], axis=1) if len(h) else np.zeros((0, 3), np.int64)
    nn = cp[rows, :3] * sg[:, :, None]
    ms = sp[np.stack([i, j, k], axis=1)] if len(h) else np.zeros((0, 3, 4))
    bb = sg * cp[rows, 3] - ms[:, :, 3]
    if len(h):
        Ra, ta = fit_svd(nn, ms[:, :, :3], bb)
        Rb, tb = fit_horn(nn, ms[:, :, :3], bb)
        Ta, Tb = rigid_stack(Ra, ta), rigid_stack(Rb, tb)
    else:
        Ta = Tb = np.zeros((0, 4, 4))
    fin = np.isfinite(Ta).all(axis=(1, 2))
    h, Ta, Tb = h[fin], Ta[fin], Tb[fin]
    routes = float(np.abs(Ta - Tb).max()) if len(h) else 0.0
    if check:
        assert routes <= T_ROUTES, 'the two routes differ by %.3g > %.3g' % (routes, T_ROUTES)
    sc_, (margins['cos'], margins['offset']) = score(Ta, cp, cs, sp, cos_tol, tol_d, check)
    return dict(tri=tri, h=h, T=Ta, T_horn=Tb, score=sc_, routes=routes, margins=margins, n_enumerated=h_end - h_begin)


def rotation_angles(R, R0):
    """Angle of R_v R0^T for R [V,3,3] by atan2(|axial vector|, (trace - 1) / 2)."""
    D = R @ R0.T
    v = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    return np.arctan2(np.linalg.norm(v, axis=1), 0.5 * (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - 1.0))


def select(h, sc, T, centre, M=N_CANDIDATES, rot=DEDUPE_ROT, trans=DEDUPE_TRANS, check=True):
    """(rows int64 [M'] into h in the order they are kept, ties, margins (rot, trans)): the greedy suppression over the valid
    hypotheses (h ascending), key (score descending, h ascending)."""
    order = np.lexsort((h, -sc.astype(np.int64)))
    for a, b in zip(order[:-1][:4 * M], order[1:][:4 * M]):
        assert sc[a] > sc[b] or (sc[a] == sc[b] and h[a] < h[b])
    alive = np.ones(len(h), dtype=bool)
    img = T[:, :3, :3] @ np.asarray(centre, dtype=np.float64) + T[:, :3, 3]
    kept, mr, mt = [], float('inf'), float('inf')
    pos = 0
    while len(kept) < M:
        while pos < len(order) and not alive[order[pos]]:
            pos += 1
        if pos == len(order):
            break
        r = order[pos]
        kept.append(r)
        live = np.flatnonzero(alive)
        ang = rotation_angles(T[live, :3, :3], T[r, :3, :3])
        dist = np.linalg.norm(img[live] - img[r], axis=1)
        mr, mt = min(mr, _near(ang, rot)), min(mt, _near(dist, trans))
        alive[live[(ang <= rot) & (dist <= trans)]] = False
        alive[r] = False
    if check:
        assert mr >= MARGIN and mt >= MARGIN, 'a suppression is decided by %.3g rad / %.3g m' % (mr, mt)
    kept = np.array(kept, dtype=np.int64)
    ties = int((np.diff(sc[kept]) == 0).sum())
    return kept, ties, (mr, mt)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """A scene of globalreg_reference.placement's layout; 'last60': the rows of the 'half_turn_z' cloud whose true position has
    x > 40 % of the room's length."""
    if name != 'last60':
        return G.placement(name)
    sc = dict(G.placement('half_turn_z'))
    q = sc['query'][A.move(sc['T_true'], sc['query'])[:, 0] > 0.4 * A.ROOM[0]]
    q = np.ascontiguousarray(q)
    q.setflags(write=False)
    sc.update(query=q, name=name)
    sc.pop('query_normals', None)
    return sc


def fit_planes(x, min_support):
    """(params [P,4], support int64 [P]) by planes_reference.fit_planes_restated with the prototype's parameters; border == 0 asserted."""
    params, indices, trace = PR.fit_planes_restated(x, THRESH, min_support=min_support, max_iterations=RANSAC_ITERS, max_models=MAX_PLANES,
                                                    eps=CLUSTER_EPS, seed=0)
    assert trace['border'] == 0, '%d inlier decisions of the plane fit lie within 1e-9 of the threshold' % trace['border']
    return np.array(params, dtype=np.float64).reshape(-1, 4), np.array([len(i) for i in indices], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def survey_planes():
    return fit_planes(A.survey()[0], SURVEY_MIN_SUPPORT)


@functools.lru_cache(maxsize=None)
def cloud_planes(name):
    return fit_planes(scene(name)['query'], MIN_SUPPORT)


@functools.lru_cache(maxsize=None)
def _survey_tree():
    return cKDTree(A.survey()[0])


def coarse_from_planes(sc, cp, cs, sp, M=N_CANDIDATES, check=True):
    """The stages after the plane fits: dict(T, hypothesis, score, fitness, runner_up, candidates [M',3], n_valid, n_triples,
    n_enumerated, n_points, error, hyp, rows, ties, margins, status)."""
    if len(cp) < 3 or len(sp) < 3:
        return dict(status='too_few_planes', T=np.eye(4), n_valid=0)
    hy = hypotheses(cp, cs, sp, check=check)
    if len(hy['tri']) == 0:
        return dict(status='too_few_planes', T=np.eye(4), n_valid=0, hyp=hy)
    q = sc['query']
    centre = 0.5 * (q.min(axis=0) + q.max(axis=0))
    rows, ties, (mr, mt) = select(hy['h'], hy['score'], hy['T'], centre, M, check=check)
    fp = q[G.voxel_filter(q, VOXEL)]
    fit, mf = [], float('inf')
    for r in rows:
        f, mg = G.fitness(_survey_tree(), hy['T'][r], fp, EPS, check=check)
        fit.append(f)
        mf = min(mf, mg)
    fit = np.array(fit, dtype=np.int64)
    out = dict(hyp=hy, rows=rows, n_valid=len(hy['h']), n_triples=len(hy['tri']), n_enumerated=hy['n_enumerated'], n_points=len(fp),
               margins=dict(hy['margins'], dedupe_rot=mr, dedupe_trans=mt, fitness=mf), ties=ties, centre=centre)
    if len(rows) == 0:
        out.update(status='no_hypothesis', T=np.eye(4))
        return out
    best = int(np.argmax(fit))                      # the first of the largest: ties go to the earlier candidate
    others = np.delete(fit, best)
    T = hy['T'][rows[best]]
    out.update(T=T, hypothesis=int(hy['h'][rows[best]]), score=int(hy['score'][rows[best]]), fitness=int(fit[best]),
               runner_up=int(others.max()) if len(others) else 0, fitness_ties=int((fit == fit[best]).sum()) - 1,
               candidates=np.stack([hy['h'][rows], hy['score'][rows], fit], axis=1), error=G.point_error(T, sc),
               status='ok' if fit[best] >= 0.5 * len(fp) else 'low_fitness')
    return out


@functools.lru_cache(maxsize=None)
def coarse(name, M=N_CANDIDATES):
    """The whole coarse stage of a scene on the oracle's own planes."""
    cp, cs = cloud_planes(name)
    sp, _ = survey_planes()
    return coarse_from_planes(scene(name), cp, cs, sp, M)


# ---- designed inputs ----------------------------------------------------------------------------------------------------------------
def random_planes(pc, ps, seed, noise=1e-3):
    """(cp [pc,4], cs [pc], sp [ps,4], T_true): survey plane r has the normal of axis r mod 3 of a random frame, jittered by 0.35 (so
    that three planes of three axes are independent and no two dot products agree by design), and a random offset; cloud plane q is
    survey plane q mod ps moved by the inverse of a rigid motion, with a random sign and ``noise`` on its normal."""
    rng = np.random.default_rng(1000 + 97 * pc + ps + seed)
    m = (np.eye(3)[np.arange(ps) % 3] + 0.35 * rng.normal(size=(ps, 3))) @ A.axis_angle(rng.normal(size=3), 0.9).T
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    sp = np.concatenate([m, rng.uniform(-5, 5, (ps, 1))], axis=1)
    R, t = A.axis_angle(rng.normal(size=3), 2.1), rng.uniform(-3, 3, 3)
    cp = np.zeros((pc, 4))
    for q in range(pc):
        r = q % ps
        n = R.T @ sp[r, :3] + rng.normal(0, noise, 3)
        n /= np.linalg.norm(n)
        sg = rng.choice([-1.0, 1.0])
        cp[q] = np.concatenate([sg * n, [sg * (sp[r, 3] + sp[r, :3] @ t)]])           # the plane m.(R x + t) + e = 0 in the cloud frame
    cs = rng.integers(40, 4000, pc).astype(np.int64)
    return np.ascontiguousarray(cp), cs, np.ascontiguousarray(sp), A.rigid(R, t)


def box_planes():
    """The six faces of the box 0 <= x <= 4, 0 <= y <= 3, 0 <= z <= 2.5 on both sides (Pc = Ps = 6): every dot product is 0 or +-1."""
    sp = np.array([[1.0, 0, 0, 0], [1.0, 0, 0, -4.0], [0, 1.0, 0, 0], [0, 1.0, 0, -3.0], [0, 0, 1.0, 0], [0, 0, 1.0, -2.5]])
    return sp.copy(), np.array([300, 310, 400, 410, 500, 510], dtype=np.int64), sp.copy()
