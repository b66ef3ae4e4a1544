"""An independent, high-precision restatement of the plane neighbourhoods (test infrastructure; shares no code with
csrc/dc_planemath.h): written from the specification in csrc/dc_planes.hip's header comment and DESIGN.md "Plane neighbourhoods".

  hypothesis plane + degeneracy rule, exact residuals, two-pass refit      mpmath, 50 digits
  DBSCAN                                                                    scipy connected components, smallest-index labels
  the fit_planes loop                                                       numpy float64 on ransac_sample, with the margins of its decisions
  plane features, every model kind                                          float64 torch expressions (autograd) and mpmath
"""
import mpmath as mp
import numpy as np
import torch

DPS = 50
KIND_CODES = {None: 0, 'Polynomial': 1, 'ScaledPolynomial': 2, 'Linear': 3, 'InvCos': 4, 'ScaledInvCos': 5}
OFFSET = np.array([4e5, 5e6, 300.0])          # the project's far-from-the-origin scene (UTM-sized coordinates)


def _v(x):
    return [mp.mpf(float(c)) for c in x]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


# ---- RANSAC ---------------------------------------------------------------------------------------------------------------------
def hyp_plane(p0, p1, p2, distinct=True):
    """(n [3], d) as mpf of the plane through three float64 points, or None for a degenerate hypothesis."""
    with mp.workdps(DPS):
        p0, p1, p2 = _v(p0), _v(p1), _v(p2)
        u, v = [b - a for a, b in zip(p0, p1)], [b - a for a, b in zip(p0, p2)]
        c = _cross(u, v)
        nc, nu, nv = mp.sqrt(_dot(c, c)), mp.sqrt(_dot(u, u)), mp.sqrt(_dot(v, v))
        if not distinct or not nc > mp.mpf(10) ** -12 * nu * nv:
            return None
        n = [ci / nc for ci in c]
        return n, -_dot(n, p0)


def exact_residuals(pl, x, thresh):
    """|n . x + d| - thresh for the float64 plane pl [4] and every row of x [n,3], as floats rounded from 50 digits: <= 0 is an
    inlier.  (The inputs are binary fractions, so the value is exact before the final rounding.)"""
    out = np.empty(len(x))
    with mp.workdps(DPS):
        n, d, t = _v(pl[:3]), mp.mpf(float(pl[3])), mp.mpf(float(thresh))
        for i, row in enumerate(np.asarray(x, dtype=np.float64)):
            if not np.all(np.isfinite(row)) or not np.isfinite(float(pl[3])):
                out[i] = np.inf
                continue
            out[i] = float(abs(_dot(n, _v(row)) + d) - t)
    return out


def refit_two_pass(pts):
    """The least-squares plane of pts [k,3] at 50 digits: centroid, covariance of the centred points, eigenvector of the smallest
    eigenvalue with its largest-magnitude component positive, d = -n . centroid -> float64 [4]."""
    with mp.workdps(DPS):
        P = [_v(r) for r in np.asarray(pts, dtype=np.float64)]
        k = len(P)
        cen = [sum(r[a] for r in P) / k for a in range(3)]
        C = mp.zeros(3, 3)
        for r in P:
            dlt = [r[a] - cen[a] for a in range(3)]
            for a in range(3):
                for b in range(3):
                    C[a, b] += dlt[a] * dlt[b]
        lam, V = mp.eigsy(C / k)
        j = min(range(3), key=lambda q: lam[q])
        n = [V[a, j] for a in range(3)]
        kmax = max(range(3), key=lambda a: abs(n[a]))
        if n[kmax] < 0:
            n = [-c for c in n]
        nn = mp.sqrt(_dot(n, n))
        n = [c / nn for c in n]
        return np.array([float(c) for c in n] + [float(-_dot(n, cen))])


def refit_numpy(pts):
    """numpy's own float64 two-pass refit (the yardstick for the refit's error bound)."""
    pts = np.asarray(pts, dtype=np.float64)
    cen = pts.mean(0)
    q = pts - cen
    lam, V = np.linalg.eigh(q.T @ q / len(pts))
    n = V[:, 0]
    if n[np.argmax(np.abs(n))] < 0:
        n = -n
    return np.concatenate([n, [-(n @ cen)]])


def params_error(a, b, scale):
    """|n_a - n_b| and |d_a - d_b| / scale as one figure (scale: the size of the coordinates, at least 1)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return max(np.abs(a[:3] - b[:3]).max(), abs(a[3] - b[3]) / max(1.0, scale))


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------------------
def neighbour_lists(x, eps):
    """Ascending neighbour lists within eps (inclusive, the point itself included): float64 (dx^2 + dy^2) + dz^2 <= eps^2.  Also the
    smallest |d^2 - eps^2| / eps^2 over the candidate pairs (0 when a pair lies exactly at eps)."""
    from scipy.spatial import cKDTree
    x = np.asarray(x, dtype=np.float64)
    cand = cKDTree(x).query_ball_point(x, eps * (1.0 + 1e-6))
    out, margin = [], np.inf
    e2 = eps * eps
    for i, c in enumerate(cand):
        c = np.sort(np.asarray(c, dtype=np.int64))
        dlt = x[c] - x[i]
        d2 = (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]
        if len(d2):
            margin = min(margin, float(np.abs(d2 - e2).min() / e2))
        out.append(c[d2 <= e2])
    return out, margin


def padded_table(nb):
    """The neighbour lists as the int32 [m, Kmax] table the kernels take (rows padded with -1 at the end)."""
    k = max(1, max(len(r) for r in nb))
    tab = np.full((len(nb), k), -1, dtype=np.int32)
    for i, r in enumerate(nb):
        tab[i, :len(r)] = r
    return tab


def dbscan_from_lists(nb, min_points):
    """(labels int [m] with -1 for noise, best label, its size): core = at least min_points neighbours (itself included), clusters =
    connected components of the core-core graph labelled by their smallest index, a non-core point takes the smallest label among
    its core neighbours, the largest cluster wins and on equal sizes the smaller label."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    m = len(nb)
    core = np.array([len(r) >= min_points for r in nb])
    rows = np.concatenate([np.full(len(r), i) for i, r in enumerate(nb)] + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    cols = np.concatenate(list(nb) + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    keep = core[rows] & core[cols]
    _, comp = connected_components(coo_matrix((np.ones(int(keep.sum())), (rows[keep], cols[keep])), shape=(m, m)), directed=False)
    first = np.full(comp.max() + 1, m)
    np.minimum.at(first, comp[core], np.flatnonzero(core))
    labels = np.full(m, -1, dtype=np.int64)
    labels[core] = first[comp[core]]
    for i in np.flatnonzero(~core):
        ls = [first[comp[j]] for j in nb[i] if core[j]]
        labels[i] = min(ls) if ls else -1
    if not (labels >= 0).any():
        return labels, -1, 0
    u, c = np.unique(labels[labels >= 0], return_counts=True)
    k = np.flatnonzero(c == c.max())[0]
    return labels, int(u[k]), int(c[k])


def dbscan(x, eps, min_points=10):
    nb, _ = neighbour_lists(x, eps)
    return dbscan_from_lists(nb, min_points)


# ---- the fit_planes loop ---------------------------------------------------------------------------------------------------------
def _np_plane(p0, p1, p2):
    u, v = p1 - p0, p2 - p0
    c = np.cross(u, v)
    nc = np.sqrt(c @ c)
    if not nc > 1e-12 * np.sqrt(u @ u) * np.sqrt(v @ v):
        return None
    n = c / nc
    return np.concatenate([n, [-(n @ p0)]])


def ransac_round_numpy(x, rem, seed, m, H, thresh):
    """(planes [H,4] with d = inf for a degenerate hypothesis, valid [H], counts [H] with -1, best h, best count, residuals
    [n_rem, H]) of round m in numpy float64."""
    from depth_correction_amd.segmentation import ransac_sample
    xr = x[rem]
    planes, valid = np.zeros((H, 4)), np.zeros(H, dtype=bool)
    planes[:, 3] = np.inf
    for h in range(H):
        j = ransac_sample(seed, m, h, len(rem))
        pl = _np_plane(*xr[list(j)]) if len(set(j)) == 3 else None
        if pl is not None:
            planes[h], valid[h] = pl, True
    with np.errstate(invalid='ignore'):
        r = np.abs(xr @ planes[:, :3].T + planes[:, 3])
    r[:, ~valid] = np.inf
    r[~np.isfinite(r)] = np.inf
    counts = np.where(valid, (r <= thresh).sum(0), -1)
    h = int(np.argmax(counts))                    # the first of the largest: ties go to the lowest h
    return planes, valid, counts, h, int(counts[h]), r


def fit_planes_restated(x, thresh, min_support=3, max_iterations=1000, max_models=10, eps=None, seed=0, min_points=10):
    """The whole loop of segmentation.fit_planes in numpy float64.  Returns (params list, indices list, trace): trace['rounds'] holds
    one dict per RANSAC call (round number passed to the sampler, n_remaining, winner, count, what happened), trace['border'] the
    number of inlier decisions whose |r| lay within 1e-9 of the threshold (0: every decision is safe against rounding)."""
    x = np.asarray(x, dtype=np.float64)
    rem = np.arange(len(x))
    params, indices = [], []
    trace = dict(rounds=[], border=0)
    m = 0
    while len(rem) >= 3:
        _, _, _, h, count, r = ransac_round_numpy(x, rem, seed, m, max_iterations, thresh)
        trace['border'] += int((np.abs(r[np.isfinite(r)] - thresh) < 1e-9).sum())
        rec = dict(round=m, n_rem=len(rem), h=h, count=count, what='plane')
        trace['rounds'].append(rec)
        m += 1
        if count < min_support:
            rec['what'] = 'halt: support'
            break
        xr = x[rem]
        plane = refit_numpy(xr[r[:, h] <= thresh])
        r2 = np.abs(xr @ plane[:3] + plane[3])
        trace['border'] += int((np.abs(r2 - thresh) < 1e-9).sum())
        mask = r2 <= thresh
        support = rem[mask]
        if len(support) < min_support:
            rec['what'] = 'halt: refit support'
            break
        keep = support
        if eps:
            labels, lbl, size = dbscan(x[support], eps, min_points)
            if size < min_support:
                rec['what'] = 'support removed'
                rem = rem[~mask]
                if len(rem) < min_support:
                    break
                continue
            keep = support[labels == lbl]
        params.append(plane)
        indices.append(keep)
        if max_models is not None and len(params) == max_models:
            rec['what'] = 'plane, halt: max_models'
            break
        rem = rem[~np.isin(rem, keep)]
        if len(rem) < min_support:
            break
    return params, indices, trace


# ---- plane features --------------------------------------------------------------------------------------------------------------
def model_torch(kind, d, g, w, e):
    """d'(d, gamma) of every model kind as a float64 torch expression; w [P], e [P] tensors."""
    if kind is None:
        return d
    if kind in ('Polynomial', 'ScaledPolynomial'):
        b = (torch.pow(g.unsqueeze(-1), e) * w).sum(-1)
        return d - b if kind == 'Polynomial' else d * (1.0 - b)
    if kind == 'Linear':
        return w[0] * d + w[1] * g + w[2]
    if kind == 'InvCos':
        return d - w[0] / torch.cos(g)
    if kind == 'ScaledInvCos':
        return d * (1.0 - w[0] / torch.cos(g).abs())
    raise ValueError(kind)


def plane_points_torch(vps, dirs, depth, idx, normal, kind, w, e):
    """Corrected points [n,3] of one plane: gamma = arccos min(|dir . n|, 1), x = vp + d'(d, gamma) dir.  Where |dir . n| >= 1 the
    arccos has no derivative and the kernel defines d gamma / d dir = 0: gamma is a constant there (detach)."""
    dd, vv, rr = dirs[idx], vps[idx], depth.reshape(-1)[idx]
    a = (dd @ normal).abs()
    flat = a >= 1.0
    g = torch.where(flat, torch.arccos(a.detach().clamp(max=1.0)), torch.arccos(torch.where(flat, torch.full_like(a, 0.5), a)))
    return vv + model_torch(kind, rr, g, w, e).unsqueeze(-1) * dd


def plane_cov_torch(vps, dirs, depth, indices, normals, kind, w=None, e=None):
    """cov [P,3,3] (Bessel) of the corrected points of every plane, float64 torch (differentiable)."""
    return torch.stack([torch.cov(plane_points_torch(vps, dirs, depth, torch.as_tensor(i).long(), n, kind, w, e).t(), correction=1)
                        for i, n in zip(indices, normals)])


def model_mp(kind, d, g, w, e):
    """(d', dd'/dd, dd'/dg, [dd'/dw_k]) at 50 digits, analytic; d, g mpf, w / e lists of mpf.  dd'/dg is None where it is infinite
    (gamma = 0 under an exponent in (0, 1))."""
    if kind is None:
        return d, mp.mpf(1), mp.mpf(0), []
    if kind in ('Polynomial', 'ScaledPolynomial'):
        terms = [g ** ek for ek in e]
        b = sum(wk * t for wk, t in zip(w, terms))
        if g == 0 and any(0 < ek < 1 for ek in e):
            db = None
        else:
            db = sum((wk * ek * g ** (ek - 1)) for wk, ek in zip(w, e) if ek != 0)
        if kind == 'Polynomial':
            return d - b, mp.mpf(1), None if db is None else -db, [-t for t in terms]
        return d * (1 - b), 1 - b, None if db is None else -d * db, [-d * t for t in terms]
    if kind == 'Linear':
        return w[0] * d + w[1] * g + w[2], w[0], w[1], [d, g, mp.mpf(1)]
    c, s = mp.cos(g), mp.sin(g)
    if kind == 'InvCos':
        return d - w[0] / c, mp.mpf(1), -w[0] * s / c ** 2, [-1 / c]
    if kind == 'ScaledInvCos':
        return d * (1 - w[0] / abs(c)), 1 - w[0] / abs(c), -d * w[0] * s / c ** 2, [-d / abs(c)]
    raise ValueError(kind)


def plane_mp(vps, dirs, depth, idx, normal, kind, w=None, e=None, gcov=None):
    """One plane at 50 digits from the float inputs: dict(cov float64 [3,3]) and, with an upstream gradient gcov [3,3], the
    gradients g_vps / g_dirs [n,3], g_depth [n], g_w [P] as float64 (the chain rule written out: dL/dx = (G + G^T)(x - mean) / (n - 1),
    x = vp + d' dir, d gamma / d dir = -sign(c) n / sqrt(1 - c^2) and 0 where |c| >= 1)."""
    with mp.workdps(DPS):
        nrm = _v(normal)
        wm = [] if w is None else _v(np.asarray(w, dtype=np.float64).reshape(-1))
        em = [mp.mpf(0)] * len(wm) if e is None else _v(np.asarray(e, dtype=np.float64).reshape(-1))
        rows = []
        for i in np.asarray(idx).reshape(-1).tolist():
            vp, dr, d = _v(vps[i]), _v(dirs[i]), mp.mpf(float(np.asarray(depth).reshape(-1)[i]))
            c = _dot(dr, nrm)
            a = min(abs(c), mp.mpf(1))
            g = mp.acos(a)
            dp, ddp_dd, ddp_dg, dw = model_mp(kind, d, g, wm, em)
            rows.append((vp, dr, d, c, g, dp, ddp_dd, ddp_dg, dw, [vp[k] + dp * dr[k] for k in range(3)]))
        n = len(rows)
        mean = [sum(r[9][k] for r in rows) / n for k in range(3)]
        out = {}
        if n > 1:
            C = np.empty((3, 3))
            for a_ in range(3):
                for b_ in range(a_, 3):
                    C[a_, b_] = C[b_, a_] = float(sum((r[9][a_] - mean[a_]) * (r[9][b_] - mean[b_]) for r in rows) / (n - 1))
            out['cov'] = C
        if gcov is None or n < 2:
            return out
        G = [[mp.mpf(float(gcov[r][c])) for c in range(3)] for r in range(3)]
        M = [[(G[r][c] + G[c][r]) / (n - 1) for c in range(3)] for r in range(3)]
        gv, gd, gdep = np.empty((n, 3)), np.empty((n, 3)), np.empty(n)
        gw = [mp.mpf(0)] * len(wm)
        for q, (vp, dr, d, c, g, dp, ddp_dd, ddp_dg, dw, x) in enumerate(rows):
            dx = [x[k] - mean[k] for k in range(3)]
            gx = [_dot(M[k], dx) for k in range(3)]
            gdp = _dot(gx, dr)
            s2 = 1 - c * c
            gg = mp.mpf(0)
            if s2 > 0 and kind is not None and c != 0:
                gg = gdp * ddp_dg * (-mp.sign(c) / mp.sqrt(s2))
            gv[q] = [float(t) for t in gx]
            gd[q] = [float(gx[k] * dp + gg * nrm[k]) for k in range(3)]
            gdep[q] = float(gdp * ddp_dd)
            gw = [a_ + gdp * b_ for a_, b_ in zip(gw, dw)]
        out.update(g_vps=gv, g_dirs=gd, g_depth=gdep, g_w=np.array([float(t) for t in gw]))
        return out
