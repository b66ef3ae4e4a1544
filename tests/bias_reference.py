"""numpy fp64 restatement of the depth-bias evaluation (include/dc_hip.h: dc_raycast_rays, dc_bias_accumulate; DESIGN "Depth bias
against the mesh"), with no call into the package: brute-force closest hit per ray, the true incidence angle, the used-ray and bin
rules, the sums with math.fsum and the least-squares fit with numpy.linalg.lstsq on the per-ray rows."""
import math

import numpy as np

TOTALS, BIN_COLS = 5, 9
POLYNOMIAL, SCALED_POLYNOMIAL = 'Polynomial', 'ScaledPolynomial'


# ---- rays and the cast ------------------------------------------------------------------------------------------------------------
def world_rays(vps, dirs, scan_offset, poses):
    """Origins and directions in the mesh frame: ray i of scan s is cast from R_s vp_i + t_s along R_s dir_i (fp64)."""
    vps, dirs = np.asarray(vps).astype(np.float64), np.asarray(dirs).astype(np.float64)          # fp32 converts exactly
    o, d = np.zeros_like(vps), np.zeros_like(dirs)
    for s in range(len(scan_offset) - 1):
        a, b = int(scan_offset[s]), int(scan_offset[s + 1])
        R, t = poses[s][:3, :3], poses[s][:3, 3]
        o[a:b] = vps[a:b] @ R.T + t
        d[a:b] = dirs[a:b] @ R.T
    return o, d


def brute_force(verts, faces, o, d, t_min, cull, chunk=128):
    """Moeller-Trumbore in fp64 over every (ray, face) -> (face of the closest hit or -1, t or inf, second-best t): the smallest t
    wins, equal t the lower face index (stable argsort)."""
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    e1, e2 = v1 - v0, v2 - v0
    nrm = np.cross(e1, e2)
    R = d.shape[0]
    best_f = np.full(R, -1)
    best_t = np.full(R, np.inf)
    second = np.full(R, np.inf)
    for s in range(0, R, chunk):
        dd, oo = d[s:s + chunk, None, :], o[s:s + chunk, None, :]
        p = np.cross(dd, e2[None])
        det = np.einsum('rfc,fc->rf', p, e1)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = 1.0 / det
            tv = oo - v0[None]
            u = np.einsum('rfc,rfc->rf', tv, p) * inv
            q = np.cross(tv, e1[None])
            v = np.einsum('rfc,rfc->rf', dd, q) * inv
            t = np.einsum('fc,rfc->rf', e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min)
        if cull:
            ok &= np.einsum('fc,rc->rf', nrm, d[s:s + chunk]) < 0
        t = np.where(ok, t, np.inf)
        if t.shape[1] == 1:
            t = np.concatenate([t, np.full_like(t, np.inf)], axis=1)
        order = np.argsort(t, axis=1, kind='stable')[:, :2]
        rows = np.arange(t.shape[0])
        best_t[s:s + chunk] = t[rows, order[:, 0]]
        second[s:s + chunk] = t[rows, order[:, 1]]
        best_f[s:s + chunk] = np.where(np.isfinite(best_t[s:s + chunk]), order[:, 0], -1)
    return best_f, best_t, second


def incidence(verts, faces, face, d):
    """(gamma, cos gamma) of the rays d on the faces `face` (-1: NaN): arccos(min(1, |n . d| / (|n| |d|))), n = (v1 - v0) x (v2 - v0)."""
    f = np.maximum(face, 0)
    v0, v1, v2 = (verts[faces[f, k]] for k in range(3))
    n = np.cross(v1 - v0, v2 - v0)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.abs(np.einsum('rc,rc->r', n, d)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
        c = np.where(face >= 0, np.minimum(1.0, c), np.nan)
        return np.arccos(c), c


# ---- per-ray rules ------------------------------------------------------------------------------------------------------------------
def bin_position(g, n_bins):
    """gamma B / (pi / 2): its floor (clamped to B - 1) is the bin."""
    return np.asarray(g, dtype=np.float64) * n_bins / (np.pi / 2)


def bins_of(g, n_bins):
    return np.minimum(n_bins - 1, np.floor(bin_position(g, n_bins))).astype(np.int64)


def distance_to_bin_edge(g, n_bins):
    """Smallest distance of gamma B / (pi / 2) from an integer over the finite angles: a bin must not hang on arccos' last bit."""
    q = bin_position(np.asarray(g)[np.isfinite(g)], n_bins)
    return float(np.abs(q - np.round(q)).min()) if q.size else np.inf


def ray_flags(depth, mask, face, t, g, max_residual=None):
    """(masked in, hit, used, beyond the gate) per ray."""
    depth = np.asarray(depth).astype(np.float64).reshape(-1)
    n = depth.size
    in_mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    hit = in_mask & (np.asarray(face) >= 0) & np.isfinite(t) & np.isfinite(g)
    cand = hit & (depth > 0) & np.isfinite(depth)
    with np.errstate(invalid='ignore'):
        r = depth - t
        inside = np.abs(r) <= max_residual if max_residual is not None and max_residual > 0 else np.ones(n, dtype=bool)
    return in_mask, hit, cand & inside, cand & ~inside


def system_len(p):
    return 2 + p + p * (p + 1) // 2


def out_count(n_bins, p):
    return TOTALS + BIN_COLS * n_bins + 2 * system_len(p)


def basis(x, exponent):
    return np.power(np.asarray(x, dtype=np.float64)[:, None], np.asarray(exponent, dtype=np.float64)[None, :])


def accumulate(depth, inc_est, mask, face, t, g, kind, exponent, n_bins, max_residual=None):
    """The `out` vector of dc_bias_accumulate with every sum taken by math.fsum -> (out, abs_sum, terms): abs_sum the sum of the
    absolute values of each entry's terms, terms their number (the error bound of a floating-point sum is stated in these)."""
    depth = np.asarray(depth).astype(np.float64).reshape(-1)
    t, g = np.asarray(t, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n, p = depth.size, len(exponent)
    in_mask, hit, used, gated = ray_flags(depth, mask, face, t, g, max_residual)
    out, ab, m = (np.zeros(out_count(n_bins, p)) for _ in range(3))

    def put(k, terms):
        terms = np.asarray(terms, dtype=np.float64)
        out[k], ab[k], m[k] = math.fsum(terms), math.fsum(np.abs(terms)), terms.size

    for k, v in enumerate((np.ones(n), in_mask, hit, used, gated)):
        put(k, np.asarray(v, dtype=np.float64)[np.asarray(v, dtype=bool)] if k else v)
    d, tt, gg = depth[used], t[used], g[used]
    r = d - tt
    rho = r / d
    if inc_est is None:
        has_est, ge = np.zeros(d.size, dtype=bool), np.zeros(d.size)
    else:
        ge = np.asarray(inc_est).astype(np.float64).reshape(-1)[used]
        has_est = np.isfinite(ge)
    delta = np.where(has_est, ge - gg, 0.0)
    b = bins_of(gg, n_bins)
    for q in range(n_bins):
        s = b == q
        cols = (np.ones(int(s.sum())), r[s], r[s] * r[s], np.abs(r[s]), rho[s], rho[s] * rho[s], delta[s], delta[s] * delta[s],
                np.ones(int((s & has_est).sum())))
        for c, terms in enumerate(cols):
            put(TOTALS + BIN_COLS * q + c, terms)
    y = rho if kind == SCALED_POLYNOMIAL else r
    for s, (x, sel) in enumerate(((gg, np.ones(d.size, dtype=bool)), (ge, has_est))):
        base = TOTALS + BIN_COLS * n_bins + s * system_len(p)
        phi, ys = basis(x[sel], exponent), y[sel]
        put(base, np.ones(ys.size))
        k = base + 1
        for a in range(p):
            for c in range(a, p):
                put(k, phi[:, a] * phi[:, c])
                k += 1
        for a in range(p):
            put(k, phi[:, a] * ys)
            k += 1
        put(k, ys * ys)
    return out, ab, m


def sum_bound(ab, m):
    """The project's bound for a floating-point total of m terms against the exact one: (m + 16) 2^-53 sum |term|."""
    return (m + 16) * 2.0 ** -53 * ab


def is_count(n_bins, p):
    """Mask of the entries of `out` that are counts (compared for equality)."""
    c = np.zeros(out_count(n_bins, p), dtype=bool)
    c[:TOTALS] = True
    for q in range(n_bins):
        c[TOTALS + BIN_COLS * q] = c[TOTALS + BIN_COLS * q + 8] = True
    for s in range(2):
        c[TOTALS + BIN_COLS * n_bins + s * system_len(p)] = True
    return c


def lstsq_fit(x, y, exponent):
    """Weights of y = sum_k w_k x^e_k by numpy.linalg.lstsq on the per-ray rows."""
    if len(x) == 0:
        return np.full(len(exponent), np.nan)
    return np.linalg.lstsq(basis(x, exponent), np.asarray(y, dtype=np.float64), rcond=None)[0]


def bin_statistics(out, n_bins):
    """Per-bin count, mean, rms, mean_abs, rel_mean, rel_rms, angle_err_mean, angle_err_rms of an `out` vector (NaN in an empty bin)."""
    rows = np.asarray(out)[TOTALS:TOTALS + BIN_COLS * n_bins].reshape(n_bins, BIN_COLS)
    n, na = rows[:, 0], rows[:, 8]
    with np.errstate(invalid='ignore', divide='ignore'):
        div = lambda a, c: np.where(c > 0, a / c, np.nan)
        return dict(count=n, mean=div(rows[:, 1], n), rms=np.sqrt(div(rows[:, 2], n)), mean_abs=div(rows[:, 3], n),
                    rel_mean=div(rows[:, 4], n), rel_rms=np.sqrt(div(rows[:, 5], n)), angle_err_mean=div(rows[:, 6], na),
                    angle_err_rms=np.sqrt(div(rows[:, 7], na)))
