"""The reference of the neighbourhood-feature tests: what dc_features_fwd and dc_features_bwd compute, from a plain high-precision
route.  Host only.

Forward: one call of eig_reference.group_reference (mpmath, 60 digits) on the valid members of each row, in row order -> mean, Bessel
covariance, eigenvalues, v0.  Everything else is exact integer or float64 arithmetic: nvalid, cmean (the validity-weighted mean),
invd = 1 / max(W - 1, 1e-6), the weights, |dir . v0| and its arccos.  With explicit mean weights the mean is the weighted one and the
covariance stays validity-weighted (dc_oracle.features(weights=...)).

Backward: the closed form the kernels implement,

    dL/dx_j = sum_{i -> j} [ (2 / D_i) (V diag(g_eig) V^T + sym(g_cov)) (x_j - cmean_i) + m_ij g_mean_i ],

with m_ij = 1 / W_i for validity weights and w_ij / sum_q w_iq for explicit mean weights, D_i = max(W_i - 1, 1e-6), V from
numpy.linalg.eigh of the reference covariance; a slot listed twice counts twice.  Rows with W <= 1 contribute nothing through the
first term (x_j - cmean = 0 exactly), a row with W = 0 nothing at all (no edge leaves it)."""
import numpy as np

import eig_reference as R
import features_cases as cases

_cache = {}


def forward(n, k, kind):
    """Reference of cases.make_case(n, k, kind), once per process: dict of float64 / integer arrays with one row per centre -- mean,
    cmean [n, 3], cov [n, 3, 3], lam [n, 3], v0 [n, 3], nvalid [n], distinct [n], invd [n], weights [n, k], absdot [n], inc [n].
    The row with W = 0 is NaN in mean, cmean, cov, lam, v0, absdot and inc."""
    key = (n, k, kind)
    if key not in _cache:
        x, dirs, tab, _ = cases.make_case(n, k, kind)
        out = dict(mean=np.full((n, 3), np.nan), cov=np.full((n, 3, 3), np.nan), lam=np.full((n, 3), np.nan), v0=np.full((n, 3), np.nan))
        for i, row in enumerate(tab):
            members = row[row >= 0]
            if len(members):
                g = R.group_reference(x[members])
                for f in out:
                    out[f][i] = g[f]
        valid = tab >= 0
        W = valid.sum(1)
        out['cmean'] = out['mean']
        out['nvalid'] = W.astype(np.int32)
        out['distinct'] = np.array([len(set(r[r >= 0].tolist())) for r in tab])
        out['invd'] = 1.0 / np.maximum(W - 1.0, 1e-6)
        out['weights'] = valid.astype(np.float64)
        out['absdot'] = np.minimum(np.abs((dirs * out['v0']).sum(1)), 1.0)
        out['inc'] = np.arccos(out['absdot'])
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def mean_weights(n, k, kind):
    """Random positive mean weights f64 [n, k] (float32 values), zero on the missing slots."""
    tab = cases.make_case(n, k, kind)[2]
    rng = np.random.default_rng(cases.make_case(n, k, kind)[3]['seed'] + 2)
    w = rng.uniform(0.25, 2.0, (n, k)).astype(np.float32).astype(np.float64)
    return np.where(tab >= 0, w, 0.0)


def weighted_mean(x, tab, w):
    """sum_q w_iq x_q / sum_q w_iq per row in float64 (NaN where the weights sum to zero)."""
    p = x[np.where(tab >= 0, tab, 0)]
    with np.errstate(divide='ignore', invalid='ignore'):
        return (w[..., None] * p).sum(1) / w.sum(1)[:, None]


def upstream(n, k, kind, which):
    """Upstream gradients (g_mean [n, 3], asymmetric g_cov [n, 3, 3], g_eig [n, 3]) as float32 values in float64; `which` names the
    ones fed ('mean', 'cov', 'eig' or 'all'), the others are None.  Rows with fewer than three distinct points have lam0 = lam1 = 0:
    g_eig[0] == g_eig[1] there, which makes the derivative well defined."""
    ref = forward(n, k, kind)
    rng = np.random.default_rng(cases.make_case(n, k, kind)[3]['seed'] + 3)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    gm, gc, ge = r32(rng.normal(size=(n, 3))), r32(rng.normal(size=(n, 3, 3))), r32(rng.normal(size=(n, 3)))
    flat = ref['distinct'] < 3
    ge[flat, 1] = ge[flat, 0]
    return (gm if which in ('mean', 'all') else None, gc if which in ('cov', 'all') else None, ge if which in ('eig', 'all') else None)


def backward(x, tab, cov, cmean, g_mean=None, g_cov=None, g_eig=None, mean_weights=None, dtype=np.float64):
    """The closed form above -> grad_points [n, 3], every operation in `dtype` (float64: the reference; float32: the yardstick of what
    the expression costs in that precision).  cov, cmean: the reference's; rows without a valid member are skipped."""
    n, k = tab.shape
    valid = tab >= 0
    W = valid.sum(1)
    live = W > 0
    T = np.dtype(dtype).type
    x, cmean = x.astype(dtype), np.where(live[:, None], cmean, 0.0).astype(dtype)
    G = np.zeros((n, 3, 3), dtype=dtype)
    if g_eig is not None:
        V = np.linalg.eigh(np.where(live[:, None, None], cov, 0.0))[1].astype(dtype)
        G += np.einsum('nak,nk,nbk->nab', V, g_eig.astype(dtype), V)
    if g_cov is not None:
        gc = g_cov.astype(dtype)
        G += T(0.5) * (gc + gc.transpose(0, 2, 1))
    coef = (T(2.0) / np.maximum(W - 1.0, 1e-6).astype(dtype))
    d = x[np.where(valid, tab, 0)] - cmean[:, None, :]
    contrib = coef[:, None, None] * np.einsum('nab,nkb->nka', G, d)
    if g_mean is not None:
        if mean_weights is None:
            m = valid.astype(dtype) / np.maximum(W, 1).astype(dtype)[:, None]
        else:
            mw = mean_weights.astype(dtype)
            m = mw / np.where(live, mw.sum(1), 1)[:, None]
        contrib = contrib + m[..., None] * g_mean.astype(dtype)[:, None, :]
    contrib = np.where(valid[..., None], contrib, T(0))
    grad = np.zeros((n, 3), dtype=dtype)
    np.add.at(grad, np.where(valid, tab, 0).reshape(-1), contrib.reshape(-1, 3))
    return grad


def gaps(ref):
    """min(lam1 - lam0, lam2 - lam1) / lam2 of the reference spectrum, inf for rows with fewer than three distinct points."""
    lam = ref['lam']
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / lam[:, 2]
    return np.where(ref['distinct'] >= 3, g, np.inf)
