"""The exact reference of the eigen-solver tests: mean, Bessel covariance, the three eigenvalues, the unit eigenvector of the
smallest one and the pointwise losses of a neighbourhood, computed with mpmath at 60 digits from the points exactly as a kernel
receives them (float32 or float64 values, read exactly), then rounded to float64 once.

The clouds of eig_cases.py give every point of a group the whole group as its neighbourhood, so the reference is computed once
per group and repeated for its k centres."""
import numpy as np
from mpmath import mp, mpf, matrix

import eig_cases as cases

DIGITS = 60
# the loss variants of test_gpu_kernels.VARIANTS: (tag, loss, normalization, sqrt)
VARIANTS = [('mineig_norm', 'min_eigval_loss', True, False), ('mineig_raw', 'min_eigval_loss', False, False),
            ('mineig_norm_sqrt', 'min_eigval_loss', True, True), ('mineig_raw_sqrt', 'min_eigval_loss', False, True),
            ('trace', 'trace_loss', False, False), ('trace_sqrt', 'trace_loss', False, True)]


def _loss(lam, tr, loss, norm, sqrt):
    """loss.py:250-289 / 330-363: min eigenvalue (divided by the trace clamped at 1e-6 when normalised) or trace; relu; sqrt."""
    if loss == 'min_eigval_loss':
        v = lam[0] / max(tr, mpf('1e-6')) if norm else lam[0]
    else:
        v = tr
    v = max(v, mpf(0))
    return mp.sqrt(v) if sqrt else v


def group_reference(pts):
    """pts [k, 3] float32 / float64 -> dict of float64 arrays: mean [3], cov [3, 3], lam [3] ascending, v0 [3], and one scalar per
    variant tag."""
    with mp.workdps(DIGITS):
        k = len(pts)
        x = [[mpf(float(v)) for v in p] for p in pts]                      # float -> mpf is exact
        mean = [sum(p[a] for p in x) / k for a in range(3)]
        d = [[p[a] - mean[a] for a in range(3)] for p in x]
        denom = max(mpf(k - 1), mpf('1e-6'))
        C = matrix(3, 3)
        for a in range(3):
            for b in range(3):
                C[a, b] = sum(r[a] * r[b] for r in d) / denom
        if all(C[a, b] == 0 for a in range(3) for b in range(3)):
            lam, v0 = [mpf(0)] * 3, [mpf(1), mpf(0), mpf(0)]
        else:
            E, Q = mp.eigsy(C)
            order = sorted(range(3), key=lambda i: E[i])
            lam = [E[i] for i in order]
            v0 = [Q[a, order[0]] for a in range(3)]
            nrm = mp.sqrt(sum(v * v for v in v0))
            v0 = [v / nrm for v in v0]
        tr = C[0, 0] + C[1, 1] + C[2, 2]
        out = dict(mean=np.array([float(v) for v in mean]), cov=np.array([[float(C[a, b]) for b in range(3)] for a in range(3)]),
                   lam=np.array([float(v) for v in lam]), v0=np.array([float(v) for v in v0]), tr=float(tr))
        for tag, loss, norm, sqrt in VARIANTS:
            out[tag] = float(_loss(lam, tr, loss, norm, sqrt))
    return out


def cloud_reference(points, k):
    """Reference of a cloud of eig_cases (groups of k consecutive points, every point a centre of its whole group): dict of float64
    arrays with one row per CENTRE -- mean [N, 3], cov [N, 3, 3], lam [N, 3], v0 [N, 3], tr [N] and every variant tag [N]."""
    points = np.asarray(points)
    assert points.dtype in (np.float32, np.float64) and len(points) % k == 0
    groups = [group_reference(g) for g in points.reshape(-1, k, 3)]
    return {f: np.repeat(np.stack([g[f] for g in groups]), k, axis=0) for f in groups[0]}


_cache = {}


def reference(case, dtype, k=cases.K, offset=20.0):
    """(points, neighbours, reference) of eig_cases.make_cloud(case, k, dtype, offset), computed once per process."""
    key = (case, np.dtype(dtype).name, k, float(offset))
    if key not in _cache:
        x, nbr = cases.make_cloud(case, k, dtype, offset)
        _cache[key] = (x, nbr, cloud_reference(x, k))
    return _cache[key]


def sequence(case, dtype, k=cases.K):
    """eig_cases.sequence_cloud(case, dtype, k), once per process (the reference of its points depends on the point format the
    plan chooses, so the caller computes it with cloud_reference)."""
    key = ('seq', case, np.dtype(dtype).name, k)
    if key not in _cache:
        _cache[key] = cases.sequence_cloud(case, dtype, k)
    return _cache[key]


def sequence_reference(case, dtype, points, k=cases.K):
    """cloud_reference of the points a plan materialised for sequence(case, dtype, k) (float64 [N, 3], the caller's order), cached by
    their bytes."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    key = ('seqref', case, np.dtype(dtype).name, k, hash(points.tobytes()))
    if key not in _cache:
        _cache[key] = cloud_reference(points, k)
    return _cache[key]


ALL = cases.FAMILIES + ('mixed', 'exact_rank')


def offset_of(case):
    """Distance of the group centres from the origin: 20 m, and none for the families whose scale a common offset would swamp."""
    return 0.0 if case in cases.SCALE_FAMILIES + ('mixed',) else 20.0


# ---- the checks the host and the GPU tests share --------------------------------------------------------------------------
def check_v0(v0, lam0, ref, norm_tol=None, store_ulp=0.0):
    """The eigenvector checks of test_hostcheck.py against the reference: residual * gap / lam_max < 1e-13 and
    (1 - |v0 . v_ref|) gap^2 < 1e-13 wherever gap = (lam1 - lam0) / lam_max > 1e-3.  store_ulp: the ulp of a narrower type the
    vector was stored in (every component within half of it: |dv| <= sqrt(3) / 2 ulp): the residual bound grows by
    |(C - lam0) dv| / lam_max <= |dv| < ulp, and the alignment -- of the vector normalised again, so that only the part of dv across
    v0 is left -- by |dv|^2 / 2 < ulp^2."""
    lmax = ref['lam'][:, 2]
    nrm = np.linalg.norm(v0, axis=1)
    if norm_tol is not None:
        assert np.abs(nrm - 1).max() < norm_tol, np.abs(nrm - 1).max()
    gap = np.zeros(len(lmax))
    np.divide(ref['lam'][:, 1] - ref['lam'][:, 0], lmax, out=gap, where=lmax > 0)
    sep = gap > 1e-3
    if not sep.any():
        return 0
    C = ref['cov']
    resid = np.linalg.norm(np.einsum('nij,nj->ni', C, v0) - lam0[:, None] * v0, axis=1)[sep] / lmax[sep]
    unit = v0 / nrm[:, None] if store_ulp else v0
    align = np.abs(np.einsum('ni,ni->n', unit, ref['v0']))[sep]
    assert (resid * gap[sep]).max() < 1e-13 + store_ulp, (resid * gap[sep]).max()
    assert ((1 - align) * gap[sep] ** 2).max() < 1e-13 + store_ulp ** 2, ((1 - align) * gap[sep] ** 2).max()
    return int(sep.sum())


def loss_bound(ref, norm, sqrt, loss, eps, out_ulp=0.0):
    """Bound on |l_dev - l_ref| per centre that follows from |dlam_i| <= eps lam_max for each eigenvalue:
      raw min-eigenvalue      eps lam_max
      trace                   3 eps lam_max                       (sum of three eigenvalues; or of three diagonal entries)
      normalised              l = lam0 / tc, tc = max(tr, 1e-6):  |dl| <= |dlam0| / tc + l |dtr| / tc = (1 + 3 l) eps lam_max / tc
      relu                    1-Lipschitz: no change
      sqrt                    |sqrt a - sqrt b| <= |a - b| / sqrt b  and  <= sqrt |a - b|: the smaller of the two, i.e. a relative
                              bound wherever the value is well above the tolerance
    plus out_ulp |l| for an output stored in a narrower type."""
    lmax = ref['lam'][:, 2]
    if loss == 'trace_loss':
        tol, val = 3 * eps * lmax, ref['tr']
    elif norm:
        tc = np.maximum(ref['tr'], 1e-6)
        val = np.maximum(ref['lam'][:, 0], 0) / tc
        tol = (1 + 3 * val) * eps * lmax / tc
    else:
        tol, val = eps * lmax, np.maximum(ref['lam'][:, 0], 0)
    if sqrt:
        s = np.sqrt(val)
        with np.errstate(divide='ignore', invalid='ignore'):
            tol = np.minimum(np.where(s > 0, tol / np.where(s > 0, s, 1.0), np.inf), np.sqrt(tol))
        val = s
    return tol + out_ulp * np.abs(val)
