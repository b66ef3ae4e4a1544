"""Designed eigenvalue spectra and synthetic neighbourhoods that realise them (plain numpy, no GPU).

The eigen-solvers of csrc/dc_eig3.h change behaviour with half = det(B) / (2 p^3) = cos(3 ang) of the scaled spectrum: the sign
of half picks the eigenvalue eig3_sym / eig3_sym_v2 isolate, half >= 0.9 sends eig3_smallest_r2 to its deflation path and
eig3_smallest_unit to a second Newton step, half >= 0.999 sends eig3_smallest_unit to its deflation path.  The families below put
spectra on every side of those switches; test_hostcheck.py feeds them to the host build as covariance matrices, the GPU tests
(test_gpu_eig_spectra.py) as neighbourhoods of points whose covariance has the spectrum."""
import numpy as np

# spectra of unit scale (largest eigenvalue <= ~1.3) and the two that test the scaling of the solvers
UNIT_FAMILIES = ('generic', 'planar', 'needle', 'double_lo', 'double_hi', 'isotropic', 'near_isotropic', 'edge', 'sign_switch',
                 'threshold', 'threshold_unit')
SCALE_FAMILIES = ('tiny', 'huge')
FAMILIES = UNIT_FAMILIES + SCALE_FAMILIES
# the cycle of 'mixed': a wavefront is 64 centres = 6.4 groups of ten, and the first six families of the cycle put it on every
# branch at once (det(B) ~ 0, > 0, < 0; direct path, second Newton step, deflation)
MIXED_CYCLE = ('sign_switch', 'needle', 'threshold_unit', 'double_hi', 'threshold', 'planar', 'generic', 'double_lo', 'isotropic',
               'near_isotropic', 'edge', 'tiny', 'huge')

G, K = 77, 10           # 770 centres: three full blocks of 256 and a partial one, 13 wavefronts with group boundaries inside them
SEQ_SCALE = 0.05        # sequence form: the coordinates are scaled by this (see sequence_cloud)


def family_lams(case, n, rng, scales=True):
    """[n, 3] eigenvalues, ascending, of the family `case`.  'mixed': row i belongs to family MIXED_CYCLE[i mod 13], so that
    consecutive neighbourhoods -- the lanes of one wavefront -- sit on different branches of the solvers (scales=False leaves
    'tiny' and 'huge' out of the cycle: clouds that must fit one fixed-point format)."""
    u = rng.uniform
    if case == 'mixed':
        fams = MIXED_CYCLE if scales else MIXED_CYCLE[:-2]
        per = -(-n // len(fams))
        parts = np.stack([family_lams(f, per, rng) for f in fams], 1)         # [per, F, 3]: cycling through the families
        return parts.reshape(-1, 3)[:n]
    if case in ('threshold', 'threshold_unit'):
        # scaled spectra 2 cos(ang + 2 pi k / 3) with cos(3 ang) swept across the switch at 0.9 (eig3_smallest_r2: deflation;
        # eig3_smallest_unit: second Newton step) and across 0.999 (eig3_smallest_unit: deflation)
        ang = np.arccos(u(0.85, 0.95, n) if case == 'threshold' else u(0.99, 0.99999, n)) / 3
        beta = np.stack([2 * np.cos(ang + 2 * np.pi / 3), 2 * np.cos(ang - 2 * np.pi / 3), 2 * np.cos(ang)], 1)
        lams = 1.0 + 0.3 * beta
    elif case == 'generic':
        lams = u(0, 1, (n, 3))
    elif case == 'planar':
        lams = np.stack([10 ** u(-10, -3, n), u(0.3, 1, n), u(0.3, 1, n)], 1)
    elif case == 'needle':
        lams = np.stack([10 ** u(-10, -4, n), 10 ** u(-10, -4, n), u(0.3, 1, n)], 1)
    elif case == 'double_lo':
        lams = np.stack([np.full(n, 0.2), np.full(n, 0.2), u(0.3, 1, n)], 1)
    elif case == 'double_hi':
        lams = np.stack([u(0.01, 0.2, n), np.full(n, 0.5), np.full(n, 0.5)], 1)
    elif case == 'isotropic':
        lams = np.full((n, 3), 0.37)
    elif case == 'near_isotropic':
        # anisotropy from round-off level up to 1e-6 of the scale
        lams = 0.37 * (1.0 + 10 ** u(-16, -6, (n, 1)) * u(-1, 1, (n, 3)))
    elif case == 'edge':
        lams = np.stack([10 ** u(-8, -3, n), 10 ** u(-3, -0.5, n), u(0.3, 1, n)], 1)
    elif case == 'sign_switch':
        # symmetric about the middle one: det(B) ~ 0, on either side of the switch of the eigenvalue eig3_sym / _v2 isolate
        lo = 0.5 - u(0.1, 0.4, n)
        lams = np.stack([lo, 0.5 + u(-1e-7, 1e-7, n), 1.0 - lo], 1)
    elif case == 'tiny':
        lams = u(0, 1, (n, 3)) * 1e-14
    elif case == 'huge':
        lams = u(0, 1, (n, 3)) * 1e12
    else:
        raise KeyError(case)
    return np.sort(lams, axis=1)


def half_of(lams):
    """cos(3 ang) of the spectra [n, 3]: the quantity the solvers branch on (NaN for an exactly isotropic spectrum)."""
    lams = np.asarray(lams, dtype=np.float64)
    b = lams - lams.mean(1, keepdims=True)
    p2 = (b * b).sum(1) / 6.0
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.clip(0.5 * b.prod(1) / (p2 * np.sqrt(p2)), -1.0, 1.0)


def spd(rng, lams):
    """Symmetric matrices Q diag(lams) Q^T for random orthogonal Q."""
    Q, _ = np.linalg.qr(rng.normal(size=(len(lams), 3, 3)))
    C = np.einsum('nij,nj,nkj->nik', Q, lams, Q)
    return 0.5 * (C + C.transpose(0, 2, 1))


def group_table(g, k):
    """Neighbour rows int32 [g k, k]: every point of a group is a centre and its row is the whole group, itself first and the others
    in cyclic order (so every lane also sums in another order)."""
    j = np.arange(k)
    rows = (j[:, None] + j[None, :]) % k                                      # [k, k], rows[i, 0] = i
    return (np.arange(g)[:, None, None] * k + rows[None]).reshape(g * k, k).astype(np.int32)


def synth_groups(lams, k, dtype, offset, rng):
    """Groups of k points whose Bessel-normalised covariance is Q diag(lams[g]) Q^T (up to round-off and the rounding to dtype):
    a random k x 3 matrix, centred, whitened with its own (k - 1)-normalised covariance, scaled by sqrt(lams), rotated, moved to a
    group centre drawn in +-offset, rounded to dtype.  Returns (points dtype [G k, 3], neighbours int32 [G k, k])."""
    lams = np.asarray(lams, dtype=np.float64)
    g = len(lams)
    a = rng.normal(size=(g, k, 3))
    a -= a.mean(1, keepdims=True)
    c = np.einsum('gki,gkj->gij', a, a) / (k - 1)
    ev, evec = np.linalg.eigh(c)
    white = np.einsum('gki,gij,gj->gkj', a, evec, 1.0 / np.sqrt(ev))           # covariance = identity
    q, _ = np.linalg.qr(rng.normal(size=(g, 3, 3)))
    x = np.einsum('gkj,gj,gij->gki', white, np.sqrt(lams), q)
    x += rng.uniform(-offset, offset, size=(g, 1, 3)) if offset else 0.0
    return np.ascontiguousarray(x.reshape(g * k, 3).astype(dtype)), group_table(g, k)


def exact_rank_groups(g, k, dtype, offset, rng, step=2.0 ** -6):
    """Groups that are exactly collinear, exactly coplanar, or k copies of one point, in turn.  Every coordinate is a multiple of
    `step` (a power of two >= 2^-9) below 64 in magnitude: exact in float32, and so is the rank deficiency."""
    x = np.zeros((g, k, 3))
    for i in range(g):
        centre = np.round(rng.uniform(-offset, offset, 3) * 16) / 16 if offset else np.zeros(3)
        d1 = rng.integers(-3, 4, 3)
        while not d1.any():
            d1 = rng.integers(-3, 4, 3)
        d2 = rng.integers(-3, 4, 3)
        while not np.cross(d1, d2).any():
            d2 = rng.integers(-3, 4, 3)
        t = rng.permutation(np.arange(-8, 9))[:k] if k <= 17 else rng.integers(-8, 9, k)        # distinct: rank one, not zero
        s = rng.integers(-8, 9, k)
        while np.all(s == s[0]) or abs(np.corrcoef(t, s)[0, 1]) > 0.999999:
            s = rng.integers(-8, 9, k)
        kind = i % 3
        if kind == 0:
            x[i] = centre + step * t[:, None] * d1
        elif kind == 1:
            x[i] = centre + step * (t[:, None] * d1 + s[:, None] * d2)
        else:
            x[i] = centre
    out = x.reshape(g * k, 3).astype(dtype)
    assert np.array_equal(out.astype(np.float64), x.reshape(g * k, 3))
    return np.ascontiguousarray(out), group_table(g, k)


def make_cloud(case, k=K, dtype=np.float64, offset=20.0, g=G, seed=0, scales=True, scale=1.0):
    """(points dtype [g k, 3], neighbours int32 [g k, k]) of one family; 'tiny' / 'huge' (and 'mixed' with them in its cycle) are
    meant for offset 0.  `scale` multiplies the coordinates' spread (the eigenvalues by its square)."""
    import zlib
    rng = np.random.default_rng([seed, k, zlib.crc32(case.encode())])
    if case == 'exact_rank':
        return exact_rank_groups(g, k, dtype, offset, rng, step=2.0 ** -6 if scale == 1.0 else 2.0 ** -9)
    lams = family_lams(case, g, rng, scales=scales) * scale ** 2
    return synth_groups(lams, k, dtype, offset, rng)


def sequence_cloud(case, dtype, k=K, g=G, seed=0, offset=8.0):
    """The same kind of cloud as one scan in the sensor frame, such that the kernels' x = vps + depth * dirs reproduces the points
    without rounding in float32 and float64: dirs = (0, 0, 1), depth = z, vps = (x, y, 0), with the groups' centres at
    z in [1.3, 1.7] and the spread scaled by SEQ_SCALE (every group then lies inside z in [1, 2]).  Incidence angles are random
    in [0.1, 1] (they enter dL/dw only).  Returns dict(points, nbr, vps, dirs, depth, inc)."""
    x, nbr = make_cloud(case, k, np.float64, offset, g, seed, scales=False, scale=SEQ_SCALE)
    import zlib
    rng = np.random.default_rng([seed, k, zlib.crc32(case.encode()), 1])
    # the group centres' z drawn in +-offset -> [1.3, 1.7], by a shift per group that is a multiple of 2^-6 (exact_rank stays exact)
    zc = x.reshape(g, k, 3)[:, :, 2].mean(1, keepdims=True)
    z = x.reshape(g, k, 3)[:, :, 2] + np.round((1.5 + 0.2 * zc / max(offset, 1e-30) - zc) * 64) / 64
    x = x.copy()
    x[:, 2] = z.reshape(-1)
    x = np.ascontiguousarray(x.astype(dtype))
    assert x[:, 2].min() >= 1.0 and x[:, 2].max() <= 2.0
    n = len(x)
    vps = x.copy()
    vps[:, 2] = 0
    dirs = np.zeros_like(x)
    dirs[:, 2] = 1
    inc = rng.uniform(0.1, 1.0, size=(n, 1)).astype(dtype)
    return dict(points=x, nbr=nbr, vps=vps, dirs=dirs, depth=np.ascontiguousarray(x[:, 2:3]), inc=inc)
