"""Reference of the global registration tests (test_globalreg_host.py, test_gpu_globalreg.py): numpy and scipy's cKDTree only, a
restatement of DESIGN "Global registration" -- nothing here calls depth_correction_amd.  The closed-form fit is
``align_reference.fit_svd`` (means, cross-covariance, SVD): a route independent of the package's moments / Horn / Jacobi.

Every discrete decision the GPU tests compare is taken here with a margin, asserted on every input they use (``MARGIN_*``):
  bin edges           |B a - k| >= 1e-9 for the inner edges k = 1 .. B - 1; a = 0 and a = 1 are not edges (``bin_margin``);
  descriptor ties     the nearest survey descriptor is strictly nearer than the second one unless the two rows are equal (``match``);
  the edge check      every comparison (lp against min_edge, rho ly; ly against rho lp) is decided by >= 1e-12 m: 500 ulp of a 10 m
                      coordinate, where the three implementations differ by a few ulp (``hypotheses``);
  the degeneracy gap  gap / max|lam| of every fitted triple is >= 1e-10, a hundred times align_solve's 1e-12, or <= 1e-14;
  the inlier rule     | |T p - y| - eps | >= 1e-9 m, for the score and for the fitness (``score``, ``fitness``);
  selection           scores and fitnesses are integers and their ties are decided by stated rules (the lower h, the earlier
                      candidate), so a tie among the top M + 1 does not depend on any rounding: ``select`` counts them (``ties``) and
                      asserts that the order it returns follows the rule.

Scenes (``placement``): the room of align_reference.py, survey N_SURVEY = 20 000 points; the cloud an independent N_CLOUD-point
sample (seed SEED + 1) with SIGMA noise and normals of random sign, moved by the inverse of the true transform: 140 deg about
(0.3, -0.2, 1), 180 deg about z, 75 deg about (1, 0.5, -0.3), and two partial clouds (the first 60 % of the room's length under the
first rotation, its middle 60 % under the third), each with a translation of a few metres.

What was tried on the CPU (SEED = 135, N_CLOUD = 8000, the first and only seeds; voxel 0.25 m, 63 neighbours within 1.5 m, eps 0.15 m,
min_edge 1 m, rho 0.9, M = 16):
  * a second partial cloud made of the LAST 60 % of the length (x > 3.2 m) was tried first and is not used: that part holds one
    pillar and, turned by 180 deg about z, lands on the other one, so a wrong pose gets score 30 and fitness 1610 of 1864 while the
    true pose never enters the 16 candidates by score, at any K up to 2^23 (its largest point error stays 5.9 m).  The fitness stage
    can only reject a wrong pose in favour of a right one that is among the candidates.  The middle 60 % replaced it.
  * K_HYPOTHESES = 2^22 is the smallest power of two at which, in all five placements, the winner lies within MAX_DIST / 2 = 0.25 m
    of the truth (largest point error) AND at least three all-inlier hypotheses survive.  Per placement at 2^22 (valid hypotheses /
    all-inlier ones / winner h, score, fitness of points / largest point error):
        turn140      26 031 / 16 / h 2 184 864, 48, 3199 of 3199 / 0.114 m        half_turn_z  20 109 /  3 / h 3 708 928, 38, 4274 of 4310 / 0.176 m
        turn75       26 292 / 20 / h    38 567, 64, 3211 of 3211 / 0.041 m        part_low     11 229 /  3 / h 2 847 174, 23, 1795 of 1844 / 0.213 m
        part_mid     24 677 /  7 / h   259 794, 24, 1652 of 1665 / 0.248 m
    At 2^21 half_turn_z has 2 all-inlier hypotheses and part_low 1 (their winners: 0.218 and 0.099 m); at 2^20 three placements
    have none.  0.86 to 2.0 % of the descriptor matches are right (within eps of the true position); 0.6 % of the hypotheses pass
    the edge check.
  * margins at 2^22, the smallest over the five placements: bin edges 8.4e-7, edge check 1.6e-7 m, degeneracy gap 6.4e-5 (nothing
    below 1e-14), inlier rule of the score 8.4e-8 m, of the fitness 1.0e-6 m; no descriptor tie; 8 to 12 score ties among the top
    17, decided by the lower h.
  * from these priors align_reference.icp (ratio 0.8, max_dist 0.5 m, 50 iterations) ends 3.3, 6.6, 3.4, 10.9 and 37 mm from the
    truth; from the identity it ends 16.8, 10.2, 5.9, 11.3 and 9.2 m away.
"""
import functools
import math

import numpy as np
from scipy.spatial import cKDTree

import align_reference as A

B = 11
NF = 3 * B
SEED = 135
N_CLOUD = 8000
SIGMA = 0.01
VOXEL = 0.25
FEATURE_K = 64
K_TAB = 64                                         # columns of the k-NN table: min(FEATURE_K + 1, 64), the point itself among them
FEATURE_RADIUS = 6 * VOXEL
EPS = 0.6 * VOXEL
MIN_EDGE = 4 * VOXEL
RHO = 0.9
N_CANDIDATES = 16
K_HYPOTHESES = 1 << 22                            # see above
MARGIN_BIN = 1e-9
MARGIN_EDGE = 1e-12
MARGIN_GAP = (1e-14, 1e-10)
MARGIN_INLIER = 1e-9
MASK64 = (1 << 64) - 1


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


# ---- pair features and histograms -------------------------------------------------------------------------------------------------
def pair_features(xi, ni, xj, nj):
    """(valid bool [...], a [...,3], L [...]) of the pairs (x_i, n_i), (x_j, n_j), arrays [...,3]."""
    with np.errstate(all='ignore'):
        d = xj - xi
        L = np.sqrt(dot3(d, d))
        li, lj = np.sqrt(dot3(ni, ni)), np.sqrt(dot3(nj, nj))
        e, u, v = d / L[..., None], ni / li[..., None], nj / lj[..., None]
        a = np.stack([np.abs(dot3(u, e)), np.abs(dot3(v, e)), np.abs(dot3(u, v))], axis=-1)
        valid = (L > 0) & np.isfinite(L) & (li > 0) & np.isfinite(li) & (lj > 0) & np.isfinite(lj) & ~np.isnan(a).any(axis=-1)
    return valid, a, L


def bins(a):
    with np.errstate(all='ignore'):
        return np.minimum(B - 1, np.floor(B * a)).astype(np.int64)


def bin_margin(a):
    """The smallest |B a - round(B a)| over the values whose nearest edge is one of the ten INNER edges 1/B .. (B - 1)/B (inf when
    there is none).  0 and 1 are not edges: a >= 0 by the absolute value and min(B - 1, .) keeps a >= 1 in the last bin, so a = 0, a = 1
    and the values a rounding error away from them (1 - ulp on a rotated coplanar pair) are safe."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    r = np.round(B * a)
    inner = (r >= 1) & (r <= B - 1)
    return float(np.abs(B * a[inner] - r[inner]).min()) if inner.any() else float('inf')


def histograms(points, normals, nbr, check=True):
    """dict(spfh f64 [n,33], m int32 [n], feat f32 [n,33], has int32 [n], margin): the descriptors over the table nbr int [n,k] (-1 or
    a row outside 0 .. n-1: missing)."""
    points, normals = np.asarray(points, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    nbr = np.asarray(nbr, dtype=np.int64)
    n, k = nbr.shape
    slot = (nbr >= 0) & (nbr < n)
    j = np.where(slot, nbr, 0)
    valid, a, L = pair_features(points[:, None, :], normals[:, None, :], points[j], normals[j])
    valid &= slot
    margin = bin_margin(a[valid])
    if check:
        assert margin >= MARGIN_BIN, 'a pair feature lies %.3g from a bin edge' % margin
    bn = np.where(valid[..., None], bins(np.where(valid[..., None], a, 0.0)), 0)
    m = valid.sum(axis=1).astype(np.int32)
    counts = np.zeros((n, NF), dtype=np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], (n, k))
    for c in range(3):
        np.add.at(counts, (rows[valid], c * B + bn[..., c][valid]), 1)
    with np.errstate(all='ignore'):
        spfh = np.where(m[:, None] > 0, counts.astype(np.float64) / m[:, None].astype(np.float64), 0.0)
        acc = np.zeros((n, NF))
        for s in range(k):                          # ascending slot order, one term at a time
            v = valid[:, s]
            w = 1.0 / L[v, s]
            acc[v] = acc[v] + w[:, None] * spfh[j[v, s]]
        inv = 1.0 / m.astype(np.float64)
        F = np.where(m[:, None] > 0, spfh + inv[:, None] * acc, 0.0)
        feat = np.zeros((n, NF), dtype=np.float32)
        for c in range(3):
            blk = F[:, c * B:(c + 1) * B]
            tot = np.zeros(n)
            for b in range(B):
                tot = tot + blk[:, b]
            scale = np.where(tot > 0.0, 100.0 / tot, 0.0)
            feat[:, c * B:(c + 1) * B] = (blk * scale[:, None]).astype(np.float32)
    return dict(spfh=spfh, m=m, feat=feat, has=(m > 0).astype(np.int32), margin=margin, counts=counts)


# ---- matching -----------------------------------------------------------------------------------------------------------------------
def feature_dist(fq, fs):
    """fp32: s = 0; s = s + t t, t = fq[b] - fs[b], b ascending; arrays [...,33] that broadcast."""
    fq, fs = np.asarray(fq, dtype=np.float32), np.asarray(fs, dtype=np.float32)
    s = np.zeros(np.broadcast(fq[..., 0], fs[..., 0]).shape, dtype=np.float32)
    for b in range(NF):
        t = fq[..., b] - fs[..., b]
        tt = t * t
        s = s + tt
    return s


def match(fq, hq, fs, hs, chunk=256, designed_ties=False):
    """(idx int32 [nq] or -1, dist f32 [nq] or +inf, ties): the nearest usable survey row, the lower row among equal distances; ``ties``
    counts the cloud rows whose two nearest survey rows are equally far without being equal rows (asserted 0 unless designed)."""
    fq, fs = np.asarray(fq, dtype=np.float32), np.asarray(fs, dtype=np.float32)
    nq = len(fq)
    idx, dist, ties = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32), 0
    use = np.flatnonzero(np.asarray(hs) != 0)
    rows = np.flatnonzero(np.asarray(hq) != 0)
    if len(use) and len(rows):
        fu = fs[use]
        for a in range(0, len(rows), chunk):
            r = rows[a:a + chunk]
            d = feature_dist(fq[r][:, None, :], fu[None, :, :])
            jj = np.argmin(d, axis=1)               # the first of the smallest: `use` ascends, so the lower survey row
            idx[r], dist[r] = use[jj], d[np.arange(len(r)), jj]
            if len(use) > 1:
                d2 = d.copy()
                d2[np.arange(len(r)), jj] = np.inf
                j2 = np.argmin(d2, axis=1)
                tie = d2[np.arange(len(r)), j2] == dist[r]
                ties += int((tie & ~(fu[jj] == fu[j2]).all(axis=1)).sum())
    if not designed_ties:
        assert ties == 0, '%d descriptor ties' % ties
    return idx, dist, ties


# ---- hypotheses ---------------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    """Vectorised over uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64_int(x):
    """The same on one Python integer: the check of the vectorised form."""
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draws(seed, K, C, h0=0):
    """int64 [K,3]: j_t = splitmix64(seed ^ (h << 2) ^ t) mod C for h = h0 .. h0 + K - 1."""
    h = np.arange(h0, h0 + K, dtype=np.uint64)
    s = np.uint64(seed & MASK64)
    return np.stack([(splitmix64(s ^ (h << np.uint64(2)) ^ np.uint64(t)) % np.uint64(C)).astype(np.int64) for t in range(3)], axis=1)


def edge_len(a, b):
    d = a - b
    return np.sqrt(dot3(d, d))


def hypotheses(P, Y, K, seed, min_edge, rho, o=None, check=True, chunk=1 << 18):
    """dict(h int64 [V] (the valid hypotheses, ascending), T [V,4,4], j [V,3] (their draws), passed (hypotheses that passed the edge
    check), edge_margin, gap_lo, gap_hi) by the rules of DESIGN, the fit by align_reference.fit_svd (which needs no origins) with the
    degeneracy rule gap <= REL_EPS max|lam| of align_reference.icp.  Hypotheses h < K' of a run with K >= K' are the run with K'."""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    C = len(P)
    hs, Ts, js, passed = [], [], [], 0
    edge_margin, lo, hi = float('inf'), 0.0, float('inf')
    for h0 in range(0, K if C >= 3 else 0, chunk):
        j = draws(seed, min(chunk, K - h0), C, h0)
        ok = (j[:, 0] != j[:, 1]) & (j[:, 0] != j[:, 2]) & (j[:, 1] != j[:, 2])
        for a, b in ((0, 1), (1, 2), (2, 0)):
            lp, ly = edge_len(P[j[:, a]], P[j[:, b]]), edge_len(Y[j[:, a]], Y[j[:, b]])
            near = np.minimum(np.abs(lp - min_edge), np.minimum(np.abs(lp - rho * ly), np.abs(ly - rho * lp)))
            if ok.any():                            # every comparison of every hypothesis that got this far
                edge_margin = min(edge_margin, float(near[ok].min()))
            ok &= (lp >= min_edge) & (lp >= rho * ly) & (ly >= rho * lp)
        passed += int(ok.sum())
        for r in np.flatnonzero(ok):
            Th, sv, d = A.fit_svd(P[j[r]], Y[j[r]])
            gap, lam_max = A.svd_gap(sv, d)
            rel = gap / lam_max if lam_max > 0 else 0.0
            if gap <= A.REL_EPS * lam_max:
                lo = max(lo, rel)
                continue
            hi = min(hi, rel)
            if np.isfinite(Th).all():
                hs.append(h0 + r)
                Ts.append(Th)
                js.append(j[r])
    if check:
        assert edge_margin >= MARGIN_EDGE, 'an edge check is decided by %.3g m' % edge_margin
        assert lo <= MARGIN_GAP[0] and hi >= MARGIN_GAP[1], 'degeneracy gaps %.3g / %.3g' % (lo, hi)
    return dict(h=np.array(hs, dtype=np.int64), T=np.array(Ts, dtype=np.float64).reshape(-1, 4, 4), j=np.array(js, dtype=np.int64).reshape(-1, 3),
                passed=passed, edge_margin=edge_margin, gap_lo=lo, gap_hi=hi)


def designed_pairs(C, seed=SEED, noise=0.01):
    """(P [C,3], Y [C,3], o [6]) whose valid triangles are all FAT, so that the bar of 1e-12 on a fitted transform is justified (see
    ``route_disagreement``): three clusters of radius 0.3 m at the corners of a triangle with 3 m sides hold the right matches (rows
    0, 1, 2 one each, then rows 3 .. 299 in turn; Y = R P + t + N(0, noise)), every later row is a wrong match whose P lies within
    0.4 m of the centre and whose Y is anywhere in a 6 m box.  With min_edge = 1 m two rows of one cluster, or two wrong matches, never
    pass the edge check: a valid triple has its points in three different places at least 1 m apart and angles far from 0 and 180 deg."""
    rng = np.random.default_rng(seed + 100 + C)
    corners = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.5], [1.5, 2.6, -0.5]])
    centre = corners.mean(axis=0)
    P = np.empty((C, 3))
    for i in range(C):
        u = rng.normal(size=3)
        u *= rng.random() ** (1 / 3) / np.linalg.norm(u)
        P[i] = corners[i % 3] + 0.3 * u if i < 300 else centre + 0.4 * u
    R, t = A.axis_angle((0.5, -0.7, 0.4), 2.5), np.array([4.0, -3.0, 1.0])
    Y = P @ R.T + t + rng.normal(0.0, noise, size=P.shape)
    Y[300:] = rng.uniform(-3.0, 3.0, size=(max(C - 300, 0), 3)) + t
    o = np.concatenate([0.5 * (P.min(axis=0) + P.max(axis=0)), 0.5 * (Y.min(axis=0) + Y.max(axis=0))])
    return np.ascontiguousarray(P), np.ascontiguousarray(Y), o


def route_disagreement(P, Y, hy, o):
    """The largest |fit_svd - fit_horn| entry over the valid hypotheses: what two correct fp64 routes to the same closed form (means
    + SVD; fsum moments about o + eigh of Horn's matrix) differ by on these triples -- the yardstick of the tests' bar on T, as
    align_reference.bars is for the ICP.  Both routes lose eps x max|lam| / gap in the rotation: on the scenes' thinnest triangles
    (gap / max|lam| 6e-5) they differ by 1.5e-12, so a flat bar of 1e-12 holds only on triangles that are not thin."""
    worst = 0.0
    for r in range(len(hy['h'])):
        j = hy['j'][r]
        Tb, _ = A.fit_horn(P[j], Y[j], o)
        worst = max(worst, float(np.abs(Tb - hy['T'][r]).max()))
    return worst


def expand(hy, K):
    """(valid int32 [K], T [K,4,4] with NaN rows for the invalid) of a ``hypotheses`` result: the layout of the kernels."""
    valid, T = np.zeros(K, dtype=np.int32), np.full((K, 4, 4), np.nan)
    valid[hy['h']], T[hy['h']] = 1, hy['T']
    return valid, T


def score(T, P, Y, eps, check=True, chunk=512):
    """(score int32 [V], margin): for every transform of T [V,4,4] the correspondences with |T p - y|^2 <= eps^2."""
    sc, margin = np.zeros(len(T), np.int32), float('inf')
    e2 = eps * eps
    for a in range(0, len(T), chunk):
        Tr = T[a:a + chunk]
        x = [((Tr[:, q, 0, None] * P[None, :, 0] + Tr[:, q, 1, None] * P[None, :, 1]) + Tr[:, q, 2, None] * P[None, :, 2]) + Tr[:, q, 3, None]
             for q in range(3)]
        d = [x[q] - Y[None, :, q] for q in range(3)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        sc[a:a + chunk] = (d2 <= e2).sum(axis=1)
        if d2.size:
            margin = min(margin, float(np.abs(np.sqrt(d2) - eps).min()))
    if check:
        assert margin >= MARGIN_INLIER, 'an inlier decision of the score has a margin of %.3g m' % margin
    return sc, margin


def fitness(tree, T, points, eps, check=True):
    """(count, margin): points whose nearest survey point under T lies within eps (d^2 < eps^2, the k-NN's rule)."""
    d, _ = tree.query(A.move(T, points))
    margin = float(np.abs(d - eps).min()) if len(d) else float('inf')
    if check:
        assert margin >= MARGIN_INLIER, 'an inlier decision of the fitness has a margin of %.3g m' % margin
    return int((d < eps).sum()), margin


def select(h, sc, M):
    """(rows int64 [M'] into h, ties): the valid hypotheses h [V] (ascending) with the largest (score, then lower h), M' = min(M, V);
    ``ties``: equal scores among the top M' + 1."""
    order = np.lexsort((h, -sc.astype(np.int64)))
    top = order[:M + 1]
    ties = int((np.diff(sc[top]) == 0).sum())
    for a, b in zip(top[:-1], top[1:]):
        assert sc[a] > sc[b] or (sc[a] == sc[b] and h[a] < h[b])
    return order[:M].astype(np.int64), ties


# ---- the clouds' preparation --------------------------------------------------------------------------------------------------------
def voxel_filter(points, voxel):
    """Rows kept by ops.voxel_filter(preserve_order=True): the LAST row of every voxel floor(p / voxel), ascending."""
    key = np.floor(points / voxel).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    last = np.full(inv.max() + 1, -1, dtype=np.int64)
    last[inv] = np.arange(len(points))              # later rows overwrite earlier ones
    return np.sort(last)


def neighbour_table(points, k_tab, r):
    """int32 [n, k_tab]: the k_tab nearest points within r (d^2 < r^2) in ascending distance, the point's own row set to -1."""
    n = len(points)
    k = min(k_tab, n)
    d, i = cKDTree(points).query(points, k=k)
    d, i = d.reshape(n, k), i.reshape(n, k)
    d2 = ((points[np.minimum(i, n - 1)] - points[:, None, :]) ** 2)
    d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    tab = np.where((i < n) & (d2 < r * r), i, -1)
    tab[tab == np.arange(n)[:, None]] = -1
    out = np.full((n, k_tab), -1, dtype=np.int32)
    out[:, :k] = tab
    return out


def descriptors(points, normals, voxel=VOXEL, k_tab=K_TAB, r=FEATURE_RADIUS, check=True):
    keep = voxel_filter(points, voxel)
    p, nrm = np.ascontiguousarray(points[keep]), np.ascontiguousarray(normals[keep])
    tab = neighbour_table(p, k_tab, r)
    h = histograms(p, nrm, tab, check=check)
    return dict(points=p, normals=nrm, nbr=tab, keep=keep, **h)


def corner_cloud(n, k, spoil=True):
    """(points [n,3], normals [n,3], nbr int32 [n,k]): a noisy two-wall corner with normals of random sign and length and its table of
    the k nearest OTHER points within 0.6 m (any distance for n < 65).  With ``spoil`` and n >= 65: row 3 is NaN, row 5 has a zero
    normal, row 7 has no neighbour, row 9 has -1 in every other slot, row 11 duplicates row 10 (which stays in its table)."""
    rng = np.random.default_rng(SEED + n)
    u, v = rng.uniform(0, 2, n), rng.uniform(0, 2, n)
    wall = rng.random(n) < 0.5
    pts = np.where(wall[:, None], np.stack([u, v, np.zeros(n)], 1), np.stack([np.zeros(n), u, v], 1)) + rng.normal(0, 0.01, (n, 3))
    nrm = np.where(wall[:, None], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)) + rng.normal(0, 0.05, (n, 3))
    nrm *= rng.choice([-1.0, 1.0], (n, 1)) * rng.uniform(0.5, 2.0, (n, 1))
    tab = neighbour_table(pts, k + 1, 0.6 if n >= 65 else 10.0)[:, 1:]        # column 0 is the point itself (distance 0)
    pts, nrm, tab = np.ascontiguousarray(pts), np.ascontiguousarray(nrm), np.ascontiguousarray(tab)
    if spoil and n >= 65:
        pts[3] = np.nan
        nrm[5] = 0.0
        tab[7] = -1
        tab[9, ::2] = -1
        pts[11] = pts[10]
    return pts, nrm, tab


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
PLACEMENTS = ('turn140', 'half_turn_z', 'turn75', 'part_low', 'part_mid')


def _placement_transform(name):
    """The true T (survey frame from the cloud's frame) of a placement."""
    R = {'turn140': A.axis_angle((0.3, -0.2, 1.0), math.radians(140.0)), 'half_turn_z': A.axis_angle((0.0, 0.0, 1.0), math.pi),
         'turn75': A.axis_angle((1.0, 0.5, -0.3), math.radians(75.0)), 'part_low': A.axis_angle((0.3, -0.2, 1.0), math.radians(140.0)),
         'part_mid': A.axis_angle((1.0, 0.5, -0.3), math.radians(75.0))}[name]
    t = {'turn140': (3.0, -1.0, 0.5), 'half_turn_z': (8.5, 6.5, 0.25), 'turn75': (-2.0, 1.5, 1.0), 'part_low': (1.0, 2.0, -0.5),
         'part_mid': (-1.5, -2.5, 0.75)}[name]
    return A.rigid(R, np.array(t))


@functools.lru_cache(maxsize=None)
def placement(name, n=N_CLOUD, sigma=SIGMA):
    """dict(survey, normals, query, query_normals, T_true, shifted=False): the scene of one placement (``query`` as align_reference's
    scenes call the cloud, so that align_reference.icp runs on it).  'part_low' keeps only the cloud points in the first 60 % of the room's length (x), 'part_mid'
    those in its middle 60 %, which has neither end wall."""
    pts, nrm = A.survey()
    cp, cn = A.survey(n=n, seed=SEED + 1)
    rng = np.random.default_rng(SEED + 2 + PLACEMENTS.index(name))
    cp = cp + rng.normal(0.0, sigma, size=cp.shape)
    cn = cn * rng.choice([-1.0, 1.0], size=(len(cn), 1))
    if name == 'part_low':
        sel = cp[:, 0] < 0.6 * A.ROOM[0]
        cp, cn = cp[sel], cn[sel]
    elif name == 'part_mid':
        sel = (cp[:, 0] > 0.2 * A.ROOM[0]) & (cp[:, 0] < 0.8 * A.ROOM[0])
        cp, cn = cp[sel], cn[sel]
    T = _placement_transform(name)
    Ti = np.linalg.inv(T)
    q = np.ascontiguousarray(A.move(Ti, cp))
    qn = np.ascontiguousarray(cn @ Ti[:3, :3].T)
    q.setflags(write=False)
    qn.setflags(write=False)
    return dict(survey=pts, normals=nrm, query=q, query_normals=qn, T_true=T, shifted=False, name=name)


@functools.lru_cache(maxsize=None)
def survey_descriptors():
    pts, nrm = A.survey()
    return descriptors(pts, nrm)


@functools.lru_cache(maxsize=None)
def correspondences(name):
    """dict(cloud (descriptors of the cloud), rows, P, Y, midx, o, right): the matches of a placement; ``right`` flags the matches whose
    survey point lies within EPS of the true position of the cloud point."""
    sc = placement(name)
    sd = survey_descriptors()
    cd = descriptors(sc['query'], sc['query_normals'])
    midx, mdist, _ = match(cd['feat'], cd['has'], sd['feat'], sd['has'])
    rows = np.flatnonzero(midx >= 0)
    P, Y = cd['points'][rows], sd['points'][midx[rows]]
    right = np.linalg.norm(A.move(sc['T_true'], P) - Y, axis=1) <= EPS
    return dict(cloud=cd, rows=rows, P=P, Y=Y, midx=midx, mdist=mdist, o=A.origins(sc['query'], sc['survey']), right=right)


@functools.lru_cache(maxsize=None)
def _hypotheses(name, K, seed):
    co = correspondences(name)
    hy = hypotheses(co['P'], co['Y'], K, seed, MIN_EDGE, RHO)
    hy['score'], hy['score_margin'] = score(hy['T'], co['P'], co['Y'], EPS)
    return hy


@functools.lru_cache(maxsize=None)
def coarse(name, K, seed=SEED, M=N_CANDIDATES):
    """The whole coarse stage of a placement with K hypotheses: dict(T, hypothesis, score, fitness, candidates [M,3], n_points,
    n_correspondences, n_valid, hyp (the ``hypotheses`` result with its scores), all_inlier (valid hypotheses whose three matches are
    right), error (the largest |T p - T_true p| over the cloud), margins, ties)."""
    sc, co = placement(name), correspondences(name)
    hy = _hypotheses(name, K, seed)
    s = hy['score']
    cand, ties = select(hy['h'], s, M)
    tree = cKDTree(sc['survey'])
    fit, m_fit = [], float('inf')
    for r in cand:
        f, mg = fitness(tree, hy['T'][r], co['cloud']['points'], EPS)
        fit.append(f)
        m_fit = min(m_fit, mg)
    fit = np.array(fit, dtype=np.int64)
    out = dict(n_points=len(co['cloud']['points']), n_correspondences=len(co['P']), n_valid=len(hy['h']), hyp=hy, ties=ties,
               margins=dict(edge=hy['edge_margin'], gap_lo=hy['gap_lo'], gap_hi=hy['gap_hi'], score=hy['score_margin'], fitness=m_fit),
               all_inlier=int(co['right'][hy['j']].all(axis=1).sum()), right_share=float(co['right'].mean()))
    if len(cand) == 0:
        out.update(T=np.eye(4), hypothesis=-1, score=0, fitness=0, candidates=np.zeros((0, 3), np.int64), error=float('inf'))
        return out
    best = int(np.argmax(fit))                      # the first of the largest: ties go to the earlier candidate
    top = np.sort(fit)[::-1]
    out['ties'] = ties + int(len(top) > 1 and top[0] == top[1])
    T = hy['T'][cand[best]]
    out.update(T=T, hypothesis=int(hy['h'][cand[best]]), score=int(s[cand[best]]), fitness=int(fit[best]),
               candidates=np.stack([hy['h'][cand], s[cand].astype(np.int64), fit], axis=1), error=point_error(T, sc))
    return out


def point_error(T, sc):
    """The largest |T p - T_true p| over the cloud of a scene."""
    return float(np.linalg.norm(A.move(T, sc['query']) - A.move(sc['T_true'], sc['query']), axis=1).max())
