"""Global registration on the host (no GPU): the rules of csrc/dc_globalreg_math.h through their host build (libdc_hostcheck.so, the
header the kernels inline) against tests/globalreg_reference.py, bit for bit; then the oracle itself end to end on the five
placements, with the hypothesis count the GPU tests use, and the control (align_reference.icp from the identity).

Figures of the end-to-end run are in the docstring of globalreg_reference.py; the tests print them again.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_reference as A  # noqa: E402
import globalreg_reference as G  # noqa: E402


def host_lib():
    """libdc_hostcheck.so with the global registration exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_pair_histograms'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_pair_feature.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.dc_host_feature_dist.restype = ctypes.c_float
    lib.dc_host_feature_dist.argtypes = [vp, vp]
    lib.dc_host_greg_draw.restype = i64
    lib.dc_host_greg_draw.argtypes = [i64, i64, ci, i64]
    lib.dc_host_greg_check_fit.argtypes = [vp, vp, vp, f64, f64, vp, vp]
    lib.dc_host_greg_residual2.restype = f64
    lib.dc_host_greg_residual2.argtypes = [vp, vp, vp]
    lib.dc_host_pair_histograms.argtypes = [vp, vp, i64, vp, ci, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_pair(lib, xi, ni, xj, nj):
    xi, ni, xj, nj = (np.ascontiguousarray(v, dtype=np.float64) for v in (xi, ni, xj, nj))
    a, bins, L = np.zeros(3), np.zeros(3, np.int32), np.zeros(1)
    ok = lib.dc_host_pair_feature(_p(xi), _p(ni), _p(xj), _p(nj), _p(a), _p(bins), _p(L))
    return ok, a, bins, L[0]


def host_histograms(lib, points, normals, nbr):
    points, normals = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(normals, dtype=np.float64)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    n, k = nbr.shape
    spfh, m = np.zeros((n, G.NF)), np.zeros(n, np.int32)
    feat, has = np.zeros((n, G.NF), np.float32), np.zeros(n, np.int32)
    assert lib.dc_host_pair_histograms(_p(points), _p(normals), n, _p(nbr), k, _p(spfh), _p(m), _p(feat), _p(has)) == 0
    return dict(spfh=spfh, m=m, feat=feat, has=has)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- pair features ------------------------------------------------------------------------------------------------------------------
def test_pair_features_random_pairs_bit_equal(lib):
    rng = np.random.default_rng(G.SEED)
    xi, xj = rng.uniform(-5, 5, (500, 3)), rng.uniform(-5, 5, (500, 3))
    ni, nj = rng.normal(size=(500, 3)) * rng.uniform(0.1, 7.0, (500, 1)), rng.normal(size=(500, 3))
    valid, a, L = G.pair_features(xi, ni, xj, nj)
    bn = G.bins(a)
    assert valid.all() and G.bin_margin(a) >= G.MARGIN_BIN
    for q in range(500):
        ok, ha, hb, hL = host_pair(lib, xi[q], ni[q], xj[q], nj[q])
        assert ok == 1 and same_bits(ha, a[q]) and hL == L[q] and (hb == bn[q]).all()
        # the sign of either normal changes nothing, bit for bit
        for si, sj in ((-1, 1), (1, -1), (-1, -1)):
            ok2, ha2, hb2, _ = host_pair(lib, xi[q], si * ni[q], xj[q], sj * nj[q])
            assert ok2 == 1 and same_bits(ha2, ha) and (hb2 == hb).all()
    assert len(np.unique(bn)) == G.B                # every bin is reached


def test_pair_features_designed(lib):
    z, x = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    o = np.zeros(3)
    # coplanar: a1 = a2 = 0 (bin 0), a3 = 1 (bin 10)
    ok, a, b, L = host_pair(lib, o, z, np.array([3.0, 4.0, 0.0]), -2.0 * z)
    assert ok == 1 and L == 5.0 and a.tolist() == [0.0, 0.0, 1.0] and b.tolist() == [0, 0, 10]
    # d along both normals: every a = 1
    ok, a, b, _ = host_pair(lib, o, z, np.array([0.0, 0.0, 2.0]), z)
    assert ok == 1 and a.tolist() == [1.0, 1.0, 1.0] and b.tolist() == [10, 10, 10]
    # perpendicular walls, the offset along one normal: a1 = 1, a2 = 0, a3 = 0
    ok, a, b, _ = host_pair(lib, o, x, np.array([0.5, 0.0, 0.0]), z)
    assert ok == 1 and a.tolist() == [1.0, 0.0, 0.0] and b.tolist() == [10, 0, 0]
    # an inner edge exactly: a1 = 6 / 11 is not representable, 0.5 is -> B a = 5.5, bin 5; and just below an edge stays below
    ok, a, b, _ = host_pair(lib, o, np.array([1.0, 0.0, 0.0]), np.array([1.0, math.sqrt(3.0), 0.0]), z)
    assert ok == 1 and b[0] == 5 and abs(a[0] - 0.5) < 1e-15
    assert G.bins(np.array([np.nextafter(5 / 11, 0), 5 / 11 + 1e-16, 1.0, 1.0 + 1e-15, 0.0])).tolist() == [4, 5, 10, 10, 0]
    # invalid pairs: L = 0, a zero normal (either side), a NaN coordinate, an infinite one, a NaN normal
    n1 = np.array([0.0, 1.0, 0.0])
    p1 = np.array([1.0, 2.0, 3.0])
    assert host_pair(lib, p1, n1, p1, n1)[0] == 0
    assert host_pair(lib, o, o, p1, n1)[0] == 0 and host_pair(lib, o, n1, p1, o)[0] == 0
    assert host_pair(lib, o, n1, np.array([np.nan, 0.0, 1.0]), n1)[0] == 0
    assert host_pair(lib, o, n1, np.array([np.inf, 0.0, 1.0]), n1)[0] == 0
    assert host_pair(lib, o, np.array([np.nan, 0.0, 1.0]), p1, n1)[0] == 0
    for args in ((p1, n1, p1, n1), (o, o, p1, n1), (o, n1, np.array([np.nan, 0.0, 1.0]), n1), (o, n1, np.array([np.inf, 0.0, 1.0]), n1)):
        assert not G.pair_features(*[np.asarray(v, dtype=np.float64) for v in args])[0]


@pytest.mark.parametrize('n,k', [(1, 1), (2, 1), (65, 10), (257, 64)])
def test_histograms_host_equals_oracle(lib, n, k):
    pts, nrm, tab = G.corner_cloud(n, k)
    want = G.histograms(pts, nrm, tab)
    got = host_histograms(lib, pts, nrm, tab)
    assert (got['m'] == want['m']).all() and (got['has'] == want['has']).all()
    assert same_bits(got['spfh'], want['spfh']) and same_bits(got['feat'], want['feat'])
    if n >= 65:
        assert want['has'][3] == 0 and want['has'][5] == 0 and want['has'][7] == 0 and want['has'].sum() >= n - 4
        sums = want['feat'][want['has'] == 1].astype(np.float64).reshape(-1, 3, G.B).sum(axis=2)
        assert np.abs(sums - 100.0).max() < 1e-3
    else:
        assert (want['has'] == (1 if n == 2 else 0)).all()


# ---- descriptor distance ------------------------------------------------------------------------------------------------------------
def test_feature_distance_order(lib):
    rng = np.random.default_rng(G.SEED + 3)
    fq = (rng.random((200, G.NF)) * 100).astype(np.float32)
    fs = (rng.random((200, G.NF)) * 100).astype(np.float32)
    want = G.feature_dist(fq, fs)
    got = np.array([lib.dc_host_feature_dist(_p(fq[i]), _p(fs[i])) for i in range(200)], dtype=np.float32)
    assert same_bits(got, want)
    # the order is part of the rule: the same terms added from the last bin down, or summed in fp64 and rounded once, differ somewhere
    rev = G.feature_dist(fq[:, ::-1], fs[:, ::-1])
    wide = ((fq.astype(np.float64) - fs.astype(np.float64)) ** 2).sum(axis=1).astype(np.float32)
    assert (rev != want).any() and (wide != want).any()
    idx, dist, ties = G.match(fq, np.ones(200, np.int32), fs, np.ones(200, np.int32))
    assert ties == 0 and (idx >= 0).all()
    # duplicated survey rows: the lower one wins; rows without a descriptor take no part
    fs2 = np.concatenate([fs[:50], fs[:50]])
    hs2 = np.ones(100, np.int32)
    hs2[:10] = 0
    hq = np.ones(200, np.int32)
    hq[::7] = 0
    idx2, dist2, ties2 = G.match(fq, hq, fs2, hs2, designed_ties=True)
    assert (idx2[::7] == -1).all() and np.isinf(dist2[::7]).all()
    live = idx2[hq == 1]
    assert ((live >= 10) & (live < 60)).all()       # rows 10..49 beat their copies 60..99; rows 0..9 are matched through 50..59
    assert G.match(fq, hq, fs2, np.zeros(100, np.int32))[0].max() == -1


# ---- draws --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 4, 2 ** 31 - 1])
def test_draws(lib, C):
    for seed in (135, 0, -1, 2 ** 63 - 1, -2 ** 63):
        j = G.draws(seed, 300, C)
        assert j.min() >= 0 and j.max() < C
        for h in list(range(40)) + [255, 299]:
            for t in range(3):
                ref = G.splitmix64_int((seed & G.MASK64) ^ (h << 2) ^ t) % C
                assert lib.dc_host_greg_draw(seed, h, t, C) == ref == j[h, t]
    far = G.draws(135, 4, C, h0=2 ** 31 - 2)        # h past 2^31: the shift is of a 64-bit word
    for q in range(4):
        for t in range(3):
            assert lib.dc_host_greg_draw(135, 2 ** 31 - 2 + q, t, C) == far[q, t]


# ---- edge check and fit -------------------------------------------------------------------------------------------------------------
def host_check_fit(lib, p, y, o, min_edge, rho):
    p, y, o = (np.ascontiguousarray(v, dtype=np.float64) for v in (p, y, o))
    T, lam = np.zeros((4, 4)), np.zeros(4)
    ok = lib.dc_host_greg_check_fit(_p(p), _p(y), _p(o), min_edge, rho, _p(T), _p(lam))
    return ok, T


def test_check_fit_designed(lib):
    R, t = A.axis_angle((0.4, -0.3, 0.8), 2.2), np.array([3.0, -1.0, 0.5])
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.1, 0.0], [0.3, 1.7, 0.4]])
    y = p @ R.T + t
    o = np.array([1.0, 1.0, 0.0, 4.0, 0.0, 1.0])
    ok, T = host_check_fit(lib, p, y, o, 1.0, 0.9)
    Ta, s, d = A.fit_svd(p, y)
    assert ok == 1 and np.abs(T - Ta).max() < 1e-12 and np.abs(T - A.rigid(R, t)).max() < 1e-12
    # 1e-12: three exact pairs a few metres from the origins; both routes carry a few hundred ulp of 1 at the most
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    # min_edge: the shortest edge is |p2 - p0| = 1.772...; just below passes, just above fails
    e = float(G.edge_len(p[2], p[0]))
    assert host_check_fit(lib, p, y, o, np.nextafter(e, 0), 0.9)[0] == 1 and host_check_fit(lib, p, y, o, e, 0.9)[0] == 1
    assert host_check_fit(lib, p, y, o, np.nextafter(e, 9), 0.9)[0] == 0
    # collinear: edges fine, the rotation is not unique
    line = np.array([[0.0, 0.0, 0.0], [1.5, 0.75, 0.3], [3.0, 1.5, 0.6]])
    assert host_check_fit(lib, line, line @ R.T + t, o, 1.0, 0.9)[0] == 0
    # two equal points: refused by min_edge; with min_edge = 0 and equal images, by the degeneracy rule
    twin = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
    assert host_check_fit(lib, twin, twin @ R.T + t, o, 1.0, 0.9)[0] == 0
    assert host_check_fit(lib, twin, twin @ R.T + t, o, 0.0, 0.9)[0] == 0
    # different images of equal points: lp = 0 < rho ly
    assert host_check_fit(lib, twin, y, o, 0.0, 0.9)[0] == 0
    # edge ratio: stretch one image edge by s -> lp / ly = 1 / s against rho = 0.9, both ways; exact in binary: p on a lattice
    q = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    for s, want in ((1.0, 1), (1.109375, 1), (1.125, 0), (0.90625, 1), (0.890625, 0)):
        yq = q * (s, 1.0, 1.0)                      # edge 0-1: lp = 4, ly = 4 s; the others change less
        ok, _ = host_check_fit(lib, q, yq, np.zeros(6), 1.0, 0.9)
        lp, ly = 4.0, 4.0 * s
        assert (lp >= 0.9 * ly and ly >= 0.9 * lp) == bool(want)
        # (edge 1-2 is 5 against sqrt(16 s^2 + 9): within 0.9 for every s here)
        assert ok == want, s


def test_check_fit_equals_oracle_on_designed_pairs(lib):
    """The oracle's vectorised edge check and independent fit against the host build on 20 000 hypotheses over designed_pairs(1000),
    whose valid triangles are fat.  The bar on T, 1e-12, is 16 x what the oracle's own two routes may differ by here (asserted:
    <= 1e-12 / 16; measured 3.9e-15; the host build differs from the oracle by 5.8e-15), as align_reference.bars sets the ICP's."""
    K = 20000
    P, Y, o = G.designed_pairs(1000)
    hy = G.hypotheses(P, Y, K, 7, 1.0, 0.9)
    valid, Tall = G.expand(hy, K)
    own = G.route_disagreement(P, Y, hy, o)
    print('valid %d of %d, edge margin %.3g m, gaps %.3g / %.3g, routes differ by %.3g' % (valid.sum(), K, hy['edge_margin'], hy['gap_lo'],
                                                                                        hy['gap_hi'], own))
    assert valid.sum() >= 20 and own <= 1e-12 / 16
    j = G.draws(7, K, 1000)
    worst = 0.0
    for h in range(K):
        distinct = len(set(j[h])) == 3
        ok, T = host_check_fit(lib, P[j[h]], Y[j[h]], o, 1.0, 0.9)
        assert (distinct and ok == 1) == bool(valid[h]), h
        if valid[h]:
            worst = max(worst, float(np.abs(T - Tall[h]).max()))
    print('host build against the oracle: %.3g' % worst)
    assert worst < 1e-12
    # residuals: the host build and the oracle's order agree to the bit, so the counts are equal
    sc, _ = G.score(hy['T'], P, Y, 0.15)
    for r in range(0, len(hy['h']), 3):
        Th = np.ascontiguousarray(hy['T'][r])
        cnt = sum(lib.dc_host_greg_residual2(_p(Th), _p(np.ascontiguousarray(P[c])), _p(np.ascontiguousarray(Y[c]))) <= 0.15 * 0.15
                  for c in range(0, 60))
        want = sum(1 for c in range(60) if G.score(hy['T'][r:r + 1], P[c:c + 1], Y[c:c + 1], 0.15, check=False)[0][0])
        assert cnt == want
    assert sc.max() >= 20


# ---- the oracle end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', G.PLACEMENTS)
def test_oracle_end_to_end(name):
    """The coarse stage of the oracle with the specified draws and K_HYPOTHESES: every margin holds (asserted inside), the winner lies
    within MAX_DIST / 2 of the truth, at least three all-inlier hypotheses survive."""
    c = G.coarse(name, G.K_HYPOTHESES)
    print('%s: %d points, %d matches (%.2f %% right), %d valid, %d all-inlier; winner h %d score %d fitness %d, error %.4f m; ties %d; '
          'margins %s' % (name, c['n_points'], c['n_correspondences'], 100 * c['right_share'], c['n_valid'], c['all_inlier'],
                          c['hypothesis'], c['score'], c['fitness'], c['error'], c['ties'], c['margins']))
    assert c['error'] <= A.MAX_DIST / 2
    assert c['all_inlier'] >= 3
    assert c['n_valid'] > 100 * G.N_CANDIDATES


def test_oracle_needs_that_many_hypotheses():
    """K_HYPOTHESES is the smallest power of two: with half of it (the first half of the same hypotheses) a placement is left with
    fewer than three all-inlier hypotheses."""
    fewest = {}
    for name in G.PLACEMENTS:
        hy, co = G.coarse(name, G.K_HYPOTHESES)['hyp'], G.correspondences(name)
        first = hy['h'] < G.K_HYPOTHESES // 2
        fewest[name] = int(co['right'][hy['j'][first]].all(axis=1).sum())
    print(fewest)
    assert min(fewest.values()) < 3


@pytest.mark.parametrize('name', G.PLACEMENTS)
def test_control_icp_from_identity_stays_away(name):
    """The control: the trimmed ICP alone, from the identity, on the same placements.  The oracle shows that it ends metres from the
    truth in all five (16.8, 10.2, 5.9, 11.3, 9.2 m), so that is asserted for all five; from the oracle's coarse prior it ends within
    4 cm (3.3, 6.6, 3.4, 10.9, 37 mm)."""
    sc = G.placement(name)
    alone = A.icp(sc, n_iters=50)
    far = G.point_error(alone['T'], sc)
    refined = A.icp(sc, init=G.coarse(name, G.K_HYPOTHESES)['T'], n_iters=50)
    near = G.point_error(refined['T'], sc)
    print('%s: from the identity %s, %.3f m from the truth; from the coarse prior %s, %.4f m' % (name, alone['status'], far,
                                                                                               refined['status'], near))
    assert far > 1.0
    assert near < 0.05
