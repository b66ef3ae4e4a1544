"""Plane neighbourhoods without a GPU: the RANSAC sampler, the configuration fields, the clear error on CPU clouds."""
import numpy as np
import pytest
import torch


def _splitmix64_np(x):
    """An independent restatement of splitmix64 in numpy uint64 arithmetic (wraps modulo 2^64)."""
    with np.errstate(over='ignore'):
        z = np.uint64(x) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))


PINNED = [((135, 0, 0, 20000), (19410, 12446, 12360)),
          ((135, 0, 499, 20000), (16091, 18908, 18719)),
          ((135, 3, 17, 12345), (9833, 7858, 6421)),
          ((0, 0, 1, 3), (1, 2, 2)),
          ((2 ** 63 + 5, 7, 250, 1000003), (694489, 264203, 478978))]


@pytest.mark.parametrize('args,want', PINNED)
def test_ransac_sampler_pinned_table(args, want):
    from depth_correction_amd.segmentation import ransac_sample
    assert ransac_sample(*args) == want


def test_ransac_sampler_matches_uint64_restatement():
    from depth_correction_amd.segmentation import ransac_sample
    for seed, m, h, n in [(135, 0, 0, 20000), (1, 2, 3, 7), (2 ** 64 - 1, 11, 1023, 99991)]:
        s = seed & (2 ** 64 - 1)
        want = tuple(_splitmix64_np(s ^ ((m << 40) & (2 ** 64 - 1)) ^ (h << 2) ^ t) % n for t in range(3))
        assert ransac_sample(seed, m, h, n) == want


def test_config_has_ransac_fields():
    from depth_correction_amd.config import Config
    cfg = Config()
    assert cfg.ransac_dist_thresh == 0.03
    assert cfg.num_ransac_iters == 500
    assert cfg.ransac_model_size == 3


def test_plane_neighbourhoods_on_cpu_need_a_gpu():
    from depth_correction_amd.config import Config, NeighborhoodType
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.preproc import establish_neighborhoods
    cfg = Config(nn_type=NeighborhoodType.plane, device='cpu')
    cloud = DepthCloud.from_points(torch.rand((100, 3), dtype=torch.float64) + 1.0)
    with pytest.raises(RuntimeError, match='needs a GPU|need a GPU'):
        establish_neighborhoods(cloud=cloud, cfg=cfg)


def test_planes_container():
    from depth_correction_amd.segmentation import Planes
    p = Planes(torch.tensor([[0.0, 0.0, 1.0, -1.0], [1.0, 0.0, 0.0, 2.0]], dtype=torch.float64),
               cloud=[None, None], indices=[torch.arange(3), torch.arange(3, 5)])
    assert len(p) == 2 and len(p.copy()) == 2
    d = p.distance(torch.tensor([[0.0, 0.0, 3.0]], dtype=torch.float64))
    assert torch.equal(d, torch.tensor([2.0, 2.0], dtype=torch.float64))
    q = p.orient(torch.tensor([[-5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]], dtype=torch.float64))
    assert len(q) == 2
    sub = p[torch.tensor([False, True])]
    assert len(sub) == 1 and torch.equal(sub.indices[0], torch.arange(3, 5))


# ---- csrc/dc_planemath.h through its host build, against the high-precision restatement (tests/planes_reference.py) -----------------
import planes_cases as C  # noqa: E402
import planes_reference as R  # noqa: E402
from helpers import (host_dbscan, host_fit_planes, host_plane_from_points, host_plane_inliers, host_plane_model, host_plane_moments,  # noqa: E402
                     host_plane_refit, host_ransac_refit, host_ransac_round, planes_host_lib)

KINDS = [None, 'Polynomial', 'ScaledPolynomial', 'Linear', 'InvCos', 'ScaledInvCos']
BORDER = 2.0 ** -40           # exact residuals nearer than BORDER * max(1, |d|) to the threshold may fall either way ...
BORDER_CAP = 1e-3             # ... and at most this share of a case's points may lie there


def _clouds():
    rng = np.random.default_rng(3)
    noisy, rem = C.ransac_cloud(3000, 2500, 17)
    off, rem_o = C.ransac_cloud(3000, 2500, 18, offset=True)
    return {'random': (rng.uniform(-5, 5, (2000, 3)), np.arange(2000, dtype=np.int32)), 'noisy planes': (noisy, rem), 'offset scene': (off, rem_o)}


@pytest.mark.parametrize('name', ['random', 'noisy planes', 'offset scene'])
def test_header_planes_and_inliers_against_exact_residuals(name):
    """Hypothesis planes to a few ulps of the 50-digit plane; inlier decisions equal to the sign of the exact residual for every
    point further than 2^-40 max(1, |d|) from the threshold; the points nearer than that are counted and capped at 0.1 %.
    (Measured on these clouds: 0 points within the border for every hypothesis checked, so the reference alone stays inside the cap.)"""
    from depth_correction_amd.segmentation import ransac_sample
    lib = planes_host_lib()
    x, rem = _clouds()[name]
    H = 6
    got = host_ransac_round(lib, x, rem, 135, 2, H, C.THRESH)
    scale = max(1.0, float(np.abs(x).max()))
    for h in range(H):
        j = ransac_sample(135, 2, h, len(rem))
        want = R.hyp_plane(*x[rem[list(j)]], distinct=len(set(j)) == 3)
        assert (want is not None) == bool(got['valid'][h])
        np.testing.assert_array_equal(got['anchor'][h], x[rem[j[0]]])
        if want is None:
            assert got['counts'][h] == -1 and np.isposinf(got['hyp'][h, 3]) and not got['hyp'][h, :3].any()
            continue
        n_ref, d_ref = np.array([float(c) for c in want[0]]), float(want[1])
        # the differences u, v are exact or rounded once, the cross product loses |u| |v| / |u x v| (_cond) to cancellation, the
        # norm, the division and the dot product add a rounding each: 8 roundings of 2^-53, times _cond; d = -n . p0 inherits the
        # error of n times the size of the coordinates
        assert np.abs(got['hyp'][h, :3] - n_ref).max() <= 8 * 2.0 ** -53 * _cond(x, rem, j)
        assert abs(got['hyp'][h, 3] - d_ref) <= 8 * 2.0 ** -53 * scale * _cond(x, rem, j)
        res = R.exact_residuals(got['hyp'][h], x[rem], C.THRESH)
        dec = host_plane_inliers(lib, got['hyp'][h], x[rem], C.THRESH)
        border = np.abs(res) <= BORDER * max(1.0, abs(got['hyp'][h, 3]))
        print('%s h=%d: %d of %d points within the border' % (name, h, int(border.sum()), len(rem)))
        assert border.sum() <= BORDER_CAP * len(rem)
        np.testing.assert_array_equal(dec[~border], (res <= 0.0)[~border])
        assert got['counts'][h] == dec.sum()


def _cond(x, rem, j):
    """How much the plane through the sample amplifies one rounding of its points: |u| |v| / |u x v| (at least 1)."""
    p = x[rem[list(j)]].astype(np.float64)
    u, v = p[1] - p[0], p[2] - p[0]
    return max(1.0, np.linalg.norm(u) * np.linalg.norm(v) / np.linalg.norm(np.cross(u, v)))


def test_header_exact_lattice_has_no_border():
    """Coordinates that are multiples of 2^-6, a hypothesis through three lattice points of z = 0: n = (0, 0, 1), d = 0 exactly; with
    thresh = 2^-5 the points at z = +-2^-5 are inliers, those at z = +-(2^-5 + 2^-6) are not.  No exclusions."""
    lib = planes_host_lib()
    x = C.lattice_cloud()
    ok, pl = host_plane_from_points(lib, x[[0, 8, 1]])
    assert ok and np.array_equal(pl, [0.0, 0.0, 1.0, 0.0])
    dec = host_plane_inliers(lib, pl, x, 2.0 ** -5)
    np.testing.assert_array_equal(dec, np.abs(x[:, 2]) <= 2.0 ** -5)
    assert dec[:192].all() and not dec[192:].any()
    assert (R.exact_residuals(pl, x, 2.0 ** -5)[64:192] == 0.0).all()


def test_degenerate_hypotheses_score_minus_one():
    from depth_correction_amd.segmentation import ransac_sample
    lib = planes_host_lib()
    # n_remaining = 3: hypothesis 1 of round 0, seed 0 draws (1, 2, 2) (the pinned table above)
    assert ransac_sample(0, 0, 1, 3) == (1, 2, 2)
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]])
    got = host_ransac_round(lib, x, np.arange(3, dtype=np.int32), 0, 0, 8, C.THRESH)
    for h in range(8):
        distinct = len(set(ransac_sample(0, 0, h, 3))) == 3
        assert bool(got['valid'][h]) == distinct and got['counts'][h] == (3 if distinct else -1)
    assert got['valid'][1] == 0 and got['counts'][1] == -1
    # every point on one line: every hypothesis is degenerate, the round returns count -1
    line = C.collinear_cloud()
    got = host_ransac_round(lib, line, np.arange(len(line), dtype=np.int32), 135, 0, 64, C.THRESH)
    assert not got['valid'].any() and (got['counts'] == -1).all() and got['best'][1] == -1
    assert R.hyp_plane(*line[[3, 50, 120]]) is None


def _first_proper_hypothesis(x, seed, m, H):
    from depth_correction_amd.segmentation import ransac_sample
    for h in range(H):
        j = ransac_sample(seed, m, h, len(x))
        if len(set(j)) == 3 and R.hyp_plane(*x[list(j)]) is not None:
            return h
    return None


def test_ties_go_to_the_lowest_proper_hypothesis():
    """64 lattice points of z = 0: every proper hypothesis counts 64, so the best is the lowest h whose triple is distinct and not
    collinear (worked out from ransac_sample and the 50-digit degeneracy rule)."""
    lib = planes_host_lib()
    x = C.flat_lattice()
    for seed, m, first in C.TIE_SEEDS:
        got = host_ransac_round(lib, x, np.arange(64, dtype=np.int32), seed, m, 256, 2.0 ** -5)
        h = _first_proper_hypothesis(x, seed, m, 256)
        assert h == first
        assert set(got['counts'].tolist()) <= {64, -1} and (got['counts'] == -1).any()
        assert got['best'].tolist() == [h, 64]


# numpy's own float64 two-pass refit (planes_reference.refit_numpy) against the 50-digit one on the same inliers, as params_error
# (the larger of |dn| and |dd| / the size of the coordinates): 1.11e-16 at the origin, 1.46e-18 at the offset scene (measured; the
# test prints them beside the header's 3.5e-19 and 1.6e-19) -> the bound is 8 x that
REFIT_NUMPY_ERR = {False: 1.11e-16, True: 1.46e-18}


@pytest.mark.parametrize('offset', [False, True])
def test_refit_against_two_pass(offset):
    lib = planes_host_lib()
    x, rem = C.ransac_cloud(3000, 2500, 23, offset=offset)
    rnd = host_ransac_round(lib, x, rem, 135, 0, 32, C.THRESH)
    assert rnd['best'][1] > 1000
    tot, params, mask = host_ransac_refit(lib, x, rem, rnd, C.THRESH)
    inl = x[rem][host_plane_inliers(lib, rnd['hyp'][rnd['best'][0]], x[rem], C.THRESH)]
    assert tot[0] == len(inl)
    want = R.refit_two_pass(inl)
    scale = float(np.abs(x).max())
    err, err_np = R.params_error(params, want, scale), R.params_error(R.refit_numpy(inl), want, scale)
    print('refit offset=%s: header %.3g, numpy two-pass %.3g' % (offset, err, err_np))
    assert err <= 8 * REFIT_NUMPY_ERR[offset]
    np.testing.assert_array_equal(mask, host_plane_inliers(lib, params, x[rem], C.THRESH))


# seeds of planes_cases.random_plane whose eigenvector leaves the Jacobi sweeps with its largest-magnitude component NEGATIVE (found by
# a seeded search over 3000 planes: 9 with that component on x, 5 on y, 66 on z), and three that leave it positive
FLIPPED_SEEDS = [66, 294, 505, 701, 1567, 1680, 33, 35, 50]
UNFLIPPED_SEEDS = [8, 1, 0]


def test_refit_sign_rule():
    """The sign rule where it acts: on these moments the eigenvector step (dc_host_smallest_eigvec_jacobi: the vector before the rule)
    has a negative largest-magnitude component, on x, y and z in turn, and plane_refit returns it positive, in agreement with the
    50-digit two-pass refit; three planes that need no flip keep their sign.  (With the flip taken out of plane_refit this test
    fails on all nine flipped seeds: checked once by hand.)"""
    from helpers import host_smallest_eigvec
    lib = planes_host_lib()
    axes = set()
    for seed in FLIPPED_SEEDS + UNFLIPPED_SEEDS:
        pts = C.random_plane(seed)
        v = C.moments_about(pts, pts[0])
        raw = host_smallest_eigvec(lib, C.cov6_of_moments(v))
        k = int(np.argmax(np.abs(raw)))
        assert (raw[k] < 0) == (seed in FLIPPED_SEEDS), (seed, raw)
        got, want = host_plane_refit(lib, v, pts[0]), R.refit_two_pass(pts)
        assert int(np.argmax(np.abs(got[:3]))) == k and got[k] > 0 and want[k] > 0, (seed, got, want)
        np.testing.assert_allclose(got[:3], -raw / np.linalg.norm(raw) if raw[k] < 0 else raw / np.linalg.norm(raw), rtol=0, atol=4e-16)
        assert R.params_error(got, want, 1.0) <= 1e-13          # (the sums are formed in numpy here: this test is about the sign)
        if raw[k] < 0:
            axes.add(k)
    assert axes == {0, 1, 2}


def test_refit_on_ill_scaled_and_isotropic_moments():
    """The Jacobi eigenvector step away from comfortable inputs.  Coordinates scaled by 2^+-498 (covariance entries around 1e+-300):
    every operation of plane_refit then scales by an exact power of two, so the normal keeps its bits and d scales exactly.  Two
    equal smallest eigenvalues: any unit vector of that eigenspace is right.  A multiple of the identity: the first axis."""
    from helpers import host_smallest_eigvec
    lib = planes_host_lib()
    pts = C.random_plane(33)
    base = host_plane_refit(lib, C.moments_about(pts, pts[0]), pts[0])
    for k in (-498, 498):
        f = 2.0 ** k
        v = C.moments_about(pts, pts[0]) * np.array([1.0] + 3 * [f] + 6 * [f * f])
        assert np.isfinite(v).all() and v[4:].max() > 0
        got = host_plane_refit(lib, v, pts[0] * f)
        np.testing.assert_array_equal(got[:3], base[:3])
        assert got[3] == base[3] * f
    # C = Q diag(1, 1, 4) Q^T: the smallest eigenvalue is double
    rng = np.random.default_rng(6)
    for _ in range(20):
        Q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        for lam in ([1.0, 1.0, 4.0], [1.0, 1.0 + 1e-15, 4.0], [2.0 ** -1000, 2.0 ** -1000, 2.0 ** -998]):
            Cm = (Q * lam) @ Q.T
            Cm = 0.5 * (Cm + Cm.T)
            nv = host_smallest_eigvec(lib, [Cm[0, 0], Cm[0, 1], Cm[0, 2], Cm[1, 1], Cm[1, 2], Cm[2, 2]])
            assert abs(np.linalg.norm(nv) - 1.0) <= 1e-14
            assert abs(nv @ Q[:, 2]) <= 1e-14                                    # in the plane of the double eigenvalue
            assert np.linalg.norm(Cm @ nv - lam[0] * nv) <= 1e-14 * lam[2]
    for scale in (1.0, 1e-300, 1e300, 0.0):
        np.testing.assert_array_equal(host_smallest_eigvec(lib, [scale, 0.0, 0.0, scale, 0.0, scale]), [1.0, 0.0, 0.0])


# model_eval / model_dw against mpmath: relative error per value at most MODEL_K * 2^-53.  MODEL_K = 4 x the worst error of the plain
# float64 torch expression of the same model (planes_reference.model_torch and its autograd) against mpmath on the same inputs,
# which is 3.51 * 2^-53 (ScaledPolynomial, exponents [2, 4], gamma = 1.2, dd'/dgamma); the header's own worst is 5.48 * 2^-53.
MODEL_K = 4 * 3.51
GAMMAS = [0.0, 2.0 ** -30, 0.3, 1.2, np.pi / 2 - 2.0 ** -20]
EXPONENTS = [0, 1, 2, 4, 0.5, 2.5, 8, 9]


def _model_configs(kind):
    if kind in ('Polynomial', 'ScaledPolynomial'):
        return [([0.05], [e]) for e in EXPONENTS] + [C.MODELS[kind]]
    return [C.MODELS[kind]]


@pytest.mark.parametrize('kind', KINDS)
def test_model_eval_and_dw_against_mpmath(kind):
    import mpmath as mp
    lib = planes_host_lib()
    worst = 0.0
    for w, e in _model_configs(kind):
        w = [] if w is None else w
        e = [0.0] * len(w) if e is None else e
        for g in GAMMAS:
            d = 7.3
            got = host_plane_model(lib, R.KIND_CODES[kind], w, e, d, g)
            with mp.workdps(R.DPS):
                ref = R.model_mp(kind, mp.mpf(d), mp.mpf(g), [mp.mpf(float(t)) for t in w], [mp.mpf(float(t)) for t in e])
                pairs = [(got[0], ref[0]), (got[1], ref[1]), (got[2], ref[2])] + list(zip(got[3], ref[3]))
                for a, r in pairs:
                    if r is None:                       # gamma = 0 under an exponent in (0, 1): the derivative is infinite
                        assert np.isinf(a)
                        continue
                    if r == 0:
                        assert a == 0.0
                        continue
                    err = abs(float((mp.mpf(float(a)) - r) / r)) / 2.0 ** -53
                    worst = max(worst, err)
                    assert err <= MODEL_K, (kind, w, e, g, a, float(r), err)
    print('model %s: worst %.3g * 2^-53' % (kind, worst))


@pytest.mark.parametrize('name', sorted(C.dbscan_cases()))
def test_sequential_dbscan_against_scipy(name):
    lib = planes_host_lib()
    x, eps, min_points = C.dbscan_cases()[name]
    nb, margin = R.neighbour_lists(x, eps)
    if name not in ('lattice',):
        assert margin > 1e-9 or margin == 0.0 and name == 'copies', margin          # no pair near eps except where the case puts it there
    want = R.dbscan_from_lists(nb, min_points)
    got = host_dbscan(lib, R.padded_table(nb), min_points)
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1:] == want[1:]
    lab = want[0]
    if name == 'lattice':
        g = np.round(x / 0.125).astype(int)
        inner = ((g > 0) & (g < 11)).all(1)
        face = (((g == 0) | (g == 11)).sum(1) == 1)
        assert margin == 0.0 and (lab[inner] == lab[inner].min()).all() and (lab[face] == lab[inner].min()).all()
        assert (lab[~inner & ~face] == -1).all() and want[2] == 10 ** 3 + 6 * 10 ** 2
    elif name == 'chain':
        order = np.argsort(x[:, 0])
        core_min = int(np.sort(order[1:-1])[0])
        assert (lab == core_min).all() and want[1:] == (core_min, 4096)
    elif name == 'bridge':
        assert len(nb[0]) == 3 and lab[0] == min(lab[31], lab[62]) and lab[31] != lab[62] and lab[31] == 1
    elif name == 'equal':
        assert want[1:] == (5, 40) and (lab[:5] == -1).all() and set(lab[45:].tolist()) == {45}
    elif name == 'noise':
        assert want[1:] == (-1, 0) and (lab == -1).all()
    elif name == 'single':
        assert want[1:] == (-1, 0)
    elif name == 'single_core':
        assert want[1:] == (0, 1)
    elif name == 'copies':
        assert want[1:] == (0, 25) and (lab == 0).all()


def test_fit_planes_restatement_on_the_scenes():
    """The numpy restatement of the whole loop on the scenes the GPU tests use: the dense planes are found, no inlier decision lies
    within 1e-9 of the threshold (so float64 rounding cannot change an index), and on the sparse-plane scene the loop removes a
    support that has no cluster, goes on, and the round counter it hands the sampler includes that round."""
    x = C.scene_three_planes()
    for eps in (None, C.SCENE_EPS):
        params, indices, trace = R.fit_planes_restated(x, eps=eps, **_loop_args())
        assert trace['border'] == 0
        sizes = sorted(len(i) for i in indices)
        assert len(params) >= 3 and sizes[-3:][0] > 900 and sizes[-1] > 1900, sizes
    x = C.scene_sparse_plane()
    params, indices, trace = R.fit_planes_restated(x, eps=C.SCENE_EPS, **_loop_args())
    assert trace['border'] == 0
    what = [r['what'] for r in trace['rounds']]
    k = what.index('support removed')
    assert [r['round'] for r in trace['rounds']] == list(range(len(what)))          # every RANSAC call counts, this one included
    assert trace['rounds'][k]['count'] > 1500 and what[k + 1].startswith('plane') and trace['rounds'][k + 1]['round'] == k + 1
    assert trace['rounds'][k + 1]['n_rem'] < trace['rounds'][k]['n_rem'] - 1500          # the sparse support is gone
    sizes = sorted(len(i) for i in indices)
    assert len(params) >= 2 and sizes[-2] > 850 and sizes[-1] > 1250, sizes
    near_sparse = [np.abs(x[i][:, 2] - 3.0).max() < 0.1 for i in indices]
    assert not any(near_sparse)
    assert len(R.fit_planes_restated(x, eps=C.SCENE_EPS, **dict(_loop_args(), max_models=1))[0]) == 1
    # the same loop on the header oracle picks the same points, plane by plane, and its planes agree to the refit's bound
    lib = planes_host_lib()
    hp, hi = host_fit_planes(lib, x, eps=C.SCENE_EPS, **C.SCENE_ARGS)
    assert len(hi) == len(indices)
    for a, b, pa, pb in zip(hi, indices, hp, params):
        np.testing.assert_array_equal(a, b)
        assert R.params_error(pa, pb, float(np.abs(x).max())) <= 2 * 8 * REFIT_NUMPY_ERR[False]          # both sides carry an error of that size
    assert len(R.fit_planes_restated(x, eps=C.SCENE_EPS, **dict(_loop_args(), min_support=10000))[0]) == 0


def _loop_args():
    a = dict(C.SCENE_ARGS)
    a['thresh'] = a.pop('distance_threshold')
    return a


# Plane moments through the header against mpmath: planes of 2, 3 and 40 points with the three special directions.  Every bound is
# 8 x the error of the float64 torch restatement (planes_reference.plane_cov_torch and its autograd) against mpmath on the same scene,
# the worst of the six model kinds, relative to the largest entry of the quantity; the test prints both sides' figures.  Away from
# the origin the corrected point x = vp + d' dir is itself rounded at the size of vp (2^-53 * 5e6 = 6e-10 m), for the restatement
# as for the header: that, not the summation, is the error there.
MOMENT_TORCH_ERR = {False: dict(cov=4.2e-16, g_vps=2.9e-16, g_dirs=2.5e-16, g_depth=3.8e-16, g_w=4.2e-16),
                    True: dict(cov=3.7e-10, g_vps=1.5e-10, g_dirs=1.5e-10, g_depth=1.2e-10, g_w=1.1e-10)}


def _small_moments_case(kind, offset):
    c = C.moments_cloud(kind, offset=offset, sizes=(2, 3, 2047), seed=5)
    # 40 rows of the large plane, the three special points among them (rows 5, 6, 7 of the plane as generated)
    c['indices'][2] = c['indices'][2][:40]
    return c


@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_plane_moments_header_against_mpmath(kind, offset):
    lib = planes_host_lib()
    c = _small_moments_case(kind, offset)
    w, e = C.MODELS[kind]
    rng = np.random.default_rng(2)
    vps, dirs, depth = (torch.tensor(c[k], requires_grad=True) for k in ('vps', 'dirs', 'depth'))
    wt = None if w is None else torch.tensor(w, dtype=torch.float64, requires_grad=True)
    et = None if w is None else torch.tensor(e if e is not None else [0.0] * len(w), dtype=torch.float64)
    cov_t = R.plane_cov_torch(vps, dirs, depth, c['indices'], torch.tensor(c['normals']), kind, wt, et)
    gcov = rng.normal(size=(3, 3, 3))
    (cov_t * torch.tensor(gcov)).sum().backward()
    worst = dict.fromkeys(MOMENT_TORCH_ERR[offset], 0.0)
    worst_t = dict(worst)
    gw_h, gw_m = 0.0, 0.0
    for p, idx in enumerate(c['indices']):
        got = host_plane_moments(lib, c['vps'], c['dirs'], c['depth'], idx, c['normals'][p], R.KIND_CODES[kind], w, e, gcov[p])
        ref = R.plane_mp(c['vps'], c['dirs'], c['depth'], idx, c['normals'][p], kind, w, e, gcov[p])
        if p == 2:
            cs = np.abs(c['dirs'][idx] @ c['normals'][p])
            assert (cs == 1.0).sum() == 2 and ((cs == 0.0).sum() == 1) == (kind in C.PERP_KINDS)
        tor = dict(cov=cov_t[p].detach().numpy(), g_vps=vps.grad[idx].numpy(), g_dirs=dirs.grad[idx].numpy(),
                   g_depth=depth.grad[idx].numpy().reshape(-1))
        for k in ('cov', 'g_vps', 'g_dirs', 'g_depth'):
            s = np.abs(ref[k]).max()
            worst[k] = max(worst[k], np.abs(got[k] - ref[k]).max() / s)
            worst_t[k] = max(worst_t[k], np.abs(tor[k] - ref[k]).max() / s)
        if w is not None:
            gw_h, gw_m = gw_h + got['g_w'], gw_m + ref['g_w']
    if w is not None:
        worst['g_w'] = np.abs(gw_h - gw_m).max() / np.abs(gw_m).max()
        worst_t['g_w'] = np.abs(wt.grad.numpy() - gw_m).max() / np.abs(gw_m).max()
    print('moments %s offset=%s: header %s | torch %s' % (kind, offset, {k: '%.2g' % v for k, v in worst.items()},
                                                          {k: '%.2g' % v for k, v in worst_t.items()}))
    for k, b in MOMENT_TORCH_ERR[offset].items():
        assert worst[k] <= 8 * b, (k, worst[k], b)


def test_size_one_plane_is_nan_on_the_host():
    lib = planes_host_lib()
    c = _small_moments_case(None, False)
    got = host_plane_moments(lib, c['vps'], c['dirs'], c['depth'], c['indices'][2][:1], c['normals'][2], 0)
    assert np.isnan(got['cov']).all()


def test_plane_csr_refuses_a_plane_without_indices():
    """A plane with no indices would make plane_fwd_kernel read idx[plane_ptr[p]] one past the end for the last plane: refused on the
    host, before any launch."""
    from depth_correction_amd.segmentation import _PlaneCSR
    with pytest.raises(ValueError, match='no indices'):
        _PlaneCSR([torch.arange(3), torch.empty((0,), dtype=torch.int64)], 'cpu')
    with pytest.raises(ValueError, match='no indices'):
        _PlaneCSR([torch.empty((0,), dtype=torch.int64), torch.arange(3)], 'cpu')
    assert _PlaneCSR([torch.arange(3), torch.arange(3, 5)], 'cpu').n_blocks == 2
