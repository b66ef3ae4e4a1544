"""The plane kernels (csrc/dc_planes.hip) at their edges.  RANSAC and the refit are compared bit for bit with the header oracle
(csrc/dc_planemath.h through libdc_hostcheck.so: the same per-element arithmetic, brute force, no blocks and no LDS), which the host
tests pin against a 50-digit reference (tests/test_planes_host.py, tests/planes_reference.py); DBSCAN with a scipy restatement,
exactly; fit_planes end to end with a numpy restatement of the whole loop; the plane moments with mpmath and float64 autograd.
The inputs are those of tests/planes_cases.py, shared with the host tests."""
import numpy as np
import pytest
import torch

import planes_cases as C
import planes_reference as R
from helpers import host_fit_planes, host_plane_inliers, host_ransac_refit, host_ransac_round, planes_host_lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _bufs(H):
    return dict(hyp=torch.empty((H, 4), dtype=torch.float64, device=DEV), anchor=torch.empty((H, 3), dtype=torch.float64, device=DEV),
                valid=torch.empty((H,), dtype=torch.int32, device=DEV), counts=torch.empty((H,), dtype=torch.int32, device=DEV),
                best=torch.empty((2,), dtype=torch.int32, device=DEV))


def _round_and_refit(x, rem, seed, m, H, thresh):
    """One RANSAC round and, when it has a winner, its refit, on the device and through the oracle; everything compared bitwise.
    Returns the oracle's round and (params, mask) or None."""
    from depth_correction_amd import segmentation as S
    lib = planes_host_lib()
    xd, rd = torch.tensor(x, device=DEV), torch.tensor(rem, device=DEV)
    bufs = _bufs(H)
    h, c = S._ransac_round(xd, rd, seed, m, H, thresh, bufs)
    want = host_ransac_round(lib, x, rem, seed, m, H, thresh)
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    np.testing.assert_array_equal(got['valid'], want['valid'])
    np.testing.assert_array_equal(_bits(got['anchor']), _bits(want['anchor']))
    np.testing.assert_array_equal(_bits(got['hyp']), _bits(want['hyp']))
    np.testing.assert_array_equal(got['counts'], want['counts'])
    assert (got['counts'][want['valid'] == 0] == -1).all()
    assert [h, c] == want['best'].tolist() == got['best'].tolist()
    if c < 1:
        return want, None
    params, mask = S._refit(xd, rd, thresh, bufs)
    _, p_want, m_want = host_ransac_refit(lib, x, rem, want, thresh)
    np.testing.assert_array_equal(_bits(params.cpu().numpy()), _bits(p_want))
    np.testing.assert_array_equal(mask.cpu().numpy().astype(bool), m_want)
    return want, (p_want, m_want)


@pytest.mark.parametrize('n_rem,H,dtype,m,seed', C.RANSAC_CASES)
def test_ransac_round_and_refit_bitwise(n_rem, H, dtype, m, seed):
    """`remaining` is a shuffled strict subset of a larger cloud; the sizes sit on the ends of the 1024-point scoring block and of the
    256-thread hypothesis and best-reduction blocks; H = 1024 fills the 48 KB of dynamic LDS; rounds > 0 reach the m << 40 term."""
    x, rem = C.ransac_cloud(n_rem + 61, n_rem, 1000 + n_rem + H, dtype=dtype, offset=(n_rem == 1023))
    want, refit = _round_and_refit(x, rem, seed, m, H, C.THRESH)
    if n_rem >= 255 and H >= 255:
        assert want['best'][1] > 0.5 * n_rem and refit is not None          # the large plane was found


def test_ransac_exact_lattice():
    """Coordinates that are multiples of 2^-6, thresh = 2^-5: a hypothesis through three rows of the z = 0 lattice is exactly
    (0, 0, +-1, 0) and counts exactly the 192 points with |z| <= 2^-5 (128 of them exactly on the border).  No exclusions."""
    from depth_correction_amd.segmentation import ransac_sample
    x = C.lattice_cloud()
    rem = np.arange(len(x), dtype=np.int32)
    H, seed, m = 1024, 135, 1
    want, refit = _round_and_refit(x, rem, seed, m, H, 2.0 ** -5)
    flat = [h for h in range(H) if max(ransac_sample(seed, m, h, len(x))) < 64 and want['valid'][h]]
    assert len(flat) >= 3
    for h in flat:
        assert np.array_equal(np.abs(want['hyp'][h]), [0.0, 0.0, 1.0, 0.0]) and want['counts'][h] == 192
    assert want['best'][1] >= 192 and refit is not None


def test_ransac_all_collinear():
    """Every hypothesis degenerate: best = (.., -1) and fit_planes returns no plane (and returns)."""
    from depth_correction_amd import segmentation as S
    x = C.collinear_cloud()
    want, refit = _round_and_refit(x, np.arange(len(x), dtype=np.int32), 135, 0, 64, C.THRESH)
    assert want['best'][1] == -1 and refit is None and not want['valid'].any()
    planes = S.fit_planes(torch.tensor(x, device=DEV), C.THRESH, min_support=3, max_iterations=64, seed=135)
    assert len(planes) == 0 and planes.params.shape == (0, 4)


@pytest.mark.parametrize('seed,m,lowest', C.TIE_SEEDS)
def test_ransac_ties_go_to_the_lowest_h(seed, m, lowest):
    from depth_correction_amd.segmentation import ransac_sample
    x = C.flat_lattice()
    want, _ = _round_and_refit(x, np.arange(64, dtype=np.int32), seed, m, 256, 2.0 ** -5)
    first = next(h for h in range(256) if len(set(ransac_sample(seed, m, h, 64))) == 3 and
                 R.hyp_plane(*x[list(ransac_sample(seed, m, h, 64))]) is not None)
    assert first == lowest and want['best'].tolist() == [first, 64] and (want['counts'] == 64).sum() > 100


def test_ransac_nan_and_inf_rows():
    """NaN and inf rows inside `remaining` are never inliers; a hypothesis that draws one is degenerate; every other count is the
    count over the finite rows alone."""
    x, rem = C.ransac_cloud(1300, 1100, 77)
    bad = rem[[5, 300, 301, 1024, 1099]]
    x[bad[0]] = np.nan
    x[bad[1], 1] = np.inf
    x[bad[2], 2] = -np.inf
    x[bad[3], 0] = np.nan
    x[bad[4]] = np.inf
    H = 256
    want, refit = _round_and_refit(x, rem, 135, 0, H, C.THRESH)
    lib = planes_host_lib()
    fin = np.isfinite(x[rem]).all(1)
    assert (~fin).sum() == 5
    for h in range(H):
        if want['valid'][h]:
            assert want['counts'][h] == host_plane_inliers(lib, want['hyp'][h], x[rem][fin], C.THRESH).sum()
    assert (want['valid'] == 0).sum() >= 1 and refit is not None and not refit[1][~fin].any() and refit[1].sum() > 500


# numpy's own float64 two-pass refit against the 50-digit one on this case's 9979 inliers: params_error 3.33e-16 (the header's,
# and so the kernel's: 2.78e-16)
BIG_REFIT_NUMPY_ERR = 3.33e-16


def test_refit_grid_stride_path():
    """n_rem = 262144 + 257 > 1024 blocks x 256 threads: the moments kernel strides.  Bitwise against the oracle, which sums in
    the same block order (dc_ransac_refit_partial_count blocks, the 256-thread tree, the blocks in order), and within 8 x numpy's own
    error of the 50-digit two-pass refit."""
    from depth_correction_amd import segmentation as S
    from depth_correction_amd._native import lib as dclib
    lib = planes_host_lib()
    x, rem, pl, anchor = C.big_refit_case()
    assert dclib().dc_ransac_refit_partial_count(len(rem)) == 1024 == lib.dc_host_ransac_refit_partial_count(len(rem))
    bufs = _bufs(1)
    bufs['hyp'].copy_(torch.tensor(pl[None]))
    bufs['anchor'].copy_(torch.tensor(anchor[None]))
    bufs['best'].copy_(torch.tensor([0, 0], dtype=torch.int32))
    params, mask = S._refit(torch.tensor(x, device=DEV), torch.tensor(rem, device=DEV), C.THRESH, bufs)
    rnd = dict(hyp=pl[None], anchor=anchor[None], best=np.array([0, 0], np.int32))
    tot, p_want, m_want = host_ransac_refit(lib, x, rem, rnd, C.THRESH)
    np.testing.assert_array_equal(_bits(params.cpu().numpy()), _bits(p_want))
    np.testing.assert_array_equal(mask.cpu().numpy().astype(bool), m_want)
    inl = x[rem][host_plane_inliers(lib, pl, x[rem], C.THRESH)]
    assert tot[0] == len(inl) == 9979
    err = R.params_error(params.cpu().numpy(), R.refit_two_pass(inl), 4.0)
    print('grid-stride refit: params_error %.3g' % err)
    assert err <= 8 * BIG_REFIT_NUMPY_ERR


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(C.dbscan_cases()))
def test_dbscan_matches_restatement(name):
    """Labels, best label and its size equal the scipy restatement exactly (what each case is for: planes_cases.dbscan_cases and
    test_planes_host.test_sequential_dbscan_against_scipy, which also checks the restatement's answers case by case)."""
    from depth_correction_amd.segmentation import dbscan
    x, eps, min_points = C.dbscan_cases()[name]
    labels, lbl, size = dbscan(torch.tensor(x, device=DEV), eps, min_points)
    want = R.dbscan(x, eps, min_points)
    np.testing.assert_array_equal(labels.cpu().numpy(), want[0])
    assert (lbl, size) == want[1:]


# ---- fit_planes end to end -------------------------------------------------------------------------------------------------------
def _check_fit(x, eps, **over):
    from depth_correction_amd import segmentation as S
    args = dict(C.SCENE_ARGS, **over)
    planes = S.fit_planes(torch.tensor(x, device=DEV), eps=eps, **args)
    rargs = dict(args)
    rargs['thresh'] = rargs.pop('distance_threshold')
    params, indices, trace = R.fit_planes_restated(x, eps=eps, **rargs)
    assert trace['border'] == 0
    hp, hi = host_fit_planes(planes_host_lib(), x, eps=eps, **args)
    assert len(planes) == len(indices) == len(hi)
    for p in range(len(indices)):
        np.testing.assert_array_equal(planes.indices[p].cpu().numpy(), indices[p])
        np.testing.assert_array_equal(hi[p], indices[p])
        np.testing.assert_array_equal(_bits(planes.params[p].cpu().numpy()), _bits(hp[p]))
    return planes, trace


@pytest.mark.parametrize('eps', [None, C.SCENE_EPS])
def test_fit_planes_three_planes(eps):
    planes, _ = _check_fit(C.scene_three_planes(), eps)
    assert len(planes) >= 3


def test_fit_planes_removes_a_support_without_cluster():
    """The sparse plane wins a round, has no 10-point cluster, leaves the remaining points as a whole; the round still counts and the
    two dense planes are found in the later rounds with the restatement's indices."""
    x = C.scene_sparse_plane()
    planes, trace = _check_fit(x, C.SCENE_EPS)
    what = [r['what'] for r in trace['rounds']]
    assert 'support removed' in what and len(planes) >= 2
    sparse = np.flatnonzero(np.abs(x[:, 2] - 3.0) < 0.02)
    taken = np.concatenate([i.cpu().numpy() for i in planes.indices])
    assert len(sparse) > 1500 and np.isin(sparse, taken).sum() < 0.02 * len(sparse)
    assert len(_check_fit(x, C.SCENE_EPS, max_models=1)[0]) == 1
    assert len(_check_fit(x, C.SCENE_EPS, min_support=10000)[0]) == 0


# ---- plane moments ---------------------------------------------------------------------------------------------------------------
# The bounds: 8 x the error of the float64 torch restatement (planes_reference.plane_cov_torch and its autograd) against mpmath
# (planes_reference.plane_mp) on these very inputs, relative to the largest entry of the quantity.  TORCH_ERR_PER_CASE holds the
# figure measured for every case.  A single case's figure is luck as much as arithmetic: it is 0 where the restatement happened
# to round like the 50-digit value (g_w of InvCos), and in the offset scene, where every kind carries the same rounding of
# x = vp + d' dir at the size of vp (6e-10 m), g_w ranges from 4.2e-12 to 8.2e-11 over the six kinds.  So the bound of a scene is
# 8 x the worst figure of its cases (TORCH_ERR):
#   origin (float64 and float32 clouds, six kinds)   cov 7.31e-16  g_vps 5.03e-16  g_dirs 5.73e-16  g_depth 9.91e-16  g_w 8.41e-16
#   offset (4e5, 5e6, 300) (float64, six kinds)      cov 3.37e-10  g_vps 3.57e-10  g_dirs 3.28e-10  g_depth 5.67e-10  g_w 8.22e-11
# Measured on an MI355X, every figure of the kernels also lies within 8 x its own case's entry (floored at one rounding, 2^-53)
# except g_w of two offset cases: InvCos 4.77e-11 (own case 4.18e-12) and ScaledPolynomial 1.56e-10 (own case 1.78e-11), both
# inside the spread of the scene.  float32 clouds: the gradients come back in float32, one more rounding of 2^-24; so does
# the covariance when there is no model.  The test prints every figure beside its case's entry and its bound.
TORCH_ERR_PER_CASE = {          # case: (cov, g_vps, g_dirs, g_depth, g_w)
    'None_float64_origin':               (4.93e-16, 2.52e-16, 2.87e-16, 3.96e-16, None),
    'Polynomial_float64_origin':         (6.17e-16, 3.77e-16, 4.3e-16, 7.92e-16, 1.76e-16),
    'ScaledPolynomial_float64_origin':   (2.47e-16, 2.61e-16, 4.24e-16, 3.96e-16, 2.1e-16),
    'Linear_float64_origin':             (3.72e-16, 3.78e-16, 4.32e-16, 6.96e-16, 2.23e-17),
    'InvCos_float64_origin':             (4.89e-16, 5.03e-16, 5.73e-16, 9.91e-16, 0.0),
    'ScaledInvCos_float64_origin':       (3.71e-16, 3.87e-16, 4.25e-16, 4.96e-16, 1.6e-16),
    'None_float32_origin':               (7.31e-16, 1.8e-16, 2.12e-16, 2.23e-16, None),
    'Polynomial_float32_origin':         (2.47e-16, 1.74e-16, 3.18e-16, 1.99e-16, 7.06e-16),
    'ScaledPolynomial_float32_origin':   (3.7e-16, 3.93e-16, 4.3e-16, 6.93e-16, 8.41e-16),
    'Linear_float32_origin':             (3.59e-16, 3.48e-16, 4.25e-16, 2.59e-16, 3.57e-16),
    'InvCos_float32_origin':             (3.45e-16, 2.9e-16, 3.18e-16, 2.52e-16, 0.0),
    'ScaledInvCos_float32_origin':       (3.46e-16, 2.52e-16, 4.31e-16, 7.94e-16, 0.0),
    'None_float64_offset':               (3.9e-11, 1.17e-10, 1.17e-10, 1.21e-10, None),
    'Polynomial_float64_offset':         (1.82e-10, 2.29e-10, 2.22e-10, 2.88e-10, 3.93e-11),
    'ScaledPolynomial_float64_offset':   (3.37e-10, 3.57e-10, 3.28e-10, 5.67e-10, 1.78e-11),
    'Linear_float64_offset':             (1.32e-10, 1.84e-10, 1.78e-10, 2.31e-10, 2.57e-11),
    'InvCos_float64_offset':             (1.65e-10, 1.69e-10, 1.63e-10, 2.4e-10, 4.18e-12),
    'ScaledInvCos_float64_offset':       (3.21e-10, 2.21e-10, 2.03e-10, 3.48e-10, 8.22e-11),
}
TORCH_ERR = {False: dict(cov=7.31e-16, g_vps=5.03e-16, g_dirs=5.73e-16, g_depth=9.91e-16, g_w=8.41e-16),
             True: dict(cov=3.37e-10, g_vps=3.57e-10, g_dirs=3.28e-10, g_depth=5.67e-10, g_w=8.22e-11)}


class _Cloud(object):
    def __init__(self, c):
        self.vps, self.dirs, self.depth = (torch.tensor(c[k], device=DEV, requires_grad=True) for k in ('vps', 'dirs', 'depth'))

    def __len__(self):
        return len(self.dirs)


def _model(kind):
    from depth_correction_amd import model as M
    w, e = C.MODELS[kind]
    f = lambda v: torch.tensor(v, dtype=torch.float64)
    if kind is None:
        return None, []
    if kind in ('Polynomial', 'ScaledPolynomial'):
        mdl = getattr(M, kind)(w=w, exponent=e, device=DEV)
        return mdl, [mdl.w]
    if kind == 'Linear':
        mdl = M.Linear(w0=f(w[0]), w1=f(w[1]), b=f(w[2]), device=DEV)
        return mdl, [mdl.w0, mdl.w1, mdl.b]
    mdl = getattr(M, kind)(p0=f(w[0]), device=DEV)
    return mdl, [mdl.p0]


@pytest.mark.parametrize('kind,dtype,offset', C.MOMENT_CASES)
def test_plane_moments_forward_and_backward(kind, dtype, offset):
    """Planes of 2, 3, 2047, 2048, 2049 and 4097 points in one launch (CHUNK = 2048: one block and several), with a point seen
    along +n (cos = 1), one along -n and, where the model allows it, one perpendicular to n.  cov against mpmath; the gradients to vps,
    dirs, depth and the weights against float64 autograd of the restatement for a random upstream gradient.  At cos = +-1 the
    kernel defines d gamma / d dir = 0; the restatement treats that point's gamma as a constant (detach)."""
    from depth_correction_amd import segmentation as S
    c = C.moments_cloud(kind, dtype, offset)
    cs = np.concatenate([np.abs(c['dirs'][i].astype(np.float64) @ n) for i, n in zip(c['indices'], c['normals'])])
    assert (cs == 1.0).sum() == 8 and (cs == 0.0).sum() == (4 if kind in C.PERP_KINDS else 0)
    cloud = _Cloud(c)
    planes = S.Planes(torch.tensor(np.c_[c['normals'], np.zeros(len(c['normals']))]), indices=[torch.tensor(i, device=DEV) for i in c['indices']])
    mdl, wparams = _model(kind)
    cov = S.plane_moments(cloud, planes, mdl)
    gcov = np.random.default_rng(2).normal(size=(len(c['indices']), 3, 3))
    (cov.double() * torch.tensor(gcov, device=DEV)).sum().backward()
    # the reference: float64 torch on the CPU from the same (float32 or float64) numbers
    w, e = C.MODELS[kind]
    vps, dirs, depth = (torch.tensor(c[k].astype(np.float64), requires_grad=True) for k in ('vps', 'dirs', 'depth'))
    wt = None if w is None else torch.tensor(w, dtype=torch.float64, requires_grad=True)
    et = None if w is None else torch.tensor(e if e is not None else [0.0] * len(w), dtype=torch.float64)
    cov_t = R.plane_cov_torch(vps, dirs, depth, c['indices'], torch.tensor(c['normals']), kind, wt, et)
    (cov_t * torch.tensor(gcov)).sum().backward()
    cov_mp = C.moments_cov_mp(kind, dtype, offset, c)
    f32 = 2.0 ** -24 if dtype == np.float32 else 0.0
    got = dict(cov=cov.detach().double().cpu().numpy(), g_vps=cloud.vps.grad, g_dirs=cloud.dirs.grad, g_depth=cloud.depth.grad)
    ref = dict(cov=cov_mp, g_vps=vps.grad, g_dirs=dirs.grad, g_depth=depth.grad)
    if wparams:
        got['g_w'] = torch.stack([p.grad.reshape(-1) for p in wparams]).reshape(-1)
        ref['g_w'] = wt.grad
    assert cov.dtype == (torch.float32 if (kind is None and dtype == np.float32) else torch.float64)
    for k in got:
        a = got[k].double().cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        b = ref[k].numpy() if isinstance(ref[k], torch.Tensor) else ref[k]
        extra = 0.0 if k == 'g_w' or (k == 'cov' and kind is not None) else f32
        for p in range(len(c['indices'])) if k == 'cov' else [None]:
            aa, bb = (a[p], b[p]) if p is not None else (a, b)
            err = np.abs(aa - bb).max() / np.abs(bb).max()
            own = TORCH_ERR_PER_CASE[C.moments_key(kind, dtype, offset)][list(TORCH_ERR[offset]).index(k)]
            print('%s %s%s: %.3g (torch on this case %.3g, bound %.3g)' % (C.moments_key(kind, dtype, offset), k, '' if p is None else '[%d]' % p,
                                                                          err, own, 8 * TORCH_ERR[offset][k] + extra))
            assert err <= 8 * TORCH_ERR[offset][k] + extra, (k, p, err)


def test_size_one_plane_gives_nan_and_leaves_the_others():
    """One observation has no covariance (torch.cov gives NaN); the other planes of the same launch are unaffected."""
    from depth_correction_amd import segmentation as S
    c = C.moments_cloud('Polynomial', np.float64, False)
    mdl, _ = _model('Polynomial')
    idx = [torch.tensor(i, device=DEV) for i in c['indices']]
    nrm = np.c_[c['normals'], np.zeros(6)]
    with torch.no_grad():
        base = S.plane_moments(_Cloud(c), S.Planes(torch.tensor(nrm), indices=idx), mdl)
        one = S.plane_moments(_Cloud(c), S.Planes(torch.tensor(nrm), indices=[idx[0], idx[1][:1]] + idx[2:]), mdl)
    assert torch.isnan(one[1]).all()
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(one[keep], base[keep]) and torch.isfinite(base).all()
