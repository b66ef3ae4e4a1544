"""The exact reference of the eigen-solver tests (eig_reference.py, mpmath at 60 digits) against LAPACK and against the host build
of the kernels' own math, on the clouds the GPU tests use (eig_cases.py).  No GPU needed.

LAPACK route (numpy fp64: differences to the centre point, two-pass covariance, np.linalg.eigh) against mpmath, largest
|lam - lam_ref| / lam_max over the three eigenvalues of the 770 neighbourhoods (k = 10; offset 20 m, 0 for tiny / huge / mixed),
measured with the whitened construction of eig_cases.synth_groups:

    family           float64    float32          family           float64    float32
    generic          8.6e-16    1.2e-15          sign_switch      9.2e-16    9.5e-16
    planar           7.8e-16    8.2e-16          threshold        1.1e-15    1.3e-15
    needle           1.3e-15    1.3e-15          threshold_unit   1.1e-15    1.3e-15
    double_lo        9.2e-16    1.1e-15          tiny             1.3e-15    9.8e-16
    double_hi        6.7e-16    8.9e-16          huge             1.4e-15    9.6e-16
    isotropic        1.2e-15    1.2e-15          mixed            1.1e-15    1.1e-15
    near_isotropic   1.2e-15    1.2e-15          exact_rank       5.4e-16    5.4e-16
    edge             9.1e-16    9.2e-16

(the test prints them).  The bound of 2.5e-15 lam_max holds -- the largest figure is 1.4e-15 -- so the device bound of 1e-14 lam_max
is one the reference route itself meets with a factor seven to spare."""
import ctypes

import numpy as np
import pytest

import eig_cases as cases
import eig_reference as R
from helpers import hostcheck_lib

from eig_reference import ALL, offset_of, check_v0, loss_bound

DTYPES = [np.float64, np.float32]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope='module')
def host():
    return hostcheck_lib()


def test_cases_realise_their_spectra():
    """synth_groups: the covariance of every group has the eigenvalues asked for (to the rounding of the construction), for every k
    the tests use; the table is the whole group, the centre first; 'mixed' cycles through the families."""
    rng = np.random.default_rng(3)
    for k in (8, 10, 16):
        lams = cases.family_lams('generic', 5, rng)
        x, nbr = cases.synth_groups(lams, k, np.float64, 20.0, rng)
        assert x.shape == (5 * k, 3) and nbr.shape == (5 * k, k) and nbr.dtype == np.int32
        assert np.array_equal(nbr[:, 0], np.arange(5 * k)) and np.array_equal(np.sort(nbr, 1), np.sort(nbr[::k].repeat(k, 0), 1))
        for g in range(5):
            got = np.linalg.eigvalsh(np.cov(x[g * k:(g + 1) * k].T))
            np.testing.assert_allclose(got, lams[g], rtol=0, atol=1e-12)
    mixed = cases.family_lams('mixed', 26, np.random.default_rng(0))
    assert mixed[11].max() < 1e-13 and mixed[12].max() > 1e9 and mixed[24].max() < 1e-13           # tiny, huge, tiny again
    assert sorted(cases.MIXED_CYCLE) == sorted(cases.FAMILIES)
    assert cases.family_lams('mixed', 22, np.random.default_rng(0), scales=False).max() < 2


def test_exact_rank_groups_are_exact():
    """Collinear, coplanar and identical groups: the rank deficiency is exact in both dtypes (integer arithmetic on the grid)."""
    for dtype in DTYPES:
        for off, scale in ((20.0, 1.0), (8.0, cases.SEQ_SCALE)):
            x, nbr = cases.make_cloud('exact_rank', 10, dtype, off, scale=scale)
            q = np.round(x.astype(np.float64) * 512).astype(np.int64)
            assert np.array_equal(q / 512.0, x.astype(np.float64))
            for g, pts in enumerate(q.reshape(-1, 10, 3)):
                d = pts - pts[0]
                rank = np.linalg.matrix_rank(d.astype(np.float64))
                assert rank == (1, 2, 0)[g % 3]
    _, _, ref = R.reference('exact_rank', np.float32, 10, 20.0)
    lam = ref['lam'][::10]
    zero = lambda v: np.all(np.abs(v) < 1e-50)                         # (the division by k leaves 1e-60 in the 60-digit arithmetic)
    assert zero(lam[0::3, :2]) and np.all(lam[0::3, 2] > 1e-6)
    assert zero(lam[1::3, 0]) and np.all(lam[1::3, 1] > 1e-6) and np.all(lam[2::3] == 0)


def test_sequence_form_reproduces_points():
    """vps + depth * dirs is exact in either dtype, and every z lies in [1, 2]."""
    for dtype in DTYPES:
        for case in ('needle', 'exact_rank'):
            s = cases.sequence_cloud(case, dtype)
            assert s['points'].dtype == dtype
            assert np.array_equal(s['vps'] + s['depth'] * s['dirs'], s['points'])
            assert s['points'][:, 2].min() >= 1 and s['points'][:, 2].max() <= 2


def _lapack(x, nbr):
    x = x.astype(np.float64)
    d = x[nbr] - x[:, None, :]                                        # differences to the centre point
    d = d - d.mean(1, keepdims=True)
    C = np.einsum('nki,nkj->nij', d, d) / (nbr.shape[1] - 1)
    return np.linalg.eigh(C)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ALL)
def test_lapack_route_meets_reference(case, dtype):
    """numpy fp64 + LAPACK within 2.5e-15 lam_max of the mpmath reference for every eigenvalue of every neighbourhood (figures in
    the module docstring)."""
    x, nbr, ref = R.reference(case, dtype, 10, offset_of(case))
    lam, _ = _lapack(x, nbr)
    scale = ref['lam'][:, 2:3]
    err = np.abs(lam - ref['lam']) / np.where(scale > 0, scale, 1.0)
    print('LAPACK vs mpmath  %-15s %s  %.2e' % (case, np.dtype(dtype).name, err.max()))
    assert err.max() <= 2.5e-15


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ALL)
def test_host_neighbourhoods_meet_reference(host, case, dtype):
    """The host build of the kernels' neighbourhood math (anchored one-pass moments, cov_finish, eig3_sym, loss_and_coeffs) on the
    same clouds: eigenvalues within 1e-14 lam_max, eigenvector as in test_hostcheck.py, losses within the bound that follows."""
    x, nbr, ref = R.reference(case, dtype, 10, offset_of(case))
    n, k = nbr.shape
    x64 = np.ascontiguousarray(x.astype(np.float64))
    for (tag, loss, norm, sqrt) in R.VARIANTS:
        out = {f: np.zeros((n, d)) for f, d in dict(mean=3, cov6=6, lam=3, v0=3).items()}
        l, c1, c2 = np.zeros(n), np.zeros(n), np.zeros(n)
        host.dc_host_neighbourhoods(_p(x64), _p(nbr), ctypes.c_long(n), k, ctypes.c_double(0.0), 0 if loss == 'min_eigval_loss' else 1,
                                    int(norm), int(sqrt), _p(out['mean']), _p(out['cov6']), _p(out['lam']), _p(out['v0']), _p(l),
                                    _p(c1), _p(c2))
        lmax = ref['lam'][:, 2]
        assert np.all(np.abs(out['lam'] - ref['lam']) <= 1e-14 * lmax[:, None])
        assert np.abs(np.linalg.norm(out['v0'], axis=1) - 1).max() < 1e-14
        check_v0(out['v0'], out['lam'][:, 0], ref)
        assert np.all(np.abs(l - ref[tag]) <= loss_bound(ref, norm, sqrt, loss, 1e-14))


@pytest.mark.parametrize('solver', ['dc_host_eig3', 'dc_host_eig3_v2', 'dc_host_eig3_smallest', 'dc_host_eig3_smallest_r2',
                                    'dc_host_eig3_smallest_v2'])
@pytest.mark.parametrize('case', ALL)
def test_host_solvers_meet_reference(host, case, solver):
    """Every solver of dc_eig3.h (host arm) on the reference's covariance rounded to float64, against the reference's spectrum."""
    _, _, ref = R.reference(case, np.float64, 10, offset_of(case))
    C = ref['cov'][::10]
    lref, lmax = ref['lam'][::10], ref['lam'][::10, 2]
    sub = {f: v[::10] for f, v in ref.items()}
    c6 = np.ascontiguousarray(np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1))
    n = len(C)
    if solver in ('dc_host_eig3', 'dc_host_eig3_v2'):
        lam, vec = np.zeros((n, 3)), np.zeros((n, 9))
        getattr(host, solver)(_p(c6), ctypes.c_long(n), _p(lam), _p(vec))
        assert np.all(np.diff(lam, axis=1) >= 0)
        assert np.all(np.abs(lam - lref) <= 1e-14 * lmax[:, None])
        V = vec.reshape(n, 3, 3)
        assert np.abs(np.einsum('nki,nli->nkl', V, V) - np.eye(3)).max() < 1e-14
        check_v0(V[:, 0], lam[:, 0], sub)
    else:
        lam0, v0, tr = np.zeros(n), np.zeros((n, 3)), np.zeros(n)
        getattr(host, solver)(_p(c6), ctypes.c_long(n), _p(lam0), _p(v0), _p(tr))
        assert np.all(np.abs(lam0 - lref[:, 0]) <= 1e-14 * lmax)
        np.testing.assert_allclose(tr, sub['tr'], rtol=1e-14)
        assert np.abs(np.linalg.norm(v0, axis=1) - 1).max() < 1e-14
        check_v0(v0, lam0, sub)
