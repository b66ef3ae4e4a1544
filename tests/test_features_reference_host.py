"""The reference of the neighbourhood-feature tests (features_reference.py) and their cases (features_cases.py), checked on the
host: the forward against dc_oracle.features in float64, the closed-form backward against float64 torch autograd through
dc_oracle.features, the branch claims and the conditioning of every case test_gpu_features_edge.py runs, and the host arm of the
kernels' arithmetic (libdc_hostcheck.so: cov_add / cov_finish / eig3_sym) on tables with missing slots.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import dc_oracle as O
import features_cases as cases
import features_reference as FR
from helpers import hostcheck_lib

SMALL = [c for c in cases.ALL_CASES if c[0] <= 577]
BWD_HOST = [(1, 4, 'full'), (65, 4, 'designed'), (65, 10, 'designed'), (129, 8, 'designed'), (129, 16, 'designed'), (255, 3, 'ragged'),
            (257, 12, 'per_wave'), (257, 16, 'designed'), (257, 4, 'full')]
assert set(BWD_HOST) <= set(cases.ALL_CASES)
_id = lambda c: '%d-%d-%s' % c


def _oracle_table(tab):
    """The table the oracle can finish on: LAPACK refuses the NaN covariance of a row without a valid member, so that row lists its
    own centre; the caller leaves the row out of the comparison (and feeds it no gradient)."""
    tab = tab.astype(np.int64)
    dead = np.flatnonzero((tab >= 0).sum(1) == 0)
    tab[dead, 0] = dead
    return tab, dead


@pytest.mark.parametrize('case', cases.ALL_CASES, ids=_id)
def test_claims_and_conditioning(case):
    """Every branch the table's kind claims is populated, and every row with three or more distinct points has
    min(lam1 - lam0, lam2 - lam1) / lam2 >= 1e-3 on the exact spectrum: an eigenvector error of 1e-14 / 1e-3 = 1e-11 at most in a
    gradient held to 1e-9."""
    x, dirs, tab, info = cases.make_case(*case)
    cases.assert_claims(case[2], tab, info)
    ref = FR.forward(*case)
    g = FR.gaps(ref)
    print('%s: smallest gap %.2e, %d rows with fewer than three distinct points' % (_id(case), g.min(), int(np.isinf(g).sum())))
    assert np.all(g >= cases.GAP), g.min()


@pytest.mark.parametrize('case', cases.BWD_HUB, ids=_id)
def test_hub_of_in_degree_n(case):
    """The 'hub_all' tables list one point in every row.  They are exempt from the gap condition -- the far hub flattens some rows --
    and are fed g_mean and g_cov only, whose derivatives need no eigenvector."""
    x, dirs, tab, info = cases.make_case(*case)
    cases.assert_claims(case[2], tab, info)
    assert np.bincount(np.concatenate([np.unique(r[r >= 0]) for r in tab]), minlength=len(x))[info['hub']] == len(x)


@pytest.mark.parametrize('case', SMALL, ids=_id)
def test_forward_reference_vs_oracle(case):
    """float64 torch (two-pass covariance, LAPACK) against the exact reference: the mean to 2^-48 of the cloud's scale, covariance and
    eigenvalues to 1e-12 lam_max, |dir . n| to 1e-9, weights and counts exactly; and the explicitly weighted mean."""
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)
    otab, dead = _oracle_table(tab)
    keep = np.ones(n, dtype=bool)
    keep[dead] = False
    fo = O.features(torch.tensor(x), torch.tensor(otab), torch.tensor(dirs))
    lmax = ref['lam'][keep, 2]
    scale = np.abs(x).max() + np.sqrt(lmax.max())
    assert np.abs(fo['mean'].numpy() - ref['mean'])[keep].max() <= 2.0 ** -48 * scale
    assert np.all(np.abs(fo['cov'].numpy() - ref['cov'])[keep].max((1, 2)) <= 1e-12 * lmax + 1e-300)
    assert np.all(np.abs(fo['eigvals'].numpy() - ref['lam'])[keep].max(1) <= 1e-12 * lmax + 1e-300)
    assert np.array_equal(fo['weights'].numpy()[keep, :, 0], ref['weights'][keep])
    assert np.array_equal(ref['nvalid'], (tab >= 0).sum(1))
    sep = keep & (ref['distinct'] >= 3)
    absdot = np.abs((dirs * fo['normals'].numpy()).sum(1))
    assert np.abs(absdot - ref['absdot'])[sep].max(initial=0.0) <= 1e-9
    w = FR.mean_weights(*case)
    w[dead, 0] = 1.0
    fw = O.features(torch.tensor(x), torch.tensor(otab), torch.tensor(dirs), weights=torch.tensor(w)[..., None])
    assert np.abs(fw['mean'].numpy() - FR.weighted_mean(x, otab, w))[keep].max() <= 2.0 ** -48 * scale
    assert np.array_equal(fw['cov'].numpy()[keep], fo['cov'].numpy()[keep])


@pytest.mark.parametrize('weighted', [False, True], ids=['validity', 'weights'])
@pytest.mark.parametrize('case', BWD_HOST + cases.BWD_HUB, ids=_id)
def test_backward_closed_form_vs_autograd(case, weighted):
    """The closed form against float64 autograd through dc_oracle.features, fed g_mean alone, an asymmetric g_cov alone, g_eig alone and
    all three (the hub of in-degree n: the first two), with validity weights and with explicit mean weights: within 1e-12 of
    max |grad|."""
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)
    otab, dead = _oracle_table(tab)
    w = FR.mean_weights(*case) if weighted else None
    if weighted:
        wo = w.copy()
        wo[dead, 0] = 1.0
    for which in ('mean', 'cov') if kind == 'hub_all' else ('mean', 'cov', 'eig', 'all'):
        gm, gc, ge = FR.upstream(n, k, kind, which)
        want = FR.backward(x, tab, ref['cov'], ref['cmean'], gm, gc, ge, mean_weights=w)
        xt = torch.tensor(x, requires_grad=True)
        fo = O.features(xt, torch.tensor(otab), torch.tensor(dirs), weights=torch.tensor(wo)[..., None] if weighted else None)
        loss = 0.0
        for g, f in ((gm, 'mean'), (gc, 'cov'), (ge, 'eigvals')):
            if g is not None:
                g = g.copy()
                g[dead] = 0.0
                loss = loss + (torch.tensor(g) * fo[f]).sum()
        loss.backward()
        got = xt.grad.numpy()
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        print('%s %-8s %-4s closed form vs autograd: %.2e of max |grad|' % (_id(case), 'weights' if weighted else 'validity', which, err))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize('case', [c for c in SMALL if c[2] in ('ragged', 'designed')], ids=_id)
def test_hostcheck_neighbourhoods_with_missing_slots(case):
    """dc_host_neighbourhoods -- cov_add, cov_finish and eig3_sym as the kernels inline them -- on ragged and designed tables, under
    the contract of test_hostcheck.py: every eigenvalue and every covariance entry within 1e-14 lam_max of the reference, the mean
    within 2^-50 of the cloud's scale; NaN for the row without a valid member, exact zeros for the row with one."""
    n, k, kind = case
    x, dirs, tab, info = cases.make_case(*case)
    ref = FR.forward(*case)
    host = hostcheck_lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = {f: np.zeros((n, d)) for f, d in dict(mean=3, cov6=6, lam=3, v0=3).items()}
    loss, c1, c2 = np.zeros(n), np.zeros(n), np.zeros(n)
    xs, ts = np.ascontiguousarray(x), np.ascontiguousarray(tab, dtype=np.int32)
    host.dc_host_neighbourhoods(p(xs), p(ts), ctypes.c_long(n), k, ctypes.c_double(0.0), 1, 0, 0, p(out['mean']), p(out['cov6']),
                                p(out['lam']), p(out['v0']), p(loss), p(c1), p(c2))
    W = ref['nvalid']
    live = W > 0
    C = ref['cov']
    ref6 = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)
    lmax = ref['lam'][:, 2]
    lerr, cerr = np.abs(out['lam'] - ref['lam']).max(1), np.abs(out['cov6'] - ref6).max(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s host arm: |dlam| %.2e, |dcov| %.2e of lam_max' % (_id(case), np.nanmax(np.where(lmax > 0, lerr / lmax, 0)),
                                                                  np.nanmax(np.where(lmax > 0, cerr / lmax, 0))))
    assert np.all(lerr[live] <= 1e-14 * lmax[live]) and np.all(cerr[live] <= 1e-14 * lmax[live])
    scale = np.abs(x).max() + np.sqrt(lmax[live].max())
    assert np.abs(out['mean'] - ref['mean'])[live].max() <= 2.0 ** -50 * scale
    assert np.isnan(out['mean'][~live]).all() and np.isnan(out['lam'][~live]).all()
    one = W == 1
    assert np.all(out['cov6'][one] == 0) and np.all(out['lam'][one] == 0)
    if kind == 'designed':
        assert (~live).sum() == 1 and one.sum() >= 1
