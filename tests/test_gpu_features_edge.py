"""The four kernels of csrc/dc_features.hip -- features_fwd_kernel, features_fwd_tile_kernel, features_grec_kernel and
features_bwd_kernel -- against the exact reference of features_reference.py on the designed tables of features_cases.py: partial
last wavefronts, wavefronts whose lanes disagree in the two ballots, missing slots, rows with zero to three valid members, a hub and
a point nobody lists, both strides, both dtypes, every output, `want` subsets, pointers that are not 16-B aligned, and the backward
point by point.  Every launch is tiny.

The bounds of the forward are the ones test_gpu_eig_spectra.test_features_spectra states (the solvers' contract, 1e-14 lam_max per
neighbourhood, plus one float32 ulp where float32 is stored); the backward is held to 1e-9 of max |grad| in float64, the bar
test_gpu_edge.py holds consistency_bwd to, and 1e-5 in float32.  Every test prints the largest error it saw in units of its bound."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

import features_cases as cases
import features_reference as FR
from eig_reference import check_v0
from helpers import t, npy

pytestmark = pytest.mark.gpu

EPS = 1e-14
ULP32 = 2.0 ** -23
ULP64 = 2.0 ** -52
ALL = ('mean', 'cov', 'eigvals', 'eigvecs', 'normals', 'inc_angles')
TILED_K = cases.TILED_K
_id = lambda c: '%d-%d-%s' % c
_tt = lambda dtype: torch.float32 if dtype == np.float32 else torch.float64


def _points(x, dtype, stride, dev, fill=0.0):
    if stride == 4:
        x = np.concatenate([x, np.full((len(x), 1), fill)], 1)
    return t(x.astype(dtype), dev)


@contextlib.contextmanager
def _routed(tiled):
    """The A-B switch set and the launches recorded: yields a callable that names the kernel dc_features_fwd launched last."""
    from depth_correction_amd import _native as nv
    from depth_correction_amd.plan import KernelTimer
    prev = nv.lib().dc_features_set_tiled(tiled)
    try:
        with KernelTimer(every=1) as timer:
            yield lambda: timer.kernels()['features_fwd']
    finally:
        nv.lib().dc_features_set_tiled(prev)


def _kernel(tiled):
    return 'features_fwd_tile_kernel<' if tiled else 'features_fwd_kernel<'


def _forward(x, nbr, dirs, tiled, want=ALL, saved=True, weights=True, mean_weights=None):
    """ops.features_fwd with the A-B switch set -> (outputs as float64 / integer numpy arrays, the raw tensors, the kernel's name)."""
    from depth_correction_amd import ops
    with _routed(tiled) as launched:
        f = ops.features_fwd(x, nbr, dirs=dirs, want=want, want_saved=saved, want_weights=weights, mean_weights=mean_weights)
        name = launched()
    out = {key: (npy(v).astype(np.float64) if v.dtype.is_floating_point else npy(v)) for key, v in f.items() if v is not None}
    return out, f, name


def _ratio(err, bound):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if np.size(r) else 0.0


def _check_forward(o, ref, x, dirs, f32, worst, mean_ref=None):
    """Every output of one forward call against the reference, with the bounds of the module's docstring; `worst` collects the largest
    error per output in units of its bound."""
    n = len(x)
    W = ref['nvalid']
    live = W > 0
    ulp = ULP32 if f32 else 0.0

    def note(tag, err, bound):
        r = _ratio(err, bound)
        worst[tag] = max(worst.get(tag, 0.0), r)
        assert r <= 1.0, (tag, r)

    assert np.array_equal(o['nvalid'], W)
    assert np.array_equal(o['weights'], ref['weights'])
    note('invd', np.abs(o['invd'] - ref['invd']), (ULP32 if f32 else ULP64) * ref['invd'])
    # the row without a valid member: NaN like the reference's 0 / 0; its wavefront neighbours are held to the bounds below
    for f in ('mean', 'cmean', 'eigvals', 'cov'):
        assert np.isnan(o[f][~live]).all() and np.isfinite(o[f][live]).all(), f
    one = W == 1
    assert np.all(o['cov'][one] == 0) and np.all(o['eigvals'][one] == 0)
    if not live.any():
        return
    lam, V, lmax = o['eigvals'][live], o['eigvecs'][live], ref['lam'][live, 2]
    assert np.all(np.diff(lam, axis=1) >= 0)
    note('eigvals', np.abs(lam - ref['lam'][live]), EPS * lmax[:, None] + ulp * np.abs(ref['lam'][live]))
    note('cov', np.abs(o['cov'][live] - ref['cov'][live]).max((1, 2)), (EPS + ulp) * lmax)
    scale = np.abs(x).max() + np.sqrt(lmax.max())
    mtol = np.full(1, (ULP32 if f32 else 2.0 ** -50) * scale)
    note('mean', np.abs(o['mean'][live] - (ref['mean'] if mean_ref is None else mean_ref)[live]).max(keepdims=True), mtol)
    note('cmean', np.abs(o['cmean'][live] - ref['cmean'][live]).max(keepdims=True), mtol)
    note('orthonormal', np.abs(np.einsum('nji,njk->nik', V, V) - np.eye(3)).max(keepdims=True), np.full(1, 1e-12 + 2 * ulp))
    res = np.abs(np.einsum('nij,njk->nik', ref['cov'][live], V) - V * lam[:, None, :]).max((1, 2))
    note('residual', res, (1e-12 + 4 * ulp) * lmax)
    if not f32:
        check_v0(V[:, :, 0], lam[:, 0], {f: ref[f][live] for f in ('lam', 'cov', 'v0')}, norm_tol=1e-14)
    # normals: -sign(dir . v0) v0 of the device's own v0, exactly (the kernel takes the sign of the unrounded dot product: a stored
    # float32 v0 reproduces it unless the product is within rounding of zero)
    v0, nrm = o['eigvecs'][:, :, 0], o['normals']
    with np.errstate(invalid='ignore'):
        c = (dirs * v0).sum(1)
        sure = live & (np.abs(c) > 1e-6)
    assert np.array_equal(nrm[sure], (-np.sign(c)[:, None] * v0)[sure])
    assert np.all((dirs * nrm).sum(1)[sure] < 0)
    # against the reference wherever v0 is defined: three distinct points or more (features_cases keeps their spectra separated)
    sep = live & (ref['distinct'] >= 3)
    absdot = np.abs((dirs * nrm).sum(1))
    note('absdot', np.abs(absdot - ref['absdot'])[sep], np.full(int(sep.sum()), 1e-5 if f32 else 1e-9))
    ang = sep & (ref['absdot'] < 0.999)
    note('inc_angles', np.abs(o['inc_angles'][:, 0] - ref['inc'])[ang], np.full(int(ang.sum()), 1e-7))


def _report(tag, worst):
    print('%s  worst error / bound: %s' % (tag, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------------------------------------------------
# A. forward against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [3, 4])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', cases.FWD_TILED + cases.FWD_GENERAL, ids=_id)
def test_forward_vs_reference(dev, case, dtype, stride):
    """All six outputs, the saved tensors and the weights of one call, through features_fwd_tile_kernel where k is compiled in and,
    with dc_features_set_tiled(0) or any other k, through features_fwd_kernel; the kernel that ran is asserted by name."""
    n, k, kind = case
    x, dirs, tab, info = cases.make_case(*case)
    ref = FR.forward(*case)
    f32 = dtype == np.float32
    xd, dd, nd = _points(x, dtype, stride, dev), t(dirs.astype(dtype), dev), t(tab.copy(), dev)
    for tiled in ((1, 0) if k in TILED_K else (0,)):
        o, _, name = _forward(xd, nd, dd, tiled)
        assert name.startswith(_kernel(tiled)), name
        worst = {}
        try:
            _check_forward(o, ref, x, dirs, f32, worst)
        finally:
            _report('forward %-16s %s stride %d %-7s' % (_id(case), np.dtype(dtype).name, stride, 'tiled' if tiled else 'general'), worst)


def test_forward_explicit_mean_weights(dev):
    """Explicit mean weights take the general kernel: the mean is the weighted one, everything else as with validity weights."""
    case = (129, 10, 'designed')
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)
    w = FR.mean_weights(*case)
    for dtype in (np.float64, np.float32):
        o, _, name = _forward(_points(x, dtype, 3, dev), t(tab.copy(), dev), t(dirs.astype(dtype), dev), 1, mean_weights=t(w.astype(dtype), dev))
        assert name.startswith('features_fwd_kernel<'), name
        worst = {}
        _check_forward(o, ref, x, dirs, dtype == np.float32, worst, mean_ref=FR.weighted_mean(x, tab, w))
        _report('forward weighted mean %s' % np.dtype(dtype).name, worst)


# ---------------------------------------------------------------------------------------------------------------------
# B. invariances, bit for bit: each pair is the same kernel doing the same arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', [(129, 10, 'designed'), (65, 4, 'designed'), (577, 16, 'per_wave'), (256, 5, 'designed')], ids=_id)
def test_forward_invariances(dev, case, dtype):
    """(1) Every single-output and two-output `want` subset against the all-outputs call: the outputs pass through one LDS region in
    turn, so a subset changes the hand-over sequence.  (2) Stride 4 with 1e30 in the fourth column against stride 3.  (3) Points
    renumbered, the table's rows permuted with them: nvalid and the weights gathered back (summation order changes the rest).  On both
    routes; whether the two routes agree with each other bit for bit is printed, not asserted."""
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    x3, x4, dd, nd = _points(x, dtype, 3, dev), _points(x, dtype, 4, dev, fill=1e30), t(dirs.astype(dtype), dev), t(tab.copy(), dev)
    rng = np.random.default_rng(n + k)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    ptab = np.where(tab[perm] >= 0, inv[np.where(tab[perm] >= 0, tab[perm], 0)], -1).astype(np.int32)
    xp, dp, npd = _points(x[perm], dtype, 3, dev), t(dirs[perm].astype(dtype), dev), t(ptab, dev)
    pd = torch.as_tensor(perm, device=dev)
    full = {}
    for tiled in ((1, 0) if k in TILED_K else (0,)):
        _, base, name = _forward(x3, nd, dd, tiled)
        assert name.startswith(_kernel(tiled)), name
        full[tiled] = base
        subsets = [(f,) for f in ALL] + list(itertools.combinations(ALL, 2))
        for want in subsets:
            _, sub, _ = _forward(x3, nd, dd, tiled, want=want, saved=False, weights=False)
            for f in ALL:
                assert (sub[f] is not None) == (f in want)
                if f in want:
                    assert _same_bits(sub[f], base[f]), (want, f, tiled)
        _, sub, _ = _forward(x3, nd, None, tiled, want=(), saved=True, weights=True)
        for f in ('nvalid', 'cmean', 'invd', 'weights'):
            assert _same_bits(sub[f], base[f]), ('saved only', f, tiled)
        _, s4, _ = _forward(x4, nd, dd, tiled)
        for f, v in base.items():
            assert _same_bits(s4[f], v), ('stride 4', f, tiled)
        _, pp, _ = _forward(xp, npd, dp, tiled)
        assert _same_bits(pp['nvalid'], base['nvalid'][pd]) and _same_bits(pp['weights'], base['weights'][pd])
    if len(full) == 2:
        print('invariances %-16s %s: tiled and general agree bit for bit in: %s' % (
            _id(case), np.dtype(dtype).name, ', '.join(f for f, v in full[1].items() if _same_bits(v, full[0][f])) or 'nothing'))


# ---------------------------------------------------------------------------------------------------------------------
# C. alignment fallback and stray writes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['points', 'dirs', 'table'])
def test_unaligned_view_takes_the_general_kernel(dev, which):
    """One operand as a big[1:] view -- float32 rows of three start 12 B off, int32 rows of ten 40 B off, neither a multiple of 16 B
    -- must leave the tiled kernel (it reads and writes 16-B words) for features_fwd_kernel, with the results within the bounds."""
    case = (129, 10, 'designed')
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)

    def view(a, off):
        if not off:
            return t(a.copy(), dev)
        v = t(np.concatenate([np.zeros((1,) + a.shape[1:], dtype=a.dtype), a]), dev)[1:]
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v

    xd = view(x.astype(np.float32), which == 'points')
    dd = view(dirs.astype(np.float32), which == 'dirs')
    nd = view(tab, which == 'table')
    o, _, name = _forward(xd, nd, dd, 1)
    assert name.startswith('features_fwd_kernel<'), name
    worst = {}
    _check_forward(o, ref, x, dirs, True, worst)
    _report('unaligned %s' % which, worst)


_PAD = 64                                   # elements: 256 B and more, so that every window stays 16-B aligned


def _window(count, ttype, dev, canary):
    buf = torch.full((_PAD + count + _PAD,), canary, dtype=ttype, device=dev)
    win = buf[_PAD:_PAD + count]
    assert win.data_ptr() % 16 == 0
    return buf, win


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('n,k', [(n, k) for n in (1, 63, 65, 129) for k in (4, 16)])
def test_no_store_outside_the_outputs(dev, n, k, dtype):
    """dc_features_fwd called directly with every output a 16-B aligned window inside a larger buffer of canaries (ops.features_fwd
    allocates exact sizes, where a store by an idle lane of the last wavefront would go unseen): the canaries before and after every
    output are untouched on both routes, and the windows hold what ops.features_fwd returns, bit for bit."""
    from depth_correction_amd import _native as nv
    kind = 'full' if n < 64 else 'designed'
    x, dirs, tab, _ = cases.make_case(n, k, kind)
    tt = _tt(dtype)
    xd, dd, nd = _points(x, dtype, 3, dev), t(dirs.astype(dtype), dev), t(tab.copy(), dev)
    counts = dict(mean=3, cov=9, eigvals=3, eigvecs=9, normals=3, inc_angles=1, nvalid=1, weights=k, cmean=3, invd=1)
    for tiled in (1, 0):
        _, base, _ = _forward(xd, nd, dd, tiled)
        win = {f: _window(n * c, torch.int32 if f == 'nvalid' else tt, dev, -77 if f == 'nvalid' else -12345.6789) for f, c in counts.items()}
        p = lambda f: nv.ptr(win[f][1])
        with _routed(tiled) as launched:
            nv.check(nv.lib().dc_features_fwd(nv.ptr(xd), 3, nv.dtype_code(xd), nv.ptr(nd), n, k, None, 0.0, nv.ptr(dd), p('mean'), p('cov'),
                                              p('eigvals'), p('eigvecs'), p('normals'), p('inc_angles'), p('nvalid'), p('weights'),
                                              p('cmean'), p('invd'), nv.stream_ptr()), 'dc_features_fwd')
            name = launched()
        assert name.startswith(_kernel(tiled)), name           # a window off the 16-B grid would fall back without a word
        torch.cuda.synchronize()
        for f, (buf, w) in win.items():
            canary = buf.new_full((_PAD,), -77 if f == 'nvalid' else -12345.6789)
            assert torch.equal(buf[:_PAD], canary), ('before', f, tiled)
            assert torch.equal(buf[-_PAD:], canary), ('after', f, tiled)
            assert _same_bits(w, base[f].reshape(-1)), (f, tiled)


# ---------------------------------------------------------------------------------------------------------------------
# D. backward against the closed form
# ---------------------------------------------------------------------------------------------------------------------
def _g(a, dtype, dev):
    return None if a is None else t(a.astype(dtype), dev)


@pytest.mark.parametrize('stride', [3, 4])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', cases.BWD + cases.BWD_HUB, ids=_id)
def test_backward_vs_closed_form(dev, case, dtype, stride):
    """grad_points of dc_features_bwd, point by point, against the closed form in float64 (features_reference.backward): called
    directly with cmean, invd, nvalid and eigvecs of the device's forward and g_mean alone, an asymmetric g_cov alone, g_eig alone and
    all three (None for the absent ones; the hub of in-degree n, 'hub_all': the first two), then through
    autograd.neighborhood_features(...).backward().  float64: within 1e-9 of max |ref|; float32: within 1e-5.  Exactly zero: a point nobody lists, the fourth column of a stride-4 gradient; and the NaN record
    of the row without a valid member reaches no point.

    float32, measured on an MI355X over these cases: the device's error is 2.0e-8 to 2.9e-6 of max |ref|, the same expression
    evaluated in float32 numpy on the host errs 5.2e-8 to 2.9e-6; the ratio device / host lies between 0.03 (g_mean alone: the kernel
    sums in float64 and rounds once) and 3.3, and is 1.00 where the error is largest (2305 points, k = 4, full table, g_cov alone:
    2.86e-6 against 2.85e-6 -- the rounding of the stored cmean to float32 in x_j - cmean -- which is 0.286 of the bound).  float64:
    2.9e-15 at most.
    (The test prints both.)"""
    from depth_correction_amd import ops
    from depth_correction_amd.autograd import NeighborhoodGraph, neighborhood_features
    n, k, kind = case
    x, dirs, tab, info = cases.make_case(*case)
    ref = FR.forward(*case)
    f32 = dtype == np.float32
    tol = 1e-5 if f32 else 1e-9
    xd, nd = _points(x, dtype, stride, dev), t(tab.copy(), dev)
    _, f, _ = _forward(xd, nd, None, 1, want=('mean', 'cov', 'eigvals', 'eigvecs'))
    cp, cs = ops.knn_transpose(nd)
    indeg = np.bincount(tab[tab >= 0], minlength=n)
    if kind == 'designed':
        assert indeg[info['orphan']] == 0 and indeg[info['hub']] >= 0.5 * n
    if kind == 'hub_all':
        assert indeg[info['hub']] >= n

    def check(gp, gs, want, tag):
        gp = npy(gp).astype(np.float64)
        assert gp.shape == (n, stride) and np.isfinite(gp).all(), tag
        if stride == 4:
            assert np.all(gp[:, 3] == 0), tag
        assert np.all(gp[indeg == 0, :3] == 0), tag
        if not np.abs(want).max():               # a single centre: x_j - cmean = 0 exactly
            assert np.all(gp == 0), tag
            return
        err = np.abs(gp[:, :3] - want).max() / np.abs(want).max()
        line = 'backward %-16s %s stride %d %-13s error %.2e of max |ref| (%.3f of the bound)' % (
            _id(case), np.dtype(dtype).name, stride, tag, err, err / tol)
        if f32:
            host = FR.backward(x, tab, ref['cov'], ref['cmean'], *gs, dtype=np.float32)
            herr = np.abs(host - want).max() / np.abs(want).max()
            line += '; float32 on the host %.2e, ratio %.2f' % (herr, err / herr if herr else np.inf)
        print(line)
        assert err <= tol, (tag, err)

    for which in ('mean', 'cov') if kind == 'hub_all' else ('mean', 'cov', 'eig', 'all'):
        gs = FR.upstream(n, k, kind, which)
        want = FR.backward(x, tab, ref['cov'], ref['cmean'], *gs)
        gm, gc, ge = (_g(a, dtype, dev) for a in gs)
        gp = ops.features_bwd(xd, cp, cs, f['cmean'], f['invd'], f['nvalid'], eigvecs=f['eigvecs'], grad_mean=gm, grad_cov=gc,
                              grad_eigvals=ge)
        check(gp, gs, want, which)
        # the same through the autograd bridge: L = <g_mean, mean> + <g_cov, cov> + <g_eig, eigvals> (the row without a valid member
        # makes L itself NaN; its gradient is not)
        xa = xd.clone().requires_grad_(True)
        mean, cov, lam = neighborhood_features(xa, NeighborhoodGraph(nd, nbr=nd))[:3]
        loss = sum((g * o).sum() for g, o in ((gm, mean), (gc, cov), (ge, lam)) if g is not None)
        loss.backward()
        check(xa.grad, gs, want, which + ' (autograd)')


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_backward_with_explicit_mean_weights_is_refused(dev, dtype):
    """dc_features_bwd spreads g_mean / W over a row's edges, which is the derivative of the mean only for validity weights; with
    explicit mean weights the forward computes sum w_ij x_j / sum w_ij, whose derivative is w_ij g_mean / sum_q w_iq per edge (the
    reference this test computes; g_mean / W, which the kernels return whatever the weights, misses it by 0.41 of max |grad| here).
    The contract: the autograd bridge refuses a gradient through that mean with NotImplementedError, as it refuses `scale`; a loss
    that never touches the mean still runs (the covariance and the eigenvalues do not depend on the mean weights) and meets the
    closed form; the validity-weight path is unchanged."""
    from depth_correction_amd.autograd import NeighborhoodGraph, neighborhood_features
    case = (65, 10, 'designed')
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)
    f32 = dtype == np.float32
    tol = 1e-5 if f32 else 1e-9
    w = FR.mean_weights(*case)
    xd, nd, wd = _points(x, dtype, 3, dev), t(tab.copy(), dev), t(w.astype(dtype), dev)
    graph = NeighborhoodGraph(nd, nbr=nd)
    gm, gc, ge = FR.upstream(n, k, kind, 'all')
    weighted = FR.backward(x, tab, ref['cov'], ref['cmean'], gm, None, None, mean_weights=w)
    plain = FR.backward(x, tab, ref['cov'], ref['cmean'], gm, None, None)
    off = np.abs(plain - weighted).max() / np.abs(weighted).max()
    print('explicit mean weights: the validity-weight formula is off by %.2f of max |grad|' % off)
    assert off > 0.05                            # these inputs tell the two contracts apart
    # through the mean: refused
    xa = xd.clone().requires_grad_(True)
    mean = neighborhood_features(xa, graph, mean_weights=wd)[0]
    live = t(ref['nvalid'] > 0, dev)
    scale = np.abs(x).max() + np.sqrt(ref['lam'][ref['nvalid'] > 0, 2].max())
    assert np.abs(npy(mean).astype(np.float64) - FR.weighted_mean(x, tab, w))[npy(live)].max() <= (ULP32 if f32 else 2.0 ** -50) * scale
    with pytest.raises(NotImplementedError):
        (_g(gm, dtype, dev) * mean)[live].sum().backward()
    assert xa.grad is None
    # not through the mean: runs, and the mean weights do not enter
    xa = xd.clone().requires_grad_(True)
    _, cov, lam = neighborhood_features(xa, graph, mean_weights=wd)[:3]
    ((_g(gc, dtype, dev) * cov)[live].sum() + (_g(ge, dtype, dev) * lam)[live].sum()).backward()
    want = FR.backward(x, tab, ref['cov'], ref['cmean'], None, gc, ge)
    err = np.abs(npy(xa.grad).astype(np.float64) - want).max() / np.abs(want).max()
    print('explicit mean weights, loss of cov and eigvals: error %.2e of max |ref|' % err)
    assert err <= tol
    # validity weights: the mean's gradient as before
    xa = xd.clone().requires_grad_(True)
    mean = neighborhood_features(xa, graph)[0]
    (_g(gm, dtype, dev) * mean)[live].sum().backward()
    err = np.abs(npy(xa.grad).astype(np.float64) - plain).max() / np.abs(plain).max()
    assert err <= tol


def test_depth_cloud_with_explicit_weights_meets_the_same_contract(dev):
    """The refusal where users meet it: a DepthCloud whose `weights` are not the validity tensor hands them to the forward as mean
    weights (DepthCloud._features).  A loss through its `mean` raises, a loss through its `cov` runs and meets the closed form, and
    with the validity weights update_neighbors would have written the mean's gradient is the closed form's."""
    from depth_correction_amd import ops
    from depth_correction_amd.depth_cloud import DepthCloud
    case = (65, 10, 'designed')
    n, k, kind = case
    x, dirs, tab, _ = cases.make_case(*case)
    ref = FR.forward(*case)
    gm, gc, _ = FR.upstream(n, k, kind, 'all')
    live = t(ref['nvalid'] > 0, dev)
    nd = t(tab.copy(), dev)

    def cloud(weights):
        dc = DepthCloud.from_points(t(x.copy(), dev))
        dc.points = t(x.copy(), dev).requires_grad_(True)
        dc.neighbors = nd.long()
        dc.weights = weights
        return dc

    dc = cloud(t(FR.mean_weights(*case), dev)[..., None])
    dc.update_mean()
    assert dc.mean.requires_grad
    with pytest.raises(NotImplementedError):
        (t(gm, dev) * dc.mean)[live].sum().backward()
    dc.update_cov()
    (t(gc, dev) * dc.cov)[live].sum().backward()
    want = FR.backward(x, tab, ref['cov'], ref['cmean'], None, gc, None)
    assert np.abs(npy(dc.points.grad) - want).max() <= 1e-9 * np.abs(want).max()
    valid = ops.valid_weights(nd)
    valid._dc_validity = True
    dc = cloud(valid)
    dc.update_mean()
    (t(gm, dev) * dc.mean)[live].sum().backward()
    want = FR.backward(x, tab, ref['cov'], ref['cmean'], gm, None, None)
    assert np.abs(npy(dc.points.grad) - want).max() <= 1e-9 * np.abs(want).max()
