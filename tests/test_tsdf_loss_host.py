"""The loss against the fused volume on the host (no GPU): the rules of csrc/dc_tsdf_loss_math.h through their host build
(libdc_hostcheck.so, the header the kernels inline) against tests/tsdf_loss_reference.py and the hand-written figures of
tests/tsdf_loss_cases.py; the subtraction of a scan's own volume against explicit re-fusion of the other scans; the closed-form
gradient against central differences; and the method itself: the re-fuse / gradient-descent loop recovers a depth bias.

dc_host_tsdf_loss adds the points one after the other in index order, which is NOT the kernels' order: its totals are held to the
extended-precision oracle within tsdf_loss_reference.bound, its per-point outputs to the bit.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_loss_cases as C  # noqa: E402
import tsdf_loss_reference as L  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
import tsdf_track_reference as K  # noqa: E402
from tsdf_loss_cases import COUNTS, DTYPES, MODELS, assert_within_bounds, random_scene  # noqa: E402,F401

KIND_CODES = {None: 0, 'Polynomial': 1, 'ScaledPolynomial': 2}


def host_lib():
    """libdc_hostcheck.so with the loss exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_tsdf_loss'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_tsdf_loss_point.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, f64, f64, ci, vp, ci, f64, vp, vp, vp, vp]
    lib.dc_host_tsdf_loss.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, f64, f64, ci, vp, vp, vp, vp, vp, vp, ci, i64,
                                      vp, vp, ci, ci, ci, vp, vp, ci, ci, f64, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _table(vol):
    return np.ascontiguousarray(vol.keys, np.uint64), np.ascontiguousarray(vol.slots, np.int32)


def host_point(lib, total, own, x, min_count=1, squared=True, max_residual=None):
    """dc_host_tsdf_loss_point at the points x [m, 3] -> dict(cls, phi, grad, l, dl)."""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    m = x.shape[0]
    keys, slots = _table(total)
    okeys, oslots = _table(own) if own is not None else (None, None)
    mr = total.trunc if max_residual is None else max_residual
    out = dict(cls=np.zeros(m, np.uint8), phi=np.zeros(m), grad=np.zeros((m, 3)), l=np.zeros(m), dl=np.zeros((m, 3)))
    for j in range(m):
        phi, l, grad, dl = np.zeros(1), np.zeros(1), np.zeros(3), np.zeros(3)
        args = (None, None, 0, 1, None, None) if own is None else (_p(okeys), _p(oslots), own.n_blocks, own.capacity, _p(own.sum), _p(own.count))
        if own is not None and own.n_blocks == 0:              # a table without keys is still a table
            args = (_p(own.sum), _p(own.sum)) + args[2:]
        out['cls'][j] = lib.dc_host_tsdf_loss_point(_p(keys), _p(slots), total.n_blocks, total.capacity, _p(total.sum), _p(total.count), *args,
                                                    _p(total.origin), total.voxel, total.trunc, min_count, _p(x[j].copy()), int(squared), mr,
                                                    _p(phi), _p(grad), _p(l), _p(dl))
        out['phi'][j], out['grad'][j], out['l'][j], out['dl'][j] = phi[0], grad, l[0], dl
    return out


def host_loss(lib, total, owns, scans, poses, kind=None, w=(), e=(), mask=None, squared=True, max_residual=None, min_count=1,
              want_exponent=True, dtype='float64'):
    """dc_host_tsdf_loss -> dict(loss, used, gated, unobserved, invalid, gw, ge, gT, value, cls, x)."""
    npdt, code = DTYPES[dtype]
    cat = lambda k, width: np.ascontiguousarray(np.concatenate([np.asarray(c[k]).reshape(-1, width) for c in scans]).astype(npdt))
    vps, dirs, depth, inc = cat('vps', 3), cat('dirs', 3), cat('depth', 1), cat('inc', 1)
    lmask = np.ascontiguousarray(np.concatenate([np.asarray(c['lmask']) for c in scans]).astype(np.uint8))
    sizes = [len(c['depth']) for c in scans]
    n, ns = sum(sizes), len(scans)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P12 = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, :].reshape(-1, 12))
    w, e = np.ascontiguousarray(w, np.float64), np.ascontiguousarray(e, np.float64)
    nt = 0 if kind is None else w.size
    keys, slots = _table(total)
    own_args = (None, None, None, 0, 0, None, None)
    if owns is not None:
        ok, osl, optr, osum, ocnt = L.own_tables(owns)
        own_args = (_p(ok) if ok.size else _p(osum), _p(osl) if osl.size else _p(osum), _p(optr), ok.size, osum.shape[0], _p(osum), _p(ocnt))
        keep = (ok, osl, optr, osum, ocnt)                      # noqa: F841 (alive during the call)
    m8 = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    out = np.full(5 + 2 * nt + 12 * ns, 7.0)
    value, flag, x = np.full(n, 7.0), np.full(n, 7, np.uint8), np.full((n, 3), 7.0)
    mr = total.trunc if max_residual is None else max_residual
    rc = lib.dc_host_tsdf_loss(_p(keys), _p(slots), _p(np.array([total.n_blocks], np.int64)), total.capacity, _p(total.sum), _p(total.count),
                               *own_args, _p(total.origin), total.voxel, total.trunc, min_count, _p(vps), _p(dirs), _p(depth), _p(inc),
                               _p(lmask), _p(m8), code, n, _p(ptr), _p(P12), ns, KIND_CODES[kind], nt, _p(w) if nt else None,
                               _p(e) if nt else None, int(want_exponent), int(squared), mr, _p(value), _p(flag), _p(x), _p(out))
    assert rc == 0, rc
    return dict(loss=out[0], used=int(out[1]), gated=int(out[2]), unobserved=int(out[3]), invalid=int(out[4]), gw=out[5:5 + nt],
                ge=out[5 + nt:5 + 2 * nt], gT=out[5 + 2 * nt:].reshape(ns, 3, 4), value=value, cls=flag, x=x)


# ---- 1. the designed points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [True, False])
def test_designed_points_host_equals_oracle_and_hand(lib, squared):
    total, own_a, own_none = C.volumes()
    owns = {'A': own_a, 'none': own_none, None: None}
    seen = set()
    for case in C.point_cases():
        own = owns[case['own']]
        x = np.array([case['x']])
        got = host_point(lib, total, own, x, case['min_count'], squared, case['max_residual'])
        smp = L.sample_minus(total, own, x, case['min_count'])
        cls = L.classify(smp, case['max_residual'])
        name = case['name']
        assert got['cls'][0] == cls[0] == case['cls'], name
        assert np.array_equal(got['phi'], smp['value'], equal_nan=True) and np.array_equal(got['grad'], smp['grad']), name
        assert np.array_equal(got['phi'], [case['phi']], equal_nan=True) and np.array_equal(got['grad'][0], case['grad']), name
        if case['cls'] == C.USED:
            l, dl = L.term(smp['value'], smp['grad'], squared)
            assert np.array_equal(got['l'], l) and np.array_equal(got['dl'], dl), name
            phi, grad = case['phi'], np.array(case['grad'])
            hand_l = phi * phi if squared else abs(phi)
            hand_dl = (2.0 * phi if squared else float(np.sign(phi))) * grad
            assert got['l'][0] == hand_l and np.array_equal(got['dl'][0], hand_dl), name
        else:
            assert got['l'][0] == 0.0 and not got['dl'].any(), name
        if own is None:                                        # without an own table: the tracker's sample, to the bit
            ref = K.sample(total, x, None, case['min_count'])
            assert np.array_equal(got['phi'], ref['value'], equal_nan=True) and np.array_equal(got['grad'], ref['grad']), name
        seen.add(case['cls'])
    assert seen == {C.USED, C.INVALID, C.UNOBSERVED, C.GATED}
    zero = host_point(lib, total, None, np.array([C.X_ZERO]), squared=False)
    assert zero['cls'][0] == C.USED and zero['l'][0] == 0.0 and not zero['dl'].any()          # |phi| form at phi = 0: no direction


@pytest.mark.parametrize('squared', [True, False])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_designed_call(lib, dtype, squared):
    """Three scans, the middle one empty, own volumes per scan, a masked and a NaN point: per-point outputs by hand, totals by hand."""
    case = C.call_case(DTYPES[dtype][0])
    got = host_loss(lib, case['total'], case['owns'], case['scans'], case['poses'], mask=case['mask'], squared=squared, dtype=dtype)
    assert np.array_equal(got['cls'], case['cls'])
    seen = (case['cls'] == C.USED) | (case['cls'] == C.GATED)
    assert np.array_equal(got['value'][seen], case['phi'][seen]) and np.isnan(got['value'][~seen]).all()
    assert np.isnan(got['x'][case['cls'] == C.MASKED]).all()
    used = case['cls'] == C.USED
    phi, grad = case['phi'][used], case['grad'][used]
    l = phi * phi if squared else np.abs(phi)
    assert got['used'] == used.sum() and got['unobserved'] == 3 and got['invalid'] == 1 and got['gated'] == 0
    assert got['loss'] == l.sum() / used.sum()                 # dyadic figures: every sum is exact
    ref = L.loss(case['total'], case['owns'], case['scans'], case['poses'], mask=case['mask'], squared=squared, x=got['x'])
    assert np.array_equal(ref['cls'], case['cls'])
    assert_within_bounds(got, ref, 'designed call')
    dl = (2.0 * phi if squared else np.sign(phi))[:, None] * grad
    n0 = len(case['scans'][0]['depth'])
    first = np.nonzero(used)[0] < n0
    assert np.array_equal(got['gT'][0][:, 3], dl[first].sum(axis=0) / used.sum())
    assert np.array_equal(got['gT'][2][:, 3], dl[~first].sum(axis=0) / used.sum()) and not got['gT'][1].any()


# ---- 2. the random posed scene of the sparse tests --------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'ScaledPolynomial', 'Polynomial'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_random_scene_host_equals_oracle(lib, dtype, kind):
    scans, poses, total, owns, _ = random_scene(dtype)
    w, e = MODELS[kind]
    ratios = []
    for with_own in (True, False):
        for squared in (True, False):
            mr = None if squared else 0.2                      # (the truncation gates nothing here; 0.2 m does)
            got = host_loss(lib, total, owns if with_own else None, scans, poses, kind, w, e, squared=squared, max_residual=mr, dtype=dtype)
            ref = L.loss(total, owns if with_own else None, scans, poses, kind, w, e, squared=squared, max_residual=mr, x=got['x'])
            assert np.array_equal(got['cls'], ref['cls']) and np.array_equal(got['value'], ref['value'], equal_nan=True)
            assert ref['used'] > 300 and ref['unobserved'] > 0 and ref['invalid'] > 0 and (ref['gated'] > 0) == (not squared)
            ratios.append(assert_within_bounds(got, ref, (dtype, kind, with_own, squared)))
            # the points themselves: the oracle's fp64 points agree with the host's to rounding
            mine = np.concatenate([L.posed_points(c, T, kind, w, e) for c, T in zip(scans, poses)])
            fin = np.isfinite(mine).all(axis=1)
            assert np.array_equal(fin, np.isfinite(got['x']).all(axis=1)) and np.abs(mine[fin] - got['x'][fin]).max() < 1e-14
    # sample and term, point by point, to the bit
    off = 0
    for s, c in enumerate(scans):
        n = len(c['depth'])
        x = got['x'][off:off + n]
        pt = host_point(lib, total, owns[s], x)
        smp = L.sample_minus(total, owns[s], x)
        assert np.array_equal(pt['phi'], smp['value'], equal_nan=True) and np.array_equal(pt['grad'], smp['grad'])
        assert np.array_equal(pt['cls'], L.classify(smp, total.trunc))
        u = pt['cls'] == C.USED
        l, dl = L.term(smp['value'][u], smp['grad'][u], True)
        assert np.array_equal(pt['l'][u], l) and np.array_equal(pt['dl'][u], dl)
        off += n
    assert (S.key_block(total.keys) < 0).any()                # negative blocks
    print('%s %s: largest |host - oracle| / bound %.3g' % (dtype, kind, max(ratios)))


# ---- 3. subtraction equals re-fusion ------------------------------------------------------------------------------------------------
def test_subtraction_equals_refusion(lib):
    scans, poses, total, owns, fuse = random_scene('float64')
    assert len(scans) == 4
    n_points = 0
    for s in range(4):
        others = fuse([j for j in range(4) if j != s])
        # every voxel of every block of the total: total - own == the volume of the other three
        blocks = S.key_block(total.keys)
        idx = (blocks[:, None, :] * 8 + np.stack(np.unravel_index(np.arange(512), (8, 8, 8)), axis=1)[None, :, :]).reshape(-1, 3)
        _, st, ct = L._gather(total, idx)
        _, so, co = L._gather(owns[s], idx)
        have, sr, cr = L._gather(others, idx)
        assert np.array_equal(st - so, sr) and np.array_equal(ct - co, cr)
        assert set(others.keys.tolist()) <= set(total.keys.tolist()) and (cr[~have] == 0).all()
        # every point's sample, both routes, oracle and host
        x = np.concatenate([L.posed_points(c, T, None, (), ()) for c, T in zip(scans, poses)])
        a = L.sample_minus(total, owns[s], x)
        b = K.sample(others, x)
        for k in ('value', 'grad', 'flag'):
            assert np.array_equal(a[k], b[k], equal_nan=True), (s, k)
        h = host_point(lib, total, owns[s], x)
        assert np.array_equal(h['phi'], b['value'], equal_nan=True) and np.array_equal(h['grad'], b['grad'])
        assert np.array_equal(h['cls'], L.classify(b, total.trunc))
        n_points += int((b['flag'] == 0).sum())
        assert (a['flag'] == 0).sum() < (K.sample(total, x)['flag'] == 0).sum()          # the exclusion takes something away
    assert n_points > 2000


# ---- 4. the closed-form gradient against central differences ----------------------------------------------------------------------
FD_BAR = 3e-9            # a decade above the agreement reached (see the test)


def test_gradient_against_central_differences():
    """At a frozen volume, points at least 1e-4 voxels from any cell face (asserted), steps of 1e-6 that cross no face and no gate
    (asserted: the classes do not change, the face margin stays positive).  The loss is a cubic in x inside a cell, so a central
    difference with step h is off by O(h^2) times its third derivative plus the loss's rounding over h, which is an ABSOLUTE error:
    the differences are therefore measured against the largest entry of the call's whole gradient.  Agreement reached over the
    weights, the exponents and the poses of four scans: 2.9e-10 (squared form; largest |difference| 1.5e-12 at a largest entry of
    5.2e-3) and 2.1e-10 (|phi| form; 6.1e-12 at 2.9e-2).  The bar is a decade above: 3e-9."""
    scans, poses, total, owns, _ = random_scene('float64')
    kind, (w, e) = 'ScaledPolynomial', MODELS['ScaledPolynomial']
    w, e = np.array(w), np.array(e)
    x = np.concatenate([L.posed_points(c, T, kind, w, e) for c, T in zip(scans, poses)])
    q = (x - total.origin) / total.voxel - 0.5
    with np.errstate(invalid='ignore'):
        mask = np.isfinite(q).all(axis=1) & (np.abs(q - np.rint(q)) >= 1e-4).all(axis=1)
    h = 1e-6
    for squared in (True, False):
        ref = L.loss(total, owns, scans, poses, kind, w, e, mask=mask, squared=squared)
        assert ref['face_margin'] >= 1e-4 and ref['used'] > 300
        scale = max(np.abs(ref[name]).max() for name in ('gw', 'ge', 'gT'))
        worst = 0.0
        for name, size in (('gw', 2), ('ge', 2), ('gT', 12 * len(scans))):
            num = np.zeros(size)
            for k in range(size):
                w_, e_ = [w.copy(), w.copy()], [e.copy(), e.copy()]
                T_ = [poses.copy(), poses.copy()]
                for side, step in enumerate((-h, +h)):
                    if name == 'gw':
                        w_[side][k] += step
                    elif name == 'ge':
                        e_[side][k] += step
                    else:
                        T_[side][k // 12, (k % 12) // 4, k % 4] += step
                lo, hi = (L.loss(total, owns, scans, T_[i], kind, w_[i], e_[i], mask=mask, squared=squared) for i in (0, 1))
                assert np.array_equal(lo['cls'], ref['cls']) and np.array_equal(hi['cls'], ref['cls'])
                assert min(lo['face_margin'], hi['face_margin']) > 5e-5
                num[k] = (hi['loss'] - lo['loss']) / (2 * h)
            err = np.abs(num - ref[name].reshape(-1)).max()
            print('squared %s %s: largest |central difference - closed form| %.3g (largest entry %.3g, of the whole gradient %.3g)'
                  % (squared, name, err, np.abs(ref[name]).max(), scale))
            worst = max(worst, err / scale)
        print('squared %s: agreement %.3g of the largest gradient entry (bar %.3g)' % (squared, worst, FD_BAR))
        assert worst <= FD_BAR


# ---- 5. the method: the re-fuse / gradient-descent loop recovers the bias -----------------------------------------------------------
VOXEL, TRUNC = 0.1, 0.3
LR = C.LOOP_LR           # plain gradient descent on the mean of phi^2: about the Gauss-Newton step, 1 / mean (2 (dphi/dw)^2)


def recovery(leave_one_out, steps, lr=LR):
    scans, poses = L.box_scene()
    assert sum(len(c['depth']) for c in scans) > 9000
    w, history = 0.0, []
    for _ in range(steps):
        w, ref = L.descent_step(scans, poses, w, VOXEL, TRUNC, leave_one_out, lr)
        history.append((w, float(np.sqrt(ref['loss']))))
    return history


def test_recovery_leave_one_out():
    """Conditions on the method: from w = 0 the leave-one-out loop ends at 0.8 x 0.05 or beyond."""
    hist = recovery(True, 16)
    print('leave-one-out: w %s; rms phi %.1f -> %.1f mm' % (' '.join('%.4f' % w for w, _ in hist[::2]), 1e3 * hist[0][1], 1e3 * hist[-1][1]))
    assert hist[-1][0] >= 0.8 * L.TRUE_W and abs(hist[-1][0] - hist[-2][0]) < 2e-4
    assert hist[-1][1] < hist[0][1]


def test_summation_order_sensitivity_of_the_loop():
    """The figure the device loop's bar (tests/test_gpu_tsdf_loss.py) is made of, recomputed over three orders of the gradient sum: no
    order moves the oracle's w of any of the six steps by more than the largest change recorded over 200 orders."""
    scans, poses = L.box_scene()

    def run(order):
        w, out = 0.0, []
        for _ in range(C.LOOP_STEPS):
            w, _ = L.descent_step(scans, poses, w, VOXEL, TRUNC, True, C.LOOP_LR, order=order)
            out.append(w)
        return np.array(out)
    base = run(None)
    worst = max(float(np.abs(run(seed) - base).max()) for seed in (5, 105, 199))
    print('largest change of w over three orders: %.3g (recorded over 200: %.3g)' % (worst, C.W_SENSITIVITY))
    assert base[-1] > 0.04 and worst <= C.W_SENSITIVITY


def test_recovery_all_scans():
    """The all-scans loop (every scan scored against a volume that holds it) ends at 0.5 x 0.05 or beyond, and below leave-one-out."""
    hist = recovery(False, 36)
    print('all scans: w %s; rms phi %.1f -> %.1f mm' % (' '.join('%.4f' % w for w, _ in hist[::4]), 1e3 * hist[0][1], 1e3 * hist[-1][1]))
    assert hist[-1][0] >= 0.5 * L.TRUE_W and abs(hist[-1][0] - hist[-2][0]) < 2e-4
    assert hist[-1][1] < hist[0][1]
