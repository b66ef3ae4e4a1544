"""The loss against the fused volume on the MI355X (csrc/dc_tsdf_loss.hip, ops.tsdf_loss, loss.TsdfTarget, loss.tsdf_loss, train() with
cfg.loss = 'tsdf_loss') against the numpy oracle of tests/tsdf_loss_reference.py, which tests/test_tsdf_loss_host.py holds to the
hand-written cases, to explicit re-fusion and to central differences.

Bars, all from reference quantities (nothing is tuned to the kernel):
  per point    value and flag bit-equal to the oracle sampled at the device's own x; x bit-equal to ops.points_fwd; without exclusion
               value and flag bit-equal to ops.tsdf_sparse_sample at x
  totals       counts equal; L and every gradient entry within 1.0 x (n + 16) 2^-53 sum |term| of the extended-precision oracle
               (tsdf_loss_reference.bound), n the points of the call
  fused vs. un-fused   COMPOSITION_ROUNDINGS = 16 times that bound plus tsdf_loss_reference.move_bound at 16 roundings: the tensor
               composition forms x with its own 13 roundings (the power, its product with w, the sum over the terms, 1 - bias, times
               d, times dir (3), plus vp, three products and two sums of the rotation, plus t), none fused, and adds the terms in
               torch's order
  loop         W_BAR = 2 000 x the largest change of the oracle's own w over 200 random orders of its gradient sum, measured on the
               CPU (DESIGN "Self-supervised training against the fused volume" has the figures)
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_loss_cases as C  # noqa: E402
import tsdf_loss_reference as L  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
from tsdf_loss_cases import COUNTS, MODELS, assert_within_bounds, random_scene  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP = {'float32': np.float32, 'float64': np.float64}
COMPOSITION_ROUNDINGS = 16
W_BAR = 2000 * C.W_SENSITIVITY   # 1.46e-13: see tsdf_loss_cases and DESIGN; tests/test_tsdf_loss_host.py recomputes the figure
MARGIN_FLOOR = 1e-9
_cache = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def tables(vol):
    """The oracle volume on the device as ops.TsdfTables."""
    from depth_correction_amd import ops
    cap = vol.capacity
    keys, slots = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    keys[:vol.n_blocks], slots[:vol.n_blocks] = vol.keys.view(np.int64), vol.slots
    return ops.TsdfTables(_t(keys), _t(slots), _t(np.array([vol.n_blocks], np.int64)), _t(vol.sum), _t(vol.count), vol.origin, vol.voxel,
                          vol.trunc)


def own_tables(owns):
    from depth_correction_amd import ops
    keys, slots, ptr, sm, cnt = L.own_tables(owns)
    return ops.TsdfOwnTables(_t(keys.view(np.int64)), _t(slots), _t(ptr), _t(sm), _t(cnt))


class Call(object):
    """Scans (dicts of numpy fields), poses, a total volume and own volumes on the device in one cloud dtype."""

    def __init__(self, scans, poses, total, owns, dtype):
        from depth_correction_amd import ops
        self.scans, self.poses, self.total, self.owns, self.dtype = scans, np.asarray(poses, np.float64), total, owns, dtype
        npdt = NP[dtype]
        cat = lambda k, width: np.concatenate([np.asarray(c[k]).reshape(-1, width) for c in scans]).astype(npdt)
        self.sizes = [len(c['depth']) for c in scans]
        self.n = sum(self.sizes)
        self.ps = ops.PointSet(_t(cat('vps', 3)), _t(cat('dirs', 3)), _t(cat('depth', 1).reshape(-1)), _t(cat('inc', 1).reshape(-1)),
                               _t(np.concatenate([np.asarray(c['lmask'], bool) for c in scans])))
        self.scan_ptr = _t(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64))
        self.poses12 = _t(self.poses[:, :3, :].reshape(-1, 12))
        self.tables = tables(total)
        self.own = None if owns is None else own_tables(owns)

    def model(self, kind):
        w, e = MODELS[kind]
        return (None, None, None) if kind is None else (kind, _t(np.array(w), torch.float64), _t(np.array(e), torch.float64))

    def run(self, kind=None, with_own=True, **kw):
        from depth_correction_amd import ops
        k, w, e = self.model(kind)
        out = ops.tsdf_loss(self.tables, self.ps, self.scan_ptr, self.poses12, k, w, e, own=self.own if with_own else None, **kw)
        torch.cuda.synchronize()
        return out

    def split(self, out, kind):
        o = out.cpu().numpy()
        nt, ns = (0 if kind is None else len(MODELS[kind][0])), len(self.sizes)
        assert o.shape == (5 + 2 * nt + 12 * ns,)
        return dict(loss=o[0], used=int(o[1]), gated=int(o[2]), unobserved=int(o[3]), invalid=int(o[4]), gw=o[5:5 + nt],
                    ge=o[5 + nt:5 + 2 * nt], gT=o[5 + 2 * nt:].reshape(ns, 3, 4))

    def reference(self, kind, x, with_own=True, **kw):
        w, e = MODELS[kind]
        return L.loss(self.total, self.owns if with_own else None, self.scans, self.poses, kind, w, e, x=x, **kw)

    def points64(self, kind):
        """The same fields in fp64 through the un-fused point kernel."""
        from depth_correction_amd import ops
        k, w, e = self.model(kind)
        f64 = lambda t: None if t is None else t.double().contiguous()
        sid = torch.repeat_interleave(torch.arange(len(self.sizes), device=DEV), _t(np.array(self.sizes))).to(torch.int32).contiguous()
        ps64 = ops.PointSet(f64(self.ps.vps), f64(self.ps.dirs), f64(self.ps.depth), f64(self.ps.inc), self.ps.lmask, sid)
        return ops.points_fwd(ps64, self.poses12, k, w, e)


def _random(dtype):
    if ('random', dtype) not in _cache:
        scans, poses, total, owns, _ = random_scene(dtype)
        _cache['random', dtype] = Call(scans, poses, total, owns, dtype)
    return _cache['random', dtype]


def _sizes(dtype):
    """Scans of 1, 127, 128, 129 and 0 points cut from scan 0 of the random scene (its pose for all of them), each with the volume of
    its own rays as its own volume; the total is the random scene's, which holds them all."""
    if ('sizes', dtype) not in _cache:
        scans, poses, total, _, _ = random_scene(dtype)
        src, parts, owns, off = scans[0], [], [], 0
        for n in (1, 127, 128, 129, 0):
            part = {k: (v[off:off + n] if isinstance(v, np.ndarray) else v) for k, v in src.items()}
            vol = S.SparseVolume(total.voxel, trunc=total.trunc, origin=total.origin, capacity=64)
            if n:
                S.fuse(vol, vps=part['vps'], dirs=part['dirs'], depth=part['depth'], pose=poses[0], mask=part['lmask'], **src['rules'])
            parts.append(part)
            owns.append(vol)
            off += n
        _cache['sizes', dtype] = Call(parts, np.stack([poses[0]] * 5), total, owns, dtype)
    return _cache['sizes', dtype]


# ---- 1. per-point outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_per_point_outputs_designed(dtype):
    case = C.call_case(NP[dtype])
    call = Call(case['scans'], case['poses'], case['total'], case['owns'], dtype)
    for squared in (True, False):
        out, value, flag, x = call.run(mask=_t(case['mask']), squared=squared, want_points=True)
        flag, value, x = flag.cpu().numpy(), value.cpu().numpy(), x.cpu().numpy()
        assert np.array_equal(flag, case['cls'])
        seen = (case['cls'] == C.USED) | (case['cls'] == C.GATED)
        assert np.array_equal(value[seen], case['phi'][seen]) and np.isnan(value[~seen]).all()
        want_x = np.concatenate([c['vps'].astype(np.float64) + np.array([0.0, 0.0, 1.0]) for c in case['scans']])
        inside = case['cls'] != C.MASKED
        finite = np.isfinite(want_x).all(axis=1)                   # (the NaN point: 0 x NaN in the rotation, every component NaN)
        assert np.array_equal(x[inside & finite], want_x[inside & finite]) and np.isnan(x[~inside | ~finite]).all()
        got = call.split(out, None)
        used = case['cls'] == C.USED
        phi = case['phi'][used]
        assert got['used'] == used.sum() and got['unobserved'] == 3 and got['invalid'] == 1 and got['gated'] == 0
        assert got['loss'] == (phi * phi if squared else np.abs(phi)).sum() / used.sum()     # dyadic figures: every sum is exact
        ref = L.loss(case['total'], case['owns'], case['scans'], case['poses'], mask=case['mask'], squared=squared, x=x)
        assert_within_bounds(got, ref, 'designed call on the device')
        assert not got['gT'][1].any()                           # the empty scan between the two others


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_designed_points_on_the_device(dtype):
    """Every designed point of tests/tsdf_loss_cases.py through ops.tsdf_loss, grouped by (own volume, min_count, max_residual): one
    scan a group, identity pose, x = vp + 1 (0, 0, 1) exactly.  Flag, value, the counts and the loss equal the hand-written figures to
    the bit -- min_count above 1 (the count left = min_count - 1 and = min_count), |phi| one ulp below max_residual and equal to it
    included."""
    total, own_a, own_none = C.volumes()
    owns = {'A': own_a, 'none': own_none, None: None}
    groups = {}
    for case in C.point_cases():
        groups.setdefault((case['own'], case['min_count'], case['max_residual']), []).append(case)
    assert len(groups) >= 6 and {k[1] for k in groups} == {1, 2, 3} and {k[2] for k in groups} == {C.TAU, C.JUST_ABOVE, 1.25}
    seen = set()
    for (own, min_count, max_residual), cases in groups.items():
        p = np.array([c['x'] for c in cases], np.float64).reshape(-1, 3)
        n = p.shape[0]
        scan = dict(vps=(p - np.array([0.0, 0.0, 1.0])).astype(NP[dtype]), dirs=np.tile(np.array([0.0, 0.0, 1.0], NP[dtype]), (n, 1)),
                    depth=np.ones(n, NP[dtype]), inc=np.zeros(n, NP[dtype]), lmask=np.ones(n, bool))
        call = Call([scan], np.eye(4)[None], total, None if own is None else [owns[own]], dtype)
        cls = np.array([c['cls'] for c in cases], np.uint8)
        phi = np.array([c['phi'] for c in cases])
        valid = (cls == C.USED) | (cls == C.GATED)
        for squared in (True, False):
            out, value, flag, _ = call.run(None, own is not None, min_count=min_count, max_residual=max_residual, squared=squared,
                                           want_points=True)
            what = (own, min_count, max_residual, squared, [c['name'] for c in cases])
            assert np.array_equal(flag.cpu().numpy(), cls), what
            value = value.cpu().numpy()
            assert np.array_equal(value[valid], phi[valid]) and np.isnan(value[~valid]).all(), what
            got = call.split(out, None)
            assert [got[k] for k in COUNTS] == [int((cls == code).sum()) for code in (C.USED, C.GATED, C.UNOBSERVED, C.INVALID)], what
            used = cls == C.USED
            if used.any():
                l = phi[used] * phi[used] if squared else np.abs(phi[used])
                assert got['loss'] == l.sum() / used.sum(), what               # dyadic figures: every sum is exact
                dl = (2.0 * phi[used] if squared else np.sign(phi[used]))[:, None] * np.array([c['grad'] for c in cases])[used]
                assert np.array_equal(got['gT'][0][:, 3], dl.sum(axis=0) / used.sum()), what
            else:
                assert math.isnan(got['loss']) and not got['gT'].any(), what
        seen |= set(cls.tolist())
    assert seen == {C.USED, C.INVALID, C.UNOBSERVED, C.GATED}


@pytest.mark.parametrize('kind', ['ScaledPolynomial', None])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_per_point_outputs_random(dtype, kind):
    from depth_correction_amd import ops
    call = _random(dtype)
    x64 = call.points64(kind)
    for with_own in (True, False):
        out, value, flag, x = call.run(kind, with_own, max_residual=0.2, want_points=True)
        assert torch.equal(x, x64) or np.array_equal(x.cpu().numpy(), x64.cpu().numpy(), equal_nan=True)
        ref = call.reference(kind, x.cpu().numpy(), with_own, max_residual=0.2)
        assert np.array_equal(flag.cpu().numpy(), ref['cls']) and np.array_equal(value.cpu().numpy(), ref['value'], equal_nan=True)
        assert ref['used'] > 300 and ref['gated'] > 0 and ref['unobserved'] > 0 and ref['invalid'] > 0
        if not with_own:
            tb = call.tables
            smp = ops.tsdf_sparse_sample(tb.keys, tb.slots, tb.n_blocks, tb.sum, tb.count, tb.origin, tb.voxel, tb.trunc, x.contiguous())
            torch.cuda.synchronize()
            assert np.array_equal(value.cpu().numpy(), smp['value'].cpu().numpy(), equal_nan=True)
            sample_flag = smp['flag'].cpu().numpy()
            want = np.where(sample_flag == 1, C.INVALID, np.where(sample_flag == 2, C.UNOBSERVED,
                                                                   np.where(smp['dist'].cpu().numpy() < 0.2, C.USED, C.GATED)))
            assert np.array_equal(flag.cpu().numpy(), want)


# ---- 2. totals ------------------------------------------------------------------------------------------------------------------------
RATIOS = []


@pytest.mark.parametrize('kind,want_e', [(None, False), ('ScaledPolynomial', True), ('Polynomial', False)])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_totals_scan_sizes_and_models(dtype, kind, want_e):
    """Scans of 1, 127, 128, 129 and 0 points in one call, and the random scene (eight blocks a scan), with and without exclusion, both
    forms: counts equal to the oracle, L and every gradient entry within the derived bound, two runs bit-equal."""
    for call in (_sizes(dtype), _random(dtype)):
        for with_own in (True, False):
            for squared in (True, False):
                kw = dict(squared=squared, max_residual=None if squared else 0.2)
                out, _, _, x = call.run(kind, with_own, want_exponent=want_e, want_points=True, **kw)
                again = call.run(kind, with_own, want_exponent=want_e, **kw)
                assert torch.equal(out.view(torch.int64), again.view(torch.int64))
                got = call.split(out, kind)
                ref = call.reference(kind, x.cpu().numpy(), with_own, **kw)
                ratio = assert_within_bounds(got, ref, (dtype, kind, call.sizes, with_own, squared), with_e=want_e)
                RATIOS.append(ratio)
                assert ref['used'] > 50
                if kind is not None:
                    assert np.abs(got['gw']).max() > 0 and (np.abs(got['ge']).max() > 0) == want_e
    print('%s %s: largest |device - oracle| / bound so far %.3g' % (dtype, kind, max(RATIOS)))


def test_no_points_and_nothing_used():
    from depth_correction_amd import ops
    call = _random('float64')
    kind, w, e = call.model('ScaledPolynomial')
    ps0 = ops.PointSet(*(t[:0].contiguous() for t in (call.ps.vps, call.ps.dirs, call.ps.depth, call.ps.inc, call.ps.lmask)))
    ptr0 = torch.zeros((5,), dtype=torch.int64, device=DEV)
    out = ops.tsdf_loss(call.tables, ps0, ptr0, call.poses12, kind, w, e, own=call.own).cpu().numpy()
    assert out.shape == (5 + 4 + 48,) and math.isnan(out[0]) and not out[1:].any()
    none = call.split(call.run('ScaledPolynomial', max_residual=0.0), 'ScaledPolynomial')                  # every observed point gated
    assert math.isnan(none['loss']) and none['used'] == 0 and none['gated'] > 300 and not none['gw'].any() and not none['gT'].any()
    with pytest.raises(ValueError):
        ops.tsdf_loss(call.tables, call.ps, call.scan_ptr, call.poses12, kind, w, e, max_residual=float('nan'))
    with pytest.raises(ValueError):
        ops.tsdf_loss(call.tables, call.ps, call.scan_ptr, call.poses12, kind, w, e, min_count=0)
    with pytest.raises(TypeError):
        ops.tsdf_loss(call.total, call.ps, call.scan_ptr, call.poses12, kind, w, e)


# ---- 3. the autograd surface against the tensor form ------------------------------------------------------------------------------
def _box_clouds(rows, cols, dtype='float64'):
    from depth_correction_amd.depth_cloud import DepthCloud
    scans, poses = L.box_scene(rows=rows, cols=cols, dtype=NP[dtype])
    clouds = [DepthCloud(vps=_t(c['vps']), dirs=_t(c['dirs']), depth=_t(c['depth']).reshape(-1, 1), inc_angles=_t(c['inc']).reshape(-1, 1),
                         mask=_t(c['lmask'])) for c in scans]
    return scans, poses, clouds


@pytest.mark.parametrize('leave_one_out', [True, False])
def test_fused_against_unfused(leave_one_out):
    """loss.tsdf_loss through dc_tsdf_loss against fused=False (torch autograd over SparseTsdfVolume.sample; with leave-one-out over
    S explicitly fused volumes of the other scans): the same used set, the loss and the gradients to w and to the poses within
    COMPOSITION_ROUNDINGS x the bound of test 2 plus the reach of a point moved by as many roundings."""
    from depth_correction_amd import loss as DL, ops
    from depth_correction_amd.model import ScaledPolynomial
    scans, poses, clouds = _box_clouds(24, 96)
    res = {}
    for fused in (True, False):
        model = ScaledPolynomial(w=[0.01], exponent=[2.0], device=DEV)
        P = _t(poses, torch.float64).requires_grad_(True)
        target = DL.TsdfTarget(0.1, leave_one_out=leave_one_out, refresh_every=0)
        loss, loss_clouds = DL.tsdf_loss([clouds], [P], model, masks=[(target, None)], fused=fused)
        loss.backward()
        torch.cuda.synchronize()
        assert target.refreshes == 1 and target.evaluations == 1 and len(loss_clouds) == 1
        res[fused] = dict(loss=loss.item(), gw=model.w.grad.cpu().numpy().reshape(-1), gT=P.grad.cpu().numpy()[:, :3, :], target=target,
                          model=model)
        assert not P.grad.cpu().numpy()[:, 3, :].any()
    # the used sets: the kernel's flags against the tensor form's
    tgt = res[True]['target']
    cat = lambda k, width: np.concatenate([np.asarray(c[k]).reshape(-1, width) for c in scans])
    ps = ops.PointSet(_t(cat('vps', 3)), _t(cat('dirs', 3)), _t(cat('depth', 1).reshape(-1)), _t(cat('inc', 1).reshape(-1)),
                      _t(np.concatenate([c['lmask'] for c in scans])))
    sizes = [len(c['depth']) for c in scans]
    ptr = _t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    w, e = res[True]['model'].kernel_params()
    out, value, flag, x = ops.tsdf_loss(tgt.tables, ps, ptr, _t(poses[:, :3, :].reshape(-1, 12)), 'ScaledPolynomial',
                                        w.detach().reshape(-1).double().contiguous(), e.detach().reshape(-1).double().contiguous(), own=tgt.own,
                                        want_points=True)
    _, used = DL._unfused_tsdf_sequence(clouds, _t(poses, torch.float64), res[False]['model'], res[False]['target'], None, True, None,
                                        return_used=True)
    torch.cuda.synchronize()
    assert torch.equal(flag == 0, used) and int(used.sum()) > 1000
    assert out[0].item() == res[True]['loss']
    # the oracle on the volumes the device fused (read back), for the bounds
    total = _read_volume(tgt.total)
    owns = None
    if leave_one_out:
        own = tgt.own
        kb, sl, pt = own.keys.cpu().numpy().view(np.uint64), own.slots.cpu().numpy(), own.ptr.cpu().numpy()
        sm, cn = own.sum.cpu().numpy(), own.count.cpu().numpy()
        owns = []
        for s in range(len(scans)):
            v = S.SparseVolume(0.1, trunc=tgt.trunc, capacity=sm.shape[0])
            v.keys, v.slots, v.sum, v.count = kb[pt[s]:pt[s + 1]], sl[pt[s]:pt[s + 1]], sm, cn
            owns.append(v)
    ref = L.loss(total, owns, scans, poses, 'ScaledPolynomial', [0.01], [2.0], x=x.cpu().numpy())
    assert ref['face_margin'] >= MARGIN_FLOOR and ref['gate_margin'] >= MARGIN_FLOOR and ref['used'] == int(used.sum())
    for name in ('loss', 'gw', 'gT'):
        bar = COMPOSITION_ROUNDINGS * np.asarray(L.bound(ref, name)) + np.asarray(L.move_bound(ref, name, COMPOSITION_ROUNDINGS))
        err = np.abs(np.asarray(res[True][name]) - np.asarray(res[False][name]))
        print('leave-one-out %s %s: largest |fused - un-fused| %.3g (bar there %.3g); |fused - oracle| %.3g'
              % (leave_one_out, name, err.max(), np.asarray(bar).reshape(-1)[np.argmax(err)], np.abs(np.asarray(res[True][name]) - ref[name]).max()))
        assert (err <= bar).all(), (name, err, bar)
        assert (np.abs(np.asarray(res[True][name]) - ref[name]) <= L.bound(ref, name)).all()
    assert np.abs(res[True]['gw']).max() > 0 and np.abs(res[True]['gT']).max() > 0


def test_target_min_count_reaches_the_kernel():
    """TsdfTarget(min_count=...) through _TsdfLossPlan into the kernel: at min_count 2 the fused loss is the ops call's at min_count 2,
    its used set is the tensor form's (which passes min_count to SparseTsdfVolume.sample) and smaller than at min_count 1."""
    from depth_correction_amd import loss as DL, ops
    from depth_correction_amd.model import ScaledPolynomial
    scans, poses, clouds = _box_clouds(24, 96)
    P = _t(poses, torch.float64)
    cat = lambda k, width: np.concatenate([np.asarray(c[k]).reshape(-1, width) for c in scans])
    ps = ops.PointSet(_t(cat('vps', 3)), _t(cat('dirs', 3)), _t(cat('depth', 1).reshape(-1)), _t(cat('inc', 1).reshape(-1)),
                      _t(np.concatenate([c['lmask'] for c in scans])))
    ptr = _t(np.concatenate([[0], np.cumsum([len(c['depth']) for c in scans])]).astype(np.int64))
    model = ScaledPolynomial(w=[0.01], exponent=[2.0], device=DEV)
    w, e = (v.detach().reshape(-1).double().contiguous() for v in model.kernel_params())
    counts, losses = {}, {}
    for mc in (1, 2):
        target = DL.TsdfTarget(0.1, leave_one_out=True, refresh_every=0, min_count=mc)
        with torch.no_grad():
            fused, _ = DL.tsdf_loss([clouds], [P], model, masks=[(target, None)])
            unfused, used = DL._unfused_tsdf_sequence(clouds, P, model, target, None, True, None, return_used=True)
        out, _, flag, _ = ops.tsdf_loss(target.tables, ps, ptr, _t(poses[:, :3, :].reshape(-1, 12)), 'ScaledPolynomial', w, e, own=target.own,
                                        min_count=mc, want_points=True)
        torch.cuda.synchronize()
        assert fused.item() == out[0].item() and torch.equal(flag == 0, used) and int(out[1].item()) == int(used.sum())
        counts[mc], losses[mc] = int(used.sum()), fused.item()
    print('used at min_count 1 / 2: %d / %d; loss %.9g / %.9g' % (counts[1], counts[2], losses[1], losses[2]))
    assert 0 < counts[2] < counts[1] and losses[1] != losses[2]


def _read_volume(volume):
    """A device SparseTsdfVolume as an oracle SparseVolume."""
    n = volume.n_blocks
    v = S.SparseVolume(volume.voxel_size, trunc=volume.trunc, origin=volume.origin, capacity=volume.capacity)
    v.keys, v.slots = volume._keys[:n].cpu().numpy().view(np.uint64), volume._slots[:n].cpu().numpy()
    v.sum, v.count = volume._sum.cpu().numpy(), volume._count.cpu().numpy()
    return v


# ---- 4. the recovery loop, step by step -----------------------------------------------------------------------------------------------
LOOP_STEPS, LOOP_LR = C.LOOP_STEPS, C.LOOP_LR


def test_recovery_loop_step_by_step():
    """The re-fuse / gradient-descent loop of tests/test_tsdf_loss_host.py on the device (TsdfTarget re-fusing before every
    evaluation, loss.tsdf_loss, autograd, w <- w - lr dL/dw) against the oracle running on its own: 5 x 24 x 96 rays, leave-one-out.
    Every decision of the oracle has a margin of 1e-9 or more (cell faces in voxels, the gate in metres), the used sets are equal in
    every step, and w stays within W_BAR."""
    from depth_correction_amd import loss as DL, ops
    from depth_correction_amd.model import ScaledPolynomial
    scans, poses, clouds = _box_clouds(24, 96)
    P = _t(poses, torch.float64)
    target = DL.TsdfTarget(0.1, trunc=0.3, leave_one_out=True, refresh_every=1)
    cat = lambda k, width: np.concatenate([np.asarray(c[k]).reshape(-1, width) for c in scans])
    ps = ops.PointSet(_t(cat('vps', 3)), _t(cat('dirs', 3)), _t(cat('depth', 1).reshape(-1)), _t(cat('inc', 1).reshape(-1)),
                      _t(np.concatenate([c['lmask'] for c in scans])))
    ptr = _t(np.concatenate([[0], np.cumsum([len(c['depth']) for c in scans])]).astype(np.int64))
    P12 = _t(poses[:, :3, :].reshape(-1, 12))
    w_dev = w_ref = 0.0
    worst = 0.0
    for step in range(LOOP_STEPS):
        model = ScaledPolynomial(w=[w_dev], exponent=[2.0], device=DEV)
        loss, _ = DL.tsdf_loss([clouds], [P], model, masks=[(target, None)])
        loss.backward()
        wt = _t(np.array([w_dev]), torch.float64)
        _, _, flag, _ = ops.tsdf_loss(target.tables, ps, ptr, P12, 'ScaledPolynomial', wt, _t(np.array([2.0])), own=target.own, want_points=True)
        torch.cuda.synchronize()
        w_dev = w_dev - LOOP_LR * float(model.w.grad.reshape(-1)[0].item())
        w_ref, ref = L.descent_step(scans, poses, w_ref, 0.1, 0.3, True, LOOP_LR)
        assert ref['face_margin'] >= MARGIN_FLOOR and ref['gate_margin'] >= MARGIN_FLOOR, (step, ref['face_margin'], ref['gate_margin'])
        assert np.array_equal(flag.cpu().numpy() == 0, ref['cls'] == L.USED), step
        assert target.refreshes == step + 1
        worst = max(worst, abs(w_dev - w_ref))
        print('step %d: w %.15g (oracle %.15g, |diff| %.3g, bar %.3g), used %d, rms phi %.2f mm'
              % (step, w_dev, w_ref, abs(w_dev - w_ref), W_BAR, ref['used'], 1e3 * math.sqrt(ref['loss'])))
        assert abs(w_dev - w_ref) <= W_BAR, step
    assert w_dev > 0.03


# ---- 5. train() -----------------------------------------------------------------------------------------------------------------------
def _pose(yaw, t):
    T = np.eye(4)
    T[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


@pytest.mark.parametrize('pose_correction', ['none', 'pose'])
def test_train_end_to_end(tmp_path, capsys, monkeypatch, pose_correction):
    """train() with cfg.loss = 'tsdf_loss' on a rendered room (4 poses x 16 x 256 rays), four iterations, the model alone and with
    per-pose corrections: the losses are finite, the weights move, the corrections receive a gradient (they move from zero),
    refresh_every = 2 re-fuses at evaluations 0 and 2, and eval_loss_clouds runs with the same configuration."""
    import meshloss_reference as M
    from depth_correction_amd import loss as DL
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.eval import eval_loss_clouds, initialize_pose_corrections, tsdf_masks
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.train import train, _load_sequences
    path = tmp_path / 'room.ply'
    M.room().save_ply(str(path))
    cfg = Config(device=DEV, float_type='float64', min_depth=0.3, max_depth=25.0, grid_res=0.05, nn_k=0, nn_r=0.6, loss='tsdf_loss',
                 n_opt_iters=4, lr=1e-3, log_dir=str(tmp_path / 'model'), pose_correction=pose_correction,
                 model_kwargs={'w': [0.0, 0.0], 'exponent': list(M.E_TRUE)})
    cfg.loss_kwargs = dict(cfg.loss_kwargs, tsdf_voxel_size=0.1, tsdf_refresh_every=2)
    gt = ScaledPolynomial(w=list(M.W_TRUE), exponent=list(M.E_TRUE), device=DEV)
    poses = np.stack([_pose(0.4 * i, (-2.0 + 1.2 * i, 0.3 * i - 0.5, 0.1 * i)) for i in range(4)])
    ds = DepthBiasDataset(RenderedMeshDataset(str(path), poses=poses, size=(16, 256), fov=(45.0, 360.0), num_segments=8, device=DEV), gt, cfg=cfg)
    made, calls = [], []
    real_init, real_refresh = DL.TsdfTarget.__init__, DL.TsdfTarget.refresh

    def init(self, *a, **kw):
        real_init(self, *a, **kw)
        made.append(self)

    def refresh(self, seq_clouds, seq_poses=None, model=None):
        calls.append((self.evaluations, model.w.detach().cpu().numpy().reshape(-1).copy(), torch.stack(list(seq_poses)).detach().cpu().numpy()))
        return real_refresh(self, seq_clouds, seq_poses, model)
    monkeypatch.setattr(DL.TsdfTarget, '__init__', init)
    monkeypatch.setattr(DL.TsdfTarget, 'refresh', refresh)
    os.makedirs(cfg.log_dir)
    capsys.readouterr()
    best = train(cfg, train_datasets=[ds], val_datasets=[])
    text = capsys.readouterr().out
    losses = [float(m) for m in re.findall(r'^It\. \d+: train loss: (-?[0-9.eE+-]+|nan)', text, flags=re.M)]
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses) and best is not None, text[-2000:]
    assert len(made) == 1 and made[0].refresh_every == 2 and made[0].leave_one_out and made[0].evaluations == 4
    assert [at for at, _, _ in calls] == [0, 2]                # re-fused before evaluations 0 and 2, and only then
    (_, w0, poses0), (_, w2, poses2) = calls
    print('%s: train losses %s; w at evaluation 2: %s' % (pose_correction, losses, w2))
    assert not w0.any() and np.abs(w2).max() > 0              # the weights move
    trained = ScaledPolynomial(w=[0.0, 0.0], exponent=list(M.E_TRUE), device=DEV)
    trained.load_state_dict(torch.load(best.model_state_dict))
    if pose_correction == 'pose':                             # the poses receive a gradient: all but the first, which stays fixed
        assert np.array_equal(poses0[0], poses2[0]) and all(np.abs(poses2[i] - poses0[i]).max() > 0 for i in range(1, 4))
    else:
        assert np.array_equal(poses0, poses2)
    # the same configuration through eval_loss_clouds
    clouds, seq_poses = _load_sequences([ds], cfg)
    masks = tsdf_masks([ds], ['room'], clouds, cfg)
    loss, loss_clouds, _, _ = eval_loss_clouds(clouds, seq_poses, initialize_pose_corrections([ds], cfg), masks, [None], trained,
                                               DL.create_loss(cfg), cfg)
    assert math.isfinite(loss.item()) and masks[0][0].refreshes == 1


def test_sharded_training_is_refused(monkeypatch, tmp_path):
    from depth_correction_amd import train as T
    from depth_correction_amd.config import Config
    monkeypatch.setattr(T, '_sharding', lambda cfg: (0, 2, True))
    with pytest.raises(NotImplementedError, match='tsdf_loss'):
        T.train(Config(device=DEV, loss='tsdf_loss', log_dir=str(tmp_path)), train_datasets=[], val_datasets=[])
