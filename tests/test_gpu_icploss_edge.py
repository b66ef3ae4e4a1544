"""csrc/dc_icp.hip against the exact reference of icploss_reference.py on the designed inputs of icploss_cases.py: the pair kernels,
the sequence kernels and both reductions, the one-launch fused iteration with and without its finishing step, the pose-correction
chain forward and backward, dc_pose_train_finish and dc_pose_train_combine / combine2.  Every scan is tiny; large correspondence
counts repeat indices.

Bounds: every output is held to c 2^-52 magnitude, with the magnitude the reference carries next to each value (the expression with
absolute values at every addition) and c the number of roundings on the longest path to that output, counted in icploss_reference.py
(c_sums, C_CHAIN_FWD, C_CHAIN_BWD, C_FINISH) before any kernel was run.  An output whose magnitude is zero must be exactly zero.
Every test prints the largest error it saw in units of its bound; float64 torch autograd of the same formulas sits at 0.006 to 0.04
of these bounds (test_icploss_reference_host.py), DESIGN.md "ICP loss at its edges" has the kernels' figures.

Branch of dc_icp.hip                                            reached by
--------------------------------------------------------------  -------------------------------------------------------------------
k12 == 0, |x2 - x1| == 0 (sign(0) = 0, norm at zero)            pair single0, single1; every `mixed` list
|n| == 0 on one side / both                                     pair single2 / single3; every `mixed` list
inc == 0 in the exponent gradient, pow_term(0, e)               pair single4, single6 (exponents 0, 8, 2.5); every `mixed` list
lmask false                                                     pair single5, single6; random points (15 %)
pow_term's fast path at 0 and 8, pow() beside it                every polynomial case with three or eight terms
the fp32 cast, both dtypes, vps NULL                            every case (poses ~400 m out); kind-*-float32 / -float64
every model kind and none                                       pair kind-*, m*; sequence `none`
icp_block_sums: partial wavefront, partial block, one thread    pair m1, m63, m64, m65, m255, m256, m257, m513
p2plane_reduce_kernel: strided loop (257 rows)                  pair m65537
p2plane_reduce_all_kernel: strided loop, LDS destinations       sequence big (96, 97, 257 rows); every sequence with S <= 1024
  global adds above kIcpDstScans, first and non-first chunk     sequence S1025-p17 (the 17th pair is the second launch)
chunks of kIcpSeqPairs, empty pairs skipped                     sequence p16, p17, p33, p20-4empty (one chunk), p21-4empty (two)
a scan as A and as B, a pair twice, unequal weights             sequence p2-unused, p33
fused kernel: six row phases, second trip of the in-flight loop step big (96 and 97 rows: r0 = f + 96 exists for f = 0 only at 97)
fused kernel: both ticket levels, reset by the launch           every step test (second call bit-equal, tickets zero)
fused kernel: sums in LDS (n_out <= 401) / in global memory     step S32-P8 (401) / S33-P8 (413), S257
pose_train_finish_block: register path / re-fetch loops         finish S1 .. S256 / S257, S600; step S257 with the finishing step
  shared / per-pose corrections, zero_first, lr_w == 0, w NULL  finish *-shared, S256 (w NULL), S257 (lr_w = 0), zero_first both ways
  totals, both layouts, the record ring                         finish S2-ring3x4, S257-shared, S600; ring of 1 and 3 over four steps
small-angle switch in pose_chain_fwd / _bwd, theta == 0         chain corrections zero, tiny, below*, at*, above* (shared and per pose)
pose_correct_kernel: stride over poses, block sum               chain per-pose-257 / -600, shared-generic-257 / -600, shared-at0-257
"""
import ctypes

import numpy as np
import pytest
import torch

import icploss_cases as C
import icploss_reference as R
from helpers import t, npy

pytestmark = pytest.mark.gpu

U = R.U
CANARY = -7.25e300
PAD = 64
_dev_scans = {}


def _scan(scan, dev):
    """(PointSet, normals) of a scan dict on the device, once per dict (descriptors of one sequence may share it)"""
    from depth_correction_amd import ops
    key = id(scan)
    if key not in _dev_scans:
        g = lambda f: None if scan[f] is None else t(scan[f], dev)
        _dev_scans[key] = (scan, ops.PointSet(g('vps'), g('dirs'), g('depth'), g('inc'), g('lmask')), g('normals'))
    return _dev_scans[key][1:]


def _model(case, dev):
    if case['model'] is None:
        return None, None, None
    kind, w, e = case['model']
    return kind, t(np.asarray(w, dtype=np.float64), dev), t(np.asarray(e, dtype=np.float64), dev)


def _canaried(shape, dev, dtype=torch.float64, init=None):
    """A tensor of `shape` inside a larger buffer of canaries -> (view, check()); check asserts that the neighbours are untouched"""
    n = int(np.prod(shape)) if len(shape) else 1
    fill = CANARY if dtype.is_floating_point else -12345
    big = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    view = big[PAD:PAD + n].view(*shape) if len(shape) else big[PAD:PAD + 1].view(())
    if init is not None:
        view.copy_(t(np.asarray(init), dev).reshape(view.shape))

    def check(what=''):
        assert bool((big[:PAD] == fill).all()) and bool((big[PAD + n:] == fill).all()), 'canary overwritten next to ' + what
    return view, check


def _note(worst, tag, got, val, bound):
    r = C.ratio(np.asarray(got) - val, bound)
    worst[tag] = max(worst.get(tag, 0.0), r)
    assert r <= 1.0, (tag, r)


# ---- pair kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(C.PAIR_SPECS))
def test_pair_kernels(name, dev):
    """ops.p2plane_pair / p2point_pair: all 26 + 2P outputs; p2point's second sum is exactly 0; no correspondence gives exact zeros"""
    from depth_correction_amd import ops
    case = C.settle(C.pair_case(name))
    (psa, na), (psb, nb) = _scan(case['scans'][0], dev), _scan(case['scans'][1], dev)
    kind, w, e = _model(case, dev)
    pa, pb = t(case['poses'][0], dev), t(case['poses'][1], dev)
    _, _, ia, ib, _ = case['pairs'][0]
    c = R.c_sums(-(-len(ia) // R.BLOCK))
    worst = {}
    for plane in (True, False):
        val, mag = C.reference(case, plane)
        da_all, db_all = t(ia, dev), t(ib, dev)
        for da, db, v, m in ((da_all, db_all, val, mag), (da_all[:0], db_all[:0], np.zeros_like(val), np.zeros_like(mag))):
            if plane:
                out = ops.p2plane_pair(psa, na, psb, nb, pa, pb, da, db, kind, w, e)
            else:
                out = ops.p2point_pair(psa, psb, pa, pb, da, db, kind, w, e)
            got = npy(torch.cat([o.reshape(-1) for o in out]))
            assert got.shape == v.shape
            _note(worst, 'plane' if plane else 'point', got, v, c * U * m)
            if not plane:
                assert got[1] == 0.0
    print('%s: largest error in units of the bound %s' % (name, worst))


# ---- sequences --------------------------------------------------------------------------------------------------------------------
class _Seq(object):
    """An ops.IcpSequence of a case for one loss: explicit weights on the descriptors, the workspace and `out` among canaries"""

    def __init__(self, case, plane, dev):
        from depth_correction_amd import ops, _native as nv
        self.case, self.plane, self.dev = case, plane, dev
        scans = [_scan(s, dev) for s in case['scans']]
        self.pairs = C.pairs_of(case, plane)
        self.idx = [(t(p[2], dev), t(p[3], dev)) for p in self.pairs]
        self.seq = ops.IcpSequence(scans, [(p[0], p[1], ia, ib) for p, (ia, ib) in zip(self.pairs, self.idx)], with_model=case['model'] is not None,
                                   plane=plane)
        for d, p in zip(self.seq.pair_desc, self.pairs):
            d.weight = float(p[4])
        count = nv.lib().dc_p2plane_sequence_partial_count(ctypes.cast(self.seq.pair_desc, ctypes.c_void_p), self.seq.n_pairs)
        assert self.seq.part.numel() == count
        self.seq.part, self.check_part = _canaried((count,), dev)            # exactly the documented workspace, neighbours watched
        self.kind, self.w, self.e = _model(case, dev)
        self.P = 0 if self.w is None else len(self.w)
        self.n_out = 1 + 2 * self.P + 12 * len(scans)
        self.out, self.check_out = _canaried((self.n_out,), dev)
        self.poses = t(np.asarray(case['poses'], dtype=np.float64), dev)
        rows, n_pairs = R.sequence_rows(self.pairs)
        self.c = R.c_sums(rows, n_pairs)

    def eval(self):
        self.out.fill_(CANARY)
        self.seq.eval(self.poses, self.kind, self.w, self.e, out=self.out)
        return self._read('eval')

    def step(self, fin=None, poses=None):
        self.out.fill_(CANARY)
        ok = self.seq.step(self.poses if poses is None else poses, self.kind, self.w, self.e, self.out, fin)
        return ok, (self._read('step') if ok else None)

    def _read(self, what):
        torch.cuda.synchronize()
        self.check_part('the workspace after ' + what)
        self.check_out('out after ' + what)
        return npy(self.out).copy()


@pytest.mark.parametrize('plane', [True, False], ids=['plane', 'point'])
@pytest.mark.parametrize('name', sorted(C.SEQ_SPECS))
def test_sequence_eval(name, plane, dev):
    """IcpSequence.eval, every slot; a scan in no pair and an all-empty sequence get exact zeros (their magnitudes are zero)"""
    case = C.settle(C.seq_case(name))
    val, mag = C.reference(case, plane)
    s = _Seq(case, plane, dev)
    worst = {}
    _note(worst, 'eval', s.eval(), val, s.c * U * mag)
    if name == 'all-empty':
        assert not val.any() and not mag.any()
    if name == 'p2-unused':
        assert not mag[-12:].any()
    print('%s: largest error in units of the bound %s (c = %d)' % (name, worst, s.c))


@pytest.mark.parametrize('plane', [True, False], ids=['plane', 'point'])
@pytest.mark.parametrize('name', C.FUSED)
def test_fused_step_without_finish(name, plane, dev):
    """IcpSequence.step alone: the reference's sums, bit-equal on a second call, tickets left at zero"""
    case = C.settle(C.seq_case(name))
    val, mag = C.reference(case, plane)
    s = _Seq(case, plane, dev)
    ok, got = s.step()
    assert ok is True
    worst = {}
    _note(worst, 'step', got, val, s.c * U * mag)
    ok, again = s.step()
    assert ok is True and np.array_equal(got, again)
    assert not bool(s.seq.ticket.any())
    print('%s: largest error in units of the bound %s (c = %d)' % (name, worst, s.c))


@pytest.mark.parametrize('name,takes', [('p17', False), ('p21-4empty', False), ('all-empty', False), ('p20-4empty', True), ('p16', True)])
def test_fused_step_says_what_it_cannot_take(name, takes, dev):
    """False for seventeen non-empty pairs and for no correspondence at all, True for twenty pairs of which four are empty"""
    s = _Seq(C.settle(C.seq_case(name)), True, dev)
    ok, _ = s.step()
    assert ok is takes
    assert not bool(s.seq.ticket.any())


# ---- the fused iteration with its finishing step ----------------------------------------------------------------------------------
FUSED_FINISH = [('p2-unused', False, 1), ('S32-P8', True, 1), ('S33-P8', False, 0), ('S257', False, 1), ('S257', True, 0)]


@pytest.mark.parametrize('name,shared,zero_first', FUSED_FINISH)
def test_fused_step_with_finish(name, shared, zero_first, dev):
    """Four whole iterations in a row, one launch each: sums, Adam on the weights and the corrections, next poses, record ring --
    each iteration against the reference's sums at the poses it used and the reference's finishing step fed those sums, started
    from the state the iteration found.  The next iteration evaluates at the poses this one wrote."""
    from depth_correction_amd import _native as nv
    case = C.settle(C.seq_case(name))
    plane = True
    s = _Seq(case, plane, dev)
    S, P = len(case['scans']), s.P
    rng = np.random.default_rng(11)
    nd = 1 if shared else S
    ring_rows, n_extra, steps = 3, 5, 4
    T0 = np.zeros((S, 4, 4))
    T0[:, :3, :] = np.asarray(case['poses']).reshape(S, 3, 4)
    T0[:, 3, 3] = 1.0
    T0 = T0.reshape(S, 16)
    rec_len = s.n_out + P + 6 * nd + 12 * S + n_extra
    bufs = dict(w=(P,), w_m=(P,), w_v=(P,), delta=(nd, 6), d_m=(nd, 6), d_v=(nd, 6), T0=(S, 16), T=(S, 16), P12=(S, 12), ring=(ring_rows, rec_len),
                extra=(n_extra,))
    init = dict(w=0.02 * rng.standard_normal(P), w_m=1e-2 * rng.standard_normal(P), w_v=1e-4 * rng.random(P), delta=np.zeros((nd, 6)),
                d_m=1e-3 * rng.standard_normal((nd, 6)), d_v=1e-6 * rng.random((nd, 6)), T0=T0, T=T0, P12=case['poses'],
                ring=np.full((ring_rows, rec_len), 3.5), extra=rng.standard_normal(n_extra))
    dv, checks = {}, {}
    for f, shape in bufs.items():
        dv[f], checks[f] = _canaried(shape, dev, init=init[f])
    step, checks['step'] = _canaried((), dev, dtype=torch.int64, init=np.int64(7))
    lr_w, lr_d, b1, b2, eps = 1e-3, C.ADAM['lr_d'], C.ADAM['b1'], C.ADAM['b2'], C.ADAM['eps']
    fin = nv.PoseTrainStepDesc()
    fin.w, fin.w_m, fin.w_v = dv['w'].data_ptr(), dv['w_m'].data_ptr(), dv['w_v'].data_ptr()
    fin.poses0, fin.deltas, fin.d_m, fin.d_v = dv['T0'].data_ptr(), dv['delta'].data_ptr(), dv['d_m'].data_ptr(), dv['d_v'].data_ptr()
    fin.n_deltas, fin.zero_first, fin.step = nd, zero_first, step.data_ptr()
    fin.lr_w, fin.lr_d, fin.beta1, fin.beta2, fin.eps = lr_w, lr_d, b1, b2, eps
    fin.poses_used = fin.poses_next = dv['T'].data_ptr()            # in place, as the training loop runs it
    fin.poses12_next = dv['P12'].data_ptr()
    fin.record, fin.ring_rows, fin.record_extra, fin.n_record_extra = dv['ring'].data_ptr(), ring_rows, dv['extra'].data_ptr(), n_extra
    worst = {}
    fake = dict(name=name)
    for k in range(steps):
        before = {f: npy(dv[f]).copy() for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v', 'T', 'P12', 'ring')}
        before['step'] = int(step.item())
        ok, got = s.step(fin, poses=dv['P12'])
        assert ok is True
        for f, chk in checks.items():
            chk(f)
        val, mag = C.reference(case, plane, poses=before['P12'])
        _note(worst, 'sums', got, val, s.c * U * mag)
        ref = R.finish_step(val, 1, P, S, before['w'], before['w_m'], before['w_v'], T0, before['delta'], before['d_m'], before['d_v'], zero_first,
                            before['step'], lr_w, lr_d, b1, b2, eps, before['T'], rec_extra=npy(dv['extra']),
                            sums_mag=np.maximum(np.abs(val), s.c * mag / R.C_FINISH))
        after = {f: npy(dv[f]).copy() for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v')}
        after['step'] = int(step.item())
        C.check_finish(fake, k, before, after, npy(dv['T']), worst, ref=ref)
        assert np.array_equal(npy(dv['P12']), npy(dv['T'])[:, :12])
        ring = npy(dv['ring'])
        row = before['step'] % ring_rows
        assert np.array_equal(ring[row, :s.n_out], got), 'the record holds the sums of its own iteration'
        assert np.array_equal(ring[row, s.n_out:], ref['record'][s.n_out:]), 'the record holds what the iteration used'
        others = [r for r in range(ring_rows) if r != row]
        assert np.array_equal(ring[others], before['ring'][others])
        assert not bool(s.seq.ticket.any())
    print('%s shared=%s: largest error in units of the bound %s' % (name, shared, worst))


# ---- the pose-correction chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(C.CHAIN_SPECS))
def test_corrected_poses(name, dev):
    """transform.corrected_poses forward and backward; a shared correction's gradient at 257 and 600 poses is the block sum"""
    from depth_correction_amd.transform import corrected_poses
    case, ref = C.chain_case(name), C.chain_reference(name)
    n = len(case['T0'])
    T0 = t(case['T0'], dev).reshape(n, 4, 4)
    d = t(case['deltas'], dev).requires_grad_(True)
    T = corrected_poses(T0, d)
    (T * t(case['grad'], dev).reshape(n, 4, 4)).sum().backward()
    worst = {}
    _note(worst, 'forward', npy(T).reshape(n, 16), ref['fwd'][0], R.C_CHAIN_FWD * U * ref['fwd'][1])
    c_bwd = R.C_CHAIN_BWD + (8 + -(-n // 256) if len(case['deltas']) == 1 else 0)
    _note(worst, 'backward', npy(d.grad), ref['bwd'][0], c_bwd * U * ref['bwd'][1])
    print('%s: largest error in units of the bound %s' % (name, worst))


# ---- dc_pose_train_finish and dc_pose_train_combine -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(C.FINISH_SPECS))
def test_pose_train_finish(name, dev):
    """The standalone finishing step over the case's steps, every buffer among canaries: each step against the reference started
    from the state the step found; every record row holds what its iteration used, the other rows stay."""
    from depth_correction_amd import _native as nv
    case = C.finish_case(name)
    sp = case['spec']
    S, P = sp['S'], sp['P']
    nd = 1 if sp['shared'] else S
    rec_len = C.record_len(case)
    n_sums = len(case['sums'][0])
    shapes = dict(delta=(nd, 6), d_m=(nd, 6), d_v=(nd, 6), T0=(S, 16), T_used=(S, 16), T_next=(S, 16), P12=(S, 12), ring=(sp['ring_rows'], rec_len),
                  sums=(n_sums,))
    init = dict(delta=case['delta'], d_m=case['d_m'], d_v=case['d_v'], T0=case['T0'], T_used=case['T_used'][0], T_next=np.zeros((S, 16)),
                P12=np.zeros((S, 12)), ring=np.full((sp['ring_rows'], rec_len), 3.5), sums=case['sums'][0])
    if sp['with_w']:
        shapes.update(w=(P,), w_m=(P,), w_v=(P,))
        init.update(w=case['w'], w_m=case['w_m'], w_v=case['w_v'])
    if sp['totals']:
        shapes['totals'], init['totals'] = (2 + P,), case['totals'][0]
    if sp['n_extra']:
        shapes['extra'], init['extra'] = (sp['n_extra'],), case['extra'][0]
    dv, checks = {}, {}
    for f, shape in shapes.items():
        dv[f], checks[f] = _canaried(shape, dev, init=init[f])
    step, checks['step'] = _canaried((), dev, dtype=torch.int64, init=np.int64(case['step0']))
    p_ = lambda f: nv.ptr(dv[f]) if f in dv else None
    worst = {}
    for k in range(sp['steps']):
        for f, src in (('sums', 'sums'), ('T_used', 'T_used'), ('totals', 'totals'), ('extra', 'extra')):
            if f in dv:
                dv[f].copy_(t(np.asarray(case[src][k]), dev).reshape(dv[f].shape))
        before = {f: (npy(dv[f]).copy() if f in dv else None) for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v')}
        before['step'] = int(step.item())
        ring0 = npy(dv['ring']).copy()
        rc = nv.lib().dc_pose_train_finish(p_('sums'), sp['layout'], P, S, p_('w'), p_('w_m'), p_('w_v'), p_('T0'), p_('delta'), p_('d_m'), p_('d_v'), nd,
                                           sp['zero_first'], nv.ptr(step), sp['lr_w'], C.ADAM['lr_d'], C.ADAM['b1'], C.ADAM['b2'], C.ADAM['eps'],
                                           p_('T_used'), p_('ring'), sp['ring_rows'], p_('T_next'), p_('P12'), p_('totals'), p_('extra'), sp['n_extra'],
                                           nv.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        for f, chk in checks.items():
            chk(f)
        after = {f: (npy(dv[f]).copy() if f in dv else None) for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v')}
        after['step'] = int(step.item())
        ring = npy(dv['ring'])
        row = before['step'] % sp['ring_rows']
        C.check_finish(case, k, before, after, npy(dv['T_next']), worst, record=ring[row])
        assert np.array_equal(npy(dv['P12']), npy(dv['T_next'])[:, :12])
        others = [r for r in range(sp['ring_rows']) if r != row]
        assert np.array_equal(ring[others], ring0[others])
    print('%s: largest error in units of the bound %s' % (name, worst))


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('n_seq', [1, 16])
def test_pose_train_combine(n_seq, layout, dev):
    """dc_pose_train_combine and combine2 (an empty second group gives zeros): (n_seq - 1) roundings of a serial sum"""
    from depth_correction_amd import _native as nv
    P, S = 3, 2
    rng = np.random.default_rng(100 * n_seq + layout)
    n_sums = (2 if layout == 0 else 1) + 2 * P + 12 * S
    outs = rng.standard_normal((n_seq, n_sums))
    if layout == 0:
        outs[:, 1] = rng.integers(100, 9000, n_seq)
    val, mag = R.combine(outs, layout, P)
    d_outs = [t(o, dev) for o in outs]
    arr = (ctypes.c_void_p * n_seq)(*[o.data_ptr() for o in d_outs])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    tot, chk = _canaried((2 + P,), dev)
    assert nv.lib().dc_pose_train_combine(cast(arr), n_seq, layout, P, nv.ptr(tot), nv.stream_ptr()) == 0
    torch.cuda.synchronize()
    chk('totals')
    worst = {}
    _note(worst, 'combine', npy(tot), val, max(n_seq - 1, 0) * U * mag)
    tot2, chk2 = _canaried((2, 2 + P), dev)
    assert nv.lib().dc_pose_train_combine2(cast(arr), n_seq, cast(arr), 0, layout, P, nv.ptr(tot2), nv.stream_ptr()) == 0
    torch.cuda.synchronize()
    chk2('totals2')
    got = npy(tot2)
    assert np.array_equal(got[0], npy(tot)) and not got[1].any()
    tot3, chk3 = _canaried((2, 2 + P), dev)
    assert nv.lib().dc_pose_train_combine2(cast(arr), 0, cast(arr), n_seq, layout, P, nv.ptr(tot3), nv.stream_ptr()) == 0
    torch.cuda.synchronize()
    chk3('totals2')
    got = npy(tot3)
    assert np.array_equal(got[1], npy(tot)) and not got[0].any()
    print('n_seq %d layout %d: largest error in units of the bound %s' % (n_seq, layout, worst))
