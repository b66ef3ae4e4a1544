"""Designed inputs of the ICP-loss tests (test_icploss_reference_host.py, test_gpu_icploss_edge.py): tiny scans, correspondence
lists that reach every row count and reduction route of csrc/dc_icp.hip by repeating indices, poses a few hundred metres from the
origin, every model kind, and the corrections and optimiser states of the pose-training tail.  Everything is generated from seeds.

The first DESIGNED points of every scan are placed by hand (`exact` poses: a signed permutation and an integer translation, so that
R x_l + t is exact up to the one rounding of the sum):

    0  identical world points: B's point is A's point expressed in B's frame              |x2 - x1| = 0, k12 = k21 = 0
    1  B's point lies exactly on A's plane (same height, A's normal along z)              k12 = 0, k21 != 0
    2  zero normal on side A                                                              |n1| = 0
    3  zero normals on both sides                                                         |n1| = |n2| = 0
    4  inc = 0 on side A, inside the mask                                                 exponent gradient 0, pow_term(0, e)
    5  outside the mask on side A                                                         the depth is kept, no model gradient
    6  outside the mask and inc = 0 on side B
    7  a generic point: the target of `one_point`

A coordinate next to a float32 rounding tie may round the other way in a float64 evaluation; ``reference`` redraws the depth of
such points (never a designed one) and asserts that at most 0.1 % of the case's points needed it."""
import zlib

import numpy as np

import icploss_reference as R

DESIGNED = 8
KIND_NAMES = (None, 'Polynomial', 'ScaledPolynomial', 'Linear', 'InvCos', 'ScaledInvCos')
M_LIST = (1, 63, 64, 65, 255, 256, 257, 513, 24576, 24577, 65537)
EXPONENTS = (0.0, 8.0, 2.5, 1.0, 2.0, 3.0, 4.0, 0.5)       # integer 0 and 8: the ends of pow_term's fast path; 2.5 and 0.5: pow()
REDRAW_CAP = 1e-3
U = R.U


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_model(kind, n_terms, rng):
    if kind is None:
        return None
    if kind == 'Linear':
        return kind, np.array([1.0 + 0.01 * rng.standard_normal(), 0.02 * rng.standard_normal(), 0.05 * rng.standard_normal()]), np.zeros(3)
    if kind in ('InvCos', 'ScaledInvCos'):
        return kind, np.array([0.01 * (1 + rng.random())]), np.zeros(1)
    w = 0.02 * rng.standard_normal(n_terms)
    return kind, w, np.array(EXPONENTS[:n_terms]) if n_terms > 1 else np.array([2.5])


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    r, i, j, k = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r)],
                     [2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r)],
                     [2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)]])


RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
T_EXACT = np.array([350.0, -220.0, 12.0])


def make_poses(n, rng, exact=False):
    """[n, 12] row-major [R|t], a few hundred metres out.  exact: identity / RZ90 alternating, one integer translation."""
    P = np.zeros((n, 3, 4))
    for s in range(n):
        if exact:
            P[s, :, :3] = RZ90 if s % 2 else np.eye(3)
            P[s, :, 3] = T_EXACT
        else:
            P[s, :, :3] = random_rotation(rng)
            P[s, :, 3] = T_EXACT + rng.uniform(-80, 80, 3)
    return P.reshape(n, 12)


def make_scan(n, dtype, rng, vps=True, side=0, partner=None):
    """One scan of n points; with n >= DESIGNED the first points are the designed ones (side 0: as drawn; side 1: placed against
    `partner`, a side-0 scan, under the exact poses identity / RZ90)."""
    dirs = rng.standard_normal((n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    s = dict(vps=(rng.uniform(-0.3, 0.3, (n, 3)) if vps else None), dirs=dirs, depth=rng.uniform(2.0, 30.0, n),
             inc=rng.uniform(0.05, 1.2, n), lmask=rng.random(n) < 0.85, normals=rng.standard_normal((n, 3)))
    s['normals'] /= np.linalg.norm(s['normals'], axis=1, keepdims=True) * rng.uniform(0.8, 1.25, (n, 1))
    s = {k: (v.astype(dtype) if v is not None and v.dtype != bool else v) for k, v in s.items()}
    if n >= DESIGNED:
        s['lmask'][:DESIGNED] = True
        s['normals'][2] = 0
        s['normals'][3] = 0
        if side == 0:
            s['normals'][1] = (0, 0, 1.5)
            s['inc'][4] = 0
            s['lmask'][5] = False
        else:
            s['normals'][2] = partner['normals'][7]
            s['inc'][6] = 0
            s['lmask'][6] = False
            to_b = lambda v: np.array([v[1], -v[0], v[2]], dtype=dtype)       # RZ90^T v
            for f in ('dirs', 'vps'):
                if s[f] is not None and partner[f] is not None:
                    s[f][0] = to_b(partner[f][0])
                    s[f][1, 2] = partner[f][1, 2]
            for f in ('depth', 'inc'):
                s[f][0] = partner[f][0]
                s[f][1] = partner[f][1]
    return s


def make_corr(kind, m, na, nb, rng, pool=24):
    """(idx_a, idx_b) int32 [m]: `pool` distinct random correspondences repeated in random order (`random`), the same with every
    designed correspondence in it (`mixed`), all to point 7 of B (`one_point`), idx_a == idx_b (`same_index`), one designed
    correspondence alone (an int)."""
    if isinstance(kind, int):
        return np.full(m, kind, np.int32), np.full(m, kind, np.int32)
    ua, ub = rng.integers(0, na, pool), rng.integers(0, nb, pool)
    if kind == 'mixed' and min(na, nb) >= DESIGNED:
        ua, ub = np.concatenate([np.arange(DESIGNED), ua]), np.concatenate([np.arange(DESIGNED), ub])
    if kind == 'one_point':
        ub = np.full_like(ub, min(7, nb - 1))
    if kind == 'same_index':
        ua = ub = rng.integers(0, min(na, nb), pool)
    pick = np.concatenate([np.arange(min(m, len(ua))), rng.integers(0, len(ua), max(m - len(ua), 0))])
    pick = pick[rng.permutation(m)] if m > 1 else pick
    return ua[pick].astype(np.int32), ub[pick].astype(np.int32)


# ---- pair cases -------------------------------------------------------------------------------------------------------------------
def _pair_specs():
    specs = {}
    for j, m in enumerate(M_LIST):         # every row count; kinds, dtypes and term counts rotate
        kind = KIND_NAMES[j % 6]
        specs['m%d' % m] = dict(m=m, kind=kind, nt=(1, 3, 8)[j % 3], dtype=(np.float64, np.float32)[j % 2], corr='mixed' if m >= 63 else 'random',
                                exact=True, vps=j % 4 != 3, n=40)
    for j, kind in enumerate(KIND_NAMES):  # every kind in both dtypes, generic poses, two rows with a partial one
        for dtype in (np.float32, np.float64):
            specs['kind-%s-%s' % (kind, np.dtype(dtype).name)] = dict(m=300, kind=kind, nt=(8, 1, 3)[j % 3], dtype=dtype, corr='mixed', exact=False,
                                                                     vps=(j + (dtype == np.float32)) % 2 == 0, n=40)
    for i in range(DESIGNED):              # every designed correspondence alone
        specs['single%d' % i] = dict(m=1, kind=('ScaledPolynomial', 'Polynomial')[i % 2], nt=3, dtype=(np.float64, np.float32)[i % 2], corr=i, exact=True,
                                     vps=True, n=DESIGNED)
    specs['one_point'] = dict(m=65, kind='ScaledPolynomial', nt=3, dtype=np.float64, corr='one_point', exact=True, vps=True, n=300)
    specs['same_index'] = dict(m=65, kind='Polynomial', nt=8, dtype=np.float32, corr='same_index', exact=False, vps=False, n=40)
    specs['one_point_scans'] = dict(m=64, kind='Linear', nt=3, dtype=np.float64, corr='random', exact=False, vps=True, n=1)
    return specs


PAIR_SPECS = _pair_specs()
_cases, _refs = {}, {}


def pair_case(name):
    """-> dict(scans [A, B], poses [2,12], model, pairs [(0, 1, idx_a, idx_b, 1.0)], dtype)"""
    if name not in _cases:
        sp, rng = PAIR_SPECS[name], _rng('pair-' + name)
        A = make_scan(sp['n'], sp['dtype'], rng, sp['vps'], 0)
        B = make_scan(sp['n'], sp['dtype'], rng, sp['vps'], 1, A)
        ia, ib = make_corr(sp['corr'], sp['m'], sp['n'], sp['n'], rng)
        _cases[name] = dict(name=name, scans=[A, B], poses=make_poses(2, rng, sp['exact']), model=make_model(sp['kind'], sp['nt'], rng),
                            pairs=[(0, 1, ia, ib, 1.0)], dtype=sp['dtype'], redrawn=0)
    return _cases[name]


# ---- sequence cases ---------------------------------------------------------------------------------------------------------------
def _seq_specs():
    """name -> dict(S, pairs = [(a, b, m)], kind, nt, dtype, distinct = number of distinct scan tensors, weights)"""
    consecutive = lambda n, m=lambda i: 20 + 37 * i: [(i, i + 1, m(i)) for i in range(n)]
    sp = {}
    sp['p1'] = dict(S=2, pairs=consecutive(1), kind='ScaledPolynomial', nt=3)
    sp['p2-unused'] = dict(S=4, pairs=[(0, 1, 70), (1, 2, 257)], kind='Polynomial', nt=1, dtype=np.float32)       # scan 1: B then A; scan 3 in no pair
    sp['p16'] = dict(S=17, pairs=consecutive(16), kind='Linear', nt=3)
    sp['p17'] = dict(S=18, pairs=consecutive(17), kind='ScaledPolynomial', nt=8, dtype=np.float32)
    sp['p33'] = dict(S=6, pairs=[((5 * i) % 6, (5 * i + 2 + i % 3) % 6, 9 + 31 * (i % 5)) for i in range(31)] + [(4, 1, 513), (4, 1, 513)],
                     kind='ScaledPolynomial', nt=3, weights='unequal')                                           # non-consecutive; one pair twice
    empty = (3, 9, 15, 16)
    sp['p20-4empty'] = dict(S=8, pairs=[(i % 7, i % 7 + 1, 0 if i in empty else 30 + 11 * i) for i in range(20)], kind='InvCos', nt=1)
    sp['p21-4empty'] = dict(S=8, pairs=[(i % 7, i % 7 + 1, 0 if i in empty else 30 + 11 * i) for i in range(21)], kind='ScaledInvCos', nt=1)
    sp['all-empty'] = dict(S=3, pairs=[(0, 1, 0), (1, 2, 0), (0, 2, 0)], kind='ScaledPolynomial', nt=3)
    sp['S32-P8'] = dict(S=32, pairs=[(0, 31, 65), (31, 15, 255), (15, 16, 64)], kind='ScaledPolynomial', nt=8)     # n_out = 401: LDS
    sp['S33-P8'] = dict(S=33, pairs=[(0, 32, 65), (32, 15, 255), (15, 16, 64)], kind='Polynomial', nt=8)           # n_out = 413: global
    sp['S257'] = dict(S=257, pairs=[(0, 256, 63), (256, 128, 256), (255, 1, 1)], kind='ScaledPolynomial', nt=3, distinct=4)
    far = lambda S: [((61 * i) % S, (61 * i + 7) % S, 12 + 5 * i) for i in range(15)] + [(S - 1, 0, 40), (1, S - 1, 33)]
    sp['S1024-p17'] = dict(S=1024, pairs=far(1024), kind='ScaledPolynomial', nt=3, distinct=4)                     # LDS destinations, two chunks
    sp['S1025-p17'] = dict(S=1025, pairs=far(1025), kind='Polynomial', nt=3, distinct=4, dtype=np.float32)         # global adds, non-first chunk
    sp['big'] = dict(S=3, pairs=[(0, 1, 24576), (1, 2, 24577), (2, 0, 65537)], kind='ScaledPolynomial', nt=3)     # 96, 97 and 257 rows
    sp['none'] = dict(S=3, pairs=[(0, 1, 300), (2, 1, 5)], kind=None, nt=0, dtype=np.float32)
    return sp


SEQ_SPECS = _seq_specs()
FUSED = ('p1', 'p2-unused', 'p16', 'p20-4empty', 'S32-P8', 'S33-P8', 'S257', 'big', 'none')       # at most sixteen non-empty pairs


def seq_case(name):
    """-> dict(scans [S] (descriptors may share a scan dict), scan_of [S] index into distinct, poses [S,12], model, pairs with their
    weights (icp_loss's unless the spec says `unequal`; one set per loss: weights[plane])."""
    key = 'seq-' + name
    if key not in _cases:
        sp, rng = SEQ_SPECS[name], _rng(key)
        S, dtype = sp['S'], sp.get('dtype', np.float64)
        n = 40
        nd = sp.get('distinct', S)
        distinct = []
        for s in range(nd):
            distinct.append(make_scan(n, dtype, rng, s % 3 != 2 or nd < 3, s % 2, distinct[s - 1] if s % 2 else None))
        scan_of = [s % nd for s in range(S)]
        pairs = []
        n_pairs = len(sp['pairs'])
        for i, (a, b, m) in enumerate(sp['pairs']):
            ia, ib = make_corr('mixed' if i % 2 == 0 else 'random', m, n, n, rng, pool=12)
            pairs.append((a, b, ia, ib))
        weights = {}
        for plane in (True, False):
            weights[plane] = [(0.5 if plane else 1.0) / (max(len(p[2]), 1) * n_pairs) * ((1.0 + 0.37 * (i % 4)) if sp.get('weights') == 'unequal' else 1.0)
                              for i, p in enumerate(pairs)]
        _cases[key] = dict(name=name, scans=[distinct[q] for q in scan_of], distinct=distinct, scan_of=scan_of, poses=make_poses(S, rng, exact=(S <= 4)),
                           model=make_model(sp['kind'], sp['nt'], rng), pairs=pairs, weights=weights, dtype=dtype, redrawn=0)
    return _cases[key]


def pairs_of(case, plane):
    """[(a, b, idx_a, idx_b, weight)] of a case for one loss"""
    if 'weights' not in case:
        return case['pairs']
    return [p + (w,) for p, w in zip(case['pairs'], case['weights'][plane])]


def n_points(case):
    seen = {id(s): len(s['depth']) for s in case['scans']}
    return sum(seen.values())


def reference(case, plane, flaws=(), poses=None):
    """(value, magnitude) of the case in the sequence layout -- for a pair case in the pair layout -- once per process; points next to a
    float32 tie are redrawn in the case (depth only, never a designed point) until none is left."""
    key = (case['name'], 'weights' in case, plane, tuple(flaws), None if poses is None else np.asarray(poses).tobytes())
    if key in _refs:
        return _refs[key]
    P = case['poses'] if poses is None else poses
    rng = _rng('redraw-' + case['name'])
    while True:
        if 'weights' in case:
            val, mag, ties = R.sequence(case['scans'], pairs_of(case, plane), P, case['model'], plane, flaws)
        else:
            a, b, ia, ib, _ = case['pairs'][0]
            val, mag, ties = R.pair(case['scans'][a], case['scans'][b], P[a], P[b], case['model'], ia, ib, plane, flaws)
            ties = set((a if side == 0 else b, i) for side, i in ties)
        if not ties or flaws:
            break
        assert poses is None, ('a point next to a float32 tie under poses the case was not built for', sorted(ties))
        for s, i in sorted(ties):
            assert i >= DESIGNED or len(case['scans'][s]['depth']) < DESIGNED, ('designed point next to a float32 tie', case['name'], s, i)
            case['scans'][s]['depth'][i] = rng.uniform(2.0, 30.0)
            case['redrawn'] += 1
        for k in [k for k in _refs if k[0] == case['name']]:
            del _refs[k]
        assert case['redrawn'] <= REDRAW_CAP * n_points(case), ('too many redrawn points', case['name'], case['redrawn'], n_points(case))
    for a in (val, mag):
        a.setflags(write=False)
    _refs[key] = (val, mag)
    return _refs[key]


def settle(case):
    """Both losses' references of a case, so that no point is redrawn after the inputs have been handed to a kernel"""
    while True:
        before = case['redrawn']
        reference(case, True)
        reference(case, False)
        if case['redrawn'] == before:
            return case


# ---- pose-chain cases -------------------------------------------------------------------------------------------------------------
POSE_COUNTS = (1, 2, 255, 256, 257, 600)
BELOW = float(np.nextafter(1e-6, 0.0))
ABOVE = float(np.nextafter(1e-6, 1.0))
CORRECTIONS = ('zero', 'tiny', 'below0', 'at1', 'above2', 'generic', 'near_pi', 'pi2.5', 'at0', 'below2')


def correction(kind, rng):
    """One 6-vector: a translation of a few decimetres and an axis-angle of the named kind.  Axis-aligned ones make theta exact."""
    d = np.zeros(6)
    d[:3] = rng.uniform(-0.5, 0.5, 3)
    u = rng.standard_normal(3)
    u /= np.linalg.norm(u)
    if kind == 'zero':
        pass
    elif kind == 'tiny':
        d[3:] = 1e-8 * u
    elif kind[:-1] in ('below', 'at', 'above'):
        d[3 + int(kind[-1])] = {'below': BELOW, 'at': 1e-6, 'above': ABOVE}[kind[:-1]] * (-1 if kind == 'at1' else 1)
    elif kind == 'generic':
        d[3:] = rng.uniform(0.01, 1.5) * u
    elif kind == 'near_pi':
        d[3:] = (np.pi - 1e-7) * u
    elif kind == 'pi2.5':
        d[3:] = 2.5 * np.pi * u
    else:
        raise ValueError(kind)
    return d


def make_poses44(n, rng):
    """[n,16] rigid poses a few hundred metres out"""
    T = np.zeros((n, 4, 4))
    T[:, :3, :] = make_poses(n, rng).reshape(n, 3, 4)
    T[:, 3, 3] = 1.0
    return T.reshape(n, 16)


def _chain_specs():
    sp = {}
    for n in POSE_COUNTS:
        sp['per-pose-%d' % n] = dict(n=n, shared=None)
        sp['shared-generic-%d' % n] = dict(n=n, shared='generic')
    for kind in CORRECTIONS:
        if kind != 'generic':
            sp['shared-%s-2' % kind] = dict(n=2, shared=kind)
    sp['shared-at0-257'] = dict(n=257, shared='at0')
    return sp


CHAIN_SPECS = _chain_specs()


def chain_case(name):
    """-> dict(T0 [n,16], deltas [n,6] or [1,6], grad [n,16]); per-pose corrections cycle through CORRECTIONS"""
    key = 'chain-' + name
    if key not in _cases:
        sp, rng = CHAIN_SPECS[name], _rng(key)
        n = sp['n']
        deltas = np.array([correction(sp['shared'], rng)]) if sp['shared'] else np.array([correction(CORRECTIONS[p % len(CORRECTIONS)], rng) for p in range(n)])
        _cases[key] = dict(name=name, T0=make_poses44(n, rng), deltas=deltas, grad=rng.standard_normal((n, 16)))
    return _cases[key]


def chain_reference(name):
    """-> dict(fwd=(value, magnitude) [n,16], bwd=(value, magnitude) [n_deltas,6])"""
    key = ('chain', name)
    if key not in _refs:
        c = chain_case(name)
        _refs[key] = dict(fwd=R.corrected_poses(c['T0'], c['deltas']), bwd=R.corrected_poses_bwd(c['T0'], c['deltas'], c['grad']))
    return _refs[key]


# ---- finishing-step cases ---------------------------------------------------------------------------------------------------------
def _finish_specs():
    """name -> dict(S, layout, shared, totals, zero_first, with_w, lr_w, ring_rows, n_extra, steps)"""
    sp = {}
    base = dict(layout=0, shared=False, totals=False, zero_first=1, with_w=True, lr_w=1e-3, ring_rows=1, n_extra=0, steps=1, P=3)
    add = lambda name, **kw: sp.__setitem__(name, dict(base, **kw))
    add('S1-ring1x4', S=1, steps=4, ring_rows=1, zero_first=0, n_extra=5)
    add('S2-ring3x4', S=2, steps=4, ring_rows=3, layout=1, n_extra=5, totals=True)
    add('S2-shared-x4', S=2, steps=4, ring_rows=3, shared=True, zero_first=0)
    add('S255', S=255, layout=1, shared=True)
    add('S256', S=256, zero_first=0, with_w=False)
    add('S257', S=257, layout=1, lr_w=0.0, n_extra=5, ring_rows=3)
    add('S257-shared', S=257, shared=True, totals=True, P=8)
    add('S600', S=600, layout=0, totals=True, ring_rows=3)
    add('S600-shared', S=600, layout=1, shared=True, zero_first=1, with_w=False)
    return sp


FINISH_SPECS = _finish_specs()
ADAM = dict(lr_d=2e-3, b1=0.9, b2=0.999, eps=1e-8)


def finish_case(name):
    """The state before the first step and the per-step inputs: dict(spec, T0 [S,16], delta, d_m, d_v [nd,6], w, w_m, w_v [P] | None,
    step0, sums [steps][n_sums], totals [steps][2+P] | None, extra [steps][n_extra], T_used [steps][S,16]).  Moments and the step
    counter start non-zero."""
    key = 'finish-' + name
    if key not in _cases:
        sp, rng = FINISH_SPECS[name], _rng(key)
        S, P, steps = sp['S'], sp['P'], sp['steps']
        nd = 1 if sp['shared'] else S
        head = 2 if sp['layout'] == 0 else 1
        kinds = CORRECTIONS
        delta = np.array([correction(kinds[(p + 5) % len(kinds)], rng) for p in range(nd)])
        sums = rng.standard_normal((steps, head + 2 * P + 12 * S))
        if sp['layout'] == 0:
            sums[:, 1] = rng.integers(1000, 5000, steps)
        totals = None
        if sp['totals']:
            totals = rng.standard_normal((steps, 2 + P))
            totals[:, 1] = rng.integers(2, 9000, steps)
        _cases[key] = dict(name=name, spec=sp, T0=make_poses44(S, rng), delta=delta, d_m=1e-2 * rng.standard_normal((nd, 6)),
                           d_v=1e-4 * rng.random((nd, 6)), w=(0.02 * rng.standard_normal(P) if sp['with_w'] else None),
                           w_m=(1e-2 * rng.standard_normal(P) if sp['with_w'] else None), w_v=(1e-4 * rng.random(P) if sp['with_w'] else None),
                           step0=int(rng.integers(1, 40)), sums=sums, totals=totals, extra=rng.standard_normal((steps, sp['n_extra'])),
                           T_used=np.stack([make_poses44(S, rng) for _ in range(steps)]))
    return _cases[key]


def finish_reference(case, k, state, flaws=()):
    """Step k of a finishing case from `state` = dict(w, w_m, w_v, delta, d_m, d_v, step): icploss_reference.finish_step's result"""
    sp = case['spec']
    return R.finish_step(case['sums'][k], sp['layout'], sp['P'], sp['S'], state['w'], state['w_m'], state['w_v'], case['T0'], state['delta'],
                         state['d_m'], state['d_v'], sp['zero_first'], state['step'], sp['lr_w'], ADAM['lr_d'], ADAM['b1'], ADAM['b2'], ADAM['eps'],
                         case['T_used'][k], totals=None if case['totals'] is None else case['totals'][k], rec_extra=case['extra'][k], flaws=flaws)


def finish_state0(case):
    return {f: (None if case[f] is None else np.array(case[f], copy=True)) for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v')} | dict(step=case['step0'])


def record_len(case):
    sp = case['spec']
    nd = 1 if sp['shared'] else sp['S']
    return (2 if sp['layout'] == 0 else 1) + 2 * sp['P'] + 12 * sp['S'] + sp['P'] + 6 * nd + 12 * sp['S'] + sp['n_extra']


# ---- comparing -------------------------------------------------------------------------------------------------------------------
def ratio(err, bound):
    """The largest |err| / bound; an error where the bound is zero counts as infinite"""
    err, bound = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def check_finish(case, k, before, got, T_next, worst, record=None, ref=None):
    """One step's outputs `got` (a state dict) and T_next against the reference started from `before` (or the given one); `worst`
    collects the largest error per output in units of its bound"""
    ref = finish_reference(case, k, before) if ref is None else ref
    assert got['step'] == ref['step'] == before['step'] + 1
    for f in ('w', 'w_m', 'w_v', 'delta', 'd_m', 'd_v'):
        if got[f] is None:
            assert f not in ref
            continue
        r = ratio(got[f] - ref[f][0], R.C_FINISH * U * ref[f][1])
        worst[f] = max(worst.get(f, 0.0), r)
        assert r <= 1.0, (case['name'], k, f, r)
    r = ratio(T_next - ref['T_next'][0], R.C_FINISH * U * ref['T_next'][1])
    worst['T_next'] = max(worst.get('T_next', 0.0), r)
    assert r <= 1.0, (case['name'], k, 'T_next', r)
    if record is not None:
        assert np.array_equal(record, ref['record']), (case['name'], k, 'record')
    return ref
