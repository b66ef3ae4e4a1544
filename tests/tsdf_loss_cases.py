"""Designed cases of the loss against the fused volume, at voxel size a = 1, origin 0, truncation tau = 2, with values written by hand
(nothing here goes through the oracle's trilinear form).  A point x has q = x - 0.5, corner 0 at i0 = floor(q), f = q - i0.

The total volume (every voxel below has count 2 unless noted; value = sum / (count 2^20)):
  LINEAR   voxels [-2, 10)^3 (27 blocks, coordinates -1, 0, 1): value(i) = 1/4 + ix/32 + iy/64 + iz/128.  The trilinear form of a
           linear field is the field, and every operation on these dyadic numbers is exact:
               phi(x) = 2 value(q) = 1/2 + qx/16 + qy/32 + qz/64,  grad = (1/16, 1/32, 1/64).
           It serves the corners at block 0 / -1 on each axis and at local index 7 over two, four and eight blocks.
  LAYERS   voxels {33, 34} x {1, 2}^2 (block (4, 0, 0)): value 1/4 on the layer z = 1 and 3/4 on z = 2.  At x = (34, 2, 2.25): f =
           (1/2, 1/2, 3/4), value = 1/4 + 3/4 (3/4 - 1/4) = 5/8, phi = 5/4, grad = (0, 0, 2 (3/4 - 1/4)) = (0, 0, 1).
  ZERO     voxels {49, 50} x {3, 4}^2 (block (6, 0, 0)): value -1/8 on z = 3 and +1/8 on z = 4.  At x = (50, 4, 4): f = 1/2 on every
           axis, phi = 0, grad = (0, 0, 2 (1/4)) = (0, 0, 1/2).
  ALONE    voxels {65, 66} x {1, 2}^2 (block (8, 0, 0)), count 1, value 1/2: at x = (66, 2, 2) phi = 1, grad = 0.
The own volume OWN_A (the volume of "scan 0 alone"; every voxel has count 1):
  LAYERS   value 1/2 on z = 1 (sum 2^19) and 1 on z = 2 (sum 2^20).  What is left has count 1 and the sums (1/4) 2 2^20 - 2^19 = 0 and
           (3/4) 2 2^20 - 2^20 = 2^19, so the values 0 and 1/2: at x = (34, 2, 2.25) value = 3/4 (1/2) = 3/8, phi = 3/4, grad = (0, 0, 1).
           With min_count = 2 the count left, 1, is min_count - 1: unobserved.  With min_count = 1 it equals min_count: observed.
  ALONE    the same sums and counts as the total: nothing is left, the block is in the total table only because of the own scan:
           unobserved.
  OWN_A has no LINEAR and no ZERO block (an own block missing: the total's values).  OWN_NONE has no block at all.
"""
import numpy as np

import tsdf_sparse_reference as S
from tsdf_sparse_cases import RANDOM, random_scans

A, TAU = 1.0, 2.0
ONE = 2 ** 20
USED, INVALID, UNOBSERVED, GATED, MASKED = 0, 1, 2, 3, 255
NAN = float('nan')


def build(voxels):
    """A SparseVolume holding ``voxels`` {(ix, iy, iz): (sum, count)}; the slots are handed out in DESCENDING key order, so that a
    position in the table is never its slot."""
    vol = S.SparseVolume(A, trunc=TAU, capacity=1)
    idx = np.array(sorted(voxels), np.int64).reshape(-1, 3)
    keys = np.unique(S.block_key(idx >> 3)) if len(idx) else np.zeros(0, np.uint64)
    nb = keys.shape[0]
    vol.capacity = max(nb, 1)
    vol.keys, vol.slots = keys, np.arange(nb, dtype=np.int32)[::-1].copy()
    vol.sum, vol.count = np.zeros((vol.capacity, 512), np.int64), np.zeros((vol.capacity, 512), np.int32)
    for i, (sm, cnt) in voxels.items():
        i = np.array(i, np.int64)
        slot = vol.slots[vol.find(S.block_key((i >> 3)[None, :]))[0]]
        local = ((i[0] & 7) * 8 + (i[1] & 7)) * 8 + (i[2] & 7)
        vol.sum[slot, local], vol.count[slot, local] = sm, cnt
    return vol


def _box(lo, hi):
    return [(x, y, z) for x in range(lo[0], hi[0]) for y in range(lo[1], hi[1]) for z in range(lo[2], hi[2])]


def _total_voxels():
    v = {}
    for i in _box((-2, -2, -2), (10, 10, 10)):
        # value = 1/4 + ix/32 + iy/64 + iz/128 at count 2: sum = 2 value 2^20, an integer
        v[i] = (2 * (ONE // 4 + i[0] * (ONE // 32) + i[1] * (ONE // 64) + i[2] * (ONE // 128)), 2)
    for i in _box((33, 1, 1), (35, 3, 3)):
        v[i] = (2 * (ONE // 4 if i[2] == 1 else 3 * ONE // 4), 2)
    for i in _box((49, 3, 3), (51, 5, 5)):
        v[i] = (2 * (-ONE // 8 if i[2] == 3 else ONE // 8), 2)
    for i in _box((65, 1, 1), (67, 3, 3)):
        v[i] = (ONE // 2, 1)
    return v


def _own_voxels():
    v = {}
    for i in _box((33, 1, 1), (35, 3, 3)):
        v[i] = (ONE // 2 if i[2] == 1 else ONE, 1)
    for i in _box((65, 1, 1), (67, 3, 3)):
        v[i] = (ONE // 2, 1)
    return v


def volumes():
    """(TOTAL, OWN_A, OWN_NONE)"""
    return build(_total_voxels()), build(_own_voxels()), build({})


def _linear(x):
    q = [c - 0.5 for c in x]
    return 0.5 + q[0] / 16 + q[1] / 32 + q[2] / 64, (1 / 16, 1 / 32, 1 / 64)


_LIN = {
    'block -1 | 0 on x': (0.25, 2.0, 3.0), 'block -1 | 0 on y': (2.0, 0.25, 3.0), 'block -1 | 0 on z': (2.0, 3.0, 0.25),
    'block -1 | 0 on every axis': (0.25, 0.375, -0.25),
    'local 7 over two blocks': (8.0, 2.0, 3.0), 'local 7 over four blocks': (8.0, 8.25, 3.0), 'local 7 over eight blocks': (8.0, 8.25, 7.75),
}
X_LAYERS, X_ZERO, X_ALONE = (34.0, 2.0, 2.25), (50.0, 4.0, 4.0), (66.0, 2.0, 2.0)
JUST_ABOVE = float(np.nextafter(1.25, 2.0))


def point_cases():
    """[dict(name, own ('A', 'none' or None), x, min_count, max_residual, cls, phi, grad)]; phi NaN / grad 0 where the sample is not
    valid.  The term follows from phi and grad by the rule, in either form."""
    out = []

    def add(name, own, x, cls, phi=NAN, grad=(0.0, 0.0, 0.0), min_count=1, max_residual=TAU):
        out.append(dict(name=name, own=own, x=tuple(float(c) for c in x), min_count=min_count, max_residual=max_residual, cls=cls, phi=phi,
                        grad=tuple(grad)))
    for name, x in _LIN.items():
        phi, grad = _linear(x)
        add('total only, ' + name, None, x, USED, phi, grad)
        add('own block missing, ' + name, 'A', x, USED, phi, grad)
    add('total only, layers', None, X_LAYERS, USED, 1.25, (0.0, 0.0, 1.0))
    add('own table without blocks, layers', 'none', X_LAYERS, USED, 1.25, (0.0, 0.0, 1.0))
    add('own block present: count left = min_count', 'A', X_LAYERS, USED, 0.75, (0.0, 0.0, 1.0))
    add('own block present: count left = min_count - 1', 'A', X_LAYERS, UNOBSERVED, min_count=2)
    add('total only at min_count 2', None, X_LAYERS, USED, 1.25, (0.0, 0.0, 1.0), min_count=2)
    add('total only at min_count 3', None, X_LAYERS, UNOBSERVED, min_count=3)
    add('block in the total only because of the own scan', 'A', X_ALONE, UNOBSERVED)
    add('the same block without exclusion', None, X_ALONE, USED, 1.0, (0.0, 0.0, 0.0))
    add('phi = 0', None, X_ZERO, USED, 0.0, (0.0, 0.0, 0.5))
    add('|phi| one ulp below max_residual', None, X_LAYERS, USED, 1.25, (0.0, 0.0, 1.0), max_residual=JUST_ABOVE)
    add('|phi| equal to max_residual', None, X_LAYERS, GATED, 1.25, (0.0, 0.0, 1.0), max_residual=1.25)
    add('a NaN point', None, (NAN, 1.0, 1.0), INVALID)
    add('an infinite point', 'A', (1.0, float('inf'), 1.0), INVALID)
    add('outside every block', None, (200.0, 2.0, 2.0), UNOBSERVED)
    add('half inside the linear box', None, (10.0, 2.0, 3.0), UNOBSERVED)
    return out


def call_case(dtype=np.float64):
    """The whole call on three scans, the middle one empty, identity poses, no model: x = vp + 1 (0, 0, 1) exactly.  Scan 0 carries OWN_A,
    scans 1 and 2 OWN_NONE.  Returns dict(scans, poses, mask, total, owns, cls [N], phi [N], grad [N, 3]) at min_count 1 and
    max_residual tau; a masked point and a NaN point sit in scan 2."""
    total, own_a, own_none = volumes()
    xs = list(_LIN.values()) + [X_LAYERS, X_ZERO, X_ALONE, (200.0, 2.0, 2.0)]
    exp0, exp2 = [], []
    for x in xs:
        if x in _LIN.values():
            e = (USED,) + _linear(x)
            exp0.append(e)
            exp2.append(e)
    exp0 += [(USED, 0.75, (0.0, 0.0, 1.0)), (USED, 0.0, (0.0, 0.0, 0.5)), (UNOBSERVED, NAN, (0.0, 0.0, 0.0)), (UNOBSERVED, NAN, (0.0, 0.0, 0.0))]
    exp2 += [(USED, 1.25, (0.0, 0.0, 1.0)), (USED, 0.0, (0.0, 0.0, 0.5)), (USED, 1.0, (0.0, 0.0, 0.0)), (UNOBSERVED, NAN, (0.0, 0.0, 0.0))]
    x2 = xs + [X_LAYERS, (NAN, 1.0, 1.0)]                              # the masked point, then the NaN point
    exp2 += [(MASKED, NAN, (0.0, 0.0, 0.0)), (INVALID, NAN, (0.0, 0.0, 0.0))]

    def scan(points):
        p = np.array(points, np.float64).reshape(-1, 3)
        n = p.shape[0]
        return dict(vps=(p - np.array([0.0, 0.0, 1.0])).astype(dtype), dirs=np.tile(np.array([0.0, 0.0, 1.0], dtype), (n, 1)),
                    depth=np.ones(n, dtype), inc=np.zeros(n, dtype), lmask=np.ones(n, bool))
    scans = [scan(xs), scan([]), scan(x2)]
    mask = np.ones(len(xs) + len(x2), bool)
    mask[len(xs) + len(xs)] = False
    exp = exp0 + exp2
    return dict(scans=scans, poses=np.tile(np.eye(4), (3, 1, 1)), mask=mask, total=total, owns=[own_a, own_none, own_none],
                cls=np.array([e[0] for e in exp], np.uint8), phi=np.array([e[1] for e in exp]), grad=np.array([e[2] for e in exp]))


# ---- what the host and the device tests share ------------------------------------------------------------------------------------------
DTYPES = {'float32': (np.float32, 0), 'float64': (np.float64, 1)}              # numpy type, DC_F32 / DC_F64
MODELS = {None: ((), ()), 'ScaledPolynomial': ([0.004, -0.002], [2.0, 4.0]), 'Polynomial': ([0.003, -0.001], [2.0, 3.5])}
# the re-fuse / gradient-descent loop that the device follows step by step, and the largest change of the oracle's own w over those
# steps and 200 random orders of its gradient sum (7.2858e-17, measured on the CPU; test_tsdf_loss_host.py recomputes it over three)
LOOP_STEPS, LOOP_LR = 6, 0.25
W_SENSITIVITY = 7.29e-17


COUNTS = ('used', 'gated', 'unobserved', 'invalid')


def assert_within_bounds(got, ref, what, with_e=True, factor=1.0):
    """Counts equal; loss and every gradient entry within ``factor`` x tsdf_loss_reference.bound; returns the largest ratio."""
    assert tuple(got[k] for k in COUNTS) == tuple(ref[k] for k in COUNTS), (what, [got[k] for k in COUNTS], [ref[k] for k in COUNTS])
    worst = 0.0
    if ref['used'] == 0:
        assert np.isnan(got['loss']) and not got['gw'].any() and not got['ge'].any() and not got['gT'].any(), what
        return worst
    for name in ('loss', 'gw', 'ge', 'gT'):
        want = np.asarray(ref[name]) if (name != 'ge' or with_e) else np.zeros_like(ref['ge'])
        err, bar = np.abs(np.asarray(got[name]) - want), factor * np.asarray(_reference().bound(ref, name))
        if not want.size:
            continue
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(np.max(ratio)))
        assert (err <= bar).all(), (what, name, got[name], want, err, bar)
    return worst


def _reference():
    import tsdf_loss_reference
    return tsdf_loss_reference


def random_scene(dtype, n_sets=2):
    """(scans, poses, total, owns): the posed, masked scans of tests/tsdf_sparse_cases.py (NaN rows, infinite depths, negative blocks)
    with random incidence angles, fused at RANDOM's lattice with their depths as they are."""
    npdt = DTYPES[dtype][0]
    rng = np.random.default_rng(5)
    batches = []
    for k in range(n_sets):
        batches += random_scans(offset=(0.3 * k, -0.2 * k, 0.1 * k))
    scans, poses = [], []
    for b in batches:
        n = len(b['depth'])
        scans.append(dict(vps=np.asarray(b['vps']).astype(npdt), dirs=np.asarray(b['dirs']).astype(npdt), depth=np.asarray(b['depth']).astype(npdt),
                          inc=rng.uniform(0.0, 1.3, n).astype(npdt), lmask=np.asarray(b['mask']).astype(bool),
                          rules=dict(min_depth=b['min_depth'], max_range=b['max_range'])))
        poses.append(np.asarray(b['pose'], np.float64))

    def fuse(which):
        vol = S.SparseVolume(RANDOM['voxel'], trunc=RANDOM['trunc'], origin=RANDOM['origin'], capacity=64)
        for s in which:
            c = scans[s]
            S.fuse(vol, vps=c['vps'], dirs=c['dirs'], depth=c['depth'], pose=poses[s], mask=c['lmask'], **c['rules'])
        return vol
    ns = len(scans)
    return scans, np.stack(poses), fuse(range(ns)), [fuse([s]) for s in range(ns)], fuse


MODELS = {None: ((), ()), 'ScaledPolynomial': ([0.004, -0.002], [2.0, 4.0]), 'Polynomial': ([0.003, -0.001], [2.0, 3.5])}
