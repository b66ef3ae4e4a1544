"""numpy oracle of the ray cast against the fused volume, written from the rule of DESIGN "Ray casting the fused volume" (not from the
kernel or the package), on top of tests/tsdf_loss_reference.py (the sample with exclusion) and tests/tsdf_sparse_reference.py (the
volumes).  It is the NAIVE march: every j is sampled, nothing is skipped.

Ray.  o = R vp + t, u = R dir, each row sum ((R0 v0 + R1 v1) + R2 v2) (+ t).  SKIPPED: mask 0, o or u not finite, u = 0.
Samples.  t_j = t_min + (double)j step, j = 0 .. J = floor((t_max - t_min) / step); p_j = o + t_j u; sample_minus(total, own, p_j).
March.  An invalid sample breaks the bracket; a valid one with phi > 0 opens it or moves its near end; the first valid one with phi <= 0
stops the march: a crossing iff the sample before it was valid with phi > 0, else BEHIND.  No stop: MISS.
Refinement.  t* = t0 + (t1 - t0) (phi0 / (phi0 - phi1)); ``refine`` rounds: sample at t*, invalid: LOST, phi* > 0 replaces the near end,
otherwise the far end, t* again.  The last sample at t* gives phi and the gradient g; invalid or g = 0: LOST.
Hit.  t = t*, normal = g / sqrt((g0 g0 + g1 g1) + g2 g2), cos(inc) = min(1, |n . u| / (sqrt(n . n) sqrt(u . u))) with x . y = (x0 y0 + x1
y1) + x2 y2, face = the table position of the block of the last sample's base voxel.  Not a hit: face -1, t +inf, inc / normal / phi NaN.

``samples`` is the number of samples taken (every j reached, every refinement sample); ``samples_read`` counts of those the ones that
are in range and whose base voxel's block is in the table -- what a march that skips absent blocks still has to read voxels for.
"""
import math

import numpy as np

import tsdf_loss_reference as L
import tsdf_sparse_reference as S
import tsdf_track_reference as K

HIT, SKIPPED, MISS, BEHIND, LOST = 0, 1, 2, 3, 4
FIELDS = ('face', 't', 'inc', 'normal', 'phi', 'status')


def steps(t_min, t_max, step):
    return int(math.floor((t_max - t_min) / step))


def rays(vps, dirs, pose):
    """(o [n, 3], u [n, 3]) of the rule for one scan."""
    vps, dirs = np.asarray(vps).astype(np.float64).reshape(-1, 3), np.asarray(dirs).astype(np.float64).reshape(-1, 3)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    with np.errstate(all='ignore'):
        o = np.stack([((T[r, 0] * vps[:, 0] + T[r, 1] * vps[:, 1]) + T[r, 2] * vps[:, 2]) + T[r, 3] for r in range(3)], axis=1)
        u = np.stack([(T[r, 0] * dirs[:, 0] + T[r, 1] * dirs[:, 1]) + T[r, 2] * dirs[:, 2] for r in range(3)], axis=1)
    return o, u


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def _sample(total, own, o, u, t, min_count):
    """sample_minus at o + t u (t a float or [m]) and whether each sample would read voxels."""
    t = np.broadcast_to(np.asarray(t, np.float64), (o.shape[0],))
    with np.errstate(all='ignore'):
        p = o + t[:, None] * u
    smp = L.sample_minus(total, own, p, min_count)
    in_range = smp['flag'] != K.RANGE
    read = np.zeros(o.shape[0], bool)
    if in_range.any():
        read[in_range] = total.find(S.block_key(smp['i0'][in_range] >> 3)) >= 0
    return smp, read


def cast_scan(total, own, o, u, use, t_min, t_max, step, refine=2, min_count=1):
    """The rule for the rays (o, u) [n, 3] of one scan against ``total`` minus ``own`` (None: nothing taken out); ``use`` bool [n]: the
    rays that are not SKIPPED."""
    n = o.shape[0]
    J = steps(t_min, t_max, step)
    out = dict(face=np.full(n, -1, np.int32), t=np.full(n, np.inf), inc=np.full(n, np.nan), normal=np.full((n, 3), np.nan),
               phi=np.full(n, np.nan), status=np.where(use, MISS, SKIPPED).astype(np.uint8), samples=np.zeros(n, np.int32),
               samples_read=np.zeros(n, np.int32))
    active = use.copy()
    open_ = np.zeros(n, bool)
    crossing = np.zeros(n, bool)
    t0, phi0, t1, phi1 = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(J + 1):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        t = t_min + float(j) * step
        smp, read = _sample(total, own, o[idx], u[idx], t, min_count)
        out['samples'][idx] += 1
        out['samples_read'][idx] += read
        valid = smp['flag'] == 0
        front = valid & (smp['value'] > 0.0)
        stop = valid & ~front
        open_[idx[~valid]] = False
        k = idx[front]
        open_[k], t0[k], phi0[k] = True, t, smp['value'][front]
        k = idx[stop]
        t1[k], phi1[k], crossing[k] = t, smp['value'][stop], open_[k]
        out['status'][k] = np.where(open_[k], LOST, BEHIND)               # a crossing is LOST until its last sample stands
        active[k] = False
    idx = np.nonzero(crossing)[0]
    if idx.size == 0:
        return out
    secant = lambda a: t0[a] + (t1[a] - t0[a]) * (phi0[a] / (phi0[a] - phi1[a]))
    ts = np.zeros(n)
    ts[idx] = secant(idx)
    for _ in range(refine):
        if idx.size == 0:
            break
        smp, read = _sample(total, own, o[idx], u[idx], ts[idx], min_count)
        out['samples'][idx] += 1
        out['samples_read'][idx] += read
        valid = smp['flag'] == 0
        front = valid & (smp['value'] > 0.0)
        back = valid & ~front
        k = idx[front]
        t0[k], phi0[k] = ts[k], smp['value'][front]
        k = idx[back]
        t1[k], phi1[k] = ts[k], smp['value'][back]
        idx = idx[valid]
        ts[idx] = secant(idx)
    if idx.size == 0:
        return out
    smp, read = _sample(total, own, o[idx], u[idx], ts[idx], min_count)
    out['samples'][idx] += 1
    out['samples_read'][idx] += read
    g = smp['grad']
    hit = (smp['flag'] == 0) & (g != 0.0).any(axis=1)
    k, g = idx[hit], g[hit]
    nrm = g / np.sqrt(_dot(g, g))[:, None]
    cos = np.abs(_dot(nrm, u[k])) / (np.sqrt(_dot(nrm, nrm)) * np.sqrt(_dot(u[k], u[k])))
    out['face'][k] = total.find(S.block_key(smp['i0'][hit] >> 3))
    out['t'][k], out['normal'][k], out['phi'][k], out['status'][k] = ts[k], nrm, smp['value'][hit], HIT
    out['inc'][k] = np.arccos(np.minimum(1.0, cos))
    return out


def cast(total, owns, vps, dirs, scan_offset, poses, t_min=0.0, t_max=100.0, step=None, refine=2, min_count=1, mask=None):
    """The whole call: rays vps / dirs [N, 3] scan-major, scan s = rows scan_offset[s] .. scan_offset[s + 1] under poses[s]; owns: one
    SparseVolume per scan, or None.  Returns the dict of the outputs plus ``samples_read``."""
    dirs = np.asarray(dirs).reshape(-1, 3)
    n = dirs.shape[0]
    vps = np.asarray(vps).reshape(-1, 3)
    step = total.voxel / 2.0 if step is None else float(step)
    assert 0.0 <= t_min < t_max and math.isfinite(t_max) and 0.0 < step <= total.trunc and steps(t_min, t_max, step) <= 2 ** 24
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0
    parts = []
    for s in range(len(scan_offset) - 1):
        a, b = int(scan_offset[s]), int(scan_offset[s + 1])
        o, u = rays(vps[a:b], dirs[a:b], np.asarray(poses, np.float64).reshape(-1, 4, 4)[s])
        use = keep[a:b] & np.isfinite(o).all(axis=1) & np.isfinite(u).all(axis=1) & (u != 0.0).any(axis=1)
        o, u = np.where(use[:, None], o, 0.0), np.where(use[:, None], u, 0.0)
        parts.append(cast_scan(total, None if owns is None else owns[s], o, u, use, t_min, t_max, step, refine, min_count))
    if not parts:
        parts = [cast_scan(total, None, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, bool), t_min, t_max, step, refine, min_count)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def assert_equal(got, want, what='', samples=None):
    """``got`` equals the oracle's ``want``: face, status, t, normal and phi to the bit (NaN == NaN), inc through cos(inc) within 1e-13 (the
    bar of tests/test_gpu_raycast_edge.py), NaN where the oracle has NaN.  ``samples``: the oracle's field ``got['samples']`` must equal."""
    for k in ('status', 'face'):
        assert np.array_equal(np.asarray(got[k]), want[k]), (what, k, np.nonzero(np.asarray(got[k]) != want[k])[0][:8])
    for k in ('t', 'phi', 'normal'):
        a, b = np.ascontiguousarray(got[k], np.float64), np.ascontiguousarray(want[k], np.float64)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (what, k, np.nonzero(~same.reshape(a.shape[0], -1).all(axis=1))[0][:8])
    a, b = np.asarray(got['inc'], np.float64), want['inc']
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, 'inc')
    ok = ~np.isnan(b)
    if ok.any():
        assert float(np.abs(np.cos(a[ok]) - np.cos(b[ok])).max()) <= 1e-13, (what, 'inc', float(np.abs(np.cos(a[ok]) - np.cos(b[ok])).max()))
    if samples is not None:
        assert np.array_equal(np.asarray(got['samples']), want[samples]), (what, samples)


# ---- designed volumes and rays, written by hand at a = 1, og = 0 -----------------------------------------------------------------------
ONE = 2 ** 20
NAN, INF = float('nan'), float('inf')


def build(voxels, trunc=2.0):
    """A SparseVolume (a = 1, og = 0) holding ``voxels`` {(ix, iy, iz): (sum, count)}; the slots are handed out in DESCENDING key order,
    so that a position in the table is never its slot."""
    vol = S.SparseVolume(1.0, trunc=trunc, capacity=1)
    idx = np.array(sorted(voxels), np.int64).reshape(-1, 3)
    keys = np.unique(S.block_key(idx >> 3)) if len(idx) else np.zeros(0, np.uint64)
    nb = keys.shape[0]
    vol.capacity = max(nb, 1)
    vol.keys, vol.slots = keys, np.arange(nb, dtype=np.int32)[::-1].copy()
    vol.sum, vol.count = np.zeros((vol.capacity, 512), np.int64), np.zeros((vol.capacity, 512), np.int32)
    pos = vol.find(S.block_key(idx >> 3))
    local = ((idx[:, 0] & 7) * 8 + (idx[:, 1] & 7)) * 8 + (idx[:, 2] & 7)
    vals = np.array([voxels[tuple(i)] for i in idx.tolist()], np.int64).reshape(-1, 2)
    vol.sum[vol.slots[pos], local], vol.count[vol.slots[pos], local] = vals[:, 0], vals[:, 1]
    return vol


def wall_voxels(x_lo=0, x_hi=32, zero=16, slope=16, yz=(0, 8), y0=0, count=2, sign=1):
    """value(ix) = sign (zero - ix) / slope on ix in [x_lo, x_hi), iy in y0 + yz, iz in yz: linear in the x index with a power-of-two slope,
    so every interpolation is exact; phi(q) = tau sign (zero - qx) / slope, zero at x = zero + 1/2."""
    return {(x, y0 + y, z): (sign * count * (zero - x) * (ONE // slope), count) for x in range(x_lo, x_hi) for y in range(*yz)
            for z in range(*yz)}


def volumes():
    """The designed volumes by name.
      WALL     ix in [0, 32) (blocks 0 .. 3 on x), count 2, value (16 - ix) / 16, tau 2: phi = (16 - qx) / 8, the surface x = 16.5, the
               normal (-1, 0, 0).
      THIN     WALL with the count of voxel (11, 1, 1) at 1 = min_count - 1 for min_count = 2 (its value unchanged).
      GAP      WALL without its block 1 (ix in [8, 16)).
      BEND     value (16 - ix) (8 + iy) / 256: the same surface, a field that is quadratic along an oblique ray.
      HOLE     WALL at tau 3 with the voxels (15, 3, 1) and (17, 2, 1) unobserved.
      FAR      one block (200, 0, 0), value (1604 - ix) / 4: 200 absent blocks in front of it along +x.
      CORNER   one block (200, 200, 200), the same values: the diagonal from the origin runs through block corners.
      MINUS    one block (-200, -100, 0), value (ix + 1596) / 4: free towards +x, met from there through negative blocks."""
    wall = wall_voxels()
    thin = dict(wall)
    thin[(11, 1, 1)] = ((16 - 11) * (ONE // 16), 1)
    gap = {i: v for i, v in wall.items() if not 8 <= i[0] < 16}
    bend = {(x, y, z): (2 * (16 - x) * (8 + y) * (ONE // 256), 2) for x in range(32) for y in range(8) for z in range(8)}
    hole = {i: v for i, v in wall.items() if i not in ((15, 3, 1), (17, 2, 1))}
    far = wall_voxels(1600, 1608, 1604, 4)
    corner = {(x, 1600 + y, 1600 + z): v for (x, y, z), v in far.items()}
    minus = wall_voxels(-1600, -1592, -1596, 4, y0=-800, sign=-1)
    return dict(WALL=build(wall), THIN=build(thin), GAP=build(gap), BEND=build(bend), HOLE=build(hole, trunc=3.0), FAR=build(far),
                CORNER=build(corner), MINUS=build(minus))


S2 = math.sqrt(2.0)


def _case(name, volume, vp, dir_, status, t=INF, normal=(NAN, NAN, NAN), cos_inc=NAN, phi=NAN, face=-1, **kw):
    return dict(name=name, volume=volume, vp=vp, dir=dir_, status=status, t=t, normal=normal, cos_inc=cos_inc, phi=phi, face=face, kw=kw)


def ray_cases():
    """Single rays with their results by hand (step 1/2 = a / 2 and t_max 10 unless a case says otherwise).  With x = vp + t dir and q = x -
    1/2, WALL has phi = (16 - qx) / 8."""
    X, Y = (1.0, 0.0, 0.0), (2.0, 2.0)
    out = [
        # q = 13.75 + j / 2: phi_4 = 1/32 at t = 2, phi_5 = -1/32 at t = 2.5, t* = 2 + (1/2)(1/2); base voxel (16, 1, 1) in block 2
        _case('wall, +x', 'WALL', (14.25,) + Y, X, HIT, 2.25, (-1.0, 0.0, 0.0), 1.0, 0.0, 2),
        # qx = 13.75 + t, qy = 0.25 + t: the same crossing in units of |dir| = sqrt 2, at 45 degrees
        _case('wall, dir (1, 1, 0)', 'WALL', (14.25, 0.75, 2.0), (1.0, 1.0, 0.0), HIT, 2.25, (-1.0, 0.0, 0.0), 1.0 / S2, 0.0, 2),
        _case('wall, -x from behind', 'WALL', (20.0,) + Y, (-1.0, 0.0, 0.0), BEHIND),
        # q = 13.5 + j / 2: phi_5 = 0 exactly
        _case('crossing at a sample', 'WALL', (14.0,) + Y, X, HIT, 2.5, (-1.0, 0.0, 0.0), 1.0, 0.0, 2),
        _case('phi_0 < 0', 'WALL', (18.0,) + Y, X, BEHIND),
        _case('phi_0 == 0', 'WALL', (16.5,) + Y, X, BEHIND),
        _case('t_min beyond the wall, in the volume', 'WALL', (14.25,) + Y, X, BEHIND, t_min=3.0),
        _case('t_min beyond the volume', 'WALL', (14.25,) + Y, X, MISS, t_min=30.0, t_max=35.0),
        _case('t_max one step short', 'WALL', (14.25,) + Y, X, MISS, t_max=2.0),
        _case('t_max at the far end of the bracket', 'WALL', (14.25,) + Y, X, HIT, 2.25, (-1.0, 0.0, 0.0), 1.0, 0.0, 2, t_max=2.5),
        # dir (8, 0, 0), step 1: q = 3, 11, 19 with the corners {3, 4}, {11, 12}, {19, 20} on x: phi = 13/8, 5/8, -3/8
        _case('broken bracket, count = min_count - 1', 'THIN', (3.5,) + Y, (8.0, 0.0, 0.0), BEHIND, step=1.0, t_max=3.0, min_count=2),
        _case('broken bracket, missing block', 'GAP', (3.5,) + Y, (8.0, 0.0, 0.0), BEHIND, step=1.0, t_max=3.0, min_count=2),
        # t* = 1 + (5/8) / (5/8 + 3/8) = 1.625: q = 16; base voxel (16, 1, 1)
        _case('bracket whole, count = min_count', 'WALL', (3.5,) + Y, (8.0, 0.0, 0.0), HIT, 1.625, (-1.0, 0.0, 0.0), 1.0, 0.0, 2, step=1.0,
              t_max=3.0, min_count=2),
        # step 2 along (0.6, 0.8, 0): q = (15.1, 1.5), (16.3, 3.1); t* has q = (16, 2.7) up to rounding: its cell has the corners x {15, 16} or
        # {16, 17}, y {2, 3} -- one of the two voxels HOLE lacks, which neither end of the bracket touches
        _case('refinement sample unobserved', 'HOLE', (15.6, 2.0, 2.0), (0.6, 0.8, 0.0), LOST, step=2.0),
        _case('the same ray, volume whole', 'WALL', (15.6, 2.0, 2.0), (0.6, 0.8, 0.0), HIT, None, (-1.0, 0.0, 0.0), 0.6, None, None, step=2.0),
        _case('mask 0', 'WALL', (14.25,) + Y, X, SKIPPED, mask=0),
        _case('NaN in vp', 'WALL', (14.25, NAN, 2.0), X, SKIPPED),
        _case('inf in vp', 'WALL', (INF, 2.0, 2.0), X, SKIPPED),
        _case('NaN in dir', 'WALL', (14.25,) + Y, (1.0, 0.0, NAN), SKIPPED),
        _case('inf in dir', 'WALL', (14.25,) + Y, (-INF, 0.0, 0.0), SKIPPED),
        _case('dir = 0', 'WALL', (14.25,) + Y, (0.0, 0.0, 0.0), SKIPPED),
        # q reaches 2^23 - 1 after a few samples: flag RANGE, the march goes on to t_max
        _case('leaves the lattice range', 'WALL', (8388600.0,) + Y, X, MISS, t_max=20.0),
    ]
    return out


BEND_RAY = dict(volume='BEND', vp=(14.3, 1.1, 2.2), dir=(0.8, 0.55, 0.1))
REFINES = (0, 1, 2, 4)


def skip_cases():
    """Rays through 200 absent blocks to a block with a wall (step 1/2, t_max 1700: J = 3400): along an axis, along the diagonal through
    block corners, and with negative direction components through negative blocks.  t by hand."""
    return [
        # q = 0.25 + j / 2; phi = (1604 - qx) / 2 is 1/8 at t = 1603.5 and -1/8 at t = 1604
        _case('axis', 'FAR', (0.75, 2.0, 2.0), (1.0, 0.0, 0.0), HIT, 1603.75, (-1.0, 0.0, 0.0), 1.0, 0.0, 0),
        # q = t (1, 1, 1): phi = 0 exactly at the sample t = 1604
        _case('diagonal', 'CORNER', (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), HIT, 1604.0, (-1.0, 0.0, 0.0), 1.0 / math.sqrt(3.0), 0.0, 0),
        # q = (-1.25 - t, -0.9 - t / 2, 1.5); phi = (qx + 1596) / 2 is 1/8 at t = 1594.5 and -1/8 at t = 1595
        _case('negative', 'MINUS', (-0.75, -0.4, 2.0), (-1.0, -0.5, 0.0), HIT, 1594.75, (1.0, 0.0, 0.0), 1.0 / math.sqrt(1.25), 0.0, 0),
    ]


SKIP_KW = dict(t_max=1700.0)
DEFAULT_KW = dict(t_min=0.0, t_max=10.0, step=0.5, refine=2, min_count=1)
IDENTITY = np.eye(4)[None]


def run_case(cast_fn, vols, case, **over):
    """cast_fn(volume, vps [1, 3], dirs [1, 3], mask or None, **rule) for one case -> its output dict."""
    kw = dict(DEFAULT_KW, **case['kw'])
    kw.update(over)
    mask = kw.pop('mask', None)
    return cast_fn(vols[case['volume']], np.array([case['vp']], np.float64), np.array([case['dir']], np.float64),
                   None if mask is None else np.array([mask], np.uint8), **kw)


def assert_hand(got, case):
    """The outputs of one ray against the case's hand-computed values (None: not stated by hand)."""
    name = case['name']
    assert int(got['status'][0]) == case['status'], (name, int(got['status'][0]))
    if case['status'] != HIT:
        assert int(got['face'][0]) == -1 and got['t'][0] == INF and np.isnan(got['inc'][0]) and np.isnan(got['normal'][0]).all() and \
            np.isnan(got['phi'][0]), name
        return
    if case['t'] is not None:
        assert got['t'][0] == case['t'], (name, got['t'][0])
    if case['phi'] is not None:
        assert got['phi'][0] == case['phi'], (name, got['phi'][0])
    if case['face'] is not None:
        assert int(got['face'][0]) == case['face'], (name, int(got['face'][0]))
    assert np.array_equal(np.asarray(got['normal'][0]) + 0.0, np.asarray(case['normal']) + 0.0), (name, got['normal'][0])
    assert abs(math.cos(got['inc'][0]) - case['cos_inc']) <= 1e-13, (name, got['inc'][0])


# ---- the random posed scene of the sparse tests ------------------------------------------------------------------------------------------
_SCENES = {}


def random_scene(dtype):
    """The posed scans of tests/tsdf_loss_cases.random_scene (negative blocks, NaN rows; pools fused from ``dtype`` scans) with rays
    from the scans' view points towards their end points jittered by up to a voxel, ``dtype`` too.  The rays are chosen here, on the
    oracle alone: every candidate that hits and, of the others, at most twice as many, so that a third of the rays hit.  Returns
    dict(total, owns, fuse, vps, dirs, mask, offset, poses, rule, n, counts {status: rays}, oracle {(min_count, with own): outputs});
    computed once a process."""
    if dtype in _SCENES:
        return _SCENES[dtype]
    import tsdf_loss_cases as LC
    scans, poses, total, owns, fuse = LC.random_scene(dtype)
    npdt = LC.DTYPES[dtype][0]
    rng = np.random.default_rng(41)
    rule = dict(t_min=0.0, t_max=2.5, step=total.voxel / 2.0, refine=2)
    vps, dirs, mask, sizes = [], [], [], []
    for s, c in enumerate(scans):
        n = len(c['depth'])
        with np.errstate(all='ignore'):
            d = np.where(np.isfinite(c['depth'].astype(np.float64)), c['depth'].astype(np.float64), 1.0)
            end = c['vps'].astype(np.float64) + d[:, None] * c['dirs'].astype(np.float64) + rng.uniform(-0.1, 0.1, (n, 3))
            dr = ((end - c['vps'].astype(np.float64)) * rng.uniform(0.5, 1.5, (n, 1))).astype(npdt)        # not unit
        vp = c['vps'].astype(npdt)
        keep = np.ones(n, bool)
        keep[rng.integers(0, n, 6)] = False
        # choose on the oracle: no exclusion, min_count 1
        ref = cast(total, None, vp, dr, [0, n], poses[s:s + 1], mask=keep, **rule)
        hit = np.nonzero(ref['status'] == HIT)[0]
        rest = np.nonzero(ref['status'] != HIT)[0]
        pick = np.sort(np.concatenate([hit, rest[:2 * hit.size]]))
        vps.append(vp[pick]); dirs.append(dr[pick]); mask.append(keep[pick]); sizes.append(pick.size)
    sc = dict(total=total, owns=owns, fuse=fuse, vps=np.concatenate(vps), dirs=np.concatenate(dirs), mask=np.concatenate(mask),
              offset=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), poses=poses, rule=rule)
    sc['n'] = int(sc['offset'][-1])
    sc['oracle'] = {(mc, own): cast(total, owns if own else None, sc['vps'], sc['dirs'], sc['offset'], poses, mask=sc['mask'], min_count=mc,
                                    **rule) for mc in (1, 2) for own in (False, True)}
    first = sc['oracle'][(1, False)]['status']
    sc['counts'] = {k: int((first == k).sum()) for k in (HIT, SKIPPED, MISS, BEHIND, LOST)}
    _SCENES[dtype] = sc
    return sc


# ---- the depth bias against the fused volume: the oracle's loop ---------------------------------------------------------------------------
BIAS_VOXEL, BIAS_TRUNC = 0.1, 0.3
_BIAS = {}


def bias_fit_terms(scans, hit, depths):
    """(x, y) of the used rays of depth_bias' ScaledPolynomial fit with the exponent 2: x = inc^2 at the cast's angle, y = (d - t) / d;
    used: in the scan's mask, HIT, d > 0 and finite (no residual gate).  Also r = d - t of those rays."""
    d = np.concatenate([np.asarray(v, np.float64) for v in depths])
    mask = np.concatenate([np.asarray(c['lmask'], bool) for c in scans])
    used = mask & (hit['face'] >= 0) & np.isfinite(hit['t']) & np.isfinite(hit['inc']) & (d > 0.0) & np.isfinite(d)
    r = d[used] - hit['t'][used]
    return hit['inc'][used] ** 2, r / d[used], r, used


def fit_weight(x, y, order=None):
    """w = sum x y / sum x x, the sums taken one term after the other in fp64, in index order or in the random order of the seed."""
    if order is not None:
        p = np.random.default_rng(order).permutation(x.size)
        x, y = x[p], y[p]
    return float(np.add.accumulate(x * y)[-1] / np.add.accumulate(x * x)[-1])


def bias_oracle():
    """The biased box room of the tsdf_loss tests (5 x 24 x 96 rays, bias 0.05 inc^2, true poses), fused at 0.1 m with leave-one-out,
    every scan cast against the volume of the others: ``before`` with the depths as measured, ``after`` with the volumes re-fused from
    the depths the generating model corrects and the rays cast again.  Returns dict(scans, poses, before, after: dict(hit, used, r, w),
    spread: max - min of before's w over 8 random summation orders); computed once a process."""
    if _BIAS:
        return _BIAS
    scans, poses = L.box_scene(rows=24, cols=96)
    n = [len(c['depth']) for c in scans]
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    vps, dirs = np.concatenate([c['vps'] for c in scans]), np.concatenate([c['dirs'] for c in scans])
    t_max = max(float(c['depth'].max()) for c in scans) + BIAS_TRUNC
    out = dict(scans=scans, poses=poses, offset=off, t_max=t_max)
    for part, (kind, w) in (('before', (None, ())), ('after', ('ScaledPolynomial', (L.TRUE_W,)))):
        depths = [L.corrected_depth(c, kind, w, (2.0,)) for c in scans]
        total, owns = L.targets(scans, poses, None, (), (), BIAS_VOXEL, BIAS_TRUNC, True, depths=depths)
        hit = cast(total, owns, vps, dirs, off, poses, t_max=t_max)
        x, y, r, used = bias_fit_terms(scans, hit, depths)
        out[part] = dict(hit=hit, used=used, r=r, x=x, y=y, w=fit_weight(x, y), total=total, owns=owns)
    ws = [fit_weight(out['before']['x'], out['before']['y'], order=s) for s in range(8)]
    out['spread'] = max(ws) - min(ws)
    _BIAS.update(out)
    return _BIAS
