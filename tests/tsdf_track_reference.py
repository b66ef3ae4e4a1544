"""numpy oracle of the scan-to-TSDF registration, written from the rule of DESIGN "Scan-to-TSDF registration" (not from the kernels or
the package): sampling a sparse volume (tests/tsdf_sparse_reference.py's SparseVolume) to the bit, the point-to-surface row in extended
precision, and a reference mapper that runs sample -> quantile -> row -> tests/slam_reference.py's finish.

Sampling.  q = (x - og) / a - 0.5; RANGE (1) unless x is finite and -2^23 <= q < 2^23 - 1 on every axis; i0 = floor(q), f = q - i0;
corner c = bx + 2 by + 4 bz is voxel i0 + (bx, by, bz), observed iff its block is in the table and count >= min_count, value sum /
(count 2^20); UNOBSERVED (2) unless all eight are.  With lerp(p, q, t) = p + t (q - p), every operation rounded on its own:
    phi  = tau lerp(lerp(lerp(v0, v1, fx), lerp(v2, v3, fx), fy), lerp(lerp(v4, v5, fx), lerp(v6, v7, fx), fy), fz)
    gx   = lerp(lerp(v1 - v0, v3 - v2, fy), lerp(v5 - v4, v7 - v6, fy), fz)
    gy   = lerp(lerp(v2 - v0, v3 - v1, fx), lerp(v6 - v4, v7 - v5, fx), fz)
    gz   = lerp(lerp(v4 - v0, v5 - v1, fx), lerp(v6 - v2, v7 - v3, fx), fy)
    grad = (tau / a) (gx, gy, gz)
An invalid point has phi NaN, grad 0, dist +inf; dist = |phi| otherwise.
Pair: flag == 0, dist <= thr, dist < max_residual.  Row: r = phi, J = [x cross grad, grad], the 30 sums of slam_reference.

Every discrete decision of the reference mapper comes with its margin, as in slam_reference.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import slam_reference as R
import tsdf_sparse_reference as S

RANGE, UNOBSERVED = 1, 2
LIMIT = 2.0 ** 23
LD = np.longdouble


def lerp(p, q, t):
    return p + t * (q - p)


def trilinear(v, f):
    """(value, g [n, 3]) in units of tau and tau per voxel from v [n, 8] and f [n, 3], in the rule's order."""
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[:, c] for c in range(8))
    value = lerp(lerp(lerp(v0, v1, fx), lerp(v2, v3, fx), fy), lerp(lerp(v4, v5, fx), lerp(v6, v7, fx), fy), fz)
    gx = lerp(lerp(v1 - v0, v3 - v2, fy), lerp(v5 - v4, v7 - v6, fy), fz)
    gy = lerp(lerp(v2 - v0, v3 - v1, fx), lerp(v6 - v4, v7 - v5, fx), fz)
    gz = lerp(lerp(v4 - v0, v5 - v1, fx), lerp(v6 - v2, v7 - v3, fx), fy)
    return value, np.stack([gx, gy, gz], axis=1)


def sample(vol, points, pose=None, min_count=1):
    """dict(x [m, 3], value [m], grad [m, 3], dist [m], flag uint8 [m]) of the volume sampled at ``points`` moved by ``pose``."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    m = p.shape[0]
    with np.errstate(all='ignore'):
        x = R.moved(pose, p) if pose is not None else p.copy()
        q = (x - vol.origin[None, :]) / vol.voxel - 0.5
        ok = np.isfinite(x).all(axis=1) & ((q >= -LIMIT) & (q < LIMIT - 1.0)).all(axis=1)
    flag = np.where(ok, 0, RANGE).astype(np.uint8)
    value, grad, dist = np.full(m, np.nan), np.zeros((m, 3)), np.full(m, np.inf)
    rows = np.nonzero(ok)[0]
    if rows.size:
        qq = q[rows]
        i0 = np.floor(qq).astype(np.int64)
        f = qq - i0.astype(np.float64)
        v = np.zeros((rows.size, 8))
        obs = np.ones(rows.size, bool)
        for c in range(8):
            i = i0 + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)
            pos = vol.find(S.block_key(i >> 3))
            have = pos >= 0
            local = ((i[:, 0] & 7) * 8 + (i[:, 1] & 7)) * 8 + (i[:, 2] & 7)
            cnt, sm = np.zeros(rows.size, np.int64), np.zeros(rows.size, np.int64)
            cnt[have] = vol.count[vol.slots[pos[have]], local[have]]
            sm[have] = vol.sum[vol.slots[pos[have]], local[have]]
            seen = have & (cnt >= min_count)
            obs &= seen
            with np.errstate(all='ignore'):
                v[:, c] = np.where(seen, sm.astype(np.float64) / (np.maximum(cnt, 1).astype(np.float64) * S.ONE), 0.0)
        flag[rows[~obs]] = UNOBSERVED
        good = rows[obs]
        val, g = trilinear(v[obs], f[obs])
        scale = vol.trunc / vol.voxel
        value[good] = vol.trunc * val
        grad[good] = scale * g
        dist[good] = np.abs(value[good])
    return dict(x=x, value=value, grad=grad, dist=dist, flag=flag)


def kept(s, thr, max_residual):
    with np.errstate(invalid='ignore'):
        return (s['flag'] == 0) & (s['dist'] <= thr) & (s['dist'] < max_residual)


def pair_terms(x, r, g):
    """The 30 summands of every pair [n, 30] (JtJ upper triangle 21, Jtr 6, 1, r^2, 1: a kept point is a used point)."""
    J = np.concatenate([np.cross(x, g), g], axis=1)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)]
    cols += [np.ones_like(r), r * r, np.ones_like(r)]
    return np.stack(cols, axis=1) if len(r) else np.zeros((0, 30))


def totals(s, thr, max_residual, order=None):
    """The pair rule and the 30 totals in extended precision (over the pairs in ``order``), rounded to fp64 once:
    dict(kept [m] bool, totals [30], abs_totals [30], n_pairs)."""
    k = kept(s, thr, max_residual)
    rows = np.nonzero(k)[0]
    if order is not None:
        rows = rows[order]
    tot, abs_tot = np.zeros(30, dtype=LD), np.zeros(30, dtype=LD)
    for a in range(0, len(rows), 1 << 18):
        sel = rows[a:a + (1 << 18)]
        terms = pair_terms(s['x'][sel], s['value'][sel], s['grad'][sel])
        tot += terms.astype(LD).sum(axis=0)
        abs_tot += np.abs(terms).astype(LD).sum(axis=0)
    return dict(kept=k, totals=np.asarray(tot, dtype=np.float64), abs_totals=np.asarray(abs_tot, dtype=np.float64), n_pairs=len(rows))


def params(cfg=None, **kw):
    """slam_reference.params plus the TSDF map's: voxel, trunc (None: 3 voxels), min_count, max_residual (None: the truncation)."""
    d = dict(slam_tsdf_voxel_size=0.1, slam_tsdf_trunc=None, slam_tsdf_min_count=1, slam_tsdf_max_residual=None)
    for name in d:
        if cfg is not None and hasattr(cfg, name):
            d[name] = getattr(cfg, name)
    d.update({k: kw.pop(k) for k in list(kw) if k in d})
    prm = R.params(cfg, **kw)
    for k, v in d.items():
        setattr(prm, k, v)
    return prm


def max_residual_of(vol, prm):
    return vol.trunc if prm.slam_tsdf_max_residual is None else float(prm.slam_tsdf_max_residual)


def iteration(vol, p, st, prm, order_seed=None):
    """One iteration on the state ``st`` (slam_reference.new_state): a record with the sample, thr, kept, totals, abs_totals, x, pose,
    code, iters, pairs, sse, overlap and the margins of its decisions."""
    T = st.pose.copy()
    s = sample(vol, p, T, int(prm.slam_tsdf_min_count))
    thr = R.quantile_finite(s['dist'], prm.icp_trim_ratio)
    mr = max_residual_of(vol, prm)
    t = totals(s, thr, mr)
    if order_seed is not None and t['n_pairs']:
        t = totals(s, thr, mr, order=np.random.default_rng(order_seed).permutation(t['n_pairs']))
    x, margins = R.finish(t['totals'], len(p), prm, st)
    fin = s['dist'][np.isfinite(s['dist'])]
    off = fin[fin != thr] if ((fin.size - 1) * prm.icp_trim_ratio) % 1.0 == 0.0 else fin
    margins['thr'] = float(np.abs(off - thr).min() / thr) if off.size and thr > 0 else float('inf')
    margins['max_residual'] = float(np.abs(fin - mr).min()) if fin.size else float('inf')
    # the flag of a point can change only where its cell does: the distance of q from the nearest cell face, in voxels
    q = (s['x'][s['flag'] != RANGE] - vol.origin[None, :]) / vol.voxel - 0.5
    margins['cell'] = float(np.abs(q - np.rint(q)).min()) if q.size else float('inf')
    return SimpleNamespace(sample=s, thr=thr, kept=t['kept'], totals=t['totals'], abs_totals=t['abs_totals'], x=x, pose=st.pose.copy(),
                           code=st.code, iters=st.iters, pairs=st.pairs, sse=st.sse, overlap=st.overlap, margins=margins)


Registration = namedtuple('Registration', 'pose status iterations overlap pairs sse poses records')


def register(vol, p, prior, prm, order_seed=None):
    """A registration from ``prior``; a failed one, an empty scan ('empty') and an empty volume ('init') return the prior."""
    prior = np.asarray(prior, dtype=np.float64).reshape(4, 4)
    if len(p) == 0:
        return Registration(prior.copy(), 'empty', 0, 0.0, 0, 0.0, [], [])
    if vol.n_blocks == 0:
        return Registration(prior.copy(), 'init', 0, 0.0, 0, 0.0, [], [])
    st = R.new_state(prior)
    recs = []
    while st.code == R.RUNNING:
        recs.append(iteration(vol, p, st, prm, None if order_seed is None else order_seed + len(recs)))
    status = R.STATUS[st.code]
    pose = prior.copy() if status in R.FAILED else st.pose.copy()
    return Registration(pose, status, st.iters, st.overlap, int(st.pairs), st.sse, [r.pose for r in recs], recs)


def new_volume(prm, capacity=256):
    return S.SparseVolume(prm.slam_tsdf_voxel_size, prm.slam_tsdf_trunc, capacity=capacity)


def run(scans, odom, prm, vol=None):
    """The reference mapper over prepared scans [dict(points, vps, dirs, depth)] with odometry ``odom``: prior[i] = slam[i-1] odom[i-1]^-1
    odom[i]; every registered scan is fused at its pose (depths up to slam_sensor_max_range); a failed one keeps its prior and the
    volume.  -> dict(slam, info, volume)."""
    odom = np.asarray(odom, dtype=np.float64)
    slam = odom.copy()
    vol = new_volume(prm) if vol is None else vol
    info = []
    for i, sc in enumerate(scans):
        prior = odom[0] if i == 0 else slam[i - 1] @ np.linalg.solve(odom[i - 1], odom[i])
        reg = register(vol, sc['points'], prior, prm)
        if reg.status not in R.FAILED:
            S.fuse(vol, vps=sc['vps'], dirs=sc['dirs'], depth=sc['depth'], pose=reg.pose, max_range=prm.slam_sensor_max_range)
        margins = {}
        for r in reg.records:
            for key in ('thr', 'max_residual', 'conv_rot', 'conv_trans'):
                if key in r.margins:
                    margins[key] = min(margins.get(key, float('inf')), r.margins[key])
        slam[i] = reg.pose
        info.append(dict(status=reg.status, iterations=reg.iterations, overlap=reg.overlap, pairs=reg.pairs, map_size=vol.n_blocks,
                         margins=margins))
    return dict(slam=slam, info=info, volume=vol)
