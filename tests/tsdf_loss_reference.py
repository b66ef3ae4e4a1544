"""numpy oracle of the loss against the fused volume, written from the rule of DESIGN "Self-supervised training against the fused
volume" (not from the kernels or the package), on top of tests/tsdf_sparse_reference.py (the volumes) and tests/tsdf_track_reference.py
(the trilinear form).

Sample with exclusion.  As tsdf_track_reference.sample, but corner voxel i has sum = sum_total(i) - sum_own(i) and count =
count_total(i) - count_own(i); a voxel whose block a table lacks contributes 0 from that table; the corner is observed iff its block is
in the TOTAL table and count >= min_count; value = (double)sum / ((double)count 2^20).  Without an own volume the result is that of
tsdf_track_reference.sample.
Term.  squared: l = phi^2, dl/dx = (2 phi) grad; otherwise l = |phi|, dl/dx = sign(phi) grad, zero at phi = 0; every product rounded on
its own.
Class of a point of the mask: INVALID (1: x not finite or out of range), UNOBSERVED (2), GATED (3: |phi| >= max_residual), USED (0);
255 outside the mask.
Whole loss.  x_j = R_s (vp_j + d'_j dir_j) + t_s with d' = d (1 - sum_k w_k g^e_k) (ScaledPolynomial), d - sum_k w_k g^e_k
(Polynomial) or d (no model, or outside the scan's local mask).  L = sum l / M over the used points, with
    dL/dw_k = sum gd_j c_j g_j^e_k / M,  gd = dir . (R^T dl/dx),  c = -d (ScaledPolynomial) or -1 (Polynomial)
    dL/de_k = sum gd_j c_j w_k g_j^e_k ln g_j / M  (zero where g = 0)
    dL/d[R|t]_s = sum over scan s of dl/dx [xl, 1]^T / M,  xl = vp + d' dir
the volume held constant.  The sums run in np.longdouble over terms formed in np.longdouble from the fp64 sample; ``abs_*`` are the
sums of the terms' magnitudes, which the tests' error bounds are made of.
"""
import numpy as np

import tsdf_sparse_reference as S
import tsdf_track_reference as K

LD = np.longdouble
USED, INVALID, UNOBSERVED, GATED, MASKED = 0, 1, 2, 3, 255
KINDS = (None, 'Polynomial', 'ScaledPolynomial')


def _gather(vol, i):
    """(have, sum, count) of the voxels i int64 [n, 3] of ``vol``; 0 where the block is missing."""
    pos = vol.find(S.block_key(i >> 3))
    have = pos >= 0
    local = ((i[:, 0] & 7) * 8 + (i[:, 1] & 7)) * 8 + (i[:, 2] & 7)
    sm, cnt = np.zeros(i.shape[0], np.int64), np.zeros(i.shape[0], np.int64)
    sm[have] = vol.sum[vol.slots[pos[have]], local[have]]
    cnt[have] = vol.count[vol.slots[pos[have]], local[have]]
    return have, sm, cnt


def sample_minus(total, own, x, min_count=1):
    """dict(value [m], grad [m, 3], dist [m], flag uint8 [m] (0, 1 RANGE, 2 UNOBSERVED), q [m, 3], i0 [m, 3]) of ``total`` minus ``own``
    (a SparseVolume on the same lattice, or None) at the world points x [m, 3]."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    m = x.shape[0]
    with np.errstate(all='ignore'):
        q = (x - total.origin[None, :]) / total.voxel - 0.5
        ok = np.isfinite(x).all(axis=1) & ((q >= -K.LIMIT) & (q < K.LIMIT - 1.0)).all(axis=1)
    flag = np.where(ok, 0, K.RANGE).astype(np.uint8)
    value, grad, dist = np.full(m, np.nan), np.zeros((m, 3)), np.full(m, np.inf)
    i0_all = np.zeros((m, 3), np.int64)
    rows = np.nonzero(ok)[0]
    if rows.size:
        qq = q[rows]
        i0 = np.floor(qq).astype(np.int64)
        i0_all[rows] = i0
        f = qq - i0.astype(np.float64)
        v = np.zeros((rows.size, 8))
        obs = np.ones(rows.size, bool)
        for c in range(8):
            i = i0 + np.array([c & 1, (c >> 1) & 1, c >> 2], np.int64)
            have, sm, cnt = _gather(total, i)
            if own is not None:
                _, sm_own, cnt_own = _gather(own, i)
                sm, cnt = sm - sm_own, cnt - cnt_own
            seen = have & (cnt >= min_count)
            obs &= seen
            with np.errstate(all='ignore'):
                v[:, c] = np.where(seen, sm.astype(np.float64) / (np.maximum(cnt, 1).astype(np.float64) * S.ONE), 0.0)
        flag[rows[~obs]] = K.UNOBSERVED
        good = rows[obs]
        val, g = K.trilinear(v[obs], f[obs])
        value[good] = total.trunc * val
        grad[good] = (total.trunc / total.voxel) * g
        dist[good] = np.abs(value[good])
    return dict(value=value, grad=grad, dist=dist, flag=flag, q=q, i0=i0_all)


def term(phi, grad, squared):
    """(l [n], dl/dx [n, 3]) of used points."""
    phi, grad = np.asarray(phi, np.float64), np.asarray(grad, np.float64).reshape(-1, 3)
    c = 2.0 * phi if squared else np.sign(phi)
    return (phi * phi if squared else np.abs(phi)), c[:, None] * grad


def classify(smp, max_residual, mask=None):
    """uint8 [m]: USED, INVALID, UNOBSERVED, GATED, or MASKED outside ``mask``."""
    with np.errstate(invalid='ignore'):
        cls = np.where(smp['flag'] == K.RANGE, INVALID,
                       np.where(smp['flag'] != 0, UNOBSERVED, np.where(smp['dist'] < max_residual, USED, GATED))).astype(np.uint8)
    if mask is not None:
        cls[~np.asarray(mask, bool)] = MASKED
    return cls


def margins(smp, cls, max_residual):
    """The margins of the oracle's decisions on the points it samples: (the least distance of q to a cell face over the points in
    range, in voxels; the least | |phi| - max_residual | over the observed points)."""
    ok = (cls != MASKED) & (smp['flag'] != K.RANGE)
    face = np.inf
    if ok.any():
        q = smp['q'][ok]
        face = float(np.abs(q - np.rint(q)).min())
    seen = (cls == USED) | (cls == GATED)
    gate = float(np.abs(smp['dist'][seen] - max_residual).min()) if seen.any() else np.inf
    return face, gate


# ---- the points -------------------------------------------------------------------------------------------------------------------
def corrected_depth(scan, kind, w, e, dtype=np.float64):
    d = np.asarray(scan['depth']).astype(dtype)
    if kind is None:
        return d
    g = np.asarray(scan['inc']).astype(dtype)
    bias = sum(dtype(wk) * g ** dtype(ek) for wk, ek in zip(w, e))
    out = d * (1 - bias) if kind == 'ScaledPolynomial' else d - bias
    lm = scan.get('lmask')
    return out if lm is None else np.where(np.asarray(lm, bool), out, d)


def posed_points(scan, pose, kind, w, e, dtype=np.float64):
    """x [n, 3] of one scan in ``dtype`` (np.float64: close to, not the bits of, the kernels' points)."""
    n = len(scan['depth'])
    T = np.asarray(pose).astype(dtype).reshape(4, 4)
    vp = np.broadcast_to(np.asarray(scan['vps']).astype(dtype).reshape(-1, 3), (n, 3))
    xl = vp + corrected_depth(scan, kind, w, e, dtype)[:, None] * np.asarray(scan['dirs']).astype(dtype)
    with np.errstate(all='ignore'):
        return xl @ T[:3, :3].T + T[:3, 3]


def loss(total, owns, scans, poses, kind=None, w=(), e=(), mask=None, squared=True, max_residual=None, min_count=1, x=None):
    """The whole call.  owns: one SparseVolume per scan, or None; mask bool [N] over the concatenated scans, or None; x [N, 3]: the
    points to sample at (None: posed_points in fp64).  Returns dict(loss, used, gated, unobserved, invalid, gw [P], ge [P], gT [S, 3, 4],
    abs_loss, abs_gw, abs_ge, abs_gT (the sums of the terms' magnitudes over M), cls uint8 [N], value [N], grad [N, 3], x [N, 3], n,
    face_margin, gate_margin)."""
    assert kind in KINDS
    w, e = np.asarray(w, np.float64).reshape(-1), np.asarray(e, np.float64).reshape(-1)
    P, ns = (0 if kind is None else w.size), len(scans)
    sizes = [len(c['depth']) for c in scans]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(ptr[-1])
    mr = total.trunc if max_residual is None else float(max_residual)
    mask = np.ones(n, bool) if mask is None else np.asarray(mask, bool).reshape(n)
    tot = dict(l=LD(0), gw=np.zeros(P, LD), ge=np.zeros(P, LD), gT=np.zeros((ns, 3, 4), LD))
    mag = dict(l=LD(0), gw=np.zeros(P, LD), ge=np.zeros(P, LD), gT=np.zeros((ns, 3, 4), LD))
    sen = dict(l=LD(0), gw=np.zeros(P, LD), ge=np.zeros(P, LD), gT=np.zeros((ns, 3, 4), LD))       # see move_bound
    cls_all, value, grad_all, x_all = np.full(n, MASKED, np.uint8), np.full(n, np.nan), np.zeros((n, 3)), np.full((n, 3), np.nan)
    face, gate = np.inf, np.inf
    for s, (scan, pose) in enumerate(zip(scans, poses)):
        a, b = int(ptr[s]), int(ptr[s + 1])
        if b == a:
            continue
        xs = posed_points(scan, pose, kind, w, e) if x is None else np.asarray(x, np.float64)[a:b]
        xs = np.where(mask[a:b, None], xs, np.nan)
        smp = sample_minus(total, None if owns is None else owns[s], xs, min_count)
        cls = classify(smp, mr, mask[a:b])
        fm, gm = margins(smp, cls, mr)
        face, gate = min(face, fm), min(gate, gm)
        cls_all[a:b], x_all[a:b], grad_all[a:b] = cls, xs, smp['grad']
        value[a:b] = np.where((cls == USED) | (cls == GATED), smp['value'], np.nan)
        u = np.nonzero(cls == USED)[0]
        if not u.size:
            continue
        l, gx = term(smp['value'][u], smp['grad'][u], squared)
        tot['l'] += l.astype(LD).sum()
        mag['l'] += np.abs(l).astype(LD).sum()
        gxl = gx.astype(LD)
        T = np.asarray(pose, np.float64).reshape(4, 4).astype(LD)
        dr = np.asarray(scan['dirs']).astype(np.float64)[u].astype(LD)
        vp = np.broadcast_to(np.asarray(scan['vps']).astype(np.float64).reshape(-1, 3), (b - a, 3))[u].astype(LD)
        dcorr = corrected_depth(scan, kind, w, e, LD)[u]
        xl1 = np.concatenate([vp + dcorr[:, None] * dr, np.ones((u.size, 1), LD)], axis=1)
        prod = gxl[:, :, None] * xl1[:, None, :]
        tot['gT'][s] += prod.sum(axis=0)
        mag['gT'][s] += np.abs(prod).sum(axis=0)
        # how far a term moves when x moves by one rounding: in the squared form a term is phi times a constant of the cell, and phi
        # moves by sum_a |grad_a| |x_a| 2^-53; in the |phi| form a term does not depend on x inside a cell
        reach = (np.abs(smp['grad'][u]) * np.abs(xs[u])).sum(axis=1).astype(LD) if squared else np.zeros(u.size, LD)
        unit = 2 * np.abs(smp['grad'][u]).astype(LD)             # |d(dl/dx)/dphi|
        sen['l'] += (2 * np.abs(smp['value'][u]).astype(LD) * reach).sum()
        sen['gT'][s] += (unit[:, :, None] * np.abs(xl1)[:, None, :] * reach[:, None, None]).sum(axis=0)
        if P:
            d = np.asarray(scan['depth']).astype(np.float64)[u].astype(LD)
            g = np.asarray(scan['inc']).astype(np.float64)[u].astype(LD)
            lm = np.ones(u.size, bool) if scan.get('lmask') is None else np.asarray(scan['lmask'], bool)[u]
            gd = (dr * (gxl @ T[:3, :3])).sum(axis=1)                      # dir . (R^T g)
            gd_mag = (np.abs(dr) * (np.abs(gxl) @ np.abs(T[:3, :3]))).sum(axis=1)
            c = -d if kind == 'ScaledPolynomial' else -np.ones_like(d)
            with np.errstate(all='ignore'):
                lng = np.where(g > 0, np.log(np.where(g > 0, g, 1)), 0)
            for k in range(P):
                pk = g ** LD(e[k])
                tw = np.where(lm, gd * c * pk, 0)
                te = np.where(lm, gd * c * LD(w[k]) * pk * lng, 0)
                tot['gw'][k] += tw.sum()
                tot['ge'][k] += te.sum()
                mag['gw'][k] += np.where(lm, gd_mag * np.abs(c) * pk, 0).sum()
                mag['ge'][k] += np.where(lm, gd_mag * np.abs(c * LD(w[k]) * pk * lng), 0).sum()
                gd_unit = (np.abs(dr) * (unit @ np.abs(T[:3, :3]))).sum(axis=1) * reach
                sen['gw'][k] += np.where(lm, gd_unit * np.abs(c) * pk, 0).sum()
                sen['ge'][k] += np.where(lm, gd_unit * np.abs(c * LD(w[k]) * pk * lng), 0).sum()
    counts = {name: int((cls_all == code).sum()) for name, code in (('used', USED), ('gated', GATED), ('unobserved', UNOBSERVED),
                                                                    ('invalid', INVALID))}
    M = LD(counts['used'])
    out = dict(counts, cls=cls_all, value=value, grad=grad_all, x=x_all, n=n, face_margin=face, gate_margin=gate)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    if counts['used']:
        out.update(loss=float(tot['l'] / M), gw=f64(tot['gw'] / M), ge=f64(tot['ge'] / M), gT=f64(tot['gT'] / M), abs_loss=float(mag['l'] / M),
                   abs_gw=f64(mag['gw'] / M), abs_ge=f64(mag['ge'] / M), abs_gT=f64(mag['gT'] / M), move_loss=float(sen['l'] / M),
                   move_gw=f64(sen['gw'] / M), move_ge=f64(sen['ge'] / M), move_gT=f64(sen['gT'] / M))
    else:
        out.update(loss=float('nan'), gw=np.zeros(P), ge=np.zeros(P), gT=np.zeros((ns, 3, 4)), abs_loss=0.0, abs_gw=np.zeros(P),
                   abs_ge=np.zeros(P), abs_gT=np.zeros((ns, 3, 4)), move_loss=0.0, move_gw=np.zeros(P), move_ge=np.zeros(P),
                   move_gT=np.zeros((ns, 3, 4)))
    return out


def bound(ref, name, n=None):
    """(n + 16) 2^-53 times the sum of the magnitudes of the terms behind ``name`` ('loss', 'gw', 'ge', 'gT'): n roundings at the most
    on the way of a term through any summation order, and sixteen for the operations that form a term in fp64 (the rotation, the dot
    product, the power, the products)."""
    n = ref['n'] if n is None else n
    return (n + 16) * 2.0 ** -53 * ref['abs_' + name]


def move_bound(ref, name, count):
    """What ``name`` may differ by between two forms that sample at points ``count`` roundings apart (the kernel forms x with fused
    multiply-adds, a tensor composition without): count 2^-53 times the sum over the used points of |d term / d phi| sum_a |grad_a|
    |x_a| -- the volume is trilinear inside a cell, and no point sits within 1e-9 voxels of a face."""
    return count * 2.0 ** -53 * ref['move_' + name]


# ---- fusing ---------------------------------------------------------------------------------------------------------------------------
def fuse_scans(scans, poses, depths, voxel, trunc=None, which=None):
    """A SparseVolume of the scans ``which`` (None: all) fused with the corrected ``depths`` (one array per scan) at their poses; the
    rays of a scan are those of its local mask, as reconstruction fuses them."""
    vol = S.SparseVolume(voxel, trunc=trunc, capacity=256)
    for s, (scan, pose) in enumerate(zip(scans, poses)):
        if which is not None and s not in which:
            continue
        n = len(scan['depth'])
        S.fuse(vol, vps=np.broadcast_to(np.asarray(scan['vps'], np.float64).reshape(-1, 3), (n, 3)), dirs=scan['dirs'], depth=depths[s],
               pose=pose, mask=scan.get('lmask'))
    return vol


def targets(scans, poses, kind, w, e, voxel, trunc=None, leave_one_out=True, depths=None):
    """(total, owns or None) as TsdfTarget.refresh fuses them; ``depths``: the corrected depths to fuse (None: corrected_depth)."""
    if depths is None:
        depths = [corrected_depth(c, kind, w, e) for c in scans]
    total = fuse_scans(scans, poses, depths, voxel, trunc)
    owns = [fuse_scans(scans, poses, depths, voxel, trunc, which=(s,)) for s in range(len(scans))] if leave_one_out else None
    return total, owns


# ---- the box room of the recovery loop ----------------------------------------------------------------------------------------------
ROOM = np.array([6.0, 4.0, 3.0])
TRUE_W = 0.05


# Five viewpoints spread over the room, four a metre from two walls each and one in the middle, at different heights and headings: a
# consistency loss can only see a bias that differs between the scans that share a surface, so every wall patch must be seen under
# different incidence angles.  (Viewpoints huddled in the middle of the room see each patch under nearly the same angle from every scan;
# the all-scans loop then stalls at a quarter of the bias.)
VIEWPOINTS = ((1.0, 1.0, 1.0), (5.0, 1.0, 1.5), (5.0, 3.0, 2.0), (1.0, 3.0, 1.2), (3.0, 2.0, 1.6))
YAWS = (0.3, 1.1, -2.0, 2.6, -0.7)


def box_scene(rows=24, cols=96, max_inc=1.3, elevation=0.7, true_w=TRUE_W, dtype=np.float64):
    """(scans, poses): one scan of rows x cols rays from each of VIEWPOINTS inside the box room [0, 6] x [0, 4] x [0, 3] m, elevation
    within +- ``elevation`` rad, rays meeting a wall at an incidence of ``max_inc`` rad or more left out; true incidence angles, true
    poses, measured depth d / (1 - true_w g^2) -- what a ScaledPolynomial with w = true_w, exponent 2 undoes."""
    scans, poses = [], []
    az = (np.arange(cols) + 0.5) / cols * 2.0 * np.pi - np.pi
    el = (np.arange(rows) + 0.5) / rows * 2.0 * elevation - elevation
    A, E = np.meshgrid(az, el)
    local = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    for position, yaw in zip(VIEWPOINTS, YAWS):
        c, s = np.cos(yaw), np.sin(yaw)
        T = np.eye(4)
        T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = position
        u = local @ T[:3, :3].T
        with np.errstate(divide='ignore', invalid='ignore'):
            t_axis = np.where(u > 0, (ROOM - T[:3, 3]) / u, np.where(u < 0, -T[:3, 3] / u, np.inf))
        axis = np.argmin(t_axis, axis=1)
        d = t_axis[np.arange(len(u)), axis]
        inc = np.arccos(np.clip(np.abs(u[np.arange(len(u)), axis]), 0.0, 1.0))
        keep = inc < max_inc
        d, inc, dirs = d[keep], inc[keep], local[keep]
        scans.append(dict(vps=np.zeros((len(d), 3), dtype), dirs=dirs.astype(dtype), depth=(d / (1.0 - true_w * inc ** 2)).astype(dtype),
                          inc=inc.astype(dtype), lmask=np.ones(len(d), bool)))
        poses.append(T)
    return scans, np.stack(poses)


def descent_step(scans, poses, w, voxel, trunc, leave_one_out, lr, depths=None, x=None, order=None):
    """One step of the re-fuse / gradient-descent loop on the one weight of a ScaledPolynomial with exponent 2: the volumes re-fused at
    w (from ``depths`` when given), the loss and dL/dw at the volumes held fixed (sampled at ``x`` when given), w <- w - lr dL/dw.
    ``order``: a permutation seed; the per-point terms of dL/dw are then summed in fp64 in that random order instead of in extended
    precision (the spread over orders is what the device comparison's bar is taken from).  Returns (new w, the loss dict)."""
    total, owns = targets(scans, poses, 'ScaledPolynomial', [w], [2.0], voxel, trunc, leave_one_out, depths)
    ref = loss(total, owns, scans, poses, 'ScaledPolynomial', [w], [2.0], squared=True, x=x)
    gw = float(ref['gw'][0])
    if order is not None:
        gw = _ordered_gw(ref, scans, poses, w, order)
    return w - lr * gw, ref


def _ordered_gw(ref, scans, poses, w, seed):
    """dL/dw of descent_step from fp64 terms added one after the other in a random order."""
    terms = []
    off = 0
    for scan, pose in zip(scans, poses):
        n = len(scan['depth'])
        u = np.nonzero(ref['cls'][off:off + n] == USED)[0]
        _, gx = term(ref['value'][off:off + n][u], ref['grad'][off:off + n][u], True)
        R = np.asarray(pose, np.float64)[:3, :3]
        gd = (scan['dirs'].astype(np.float64)[u] * (gx @ R)).sum(axis=1)
        terms.append(gd * -scan['depth'].astype(np.float64)[u] * scan['inc'].astype(np.float64)[u] ** 2)
        off += n
    t = np.concatenate(terms)
    t = t[np.random.default_rng(seed).permutation(t.size)]
    return float(np.add.accumulate(t)[-1]) / ref['used']               # (accumulate adds one after the other, not pairwise)


def own_tables(owns):
    """The own volumes as the ONE structure dc_tsdf_loss takes: (keys uint64 [sum nb], slots int32 offset into the shared pool, ptr int64
    [S + 1], sum int64 [cap, 512], count int32 [cap, 512]); the pool has at least one block."""
    keys, slots, sums, counts, ptr = [], [], [], [], [0]
    off = 0
    for v in owns:
        keys.append(v.keys)
        slots.append(v.slots.astype(np.int64) + off)
        sums.append(v.sum)
        counts.append(v.count)
        off += v.sum.shape[0]
        ptr.append(ptr[-1] + v.n_blocks)
    if off == 0:
        sums.append(np.zeros((1, S.BV), np.int64))
        counts.append(np.zeros((1, S.BV), np.int32))
    return (np.ascontiguousarray(np.concatenate(keys), np.uint64), np.ascontiguousarray(np.concatenate(slots), np.int32),
            np.asarray(ptr, np.int64), np.ascontiguousarray(np.concatenate(sums)), np.ascontiguousarray(np.concatenate(counts)))
