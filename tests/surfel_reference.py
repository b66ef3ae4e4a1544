"""References for the surfel ray caster (csrc/dc_surfelmath.h, dc_surfel_bvh_build / dc_surfel_cast_rays in csrc/dc_raycast.hip).

oracle      numpy: every (ray, disk) pair that can matter, no tree.  The decisions (hit, first hit, membership of the blend) restate
            the header's fp64 expressions operation by operation, so index, t_first and count are the header's bit for bit, and with
            window = 0 so are t and inc; the blend's sums are taken in longdouble (64-bit mantissa) over the same fp64 terms, the
            reference the header's rounding-error count is held against.
host_*      ctypes wrappers of the header's host build (libdc_hostcheck.so).
wall_scene  the statistical scene of the design note: a noisy survey of a wall and rays of uniform incidence (check_wall: its two
            assertions).
room_*      a noisy survey of a box room with rays from two posed scans, and world_rays, which forms the rays the kernel forms.
check_tree  the invariants of the LBVH.
"""
import ctypes
import math

import numpy as np

U52 = 2.0 ** -52


# ---- the host build -----------------------------------------------------------------------------------------------------------------
def surfel_host_lib():
    """helpers.raycast_host_lib() with the surfel exports (rebuilt when the library at hand predates them)."""
    from helpers import raycast_host_lib
    lib = raycast_host_lib()
    if not hasattr(lib, 'dc_host_surfel_cast_walk'):
        import __graft_entry__ as ge
        ge.build()
        lib = raycast_host_lib()
    vp, i64, f64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int
    lib.dc_host_surfel_boxes.restype = None
    lib.dc_host_surfel_boxes.argtypes = [vp, vp, vp, i64, vp]
    lib.dc_host_surfel_test_pairs.restype = None
    lib.dc_host_surfel_test_pairs.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    lib.dc_host_surfel_cast_brute.restype = None
    lib.dc_host_surfel_cast_brute.argtypes = [vp, vp, i64, vp, vp, i64, f64, f64, f64, vp, vp, vp, vp, vp]
    lib.dc_host_surfel_cast_walk.restype = None
    lib.dc_host_surfel_cast_walk.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, f64, f64, f64, vp, vp, vp, vp, vp]
    lib.dc_host_surfel_acos.restype = None
    lib.dc_host_surfel_acos.argtypes = [vp, i64, vp]
    lib.dc_host_surfel_t_err.restype = f64
    lib.dc_host_surfel_t_err.argtypes = [i32, f64, f64]
    lib.dc_host_surfel_cos_err.restype = f64
    lib.dc_host_surfel_cos_err.argtypes = [i32, f64]
    return lib


def _c64(a, cols):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def disk_rows(points, normals, radii):
    """leaf_disk rows f64 [n,8] = (p, n, fl(rho rho), 0) in survey order."""
    p, n, r = _c64(points, 3), _c64(normals, 3), _c64(radii, 0)
    return np.ascontiguousarray(np.concatenate([p, n, (r * r)[:, None], np.zeros((p.shape[0], 1))], axis=1))


def host_boxes(lib, points, normals, radii):
    p, n, r = _c64(points, 3), _c64(normals, 3), _c64(radii, 0)
    box = np.empty((p.shape[0], 6), dtype=np.float32)
    lib.dc_host_surfel_boxes(p.ctypes.data, n.ctypes.data, r.ctypes.data, p.shape[0], box.ctypes.data)
    return box


def host_test_pairs(lib, rows, o, d, t_min):
    """test_disk pair by pair: ray i against row i -> (hit bool [n], t, r2 f64 [n] as computed)."""
    rows, o, d = _c64(rows, 8), _c64(o, 3), _c64(d, 3)
    n = rows.shape[0]
    assert o.shape[0] == n and d.shape[0] == n
    t_min = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,)))
    hit, t, r2 = np.empty(n, np.uint8), np.empty(n), np.empty(n)
    lib.dc_host_surfel_test_pairs(rows.ctypes.data, o.ctypes.data, d.ctypes.data, t_min.ctypes.data, n, hit.ctypes.data, t.ctypes.data,
                                  r2.ctypes.data)
    return hit.astype(bool), t, r2


def host_cast_brute(lib, rows, o, d, t_min, window, min_cos, index=None, threads=8):
    """Both passes over every row in row order -> (index i32, t_first, t, inc f64, count i32) [R]."""
    from concurrent.futures import ThreadPoolExecutor
    rows, o, d = _c64(rows, 8), _c64(o, 3), _c64(d, 3)
    m, n = rows.shape[0], o.shape[0]
    ids = np.ascontiguousarray(np.arange(m) if index is None else index, dtype=np.int32)
    idx, t1, t, inc, cnt = np.empty(n, np.int32), np.empty(n), np.empty(n), np.empty(n), np.empty(n, np.int32)
    step = max(1, -(-n // threads))

    def run(s):
        k = min(step, n - s)
        lib.dc_host_surfel_cast_brute(rows.ctypes.data, ids.ctypes.data, m, o[s:].ctypes.data, d[s:].ctypes.data, k, float(t_min),
                                      float(window), float(min_cos), idx[s:].ctypes.data, t1[s:].ctypes.data, t[s:].ctypes.data,
                                      inc[s:].ctypes.data, cnt[s:].ctypes.data)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(run, range(0, n, step)))
    return idx, t1, t, inc, cnt


def host_cast_walk(lib, child, node_box, leaf_disk, leaf_index, o, d, t_min, window, min_cos):
    """surfel_cast_kernel on the host (dc::bvh_walk with the kernel's visitors) over the tree (child i32 [m-1,2], node_box f32
    [2m-1,6], leaf_disk [m,8], leaf_index i32 [m]) -> as host_cast_brute, the blend summed in the order of the walk."""
    child, box = np.ascontiguousarray(child, dtype=np.int32), np.ascontiguousarray(node_box, dtype=np.float32)
    rows, ids, o, d = _c64(leaf_disk, 8), np.ascontiguousarray(leaf_index, dtype=np.int32), _c64(o, 3), _c64(d, 3)
    m, n = rows.shape[0], o.shape[0]
    assert child.shape == (m - 1, 2) and box.shape == (2 * m - 1, 6) and ids.shape == (m,) and d.shape[0] == n
    idx, t1, t, inc, cnt = np.empty(n, np.int32), np.empty(n), np.empty(n), np.empty(n), np.empty(n, np.int32)
    lib.dc_host_surfel_cast_walk(child.ctypes.data, box.ctypes.data, rows.ctypes.data, ids.ctypes.data, m, o.ctypes.data, d.ctypes.data, n,
                                 float(t_min), float(window), float(min_cos), idx.ctypes.data, t1.ctypes.data, t.ctypes.data,
                                 inc.ctypes.data, cnt.ctypes.data)
    return idx, t1, t, inc, cnt


def host_acos(lib, x):
    x = _c64(x, 0)
    out = np.empty_like(x)
    lib.dc_host_surfel_acos(x.ctypes.data, x.shape[0], out.ctypes.data)
    return out


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _dot(x0, x1, x2, y0, y1, y2):
    return (x0 * y0 + x1 * y1) + x2 * y2


def acos01(x):
    """The header's arc cosine on [0, 1], operation by operation (fdlibm's rational approximation: +, *, / and sqrt only)."""
    x = np.asarray(x, dtype=np.float64)
    pio2_hi, pio2_lo = 1.57079632679489655800e+00, 6.12323399573676603587e-17
    pS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
          7.91534994289814532176e-04, 3.47933107596021167570e-05)
    qS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)

    def ratio(z):
        p = z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
        q = 1.0 + z * (qS[0] + z * (qS[1] + z * (qS[2] + z * qS[3])))
        return p / q
    with np.errstate(all='ignore'):
        small = pio2_hi - (x - (pio2_lo - ratio(x * x) * x))
        z = (1.0 - x) * 0.5
        s = np.sqrt(z)
        df = (s.view(np.uint64) & np.uint64(0xffffffff00000000)).view(np.float64)
        c = (z - df * df) / (s + df)
        w = ratio(z) * s + c
        big = 2.0 * (df + w)
        out = np.where(x < 0.5, np.where(x < 2.0 ** -57, pio2_hi + pio2_lo, small), big)
        out = np.where(x >= 1.0, 0.0, out)
    return np.where(np.isnan(x), x, out)


def _cos_inc(n, d):
    nd = _dot(n[:, 0], n[:, 1], n[:, 2], d[:, 0], d[:, 1], d[:, 2])
    nn = _dot(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2])
    dd = _dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
    return np.abs(nd) / (np.sqrt(nn) * np.sqrt(dd))


class Cast(object):
    """index i32 [R] (-1), t_first f64 [R] (inf), count i32 [R]; t / cos longdouble [R]: the blended depth and cosine from longdouble
    sums (window = 0: the fp64 values of the first disk); inc f64 [R] = acos01(min(1, fp64(cos))) (bit-exact for window = 0);
    kappa [R] = sum w / |N| of the blend (1 without one); members: (ray, disk) index arrays of the blend's members."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def oracle(points, normals, radii, o, d, t_min=0.0, window=0.0, min_cos=math.cos(math.pi / 4), chunk=256):
    """Closest disk and blend of the rays (o, d) [R,3] (world frame, fp64) over every disk."""
    P, N, rho = _c64(points, 3), _c64(normals, 3), _c64(radii, 0)
    O, D = _c64(o, 3), _c64(d, 3)
    rho2 = rho * rho
    R = O.shape[0]
    ri_all, di_all = [], []
    pp = (P * P).sum(axis=1)
    for s in range(0, R, chunk):
        Oc, Dc = O[s:s + chunk], D[s:s + chunk]
        with np.errstate(all='ignore'):
            # conservative pre-filter (not the test): a disk the ray hits has its centre within rho of the ray's line
            dl = np.linalg.norm(Dc, axis=1, keepdims=True)
            dh = Dc / dl
            po = pp[None, :] - 2.0 * (Oc @ P.T) + (Oc * Oc).sum(axis=1)[:, None]          # |p - o|^2
            al = dh @ P.T - (dh * Oc).sum(axis=1)[:, None]                                  # (p - o) . d / |d|
            scale = pp[None, :] + (Oc * Oc).sum(axis=1)[:, None]
            near = po - al * al <= 1.05 * rho2[None, :] + 1e-9 * scale
        ri, di = np.nonzero(near)
        ri_all.append(ri + s)
        di_all.append(di)
    ri, di = np.concatenate(ri_all), np.concatenate(di_all)
    # the header's test_disk, operation by operation, on the candidate pairs
    with np.errstate(all='ignore'):
        q0, q1, q2 = P[di, 0] - O[ri, 0], P[di, 1] - O[ri, 1], P[di, 2] - O[ri, 2]
        d0, d1, d2 = D[ri, 0], D[ri, 1], D[ri, 2]
        n0, n1, n2 = N[di, 0], N[di, 1], N[di, 2]
        den = _dot(n0, n1, n2, d0, d1, d2)
        nq = _dot(n0, n1, n2, q0, q1, q2)
        t = nq / den
        h0, h1, h2 = t * d0 - q0, t * d1 - q1, t * d2 - q2
        r2 = _dot(h0, h1, h2, h0, h1, h2)
        hit = (den != 0.0) & (t > t_min) & (t < np.inf) & (r2 <= rho2[di])
    ri, di, t, r2 = ri[hit], di[hit], t[hit], r2[hit]
    order = np.lexsort((di, t, ri))                      # per ray: smallest t, then lowest index
    lead = np.ones(len(order), dtype=bool)
    lead[1:] = ri[order][1:] != ri[order][:-1]
    first = order[lead]
    index = np.full(R, -1, dtype=np.int32)
    t_first = np.full(R, np.inf)
    index[ri[first]] = di[first]
    t_first[ri[first]] = t[first]
    got = index >= 0
    count = got.astype(np.int32)
    t_out = t_first.astype(np.longdouble)
    nrm = np.where(got[:, None], N[np.maximum(index, 0)], np.nan)
    with np.errstate(all='ignore'):
        cos64 = _cos_inc(nrm, D)
    cos_out = cos64.astype(np.longdouble)
    kappa = np.ones(R)
    members = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
    if window > 0.0 and len(ri):
        f = np.maximum(index[ri], 0)
        with np.errstate(all='ignore'):
            dot = _dot(N[di, 0], N[di, 1], N[di, 2], N[f, 0], N[f, 1], N[f, 2])
            ln = np.sqrt(_dot(N[di, 0], N[di, 1], N[di, 2], N[di, 0], N[di, 1], N[di, 2]))
            l1 = np.sqrt(_dot(N[f, 0], N[f, 1], N[f, 2], N[f, 0], N[f, 1], N[f, 2]))
            gate = np.abs(dot) / (ln * l1) >= min_cos
            mem = (t <= t_first[ri] + window) & (gate | (di == index[ri]))
            w = np.where(rho2[di] > 0.0, 1.0 - r2 / rho2[di], 0.0)
            a = t - t_first[ri]
        mr, md = ri[mem], di[mem]                         # sorted by ray (np.nonzero's order survives the masks)
        members = (mr, md)
        L = np.longdouble
        wl, al_, sg = w[mem].astype(L), a[mem].astype(L), np.where(dot[mem] < 0.0, -1.0, 1.0).astype(L)
        g = wl / np.sqrt((N[md].astype(L) ** 2).sum(axis=1))
        rays, start = np.unique(mr, return_index=True)
        W = np.add.reduceat(wl, start)
        S = np.add.reduceat(wl * al_, start)
        Nv = np.stack([np.add.reduceat(sg * g * N[md, k].astype(L), start) for k in range(3)], axis=1)
        count[rays] = np.add.reduceat(np.ones(len(mr), dtype=np.int64), start)
        Nlen = np.sqrt((Nv ** 2).sum(axis=1))
        ok_w = W > 0
        ok_n = ok_w & (Nlen > 0)
        with np.errstate(all='ignore'):
            t_out[rays] = np.where(ok_w, t_first[rays].astype(L) + S / W, t_first[rays].astype(L))
            Dl = D[rays].astype(L)
            cosb = np.abs((Nv * Dl).sum(axis=1)) / (Nlen * np.sqrt((Dl ** 2).sum(axis=1)))
            cos_out[rays] = np.where(ok_n, cosb, cos_out[rays])
            kappa[rays] = np.where(ok_n, (W / Nlen).astype(np.float64), 1.0)
    with np.errstate(all='ignore'):
        inc = acos01(np.minimum(1.0, cos_out.astype(np.float64)))
    return Cast(index=index, t_first=t_first, count=count, t=t_out, cos=cos_out, inc=inc, kappa=kappa, members=members)


def t_err_units(got_t, ref):
    """|t - reference| / 2^-52 of the blended depth against the oracle's longdouble value, and the header's count for it
    (surfel_t_err, restated), per ray (hits only).  The reference's own sums carry k 2^-64 relative: REF_SLACK on the bound."""
    ok = ref.index >= 0
    err = np.abs(got_t[ok].astype(np.longdouble) - ref.t[ok]).astype(np.float64) / U52
    k = ref.count[ok].astype(np.float64)
    bound = k * (ref.t[ok].astype(np.float64) - ref.t_first[ok]) + 0.5 * ref.t[ok].astype(np.float64)
    return err, bound * REF_SLACK


def cos_err_units(got_inc, ref):
    """The same for cos(inc) (surfel_cos_err, restated): the cosine of the returned angle against the oracle's longdouble cosine."""
    ok = ref.index >= 0
    err = np.abs(np.cos(got_inc[ok]).astype(np.longdouble) - np.minimum(ref.cos[ok], 1.0)).astype(np.float64) / U52
    bound = (0.5 * ref.count[ok] + 1.75) * ref.kappa[ok] + 7.5
    return err, bound * REF_SLACK


REF_SLACK = 1.0 + 2.0 ** -6          # 64 members x 2^-64 relative in the longdouble sums = 2^-6 of one unit of 2^-52


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
WALL_SIGMA, WALL_RHO, WALL_WINDOW, WALL_RANGE = 0.005, 0.06, 0.1, 1.5
WALL_SENSOR = np.array([1.0, 0.0, WALL_RANGE])


def wall_scene(seed=135, n_rays=4000):
    """A 10 m x 2 m wall (z = 0, x in [0, 10], y in [-1, 1]) surveyed at 850 points / m^2, the centres moved along the normal by
    N(0, 5 mm), true normals; a sensor 1.5 m in front of it at x = 1; rays whose incidence angle is uniform in [0, 78 deg] and whose
    azimuth about the normal is uniform in +-0.15 rad of the wall's long axis.  -> (points, normals, dirs [n_rays,3] unit, sensor
    frame = world axes, theta [n_rays] the true incidence, depth [n_rays] the exact distance to the plane z = 0)."""
    rng = np.random.default_rng(seed)
    m = int(850 * 10 * 2)
    pts = np.stack([rng.uniform(0.0, 10.0, m), rng.uniform(-1.0, 1.0, m), rng.normal(scale=WALL_SIGMA, size=m)], axis=1)
    nrm = np.tile([0.0, 0.0, 1.0], (m, 1))
    theta = rng.uniform(0.0, np.deg2rad(78.0), n_rays)
    az = rng.uniform(-0.15, 0.15, n_rays)
    dirs = np.stack([np.sin(theta) * np.cos(az), np.sin(theta) * np.sin(az), -np.cos(theta)], axis=1)
    depth = WALL_RANGE / -dirs[:, 2]
    return pts, nrm, dirs, theta, depth


def wall_bins(theta, first, blended):
    """Per 10-degree bin of the true incidence: (mean first-hit residual, mean blended residual) -- residuals t - true depth."""
    b = np.minimum((np.rad2deg(theta) // 10).astype(int), 7)
    return [(float(first[b == q].mean()), float(blended[b == q].mean())) for q in range(8)]


def check_wall(theta, first, blended, sigma=WALL_SIGMA):
    """The two assertions of the design note on the wall scene; returns the per-bin means."""
    rows = wall_bins(theta, first, blended)
    for q, (f, bl) in enumerate(rows):
        print('bin %d0-%d0 deg: first-hit mean %+.3f mm, blended mean %+.3f mm, ratio %.3f' % (q, q + 1, 1e3 * f, 1e3 * bl, abs(bl) / abs(f)))
    for q, (f, bl) in enumerate(rows):
        assert f <= -sigma, (q, f)
        assert abs(bl) <= 0.25 * abs(f), (q, f, bl)
    return rows


def check_tree(leaf_index, child, parent, node_box, n):
    """The invariants of the LBVH: leaf_index a permutation, every node but the root has the parent that lists it as a child, and
    every node's box lies inside its parent's (so every leaf box inside every ancestor's)."""
    assert np.array_equal(np.sort(leaf_index), np.arange(n))
    assert parent[0] == -1
    if n == 1:
        return
    assert child.shape == (n - 1, 2) and parent.shape == (2 * n - 1,)
    kids = child.reshape(-1)
    assert np.array_equal(np.sort(kids), np.arange(1, 2 * n - 1))
    par = np.repeat(np.arange(n - 1), 2)
    assert np.array_equal(parent[kids], par)
    assert (node_box[kids, :3] >= node_box[par, :3]).all() and (node_box[kids, 3:] <= node_box[par, 3:]).all()
    for i in range(n - 1):                                  # exact min / max of the children
        a, b = child[i]
        assert np.array_equal(node_box[i, :3], np.minimum(node_box[a, :3], node_box[b, :3]))
        assert np.array_equal(node_box[i, 3:], np.maximum(node_box[a, 3:], node_box[b, 3:]))


ROOM_HALF = np.array([2.0, 1.5, 1.0])
ROOM_POSES = np.array([[[1.0, 0.0, 0.0, 0.4], [0.0, 1.0, 0.0, -0.3], [0.0, 0.0, 1.0, 0.1], [0.0, 0.0, 0.0, 1.0]],
                       [[0.0, -1.0, 0.0, -0.9], [0.0, 0.0, 1.0, 0.5], [-1.0, 0.0, 0.0, -0.2], [0.0, 0.0, 0.0, 1.0]]])


def room_survey(seed=11, m=2000):
    """A survey of the inside of a 4 m x 3 m x 2 m box room: ``m`` points on its six walls (area-weighted), moved along the wall's
    normal by N(0, 5 mm); normals the walls' turned by about a degree, flipped at random (no orientation) and left at lengths between
    0.5 and 2; radii uniform in [0.2, 0.35] m (about ten disks over every surface point).  -> (points, normals [m,3], radii [m])."""
    rng = np.random.default_rng(seed)
    h = ROOM_HALF
    area = np.array([h[1] * h[2], h[1] * h[2], h[0] * h[2], h[0] * h[2], h[0] * h[1], h[0] * h[1]])
    wall = rng.choice(6, size=m, p=area / area.sum())
    axis, side = wall // 2, np.where(wall % 2 == 0, -1.0, 1.0)
    pts = rng.uniform(-1.0, 1.0, size=(m, 3)) * h
    nrm = rng.normal(scale=0.02, size=(m, 3))
    rows = np.arange(m)
    pts[rows, axis] = side * h[axis] + rng.normal(scale=0.005, size=m)
    nrm[rows, axis] = 1.0
    nrm *= (rng.choice([-1.0, 1.0], size=m) * rng.uniform(0.5, 2.0, size=m))[:, None]
    return pts, nrm, rng.uniform(0.2, 0.35, size=m)


def room_rays(seed=12, n=4096, n_scans=2):
    """``n`` rays in ``n_scans`` scans of unequal length: view points within 10 cm of the sensor, unit directions, both exactly
    representable in fp32 -> (vps, dirs f64 [n,3], scan_offset [n_scans+1], poses [n_scans,4,4]).  ROOM_POSES rotate by quarter turns:
    every product of the kernels' pose expressions is exact, so world_rays below forms the rays the device forms, bit for bit."""
    rng = np.random.default_rng(seed)
    vps = rng.uniform(-0.1, 0.1, size=(n, 3)).astype(np.float32).astype(np.float64)
    dirs = rng.normal(size=(n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    cut = sorted(rng.choice(np.arange(1, n), size=n_scans - 1, replace=False).tolist()) if n > 1 else [0] * (n_scans - 1)
    return vps, dirs, np.array([0] + cut + [n], dtype=np.int64), ROOM_POSES[:n_scans].copy()


def world_rays(vps, dirs, scan_offset, poses):
    """Origins and directions in the survey's frame for poses whose rotation entries are 0 and +-1 (exact products; one rounded
    addition of the translation, as in the kernels' pose_point)."""
    o, d = np.zeros_like(vps), np.zeros_like(dirs)
    for s in range(len(scan_offset) - 1):
        a, b = int(scan_offset[s]), int(scan_offset[s + 1])
        R, t = poses[s][:3, :3], poses[s][:3, 3]
        assert np.isin(R, (-1.0, 0.0, 1.0)).all() and (np.abs(R).sum(axis=1) == 1).all()
        for r in range(3):
            c = int(np.argmax(np.abs(R[r])))
            o[a:b, r] = R[r, c] * vps[a:b, c] + t[r]
            d[a:b, r] = R[r, c] * dirs[a:b, c]
    return o, d
