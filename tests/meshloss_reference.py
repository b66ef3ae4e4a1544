"""Reference for the mesh-loss tests (tests/test_meshloss_host.py, tests/test_gpu_meshloss.py): the test scene and the closed
form of the loss and its gradient in numpy fp64, no call into the package's kernels.

Scene: the pillared room room_mesh((4, 3, 1.5), cell=1, pillars=[((1, .5, -.5), (.3, .3, 1))]) (380 faces); scans of 300, 1, 0 and
129 points -- a partly filled 128-lane block, a one-point scan, an empty scan, one point over a block -- built from seeded surface
samples (tests/mesh_reference.sample) seen from seeded poses, the true depth biased by the inverse of
ScaledPolynomial(w=[-0.01, 0.004], e=[2, 4]) plus 1 cm of noise.

Closed form (DESIGN "Supervised training against the mesh"): x_j = R_s (vp_j + d'_j dir_j) + t_s, c_j the closest point of the mesh,
r_j = |x_j - c_j|, L = mean of r_j (or r_j^2) over the used points, dr/dx = (x - c) / r because c minimises the distance.
tests/test_meshloss_host.py holds it to central differences before anything is held to it."""
import numpy as np

import mesh_reference as R

ROOM = dict(half_extents=(4, 3, 1.5), cell=1.0, pillars=[((1, .5, -.5), (.3, .3, 1))])
EXTENT = 8.0                                   # the room's longest side [m]: the scale of the coordinates
BAR = 2.0 ** -40 * EXTENT                      # the distance bar of tests/test_gpu_meshdist.py (its header gives the reason)
SIZES = (300, 1, 0, 129)
W_TRUE, E_TRUE = (-0.01, 0.004), (2.0, 4.0)
KINDS = {None: 0, 'Polynomial': 1, 'ScaledPolynomial': 2, 'Linear': 3, 'InvCos': 4, 'ScaledInvCos': 5}


def room():
    from depth_correction_amd.mesh import room_mesh
    return room_mesh(**ROOM)


def _rot(rng, scale):
    """Rotation by a seeded axis-angle vector of about ``scale`` rad (Rodrigues)."""
    v = rng.normal(scale=scale, size=3)
    a = np.linalg.norm(v)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def scene(sizes=SIZES, seed=11, dtype=np.float64):
    """(mesh, scans, poses [S,4,4]): scans = list of dicts vps [n,3], dirs [n,3], depth [n], inc [n], lmask [n] (all True) in the
    sensor frame, stored in ``dtype`` (the reference then works on those stored values, in fp64)."""
    mesh = room()
    rng = np.random.default_rng(seed)
    normals = mesh.face_normals()
    scans, poses = [], []
    for s, n in enumerate(sizes):
        T = np.eye(4)
        T[:3, :3] = _rot(rng, 0.3)
        T[:3, 3] = rng.uniform(-1, 1, size=3) * np.array([2.0, 1.5, 0.6]) + np.array([-1.5, -1.0, 0.0])
        poses.append(T)
        pts, face = R.sample(mesh.vertices, mesh.faces, n, seed=100 + s) if n else (np.zeros((0, 3)), np.zeros(0, np.int64))
        local = (pts - T[:3, 3]) @ T[:3, :3]                       # R^T (p - t)
        vps = rng.normal(scale=0.03, size=(n, 3))
        ray = local - vps
        depth = np.linalg.norm(ray, axis=1)
        dirs = ray / depth[:, None]
        inc = np.arccos(np.clip(np.abs(((dirs @ T[:3, :3].T) * normals[face]).sum(axis=1)), 0.0, 1.0))
        bias = W_TRUE[0] * inc ** E_TRUE[0] + W_TRUE[1] * inc ** E_TRUE[1]
        measured = depth / (1.0 - bias) + rng.normal(scale=0.01, size=n)
        scans.append(dict(vps=vps.astype(dtype), dirs=dirs.astype(dtype), depth=measured.astype(dtype), inc=inc.astype(dtype),
                          lmask=np.ones(n, dtype=bool)))
    return mesh, scans, np.stack(poses)


def model_depth(kind, w, e, d, g, lmask):
    """(d' [n], dd'/dw [n,P], dd'/de [n,P]) of the kernel models (csrc/dc_pointmath.h) on the points of ``lmask``; others keep d."""
    code = KINDS[kind]
    P = 0 if code == 0 else len(w)
    dw, de = np.zeros((len(d), P)), np.zeros((len(d), P))
    out = d.copy()
    if code == 0:
        return out, dw, de
    w, e = np.asarray(w, np.float64), np.asarray(e, np.float64)
    if code in (1, 2):
        pk = g[:, None] ** e[None, :]
        b = pk @ w
        scale = d if code == 2 else np.ones_like(d)
        dep = d * (1.0 - b) if code == 2 else d - b
        dw = -scale[:, None] * pk
        with np.errstate(divide='ignore', invalid='ignore'):
            lg = np.where(g > 0, np.log(np.where(g > 0, g, 1.0)), 0.0)
        de = -scale[:, None] * pk * w[None, :] * lg[:, None]
    elif code == 3:
        dep = w[0] * d + w[1] * g + w[2]
        dw = np.stack([d, g, np.ones_like(d)], axis=1)
    elif code == 4:
        dep = d - w[0] / np.cos(g)
        dw = (-1.0 / np.cos(g))[:, None]
    else:
        dep = d * (1.0 - w[0] / np.abs(np.cos(g)))
        dw = (-d / np.abs(np.cos(g)))[:, None]
    out = np.where(lmask, dep, d)
    dw = np.where(lmask[:, None], dw, 0.0)
    de = np.where(lmask[:, None], de, 0.0)
    return out, dw, de


def points(scans, poses, kind=None, w=None, e=None):
    """Corrected, posed points of all scans, scan-major, with what the gradient needs: dict x [N,3], xl [N,3] (sensor frame),
    rdir [N,3] = R_s dir, dw / de [N,P], scan [N]."""
    xs, xls, rd, dws, des, sid = [], [], [], [], [], []
    for s, (c, T) in enumerate(zip(scans, poses)):
        f = {k: np.asarray(c[k], np.float64) for k in ('vps', 'dirs', 'depth', 'inc')}
        dep, dw, de = model_depth(kind, w, e, f['depth'], f['inc'], np.asarray(c['lmask'], bool))
        xl = f['vps'] + dep[:, None] * f['dirs']
        xs.append(xl @ T[:3, :3].T + T[:3, 3])
        xls.append(xl)
        rd.append(f['dirs'] @ T[:3, :3].T)
        dws.append(dw)
        des.append(de)
        sid.append(np.full(len(dep), s))
    cat = np.concatenate
    return dict(x=cat(xs), xl=cat(xls), rdir=cat(rd), dw=cat(dws), de=cat(des), scan=cat(sid))


def mesh_loss(mesh, scans, poses, kind=None, w=None, e=None, face=None, loss_mask=None, squared=False, max_dist=None):
    """The closed form.  ``face``: the face of every point (the device's), else the brute force's best.  Returns a dict: loss, used /
    gated / invalid counts, gw [P], ge [P], gT [S,3,4] (gradients of the mean), the per-point x, r, c, face, used, and ``terms``:
    {name: [N, entries]} the per-point contributions a_j of every gradient entry (already divided by M), for the tests' bounds."""
    pt = points(scans, poses, kind, w, e)
    x = pt['x']
    n, S = len(x), len(scans)
    in_mask = np.ones(n, bool) if loss_mask is None else np.asarray(loss_mask, bool)
    finite = np.isfinite(x).all(axis=1)
    ok = in_mask & finite
    r, c = np.full(n, np.inf), np.full((n, 3), np.nan)
    fc = np.full(n, -1, np.int64)
    if ok.any():
        if face is None:
            fc[ok] = R.brute_force(mesh.vertices, mesh.faces, x[ok])[0]
        else:
            fc[ok] = np.asarray(face)[ok]
        good = ok & (fc >= 0)
        r[good], c[good] = R.distance_to_faces(mesh.vertices, mesh.faces, x[good], fc[good])
    used = ok & np.isfinite(r) & ((r <= max_dist) if max_dist else True)
    M = int(used.sum())
    out = dict(used=M, gated=int((ok & ~used).sum()), invalid=int((in_mask & ~finite).sum()), x=x, r=r, c=c, face=fc, mask=used)
    P = pt['dw'].shape[1]
    g = np.zeros((n, 3))
    diff = x - c
    if squared:
        g[used] = 2.0 * diff[used]
    else:
        nz = used & (r > 0)
        g[nz] = diff[nz] / r[nz][:, None]
    if M == 0:
        out.update(loss=np.nan, gw=np.zeros(P), ge=np.zeros(P), gT=np.zeros((S, 3, 4)), terms={})
        return out
    g /= M
    ell = np.where(used, r ** 2 if squared else r, 0.0)
    gd = (pt['rdir'] * g).sum(axis=1)                               # (R dir) . g
    tw, te = gd[:, None] * pt['dw'], gd[:, None] * pt['de']
    xl1 = np.concatenate([pt['xl'], np.ones((n, 1))], axis=1)
    tT = g[:, :, None] * xl1[:, None, :]                            # [N,3,4]: g (xl, 1)^T
    tT = np.where(used[:, None, None], tT, 0.0)
    gT = np.stack([tT[pt['scan'] == s].sum(axis=0) for s in range(S)])
    out.update(loss=ell.sum() / M, gw=tw.sum(axis=0), ge=te.sum(axis=0), gT=gT,
               terms=dict(gw=tw, ge=te, gT=tT.reshape(n, 12), scan=pt['scan'], rdir=pt['rdir'], dw=pt['dw'], de=pt['de'], xl1=xl1, M=M))
    return out


def grad_bounds(ref, squared=False, bar=BAR):
    """Bound of |device - reference| per gradient entry sum_j a_j -> dict gw [P], ge [P], gT [S,3,4].  First term: 2^-40 sum |a_j|
    (fp64 summation of <= 1e3 terms, with headroom).  Second term, the error of x - c (x and c are each good to ``bar``):
    not squared, sum |a_j| 2 bar / r_j -- the conditioning of the unit vector (x - c) / r at small r; squared, where
    a_j = sum_comp 2 (x - c)_comp coef_comp / M is linear in x - c, the per-component error 2 bar times the coefficient."""
    t, used, r = ref['terms'], ref['mask'], ref['r']
    S, M = ref['gT'].shape[0], t['M']
    if squared:
        unit = np.where(used, 2.0 * bar * 2.0 / M, 0.0)                                  # error of one component of g_j
        second = dict(gw=unit[:, None] * np.abs(t['dw']) * np.abs(t['rdir']).sum(axis=1)[:, None],
                      ge=unit[:, None] * np.abs(t['de']) * np.abs(t['rdir']).sum(axis=1)[:, None],
                      gT=unit[:, None] * np.tile(np.abs(t['xl1']), (1, 3)))
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            cond = np.where(used & (r > 0), 2.0 * bar / np.where(r > 0, r, 1.0), 0.0)
        second = {name: np.abs(t[name]) * cond[:, None] for name in ('gw', 'ge', 'gT')}
    out = {}
    for name in ('gw', 'ge'):
        out[name] = 2.0 ** -40 * np.abs(t[name]).sum(axis=0) + second[name].sum(axis=0)
    per = 2.0 ** -40 * np.abs(t['gT']) + second['gT']
    out['gT'] = np.stack([per[t['scan'] == s].sum(axis=0) for s in range(S)]).reshape(S, 3, 4)
    return out
