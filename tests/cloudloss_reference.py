"""Reference for the cloud-loss tests (tests/test_cloudloss_host.py, tests/test_gpu_cloudloss.py): the test scene and the closed form
of the loss and its gradient in numpy fp64, no call into the package's kernels.

Scene: the pillared room and the scans of tests/meshloss_reference.py (300, 1, 0 and 129 points), except that the last scan's pose is
a pure translation by dyadic numbers, so that the hand-made points below are formed exactly (x = vp + t with depth 0 and no
correction: every intermediate value is representable, in fp32 storage too).  The survey: N_RANDOM points drawn from the mesh with
numpy's own generator (faces by area, uniform barycentric coordinates), carrying the face normals, behind the hand-made survey points
at the indices 0..3; random points closer than CLEAR to a hand-made query are left out, so that the hand-made cases are decided by
the hand-made points alone.

Hand-made queries, the last five points of the last scan (HAND gives their indices), and one masked-out point (MASKED):
  on_point   exactly on survey point 0 (on the floor): l = 0 in both forms, zero gradient
  tie        equidistant in fp64 from survey points 1 and 2 (d^2 = 2^-8 + 2^-10 both): the lower index wins
  inside     MAX_DIST - 2^-12 above survey point 3: matched
  outside    MAX_DIST + 2^-12 above survey point 3: gated
  nan        a NaN viewpoint coordinate: invalid

Closed form (DESIGN "Supervised training against a surveyed cloud"): x_j = R_s (vp_j + d'_j dir_j) + t_s; y_j the survey point with the
smallest d^2 = ((y0 - x0)^2 + (y1 - x1)^2) + (y2 - x2)^2 (dc_knn.hip's sqdist order; the lower index among equal d^2), matched when
d^2 < max_dist^2; trimmed when sqrt(d^2) > np.quantile(matched distances, ratio); plane form r = n_y . (x - y), l = |r|, dl/dx =
sign(r) n_y; point form l = |x - y|, dl/dx = (x - y) / l; squared: l^2 and its gradient; zero gradient where l = 0.  L is the mean
over the used points; y and n_y are constants of the gradient.  tests/test_cloudloss_host.py holds the closed form to central
differences at frozen correspondences before anything is held to it."""
import numpy as np

import meshloss_reference as M

EXTENT, BAR, SIZES, KINDS = M.EXTENT, M.BAR, M.SIZES, M.KINDS
MAX_DIST = 0.25
N_RANDOM = 4000
CLEAR = 0.6
T_LAST = np.array([0.5, -0.25, 0.125])          # the last scan's pose: identity rotation, this translation
FLOOR = -1.5
HAND_SURVEY = np.array([[0.5, 0.25, FLOOR], [-2.0, 1.0, FLOOR], [-1.875, 1.0, FLOOR], [2.0, -1.0, FLOOR]])
HAND_QUERY = dict(on_point=[0.5, 0.25, FLOOR], tie=[-1.9375, 1.0, FLOOR + 0.03125], inside=[2.0, -1.0, FLOOR + MAX_DIST - 2.0 ** -12],
                  outside=[2.0, -1.0, FLOOR + MAX_DIST + 2.0 ** -12], nan=[np.nan, 0.0, 0.0])
HAND_ORDER = ('on_point', 'tie', 'inside', 'outside', 'nan')
N_ALL = sum(SIZES)
HAND = {name: N_ALL - len(HAND_ORDER) + k for k, name in enumerate(HAND_ORDER)}
MASKED = 7


def survey(seed=3):
    """(points [M,3], unit normals [M,3]) of the test survey."""
    mesh = M.room()
    rng = np.random.default_rng(seed)
    tri = mesh.vertices[mesh.faces]
    area = mesh.face_areas()
    face = rng.choice(len(area), size=N_RANDOM, p=area / area.sum())
    u, v = rng.random(N_RANDOM), rng.random(N_RANDOM)
    s = np.sqrt(u)
    pts = (1 - s)[:, None] * tri[face, 0] + (s * (1 - v))[:, None] * tri[face, 1] + (s * v)[:, None] * tri[face, 2]
    nrm = mesh.face_normals()[face]
    q = np.array([HAND_QUERY[k] for k in HAND_ORDER if k != 'nan'])
    keep = (np.linalg.norm(pts[:, None, :] - q[None, :, :], axis=2) > CLEAR).all(axis=1)
    up = np.tile([0.0, 0.0, 1.0], (len(HAND_SURVEY), 1))
    return np.concatenate([HAND_SURVEY, pts[keep]]), np.concatenate([up, nrm[keep]])


def scene(dtype=np.float64, seed=11, sizes=SIZES):
    """(mesh, scans, poses, loss_mask): meshloss_reference.scene with the last scan re-posed and the hand-made points in place (a last
    scan of fewer points than there are hand-made ones is only re-posed)."""
    mesh, scans, poses = M.scene(sizes=sizes, seed=seed, dtype=np.float64)
    last = len(scans) - 1
    c, T = scans[last], poses[last]
    world = (c['vps'] + c['depth'][:, None] * c['dirs']) @ T[:3, :3].T + T[:3, 3]        # where the scan's points lie
    Tn = np.eye(4)
    Tn[:3, 3] = T_LAST
    vps = c['vps'].copy()
    ray = (world - T_LAST) - vps
    depth = np.linalg.norm(ray, axis=1)
    dirs = ray / depth[:, None]
    lmask = np.ones(len(depth), bool)
    k0 = len(depth) - len(HAND_ORDER)
    for k, name in enumerate(HAND_ORDER if k0 >= 0 else ()):
        vps[k0 + k] = np.array(HAND_QUERY[name]) - T_LAST
        dirs[k0 + k] = [0.0, 0.0, 1.0]
        depth[k0 + k] = 0.0
        lmask[k0 + k] = False
    scans[last] = dict(vps=vps, dirs=dirs, depth=depth, inc=c['inc'].copy(), lmask=lmask)
    poses = poses.copy()
    poses[last] = Tn
    scans = [{k: (v if k == 'lmask' else v.astype(dtype)) for k, v in s.items()} for s in scans]
    loss_mask = np.ones(sum(sizes), bool)
    loss_mask[MASKED] = False
    return mesh, scans, poses, loss_mask


def nearest(survey_pts, x, chunk=64):
    """(idx [n], d2 [n], second d2 [n]) of the brute-force 1-NN with sqdist's operation order; the lowest index among equal d2; rows
    of x that are not finite get -1 / inf / inf."""
    n = len(x)
    idx, best, second = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    ok = np.flatnonzero(np.isfinite(x).all(axis=1))
    for a in range(0, len(ok), chunk):
        rows = ok[a:a + chunk]
        d = survey_pts[None, :, :] - x[rows][:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = np.argmin(d2, axis=1)                                     # the first minimum: the lower index
        idx[rows], best[rows] = j, d2[np.arange(len(rows)), j]
        d2[np.arange(len(rows)), j] = np.inf
        second[rows] = d2.min(axis=1)
    return idx, best, second


def pair_d2(survey_pts, x, idx):
    d = survey_pts[np.maximum(idx, 0)] - x
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def cloud_loss(survey_pts, survey_nrm, scans, poses, kind=None, w=None, e=None, idx=None, loss_mask=None, plane=True, squared=False,
               max_dist=MAX_DIST, ratio=1.0):
    """The closed form.  ``idx``: the survey point of every point (the device's; < 0: none), else the brute force's.  Returns a dict:
    loss, used / gated / trimmed / invalid, threshold, gw, ge, gT (gradients of the mean), per point x, idx, dist, r, mask (used),
    matched, and ``terms`` for grad_bounds."""
    pt = M.points(scans, poses, kind, w, e)
    x = pt['x']
    n, S = len(x), len(scans)
    in_mask = np.ones(n, bool) if loss_mask is None else np.asarray(loss_mask, bool)
    finite = np.isfinite(x).all(axis=1)
    ok = in_mask & finite
    with np.errstate(invalid='ignore'):
        if idx is None:
            j, d2, _ = nearest(survey_pts, x)
            j = np.where(ok & (d2 < max_dist * max_dist), j, -1)
        else:
            j = np.where(ok, np.asarray(idx, np.int64), -1)
        d2 = np.where(j >= 0, pair_d2(survey_pts, x, j), np.inf)
    matched = j >= 0
    dist = np.sqrt(d2)
    thr = np.inf
    if ratio < 1.0:
        thr = np.quantile(dist[matched], ratio) if matched.any() else np.nan
    with np.errstate(invalid='ignore'):
        trimmed = matched & (dist > thr)
    used = matched & ~trimmed
    Mn = int(used.sum())
    y, nv = survey_pts[np.maximum(j, 0)], survey_nrm[np.maximum(j, 0)]
    diff = np.where(used[:, None], x - y, 0.0)
    P = pt['dw'].shape[1]
    g = np.zeros((n, 3))
    if plane:
        r = (nv[:, 0] * diff[:, 0] + nv[:, 1] * diff[:, 1]) + nv[:, 2] * diff[:, 2]
        ell = r * r if squared else np.abs(r)
        g = (2.0 * r)[:, None] * nv if squared else np.sign(r)[:, None] * nv
    else:
        r = np.where(used, dist, 0.0)
        ell = np.where(used, d2, 0.0) if squared else r
        if squared:
            g = 2.0 * diff
        else:
            nz = used & (r > 0)
            g[nz] = diff[nz] / r[nz][:, None]
    g = np.where(used[:, None], g, 0.0)
    out = dict(used=Mn, gated=int((ok & ~matched).sum()), trimmed=int(trimmed.sum()), invalid=int((in_mask & ~finite).sum()),
               threshold=thr, x=x, idx=np.where(used, j, -1), match=j, dist=dist, r=np.where(used, r, np.nan), mask=used, matched=matched)
    if Mn == 0:
        out.update(loss=np.nan, gw=np.zeros(P), ge=np.zeros(P), gT=np.zeros((S, 3, 4)), terms={})
        return out
    g = g / Mn
    gd = (np.where(used[:, None], pt['rdir'], 0.0) * g).sum(axis=1)
    tw, te = gd[:, None] * pt['dw'], gd[:, None] * pt['de']
    xl1 = np.concatenate([pt['xl'], np.ones((n, 1))], axis=1)
    tT = np.where(used[:, None, None], g[:, :, None] * np.where(used[:, None], xl1, 0.0)[:, None, :], 0.0)
    gT = np.stack([tT[pt['scan'] == s].sum(axis=0) for s in range(S)])
    out.update(loss=np.where(used, ell, 0.0).sum() / Mn, gw=tw.sum(axis=0), ge=te.sum(axis=0), gT=gT,
               terms=dict(gw=tw, ge=te, gT=tT.reshape(n, 12), scan=pt['scan'], rdir=np.where(used[:, None], pt['rdir'], 0.0), dw=pt['dw'],
                          de=pt['de'], xl1=np.where(used[:, None], xl1, 0.0), M=Mn))
    return out


def grad_bounds(ref, plane=True, squared=False, bar=BAR):
    """Bound of |device - reference| per gradient entry sum_j a_j -> dict gw [P], ge [P], gT [S,3,4], built like
    meshloss_reference.grad_bounds.  First term: 2^-40 sum |a_j| (fp64 summation of <= 1e3 terms, with headroom).  Second term, the
    error of x - y (x is good to ``bar``, y is exact): point form, not squared, sum |a_j| 2 bar / l_j -- the conditioning of the unit
    vector (x - y) / l at small l; squared (both forms), where dl/dx is linear in x - y (2 (x - y), or 2 n n^T (x - y) with |n| = 1),
    the per-component error 2 bar times the coefficient; plane form, not squared: dl/dx = sign(r) n does not depend on x - y beyond
    the sign: no conditioning term."""
    t, used, S, Mn = ref['terms'], ref['mask'], ref['gT'].shape[0], ref['terms']['M']
    zero = {name: np.zeros_like(t[name]) for name in ('gw', 'ge', 'gT')}
    if squared:
        unit = np.where(used, 2.0 * bar * 2.0 / Mn, 0.0)
        second = dict(gw=unit[:, None] * np.abs(t['dw']) * np.abs(t['rdir']).sum(axis=1)[:, None],
                      ge=unit[:, None] * np.abs(t['de']) * np.abs(t['rdir']).sum(axis=1)[:, None],
                      gT=unit[:, None] * np.tile(np.abs(t['xl1']), (1, 3)))
    elif plane:
        second = zero
    else:
        ell = ref['dist']
        with np.errstate(divide='ignore', invalid='ignore'):
            cond = np.where(used & (ell > 0), 2.0 * bar / np.where(used & (ell > 0), ell, 1.0), 0.0)
        second = {name: np.abs(t[name]) * cond[:, None] for name in ('gw', 'ge', 'gT')}
    out = {}
    for name in ('gw', 'ge'):
        out[name] = 2.0 ** -40 * np.abs(t[name]).sum(axis=0) + second[name].sum(axis=0)
    per = 2.0 ** -40 * np.abs(t['gT']) + second['gT']
    out['gT'] = np.stack([per[t['scan'] == s].sum(axis=0) for s in range(S)]).reshape(S, 3, 4)
    return out
