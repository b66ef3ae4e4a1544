"""References for the BVH ray caster (csrc/dc_raycast.hip, csrc/dc_raymath.h).

oracle      the kernels' own test_triangle (host build of dc_raymath.h) applied to every face in index order, no tree: what
            dc_raycast / dc_raycast_rays must return bit for bit, whatever the traversal does.
classify    an independent classifier that shares no arithmetic with the header: Moeller-Trumbore in numpy fp64 over all faces, in
            coordinates local to ``center``.  Per ray: clear hit, clear miss or borderline.
check_bvh   the invariants of test_gpu_raycast.test_bvh_structure as a function.
build_tree  trees of a chosen shape over given leaf boxes, in the library's node numbering: what the one walk (csrc/dc_bvh.h) is
            run over in tests/test_bvh_walk_host.py and tests/test_gpu_bvh_walk.py.
"""
import numpy as np

MISS, HIT, BORDERLINE = 0, 1, 2
EPS = 1e-9                  # a barycentric margin, a gap in t or a cosine below this (relative) decides nothing
COINCIDENT = 1e-12          # hits whose t agree to this (relative) lie on coincident faces: one surface, any of them may win


def oracle(lib, verts, faces, o, d, t_min, cull):
    """(face i32 [R], t, u, v f64 [R]) of the rays (o, d) [R,3] in the world frame; ``lib`` = helpers.raycast_host_lib()."""
    from helpers import host_ray_cast_brute
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces)].reshape(-1, 9)
    return host_ray_cast_brute(lib, tri, o, d, t_min, cull)


def _local(x, center):
    """x - center, which must be exact (Sterbenz: every coordinate within a factor two of the centre's, or the centre 0)."""
    y = x - center
    assert np.array_equal(y + center, x), 'the local frame must not round'
    return y


class Classified(object):
    """status [R] (MISS / HIT / BORDERLINE), t [R] of the clear hits (inf else), face [R] the lowest face index of the winning
    surface (-1 else), n_tied [R] the number of coincident faces on it, got_ok [R]: ``got_face`` is one of them (clear hits), or
    -1 (clear misses)."""

    def __init__(self, status, t, face, n_tied, got_ok):
        self.status, self.t, self.face, self.n_tied, self.got_ok = status, t, face, n_tied, got_ok


def classify(verts, faces, o, d, t_min, cull, center=(0.0, 0.0, 0.0), got_face=None):
    """Classify the rays (o, d) [R,3] against every face.  A (ray, face) pair is IN when the ray crosses the face's plane beyond
    t_min with all three barycentric weights above EPS (and the face turned towards the ray by more than EPS in cosine with
    ``cull``), OUT when one of these fails by more than EPS, undecided otherwise -- an edge-on face is OUT when the ray stays off
    its plane and undecided when it lies in it; a face of no area is OUT unless the ray's line meets its longest edge's line.  A ray
    is a clear hit at the smallest t among its IN faces when nothing undecided and no IN face off that surface comes within EPS
    (relative) of it; faces whose t agree to COINCIDENT are one surface.  A clear miss has no IN and no undecided face."""
    center = np.asarray(center, dtype=np.float64)
    V = _local(np.asarray(verts, dtype=np.float64), center)
    O = _local(np.asarray(o, dtype=np.float64).reshape(-1, 3), center)
    D = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(faces).astype(np.int64)
    R = O.shape[0]
    t_min = np.broadcast_to(np.asarray(t_min, dtype=np.float64), (R,))
    v0, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    n = np.cross(e1, e2)
    nn = np.einsum('fc,fc->f', n, n)
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    flat = ~(np.sqrt(nn) > EPS * l1 * l2)                          # no area (a zero edge included)
    nlen = np.sqrt(nn)
    size = l1 + l2 + np.linalg.norm(v0, axis=1)
    # faces of no area: the line of the longest edge
    e3 = e2 - e1
    longest = np.where((l1 >= l2)[:, None], e1, e2)
    longest = np.where((np.linalg.norm(e3, axis=1) > np.maximum(l1, l2))[:, None], e3, longest)
    base = np.where((np.linalg.norm(e3, axis=1) > np.maximum(l1, l2))[:, None], V[F[:, 1]], v0)

    status = np.full(R, BORDERLINE)
    t_out, f_out, n_tied = np.full(R, np.inf), np.full(R, -1), np.zeros(R, dtype=np.int64)
    got_ok = np.zeros(R, dtype=bool)
    chunk = max(1, 1000000 // max(1, F.shape[0]))
    for s in range(0, R, chunk):
        with np.errstate(all='ignore'):                               # infinities and NaN are sorted out by the masks
            Oc, Dc, tm = O[s:s + chunk], D[s:s + chunk], t_min[s:s + chunk, None]
            dl = np.linalg.norm(Dc, axis=1)[:, None]
            ol = np.linalg.norm(Oc, axis=1)[:, None]
            # Moeller-Trumbore, component by component on [rays, faces] arrays: p = d x e2, det = e1 . p, tv = o - v0, q = tv x e1
            dx, dy, dz = (Dc[:, k, None] for k in range(3))
            tx, ty, tz = (Oc[:, k, None] - v0[None, :, k] for k in range(3))
            e1x, e1y, e1z = (e1[None, :, k] for k in range(3))
            e2x, e2y, e2z = (e2[None, :, k] for k in range(3))
            px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
            det = e1x * px + e1y * py + e1z * pz
            qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
            inv = 1.0 / det
            u = (tx * px + ty * py + tz * pz) * inv
            v = (dx * qx + dy * qy + dz * qz) * inv
            t = (e2x * qx + e2y * qy + e2z * qz) * inv
            dn = -det                                                     # d . n
            sn = tx * n[None, :, 0] + ty * n[None, :, 1] + tz * n[None, :, 2]
            m = np.minimum(np.minimum(u, v), 1.0 - u - v)
            edge_on = np.abs(dn) <= EPS * nlen[None] * dl
            in_plane = np.abs(sn) <= EPS * nlen[None] * (ol + size[None])
            near = np.abs(t - tm) <= EPS * np.abs(tm) + 1e-12 * (ol + size[None]) / dl
            is_in = (m > EPS) & (t > tm) & ~near & ~edge_on
            is_out = (m < -EPS) | ((t <= tm) & ~near)
            if cull:
                is_in &= dn < 0
                is_out |= (dn > 0) & ~edge_on
            is_out = np.where(edge_on, ~in_plane, is_out)
            und = ~is_in & ~is_out                                        # undecided; NaN anywhere lands here
            t_und = np.where(edge_on, -np.inf, t)
            if flat.any():
                k = np.nonzero(flat)[0]
                w = np.cross(Dc[:, None, :], longest[None, k, :])         # [r, k, 3]
                wl = np.linalg.norm(w, axis=2)
                off = base[None, k, :] - Oc[:, None, :]
                with np.errstate(divide='ignore', invalid='ignore'):
                    dist = np.abs(np.einsum('rkc,rkc->rk', off, w)) / wl
                par = ~(wl > EPS * dl * np.linalg.norm(longest[k], axis=1)[None])     # parallel lines (or a point): distance point - ray line
                pd = np.linalg.norm(np.cross(off, Dc[:, None, :]), axis=2) / dl
                dist = np.where(par, pd, dist)
                touch = ~(dist > EPS * (ol + size[None, k]))
                is_in[:, k] = False
                und[:, k] = touch
                t_und[:, k] = -np.inf
            t_in = np.where(is_in, t, np.inf)
            t1 = t_in.min(axis=1)
            with np.errstate(invalid='ignore'):
                tied = is_in & (t_in <= (t1 * (1.0 + COINCIDENT))[:, None])
            rest = np.where(tied, np.inf, t_in).min(axis=1)
            rest = np.minimum(rest, np.where(und, t_und, np.inf).min(axis=1))
            with np.errstate(invalid='ignore'):
                hit = np.isfinite(t1) & (rest - t1 > EPS * t1)
            miss = np.isinf(t1) & np.isinf(rest) & (rest > 0)
            st = np.where(hit, HIT, np.where(miss, MISS, BORDERLINE))
            status[s:s + chunk] = st
            t_out[s:s + chunk] = np.where(hit, t1, np.inf)
            f_out[s:s + chunk] = np.where(hit, tied.argmax(axis=1), -1)
            n_tied[s:s + chunk] = np.where(hit, tied.sum(axis=1), 0)
            if got_face is not None:
                g = np.asarray(got_face).reshape(-1)[s:s + chunk].astype(np.int64)
                rows = np.arange(len(g))
                got_ok[s:s + chunk] = np.where(hit, tied[rows, np.maximum(g, 0)] & (g >= 0), miss & (g < 0))
    return Classified(status, t_out, f_out, n_tied, got_ok)


def check_bvh(bvh, mesh):
    """Assert that ``bvh`` (a mesh.MeshBVH, or anything with its five arrays) is a valid tree over ``mesh``: every face in exactly
    one leaf, one root, every other node the child of its parent, parents' boxes around their children's, leaf boxes around their
    fp64 vertices, every leaf within the traversal stack's depth of the root."""
    def host(x):
        return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
    n = len(mesh)
    leaf_face, child, parent = host(bvh.leaf_face), host(bvh.child), host(bvh.parent)
    box = host(bvh.node_box).astype(np.float64)
    tri = host(bvh.leaf_tri)
    assert leaf_face.shape == (n,) and parent.shape == (2 * n - 1,) and box.shape == (2 * n - 1, 6) and tri.shape == (n, 9)
    assert np.array_equal(np.sort(leaf_face), np.arange(n))
    assert np.array_equal(tri.reshape(n, 3, 3), mesh.vertices[mesh.faces[leaf_face]])
    assert parent[0] == -1
    assert np.isfinite(box).all()
    v = tri.reshape(n, 3, 3)
    assert (box[n - 1:, :3] <= v.min(axis=1)).all() and (box[n - 1:, 3:] >= v.max(axis=1)).all()
    if n == 1:
        return
    assert child.shape == (n - 1, 2)
    kids = child.reshape(-1)
    assert np.array_equal(np.sort(kids), np.arange(1, 2 * n - 1))
    assert np.array_equal(parent[kids], np.repeat(np.arange(n - 1), 2))
    for s in (0, 1):
        assert (box[child[:, s], :3] >= box[:n - 1, :3]).all() and (box[child[:, s], 3:] <= box[:n - 1, 3:]).all()
    node, depth = np.arange(n - 1, 2 * n - 1), 0
    while (node > 0).any():
        node = np.where(node > 0, parent[np.maximum(node, 0)], 0)
        depth += 1
        assert depth <= 64
    assert (node == 0).all()


MAX_DEPTH = 63              # of a tree the walk may be given (csrc/dc_bvh.h: its stack holds one postponed node per level)


def build_tree(leaf_box, comb=0):
    """A binary tree over the leaves 0 .. n-1, in this order, with the boxes leaf_box f32 [n,6]: internal nodes 0 .. n-2 numbered in
    pre-order (root 0), leaf i is node n-1+i, an inner box the exact min / max of its children's.  The first ``comb`` levels split off
    the LAST leaf of their range as the second child (a left-deep comb: the rest is the first child), the levels below split at the
    median.  -> (child i32 [n-1,2], parent i32 [2n-1], node_box f32 [2n-1,6], depth); the depth must not exceed MAX_DEPTH."""
    leaf_box = np.asarray(leaf_box, dtype=np.float32).reshape(-1, 6)
    n = len(leaf_box)
    child, parent = np.zeros((n - 1, 2), dtype=np.int32), np.full(2 * n - 1, -1, dtype=np.int32)
    box = np.concatenate([np.zeros((n - 1, 6), dtype=np.float32), leaf_box])
    used, deepest = [0], [0]

    def node(lo, hi, level):
        deepest[0] = max(deepest[0], level)
        if hi - lo == 1:
            return n - 1 + lo
        i = used[0]
        used[0] += 1
        mid = hi - 1 if level < comb else (lo + hi) // 2
        a, b = node(lo, mid, level + 1), node(mid, hi, level + 1)
        child[i], parent[[a, b]] = (a, b), i
        box[i] = np.concatenate([np.minimum(box[a, :3], box[b, :3]), np.maximum(box[a, 3:], box[b, 3:])])
        return i
    node(0, n, 0)
    assert deepest[0] <= MAX_DEPTH, deepest[0]
    return child, parent, box, deepest[0]


# ---- the scenes of tests/test_gpu_raycast_edge.py (checked on the host by tests/test_raycast_host.py) --------------------------------
class Case(object):
    """One cast: a mesh (verts, faces; ``scene_box`` None = the mesh's bounds), world-frame rays (o, d [R,3], t_min [R]) with
    ``aimed`` [R] marking the rays aimed at an edge or a vertex on purpose, ``cull``, the classifier's local frame ``center``, and the
    call that produces these rays on the device: ``api`` 'raycast' (dirs [r,3], poses [P,4,4], t_min [r]; R = P r) or 'rays' (vps,
    dirs [R,3], scan_offset, poses, a scalar t_min).  Poses rotate by the identity, so the kernels' pose products are exact and
    the world rays here are bit for bit the ones the device forms."""

    def __init__(self, name, verts, faces, cull, center=(0.0, 0.0, 0.0), scene_box=None):
        self.name, self.verts, self.faces, self.cull, self.center, self.scene_box = name, verts, np.asarray(faces), cull, center, scene_box

    def raycast(self, dirs, origins, t_min, aimed):
        dirs, origins = np.asarray(dirs, dtype=np.float64).reshape(-1, 3), np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        self.api, self.dirs, self.t_min_arg = 'raycast', dirs, np.broadcast_to(np.asarray(t_min, dtype=np.float64), (len(dirs),)).copy()
        self.poses = np.tile(np.eye(4), (len(origins), 1, 1))
        self.poses[:, :3, 3] = origins
        # M[0] s0 + M[1] s1 + M[2] s2 with the identity: s + 0 s' + 0 s'' (the sign of a zero follows the kernel's sum)
        s = dirs
        dw = np.stack([(s[:, 0] + 0.0 * s[:, 1]) + 0.0 * s[:, 2], (0.0 * s[:, 0] + s[:, 1]) + 0.0 * s[:, 2],
                       (0.0 * s[:, 0] + 0.0 * s[:, 1]) + s[:, 2]], axis=1)
        P = len(origins)
        self.o, self.d = np.repeat(origins, len(dirs), axis=0), np.tile(dw, (P, 1))
        self.t_min = np.tile(self.t_min_arg, P)
        self.aimed = np.broadcast_to(np.asarray(aimed, dtype=bool), (P, len(dirs))).reshape(-1).copy()      # [r], or [P, r]
        return self

    def rays(self, vps, dirs, counts, origins, t_min, aimed, dtype=np.float64):
        vps, dirs = np.asarray(vps, dtype=dtype).reshape(-1, 3), np.asarray(dirs, dtype=dtype).reshape(-1, 3)
        origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        self.api, self.vps, self.dirs, self.t_min_arg, self.dtype = 'rays', vps, dirs, float(t_min), dtype
        self.scan_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert self.scan_offset[-1] == len(dirs) and len(counts) == len(origins)
        self.poses = np.tile(np.eye(4), (len(origins), 1, 1))
        self.poses[:, :3, 3] = origins
        s, v = dirs.astype(np.float64), vps.astype(np.float64)
        T = np.repeat(origins, counts, axis=0)
        self.d = np.stack([(s[:, 0] + 0.0 * s[:, 1]) + 0.0 * s[:, 2], (0.0 * s[:, 0] + s[:, 1]) + 0.0 * s[:, 2],
                           (0.0 * s[:, 0] + 0.0 * s[:, 1]) + s[:, 2]], axis=1)
        self.o = np.stack([((v[:, 0] + 0.0 * v[:, 1]) + 0.0 * v[:, 2]) + T[:, 0], ((0.0 * v[:, 0] + v[:, 1]) + 0.0 * v[:, 2]) + T[:, 1],
                           ((0.0 * v[:, 0] + 0.0 * v[:, 1]) + v[:, 2]) + T[:, 2]], axis=1)
        self.t_min = np.full(len(dirs), float(t_min))
        self.aimed = np.broadcast_to(np.asarray(aimed, dtype=bool), (len(dirs),)).copy()
        return self


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _room(cell=0.25):
    from depth_correction_amd.mesh import room_mesh
    m = room_mesh((3.0, 2.0, 1.5), cell)
    return m.vertices, m.faces.astype(np.int64)


_TIE = {}


def tie_mesh():
    """The room tessellated twice (0.25 m and 0.5 m cells: coplanar faces that overlap) with an exact duplicate of every face, the
    face order shuffled: every hit is a tie, and index order has nothing to do with Morton order."""
    if not _TIE:
        v1, f1 = _room(0.25)
        v2, f2 = _room(0.5)
        verts = np.concatenate([v1, v2])
        faces = np.concatenate([f1, f2 + len(v1)])
        faces = np.concatenate([faces, faces])
        faces = faces[np.random.default_rng(21).permutation(len(faces))]
        _TIE['m'] = (verts, faces, v1, f1)
    return _TIE['m']


TIE_SENSORS = ((0.0, 0.0, 0.0), (1e-3, -2e-3, 5e-4), (0.3, -0.7, 0.25))


def tie_targets(n=700, seed=22):
    """(targets [3 n, 3], aimed [3 n]): vertices, edge midpoints and interior points of the fine tessellation."""
    _, _, v, f = tie_mesh()
    rng = np.random.default_rng(seed)
    vi = rng.choice(len(v), size=n, replace=False)
    fe, fi = rng.choice(len(f), size=n, replace=False), rng.choice(len(f), size=n, replace=False)
    k = rng.integers(3, size=n)
    mid = 0.5 * (v[f[fe, k]] + v[f[fe, (k + 1) % 3]])
    inner = 0.5 * v[f[fi, 0]] + 0.3 * v[f[fi, 1]] + 0.2 * v[f[fi, 2]]
    return np.concatenate([v[vi], mid, inner]), np.arange(3 * n) < 2 * n


def case_ties(sensor, cull):
    verts, faces, _, _ = tie_mesh()
    x, aimed = tie_targets()
    o = np.asarray(TIE_SENSORS[sensor])
    return Case('ties-%d-%s' % (sensor, cull), verts, faces, cull).raycast(_unit(x - o), [o], 0.0, aimed)


def case_zero_components():
    """Identity pose at the origin of the room: the six axis directions and the rows of a lidar pattern that hold an exact 0."""
    from depth_correction_amd.render import lidar_directions
    verts, faces = _room()
    d, t_min = lidar_directions(size=(15, 64), fov=(60.0, 360.0), num_segments=8)
    d, t_min = np.asarray(d), np.asarray(t_min)
    zero = (d == 0).any(axis=1)
    assert zero.sum() >= 64
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    dirs = np.concatenate([axes, d[zero], d[~zero][::4]])
    tm = np.concatenate([np.zeros(6), t_min[zero], t_min[~zero][::4]])
    # from the origin the axes meet the walls at vertices and the rows with z = 0 run along the tessellation line z = 0; from the
    # second sensor only the axes along x and y meet a line (y = -0.5, x = 0.25)
    n_zero = 6 + int(zero.sum())
    aimed = np.stack([np.arange(len(dirs)) < n_zero, np.arange(len(dirs)) < 6])
    return Case('zero-components', verts, faces, True).raycast(dirs, [(0.0, 0.0, 0.0), (0.25, -0.5, 0.1)], tm, aimed)


def case_grazing(cull):
    """Axis-parallel rays that run exactly along tessellation lines (they meet the far wall at a vertex or on an edge) and rays
    that lie in a wall's plane, from view points inside and on the walls; identity pose at the origin."""
    verts, faces = _room()
    rng = np.random.default_rng(23)
    vps, dirs = [], []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        half = np.array([3.0, 2.0, 1.5])
        for _ in range(150):
            p = np.zeros(3)
            p[axis] = rng.integers(-4, 5) / 8.0
            p[u] = rng.integers(-int(half[u] * 4), int(half[u] * 4) + 1) / 4.0             # on a tessellation line, walls included
            p[v] = rng.integers(-int(half[v] * 4), int(half[v] * 4) + 1) / 4.0 if rng.integers(2) else rng.uniform(-half[v], half[v])
            for sign in (1.0, -1.0):
                vps.append(p)
                dirs.append(np.eye(3)[axis] * sign)
        for _ in range(60):                                                                  # in the plane of the wall axis = -half
            p = rng.uniform(-half, half) * 0.9
            p[axis] = -half[axis]
            dd = rng.normal(size=3)
            dd[axis] = 0.0
            vps.append(p)
            dirs.append(dd / np.linalg.norm(dd))
    n = len(dirs)
    return Case('grazing-%s' % cull, verts, faces, cull).rays(vps, dirs, [n], [(0.0, 0.0, 0.0)], 0.0, True)


FAR_OFFSETS = ((0.0, 0.0, 0.0), (1e3, 2e3, 50.0), (4e5, 5e6, 300.0))


def _grid20(x):
    """x rounded to multiples of 2^-20: sums with the offsets above are exact in fp64, so a translated scene is the same scene."""
    return np.round(np.asarray(x) * 2.0 ** 20) / 2.0 ** 20


def case_far(kind, offset):
    """The room or a 2000-face soup, with four sensors, translated by FAR_OFFSETS[offset] (exactly: all coordinates on a 2^-20
    grid)."""
    off = np.asarray(FAR_OFFSETS[offset])
    rng = np.random.default_rng(24)
    if kind == 'room':
        verts, faces = _room()
        sensors = _grid20(rng.uniform(-1.0, 1.0, size=(4, 3)) * [2.5, 1.5, 1.2])
        sensors[0] = 0.0
        x, aimed = tie_targets(300)
    else:
        c = rng.uniform(-20, 20, size=(2000, 1, 3))
        verts = _grid20((c + rng.normal(scale=1.5, size=(2000, 3, 3))).reshape(-1, 3))
        faces = np.arange(6000).reshape(-1, 3)
        sensors = _grid20(rng.uniform(-25, 25, size=(4, 3)))
        sensors[0] = 0.0
        tri = verts[faces[rng.choice(2000, size=900, replace=False)]]
        x, aimed = 0.5 * tri[:, 0] + 0.3 * tri[:, 1] + 0.2 * tri[:, 2], np.zeros(900, dtype=bool)
    dirs = np.concatenate([_unit(x - s) for s in sensors] + [_unit(rng.normal(size=(400, 3)))])
    counts = [len(x)] * 3 + [len(x) + 400]
    aimed = np.concatenate([np.tile(aimed, 4), np.zeros(400, dtype=bool)])
    case = Case('far-%s-%d' % (kind, offset), verts + off, faces, kind == 'room', center=tuple(off))
    assert np.array_equal(case.verts - off, verts)
    return case.rays(np.zeros((len(dirs), 3)), dirs, counts, sensors + off, 0.0, aimed)


SHAPES = ('one', 'two', 'three', 'centroid', 'flat', 'wide-box', 'degenerate')


def case_shape(shape):
    """Trees of unusual shape: 1, 2 or 3 faces, 512 faces with one centroid (identical Morton codes), a scene of no height, a scene
    box so wide that all faces but one share a Morton cell, and a room with faces of no area mixed in."""
    rng = np.random.default_rng(25)
    scene_box, cull = None, False
    if shape in ('one', 'two', 'three'):
        F = SHAPES.index(shape) + 1
        verts = (rng.uniform(-2, 2, size=(F, 1, 3)) + rng.normal(size=(F, 3, 3))).reshape(-1, 3)
        faces = np.arange(3 * F).reshape(-1, 3)
        sensors = rng.uniform(-6, 6, size=(3, 3))
    elif shape == 'centroid':
        ang = 2 * np.pi * np.arange(512) / 512
        base = np.array([[1.0, 0.0, 0.0], [-0.5, 0.75, 0.0], [-0.5, -0.75, 0.0]])
        rot = np.stack([np.stack([np.cos(ang), np.zeros(512), np.sin(ang)], 1), np.tile([0.0, 1.0, 0.0], (512, 1)),
                        np.stack([-np.sin(ang), np.zeros(512), np.cos(ang)], 1)], 1)              # about the y axis through the centroid
        verts = np.einsum('fij,kj->fki', rot, base).reshape(-1, 3) + np.array([0.5, 0.25, -0.125])
        faces = np.arange(3 * 512).reshape(-1, 3)
        sensors = np.array([[0.0, 0.0, 0.0], [3.0, 1.0, 2.0], [0.75, 4.0, 0.125]])
    elif shape == 'flat':
        g = np.arange(-6, 7) * 0.5
        gx, gy = np.meshgrid(g, g, indexing='ij')
        verts = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.75)], 1)
        idx = np.arange(gx.size).reshape(gx.shape)
        q00, q10, q01, q11 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
        faces = np.concatenate([np.stack([q00, q10, q11], 1), np.stack([q00, q11, q01], 1)])
        sensors = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 2.0], [1.0, 1.0, -3.0]])
    elif shape == 'wide-box':
        c = rng.uniform(-2, 2, size=(599, 1, 3))
        verts = np.concatenate([(c + rng.normal(scale=0.3, size=(599, 3, 3))).reshape(-1, 3),
                                np.array([[3000.0, 0, 0], [3000.0, 1, 0], [3000.0, 0, 1]])])
        faces = np.arange(1800).reshape(-1, 3)
        scene_box = (-5000.0, -5000.0, -5000.0, 5000.0, 5000.0, 5000.0)
        sensors = np.array([[0.0, 0.0, 0.0], [2990.0, 0.3, 0.3], [-4.0, 3.0, 1.0]])
    else:
        verts, faces = _room()
        k = rng.choice(len(faces), size=300, replace=False)
        rep = faces[k].copy()
        rep[:, 2] = rep[:, 1]                                                              # a repeated vertex
        line = np.array([[i, i + 1, i + 2] for i in rng.choice(len(verts) - 2, size=300, replace=False)])
        line = line[np.linalg.norm(np.cross(verts[line[:, 1]] - verts[line[:, 0]], verts[line[:, 2]] - verts[line[:, 0]]), axis=1) == 0]
        assert len(line) >= 100                                                            # three collinear vertices of a wall
        faces = np.concatenate([faces, rep, line, faces[k][:, [0, 0, 0]]])
        faces = faces[rng.permutation(len(faces))]
        sensors, cull = np.array([[0.0, 0.0, 0.0], [0.3, -0.7, 0.25], [-1.1, 0.4, -0.6]]), True
    tri = verts[faces]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = rng.choice(np.nonzero(area > 0)[0], size=400)
    w = rng.dirichlet(np.ones(3), size=400) * 0.85 + 0.05
    x = np.einsum('nk,nkc->nc', w, tri[pick])
    vert_x = tri[pick[:100], rng.integers(3, size=100)]
    dirs = np.concatenate([_unit(np.concatenate([x, vert_x]) - s) for s in sensors] + [_unit(rng.normal(size=(200, 3)))])
    counts = [500, 500, 700]
    aimed = np.concatenate([np.tile(np.arange(500) >= 400, 3), np.zeros(200, dtype=bool)])
    case = Case('shape-%s' % shape, verts, faces, cull, scene_box=scene_box)
    return case.rays(np.zeros((len(dirs), 3)), dirs, counts, sensors, 0.0, aimed)


def case_stack(n=64):
    """``n`` faces of different shape in ONE plane (z = 2), all around the point below the sensor, the face order shuffled: a ray at
    the middle enters every box at the same distance and hits every face at the same t up to rounding, so nothing is pruned and a
    walk postpones one node per level.  Rays at the middle, at the rim (some faces only) and past every face."""
    rng = np.random.default_rng(27)
    k = 1.0 + rng.permutation(n)[:, None] * 2.0 ** -6
    verts = np.stack([np.concatenate([-k, -k, np.full((n, 1), 2.0)], 1), np.concatenate([k, -k, np.full((n, 1), 2.0)], 1),
                      np.concatenate([0 * k, k, np.full((n, 1), 2.0)], 1)], 1).reshape(-1, 3)
    x = np.concatenate([rng.uniform(-0.3, 0.3, size=(120, 2)), rng.uniform(-2.2, 2.2, size=(120, 2))])
    x = np.concatenate([x, np.full((len(x), 1), 2.0)], 1)
    o = np.array([0.125, -0.25, 4.0])
    case = Case('stack-%d' % n, verts, np.arange(3 * n).reshape(-1, 3), True)
    return case.rays(np.zeros((len(x), 3)), _unit(x - o), [len(x)], [o], 0.0, False)


def leaf_arrays(lib, case, order):
    """(leaf_tri f64 [n,9], leaf_face i32 [n], leaf boxes f32 [n,6]) of ``case`` with the faces ``order`` at the leaves 0 .. n-1."""
    from helpers import host_ray_boxes
    tri = np.ascontiguousarray(np.asarray(case.verts, dtype=np.float64)[case.faces[order]].reshape(-1, 9))
    return tri, np.asarray(order, dtype=np.int32), host_ray_boxes(lib, tri)


def all_cases():
    """Every case whose rays go to the classifier: (id, constructor)."""
    out = [('ties-%d-%s' % (s, c), lambda s=s, c=c: case_ties(s, c)) for s in range(3) for c in (True, False)]
    out.append(('zero-components', case_zero_components))
    out += [('grazing-%s' % c, lambda c=c: case_grazing(c)) for c in (True, False)]
    out += [('far-%s-%d' % (k, i), lambda k=k, i=i: case_far(k, i)) for k in ('room', 'soup') for i in range(3)]
    out += [('shape-%s' % s, lambda s=s: case_shape(s)) for s in SHAPES]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def verify(lib, case, face, t, u=None, v=None, cap=0.01):
    """Assert that (face, t, u, v) [R] of ``case`` equal the oracle bit for bit, agree with the classifier on its clear rays (the face
    on the winning surface, t to 1e-12 relative, misses missed), and that at most ``cap`` of the rays not aimed at an edge or a
    vertex are borderline.  Returns (oracle outputs, Classified)."""
    of, ot, ou, ov = oracle(lib, case.verts, case.faces, case.o, case.d, case.t_min, case.cull)
    face, t = np.asarray(face).reshape(-1), np.asarray(t).reshape(-1)
    bad = np.nonzero((face != of) | (_bits(t) != _bits(ot)))[0]
    print('%s: %d rays, %d hits, %d differ from the oracle' % (case.name, len(of), (of >= 0).sum(), len(bad)))
    assert len(bad) == 0, (case.name, len(bad), bad[:8], face[bad[:8]], of[bad[:8]], t[bad[:8]], ot[bad[:8]])
    if u is not None:
        assert np.array_equal(_bits(np.asarray(u).reshape(-1)), _bits(ou)) and np.array_equal(_bits(np.asarray(v).reshape(-1)), _bits(ov))
    cl = classify(case.verts, case.faces, case.o, case.d, case.t_min, case.cull, center=case.center, got_face=face)
    clear, hit = cl.status != BORDERLINE, cl.status == HIT
    free = ~case.aimed
    share = float((cl.status[free] == BORDERLINE).mean()) if free.any() else 0.0
    print('%s: classifier %d hits, %d misses, %d borderline; %.4f of the %d rays not aimed at an edge are borderline'
          % (case.name, hit.sum(), (cl.status == MISS).sum(), (~clear).sum(), share, free.sum()))
    assert cl.got_ok[clear].all(), (case.name, np.nonzero(clear & ~cl.got_ok)[0][:8])
    assert np.isinf(t[cl.status == MISS]).all()
    if hit.any():
        assert np.abs(t[hit] / cl.t[hit] - 1.0).max() <= 1e-12, case.name
    assert share <= cap, (case.name, share)
    return (of, ot, ou, ov), cl
