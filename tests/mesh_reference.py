"""Reference for the map-accuracy tests (tests/test_meshdist_host.py, tests/test_gpu_meshdist.py): numpy fp64, no call into
the package.

``closest_on_triangles`` is written differently from the kernel's Voronoi-region method on purpose: the closest point is the
foot of the perpendicular on the plane when that foot lies inside the triangle (three edge-function signs), else the nearest of
the three point-segment answers.  ``brute_force`` runs it over every (point, face) pair in chunks.  ``sample`` restates
dc_mesh_sample's formula.  tests/test_meshdist_host.py holds this module to analytic cases before anything is held to it.
"""
import numpy as np


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _segment(p, a, b):
    """(d2, closest) of the segments [a, b] to p, broadcasting over leading axes."""
    e = b - a
    ee = _dot(e, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(ee > 0, _dot(p - a, e) / np.where(ee > 0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    q = a + t[..., None] * e
    r = p - q
    return _dot(r, r), q


def closest_on_triangles(p, a, b, c):
    """(d2, closest point) from p [...,3] to the triangles (a, b, c) [...,3] (broadcast against each other)."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (p, a, b, c)))
    d2, q = _segment(p, a, b)
    for u, v in ((b, c), (c, a)):
        d, r = _segment(p, u, v)
        better = d < d2
        d2 = np.where(better, d, d2)
        q = np.where(better[..., None], r, q)
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    inside = nn > 0
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= _dot(np.cross(v - u, p - u), n) >= 0
    with np.errstate(divide='ignore', invalid='ignore'):
        t = _dot(p - a, n) / np.where(nn > 0, nn, 1.0)
    foot = p - t[..., None] * n
    r = p - foot
    dpl = _dot(r, r)
    use = inside & (dpl <= d2)
    return np.where(use, dpl, d2), np.where(use[..., None], foot, q)


def all_distances(verts, faces, points):
    """Distances [N,F] from every point to every face (small N: the rows a test looks at one by one)."""
    verts, faces, points = np.asarray(verts, np.float64), np.asarray(faces, np.int64), np.asarray(points, np.float64)
    a, b, c = (verts[faces[:, k]][None] for k in range(3))
    return np.sqrt(closest_on_triangles(points[:, None, :], a, b, c)[0])


def brute_force(verts, faces, points, chunk=64):
    """For every point the best face (the lowest index among exactly equal d2), the best and the second-best DISTANCE over all
    faces of the mesh: (face int64 [N], dist [N], second [N]); second is inf for a one-face mesh."""
    verts, faces, points = np.asarray(verts, np.float64), np.asarray(faces, np.int64), np.asarray(points, np.float64)
    a, b, c = (verts[faces[:, k]][None] for k in range(3))
    n = points.shape[0]
    face = np.zeros(n, dtype=np.int64)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    for s in range(0, n, chunk):
        d2, _ = closest_on_triangles(points[s:s + chunk, None, :], a, b, c)
        f = np.argmin(d2, axis=1)                       # the first of equal minima: the lowest index
        rows = np.arange(d2.shape[0])
        face[s:s + chunk] = f
        best[s:s + chunk] = np.sqrt(d2[rows, f])
        if d2.shape[1] > 1:
            d2[rows, f] = np.inf
            second[s:s + chunk] = np.sqrt(d2.min(axis=1))
    return face, best, second


def distance_to_faces(verts, faces, points, face):
    """(distance, closest point) from points [N,3] to the faces ``face`` [N] of the mesh, row by row."""
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    d2, q = closest_on_triangles(points, tri[:, 0], tri[:, 1], tri[:, 2])
    return np.sqrt(d2), q


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_uniforms(seed, i):
    """u [len(i), 3]: u_t = (splitmix64(splitmix64(seed) + 4 i + t) >> 11) 2^-53."""
    i = np.asarray(i, dtype=np.int64).astype(np.uint64)
    with np.errstate(over='ignore'):
        base = splitmix64(np.array([np.int64(seed)]).astype(np.uint64))[0] + np.uint64(4) * i
        return np.stack([(splitmix64(base + np.uint64(t)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for t in range(3)], axis=1)


def sample_faces(area_cdf, u0):
    """The first face f with u0 total < area_cdf[f]; past the end, the last face that added area."""
    cdf = np.asarray(area_cdf, dtype=np.float64)
    f = np.searchsorted(cdf, u0 * cdf[-1], side='right')
    last = int(np.searchsorted(cdf, cdf[-1], side='left'))
    return np.where(f >= len(cdf), last, f).astype(np.int64)


def sample_points(tri, u1, u2):
    """((1 - s) v0 + s (1 - u2) v1) + s u2 v2 with s = sqrt(u1), tri [N,3,3]."""
    s = np.sqrt(u1)
    w0, w1, w2 = 1.0 - s, s * (1.0 - u2), s * u2
    return (w0[:, None] * tri[:, 0] + w1[:, None] * tri[:, 1]) + w2[:, None] * tri[:, 2]


def sample(verts, faces, n, seed):
    """(points [n,3], face int64 [n]) of dc_mesh_sample; the prefix sum of the areas as TriangleMesh.area_cdf makes it."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    v = verts[faces]
    cdf = np.cumsum(0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1))
    u = sample_uniforms(seed, np.arange(n))
    f = sample_faces(cdf, u[:, 0])
    return sample_points(v[f], u[:, 1], u[:, 2]), f
