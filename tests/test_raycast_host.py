"""The ray caster's per-ray arithmetic on the host (no GPU): csrc/dc_raymath.h through its host build (libdc_hostcheck.so, the header
the kernels include).  test_triangle against exact rational arithmetic, the box test's conservativeness under the traversal's
pruning rule on a million (ray, face) pairs, the directed roundings of the leaf boxes, and the independent classifier of
raycast_reference.py against the oracle on the scenes the GPU tests use."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import raycast_reference as RR
from helpers import host_ray_box_entry, host_ray_boxes, host_ray_prune_far, host_ray_test_pairs, raycast_host_lib

EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def host():
    return raycast_host_lib()


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------------
def _fr(x):
    return [Fraction(float(c)) for c in x]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def exact_hit(tri, o, d):
    """Exact (t, (w0, w1, w2), n . d, cond) of the ray's crossing of the triangle's plane, None when the ray is parallel to it or
    the triangle has no area.  cond = L^2 / |det| and zs = max |z_i - t| / t in the frame of the watertight test (see
    test_triangle_against_exact_arithmetic)."""
    a, b, c, o, d = _fr(tri[0:3]), _fr(tri[3:6]), _fr(tri[6:9]), _fr(o), _fr(d)
    e1, e2 = _sub(b, a), _sub(c, a)
    n = _cross(e1, e2)
    dn = _dot(d, n)
    if dn == 0:
        return None
    t = _dot(_sub(a, o), n) / dn
    p = [oo + t * dd for oo, dd in zip(o, d)]
    nn = _dot(n, n)
    w1 = _dot(_cross(_sub(p, a), e2), n) / nn
    w2 = _dot(_cross(e1, _sub(p, a)), n) / nn
    kz = int(np.argmax([abs(float(x)) for x in d]))
    det = abs(dn / d[kz])                                    # U + V + W of the sheared triangle, exactly
    L = max(abs(x) for v in (a, b, c) for x in _sub(v, o))
    zs = max(abs((v[kz] - o[kz]) / d[kz] - t) for v in (a, b, c))
    return t, (1 - w1 - w2, w1, w2), dn, float(L * L / det), float(zs / abs(t)) if t != 0 else float('inf')


def _pairs(rng, n, dyadic):
    """n (triangle [9], origin, direction, kind) with the ray aimed at a vertex, an edge point, an interior or an outside point, or at
    the interior of an axis-aligned wall met face-on."""
    out = []
    for i in range(n):
        if dyadic:
            tri = rng.integers(-64, 65, size=9) / 8.0
            o = rng.integers(-64, 65, size=3) / 8.0
        else:
            tri = rng.uniform(-10, 10, size=9)
            o = rng.uniform(-10, 10, size=3)
        a, b, c = tri[0:3], tri[3:6], tri[6:9]
        kind = i % 5
        if kind == 4:                                             # a wall met along its normal's axis: every z_i equal, K = 0
            k = rng.integers(3)
            tri[k::3] = tri[k]
            w = np.array([0.25, 0.25, 0.5]) if dyadic else rng.dirichlet(np.ones(3)) * 0.85 + 0.05
            x = w[0] * a + w[1] * b + w[2] * c
            delta = rng.integers(-24, 25, size=3) / 8.0 if dyadic else rng.uniform(-3, 3, size=3)
            delta[k] = (rng.integers(32, 65) / 8.0 if dyadic else rng.uniform(4, 8)) * (1 if rng.integers(2) else -1)
            o = x - delta
        elif kind == 0:
            x = (a, b, c)[rng.integers(3)]
        elif kind == 1:
            p, q = ((a, b), (b, c), (c, a))[rng.integers(3)]
            x = p + (q - p) * (rng.integers(1, 8) / 8.0)
        elif kind == 2:
            w = rng.integers(1, 7, size=3) if dyadic else rng.uniform(0.05, 1.0, size=3)
            w = w / (8.0 if dyadic else w.sum())
            if dyadic:
                w[0] = 1.0 - w[1] - w[2]
            x = w[0] * a + w[1] * b + w[2] * c
        else:
            w = np.array([-0.25, 0.5, 0.75]) if dyadic else np.append(-rng.uniform(0.05, 1.0), rng.uniform(0.5, 1.0, size=2))
            w = rng.permutation(w / w.sum())
            x = w[0] * a + w[1] * b + w[2] * c
        d = x - o
        if not dyadic:
            d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        out.append((tri, o, d, kind))
    return out


@pytest.mark.parametrize('cull', [False, True])
def test_triangle_against_exact_arithmetic(host, cull):
    """Where exact arithmetic puts the crossing strictly inside or strictly outside by more than the rounding test_triangle itself
    carries, it agrees; t is within (6 + 108 K) 2^-52 relative.

    The bound.  With u = 2^-53 and L the largest |vertex - origin| coordinate, a sheared coordinate (a_x - o_x) - s_x A_z carries
    at most 7 u L (the two differences, the two roundings of s_x = d_x (1 / d_z), the product, the last difference); an edge
    function is a difference of two products of numbers up to 2 L, so it carries at most 72 u L^2 = 36 2^-52 L^2, and a weight
    U / det at most 36 2^-52 L^2 / det plus det's own share: 64 2^-52 cond with cond = L^2 / det is the margin below which hit or
    miss is not decided.  t = sum U_i z_i / det moves by sum dU_i (z_i - t) / det <= 3 * 36 2^-52 cond max |z_i - t|, and its own
    three products, two sums and division add 6 2^-52 t: relative (6 + 108 K) 2^-52 with K = cond max |z_i - t| / t.  For a face
    seen face-on from a few of its sizes away K is below 0.05 and the bound is 12 ulp; the test asserts that such pairs exist."""
    rng = np.random.default_rng(11)
    pairs = _pairs(rng, 2000, True) + _pairs(rng, 2000, False)
    tri = np.array([p[0] for p in pairs])
    o = np.array([p[1] for p in pairs])
    d = np.array([p[2] for p in pairs])
    hit, t, u, v = host_ray_test_pairs(host, tri, o, d, 0.0, cull)
    decided = well = worst = 0
    for i, (tr, oo, dd, kind) in enumerate(pairs):
        ex = exact_hit(tr, oo, dd)
        if ex is None:
            assert not hit[i]                            # exactly edge-on, or no area: det is exactly 0 on dyadic input
            continue
        te, w, dn, cond, zs = ex
        margin = 64 * EPS * cond
        if margin > 2.0 ** -10:
            continue
        facing = dn < 0 or not cull
        inside = min(w) > margin and te > 0 and facing
        outside = min(w) < -margin or te < 0 or (cull and dn > 0)
        if inside or outside:
            decided += 1
            assert bool(hit[i]) == inside, (i, kind, w, float(te))
        if hit[i]:
            K = cond * zs
            err = abs(Fraction(float(t[i])) - te) / abs(te)
            assert err <= (6 + 108 * K) * EPS, (i, float(err) / EPS, K)
            worst = max(worst, float(err) / EPS)
            well += K < 0.05
            wb = (1 - Fraction(float(u[i])) - Fraction(float(v[i])), Fraction(float(u[i])), Fraction(float(v[i])))
            assert max(abs(float(x - y)) for x, y in zip(wb, w)) <= margin + 4 * EPS
    print('cull=%s: %d of %d pairs decided, %d hits with K < 0.05, worst t error %.2f ulp' % (cull, decided, len(pairs), well, worst))
    kinds = np.array([p[3] for p in pairs])
    assert decided >= 0.95 * (kinds >= 2).sum() and well >= 300


def _fan(rng, dyadic, k=5):
    """k triangles around a shared centre (a closed umbrella), two of them also sharing each spoke; the ray origin above it."""
    if dyadic:
        c = rng.integers(-32, 33, size=3) / 8.0
        ring = [c + np.array([np.round(8 * 2 * np.cos(2 * np.pi * j / k)) / 8, np.round(8 * 2 * np.sin(2 * np.pi * j / k)) / 8,
                              rng.integers(-4, 5) / 8.0]) for j in range(k)]
        o = c + np.array([rng.integers(-2, 3) / 8.0, rng.integers(-2, 3) / 8.0, rng.integers(8, 40) / 8.0 * (1 if rng.integers(2) else -1)])
    else:
        c = rng.uniform(-10, 10, size=3)
        ring = [c + np.array([2 * np.cos(2 * np.pi * j / k + 0.1), 2 * np.sin(2 * np.pi * j / k + 0.1), rng.uniform(-0.5, 0.5)])
                for j in range(k)]
        o = c + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(1, 5) * (1 if rng.integers(2) else -1)])
    perm = rng.permutation(3)                                 # any axis may be the dominant one
    c, o, ring = c[perm], o[perm], [r[perm] for r in ring]
    tris = np.array([np.concatenate([c, ring[j], ring[(j + 1) % k]]) for j in range(k)])
    return c, ring, o, tris


def test_watertight_on_exact_edges_and_vertices(host):
    """A ray exactly through a shared vertex or a point of a shared edge (dyadic: the direction is exact; generic: it is rounded and
    the ray passes within an ulp) hits at least one of the faces around it, with and without culling the far side."""
    rng = np.random.default_rng(12)
    n_rays = 0
    for trial in range(600):
        c, ring, o, tris = _fan(rng, dyadic=trial % 2 == 0)
        targets = [c] + [c + (r - c) * (rng.integers(1, 8) / 8.0) for r in ring]
        for x in targets:
            d = x - o
            for scale in (1.0, 1.0 / np.linalg.norm(d)):
                dd = d * scale
                hit, t, _, _ = host_ray_test_pairs(host, tris, np.tile(o, (len(tris), 1)), np.tile(dd, (len(tris), 1)), 0.0, False)
                assert hit.any(), (trial, x)
                n_rays += 1
                # culling keeps the hit when the umbrella is wound towards the ray, and drops every face when it is wound away
                nrm = np.cross(tris[:, 3:6] - tris[:, 0:3], tris[:, 6:9] - tris[:, 0:3])
                front = nrm @ dd < 0
                hc, _, _, _ = host_ray_test_pairs(host, tris, np.tile(o, (len(tris), 1)), np.tile(dd, (len(tris), 1)), 0.0, True)
                assert not (hc & ~front).any()
                if front.all():
                    assert hc.any()
    assert n_rays >= 7000


def test_edge_on_zero_area_and_t_min(host):
    """Dyadic geometry, exact in fp64: an edge-on ray misses, faces of no area miss, and t == t_min misses while the next number
    below it hits."""
    wall = np.array([2.0, -1.0, -1.0, 2.0, 1.0, -1.0, 2.0, 0.0, 1.0])               # in the plane x = 2, normal +x
    o, d = np.zeros(3), np.array([1.0, 0.0, 0.0])
    for cull in (False, True):
        hit, t, u, v = host_ray_test_pairs(host, wall[None], o[None], d[None], 0.0, cull)
        assert bool(hit[0]) == (not cull)                                             # its back faces the ray
    flipped = np.concatenate([wall[0:3], wall[6:9], wall[3:6]])
    for cull in (False, True):
        hit, t, u, v = host_ray_test_pairs(host, flipped[None], o[None], d[None], 0.0, cull)
        assert hit[0] and t[0] == 2.0 and u[0] == 0.5 and v[0] == 0.25
        hit, _, _, _ = host_ray_test_pairs(host, flipped[None], o[None], d[None], 2.0, cull)
        assert not hit[0]                                                             # t == t_min
        hit, t, _, _ = host_ray_test_pairs(host, flipped[None], o[None], d[None], np.nextafter(2.0, 0.0), cull)
        assert hit[0] and t[0] == 2.0
        hit, _, _, _ = host_ray_test_pairs(host, flipped[None], o[None], -d[None], -10.0, cull)
        assert hit[0] == (not cull)                                                   # behind the origin: t = -2 > t_min = -10
        # in the wall's plane, along it and across it
        for dd in ([0.0, 1.0, 0.0], [0.0, 0.5, 1.0], [0.0, -1.0, 0.25]):
            hit, _, _, _ = host_ray_test_pairs(host, flipped[None], np.array([[2.0, -3.0, 0.0]]), np.array([dd]), 0.0, cull)
            assert not hit[0]
        # no area: a repeated vertex, three collinear vertices, one point
        for deg in ([2, -1, -1, 2, -1, -1, 2, 0, 1], [2, -1, -1, 2, 0, 0, 2, 1, 1], [2, 0, 0, 2, 0, 0, 2, 0, 0]):
            for dd in ([1.0, 0.0, 0.0], [2.0, -1.0, -1.0], [1.0, -0.25, -0.25]):
                hit, _, _, _ = host_ray_test_pairs(host, np.array([deg], dtype=np.float64), o[None], np.array([dd]), 0.0, cull)
                assert not hit[0]
        # a zero direction never hits
        hit, _, _, _ = host_ray_test_pairs(host, flipped[None], o[None], np.zeros((1, 3)), 0.0, cull)
        assert not hit[0]


def test_leaf_boxes_round_outward(host):
    rng = np.random.default_rng(13)
    tri = np.concatenate([rng.uniform(-50, 50, size=(2000, 9)), rng.uniform(-50, 50, size=(2000, 9)) + np.tile([4e5, 5e6, 300.0], 3),
                          rng.integers(-64, 65, size=(2000, 9)) / 8.0, rng.normal(size=(2000, 9)) * 1e-30, np.zeros((1, 9))])
    box = host_ray_boxes(host, tri)
    v = tri.reshape(-1, 3, 3)
    lo, hi = v.min(axis=1), v.max(axis=1)
    b = box.astype(np.float64)
    assert (b[:, :3] <= lo).all() and (b[:, 3:] >= hi).all()
    # the tightest fp32 numbers: the next one inward is strictly inside the fp64 bound
    assert (np.nextafter(box[:, :3], np.float32(np.inf)).astype(np.float64) > lo).all()
    assert (np.nextafter(box[:, 3:], np.float32(-np.inf)).astype(np.float64) < hi).all()
    exact = lo.astype(np.float32).astype(np.float64) == lo
    assert exact[4000:6000].all() and (b[:, :3][exact] == lo[exact]).all()          # representable bounds stay: flat boxes stay flat


# ---- conservativeness of the box test ------------------------------------------------------------------------------------------------
OFFSETS = ((0.0, 0.0, 0.0), (1e3, 2e3, 50.0), (4e5, 5e6, 300.0))
SENSORS = ('origin', '1e-3', '0.1', 'generic')
FACES = ('generic', 'flat', 'tiny')
TARGETS = ('vertex', 'edge', 'interior')
RAYS = ('generic', 'axis', 'near-axis')


def conservativeness_pairs(rng, n, target, faces, offset, sensor, rays):
    """n (triangle, origin, direction): the face's feature ``target`` lies on the ray."""
    offset = np.asarray(offset)
    shape = rng.normal(scale=0.7, size=(n, 3, 3))
    if faces == 'tiny':
        shape *= 1e-3
    flat_axis = rng.integers(3, size=n)
    if faces == 'flat':
        shape[np.arange(n), :, flat_axis] = 0.0
    if target == 'vertex':
        w = np.eye(3)[rng.integers(3, size=n)]
    elif target == 'edge':
        w = np.zeros((n, 3))
        s, k = rng.uniform(0.05, 0.95, size=n), rng.integers(3, size=n)
        w[np.arange(n), k], w[np.arange(n), (k + 1) % 3] = s, 1.0 - s
    else:
        w = rng.uniform(0.05, 1.0, size=(n, 3))
        w /= w.sum(axis=1, keepdims=True)
    feature = np.einsum('nk,nkc->nc', w, shape)
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    local = {'origin': np.zeros((n, 3)), '1e-3': 1e-3 * unit, '0.1': 0.1 * unit, 'generic': rng.uniform(-25, 25, size=(n, 3))}[sensor]
    o = offset + local
    if rays in ('axis', 'near-axis'):
        axis = flat_axis if faces == 'flat' else rng.integers(3, size=n)               # a flat face is met face-on
        d = np.eye(3)[axis] * rng.choice([-1.0, 1.0], size=(n, 1))
        if rays == 'near-axis':                                                          # the cosines of a computed right angle
            d = d + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-24, -12, size=(n, 1))
        x = o + d * rng.uniform(0.5, 40.0, size=(n, 1))
    else:
        x = offset + rng.uniform(-25, 25, size=(n, 3))
        if faces == 'flat':                                                              # walls: world-aligned planes at round places
            x[np.arange(n), flat_axis] = offset[flat_axis] + rng.integers(-100, 101, size=n) / 4.0
        d = x - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    tri = (x - feature)[:, None, :] + shape
    return tri.reshape(n, 9), o, d


def count_pruned_hits(host, n_per=5000, seed=14):
    """Over every combination of the generators: the hits of test_triangle (at t) and how many of them box_entry rejects -- the
    face's leaf box and an enclosing box, with t_far = prune_far(t) and with t_far = +inf."""
    rng = np.random.default_rng(seed)
    names = ('leaf, prune', 'enclosing, prune', 'leaf, inf', 'enclosing, inf')
    total, hits, bad, rows = 0, 0, dict.fromkeys(names, 0), []
    for cfg in itertools.product(TARGETS, FACES, OFFSETS, SENSORS, RAYS):
        tri, o, d = conservativeness_pairs(rng, n_per, *cfg)
        hit, t, _, _ = host_ray_test_pairs(host, tri, o, d, 0.0, False)
        leaf = host_ray_boxes(host, tri)
        other = np.roll(leaf, 1, axis=0)
        both = np.concatenate([np.minimum(leaf[:, :3], other[:, :3]), np.maximum(leaf[:, 3:], other[:, 3:])], axis=1)
        far = host_ray_prune_far(host, t)
        row = []
        for name, box, t_far in zip(names, (leaf, both, leaf, both), (far, far, np.inf, np.inf)):
            tn = host_ray_box_entry(host, o, d, box, t_far)
            k = int((hit & ~np.isfinite(tn)).sum())
            bad[name] += k
            row.append(k)
        total += n_per
        hits += int(hit.sum())
        if any(row):
            rows.append((cfg, int(hit.sum()), row))
    return total, hits, bad, rows


def test_box_test_is_conservative(host):
    """Whenever test_triangle reports a hit at t, box_entry keeps the face's leaf box and every box around it, both under the
    traversal's pruning rule (t_far = prune_far(t)) and before any hit (t_far = +inf): zero rejections in 1.62 million pairs aimed at
    vertices, edge points and interior points of generic, axis-aligned flat and millimetre-sized faces, in scenes at the origin and
    at UTM-sized offsets, from a sensor exactly at the scene origin, 1e-3 and 0.1 from it and anywhere, along generic,
    axis-parallel and nearly axis-parallel rays.  Before prune_far had its slack (t_far = ru(t)) and before the floors of the zero
    direction component and of the margin were 1e-30 and 1e-20 (they were 1e-20 and 1e-30), this test counted 9971 rejected leaf
    boxes and 942 enclosing boxes under the pruning rule (1588 of the leaf boxes on generic rays from a sensor at, 1e-3 from or 0.1 from the origin: the
    missing slack), and 8383 / 541 with t_far = +inf: the latter all from axis-parallel or nearly axis-parallel rays out of the
    exact origin towards a vertex on the axis."""
    total, hits, bad, rows = count_pruned_hits(host)
    print('%d pairs, %d hits, rejected: %s' % (total, hits, bad))
    for cfg, h, row in rows:
        print('  %s: %d hits, rejected %s' % (cfg, h, row))
    assert total >= 1000000 and hits >= 0.4 * total
    assert all(k == 0 for k in bad.values()), bad


# ---- the scenes of the GPU tests: the oracle against the independent classifier ---------------------------------------------------------
@pytest.mark.parametrize('name,make', RR.all_cases(), ids=[c[0] for c in RR.all_cases()])
def test_oracle_agrees_with_classifier(host, name, make):
    """On every scene of tests/test_gpu_raycast_edge.py the oracle's own answer passes the checks the device's answer has to pass:
    the classifier's clear rays agree, and the borderline share of the rays not aimed at an edge or a vertex stays within 1 %."""
    case = make()
    assert case.name == name
    face, t, u, v = RR.oracle(host, case.verts, case.faces, case.o, case.d, case.t_min, case.cull)
    (_, _, _, _), cl = RR.verify(host, case, face, t, u, v)
    free = ~case.aimed
    if free.sum() >= 100:
        assert (cl.status[free] == RR.HIT).sum() >= 0.2 * free.sum()                   # the comparison has something to compare
