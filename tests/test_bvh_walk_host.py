"""The one tree walk (csrc/dc_bvh.h: bvh_walk) on the host build, with the kernels' own visitors (dc_host_ray_cast_walk,
dc_host_surfel_cast_walk), over trees of chosen shape from raycast_reference.build_tree: the walk returns what the brute force over
every primitive returns, bit for bit, whatever the tree -- a root that is a leaf, two and three leaves, a mesh where every hit is a
tie in a balanced tree and in a comb, and a comb of the greatest depth a tree may have (63), which a ray at the middle of
case_stack descends with one postponed node per level.  No GPU."""
import numpy as np
import pytest

import raycast_reference as R
import surfel_reference as S
from helpers import host_ray_cast_walk


@pytest.fixture(scope='module')
def lib():
    return S.surfel_host_lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, ref, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g), np.asarray(r)
        same = np.array_equal(_bits(g), _bits(r)) if g.dtype == np.float64 else np.array_equal(g, r)
        assert same, (what, k, np.nonzero((g != r) & ~(np.isnan(g) & np.isnan(r)))[0][:8])


def tri_trees(lib, case):
    """name -> (child, node_box, leaf_tri, leaf_face, depth, parent): two trees of different shape over different leaf orders."""
    n = len(case.faces)
    centre = np.asarray(case.verts)[case.faces].mean(axis=1)
    orders = dict(balanced=np.lexsort(centre.T[::-1]), comb=np.random.default_rng(31).permutation(n))
    out = {}
    for name, order in orders.items():
        tri, ids, boxes = R.leaf_arrays(lib, case, order)
        comb = 0 if name == 'balanced' else (n - 1 if n - 1 <= R.MAX_DEPTH else R.MAX_DEPTH - int(np.ceil(np.log2(n))))
        child, parent, box, depth = R.build_tree(boxes, comb=comb)
        out[name] = (child, box, tri, ids, depth, parent)
    return out


TRI_CASES = dict(one=lambda: R.case_shape('one'), two=lambda: R.case_shape('two'), three=lambda: R.case_shape('three'),
                 ties=lambda: R.case_ties(2, True), stack=R.case_stack)


@pytest.mark.parametrize('name', sorted(TRI_CASES))
def test_triangle_walk_is_the_brute_force_in_every_tree(lib, name):
    case = TRI_CASES[name]()
    ref = R.oracle(lib, case.verts, case.faces, case.o, case.d, case.t_min, case.cull)
    assert (ref[0] >= 0).sum() >= 0.4 * len(ref[0]) and (name in ('ties',) or (ref[0] < 0).any())
    trees = tri_trees(lib, case)
    for shape, (child, box, tri, ids, depth, _) in trees.items():
        got = host_ray_cast_walk(lib, child, box, tri, ids, case.o, case.d, case.t_min, case.cull)
        print('%s / %s: %d faces, depth %d, %d rays, %d hits' % (name, shape, len(ids), depth, len(got[0]), (got[0] >= 0).sum()))
        _same(got, ref, (name, shape))
    if name in ('ties', 'stack'):
        assert trees['comb'][4] > 50 and trees['balanced'][4] < 16
    if name == 'stack':                        # depth 63 exactly; the first 120 rays meet every face, at t equal up to rounding
        assert trees['comb'][4] == R.MAX_DEPTH and (ref[0][:120] >= 0).all() and len(set(ref[0])) > 10


def _disk_scene(kind):
    """(points, normals, radii, o, d): a survey of 1 or 3 disks, or 64 disks in one plane below the sensor (case_stack's idea)."""
    rng = np.random.default_rng(33)
    if kind == 'stack':
        n = 64
        pts = np.concatenate([rng.uniform(-0.125, 0.125, size=(n, 2)), np.full((n, 1), 2.0)], 1)
        nrm = np.array([0.0, 0.0, 1.0]) * (rng.choice([-1.0, 1.0], size=n) * rng.choice([0.5, 1.0, 2.0], size=n))[:, None]
        rho = 1.0 + rng.permutation(n) * 2.0 ** -6
        x = np.concatenate([rng.uniform(-0.5, 0.5, size=(120, 2)), rng.uniform(-2.5, 2.5, size=(120, 2))])
        o = np.tile([0.125, -0.25, 4.0], (len(x), 1))
        return pts, nrm, rho, o, R._unit(np.concatenate([x, np.full((len(x), 1), 2.0)], 1) - o)
    n = dict(one=1, three=3)[kind]
    pts, nrm, rho = S.room_survey(seed=34, m=n)
    o = rng.uniform(-0.5, 0.5, size=(300, 3))
    target = pts[rng.integers(n, size=300)] + rng.normal(scale=0.15, size=(300, 3))
    return pts, nrm, rho, o, R._unit(target - o)


def disk_trees(lib, pts, nrm, rho):
    n = len(pts)
    out = {}
    for name, order in dict(balanced=np.lexsort(pts.T[::-1]), comb=np.random.default_rng(35).permutation(n)).items():
        child, parent, box, depth = R.build_tree(S.host_boxes(lib, pts[order], nrm[order], rho[order]), comb=0 if name == 'balanced' else n - 1)
        out[name] = (child, box, S.disk_rows(pts[order], nrm[order], rho[order]), order.astype(np.int32), depth, parent)
    return out


@pytest.mark.parametrize('kind', ['one', 'three', 'stack'])
@pytest.mark.parametrize('window', [0.0, 0.25])
def test_surfel_walk_is_the_brute_force_in_every_tree(lib, kind, window):
    pts, nrm, rho, o, d = _disk_scene(kind)
    min_cos = 0.5
    ref = S.host_cast_brute(lib, S.disk_rows(pts, nrm, rho), o, d, 0.0, window, min_cos)
    assert (ref[0] >= 0).sum() >= 0.3 * len(o) and (ref[0] < 0).any()
    for shape, (child, box, rows, ids, depth, _) in disk_trees(lib, pts, nrm, rho).items():
        got = S.host_cast_walk(lib, child, box, rows, ids, o, d, 0.0, window, min_cos)
        print('%s / %s: depth %d, %d hits, up to %d blended' % (kind, shape, depth, (got[0] >= 0).sum(), got[4].max()))
        assert depth == (len(pts) - 1 if shape == 'comb' else int(np.ceil(np.log2(len(pts)))))
        _same((got[0], got[1], got[4]), (ref[0], ref[1], ref[4]), (kind, shape, 'first hit and count'))
        if window == 0.0:
            _same(got[2:4], ref[2:4], (kind, shape, 'window 0'))
        else:
            # the blend's sums are taken in the order of the walk, the brute force's in index order: equal members (the counts above), the
            # results apart by rounding only -- within the header's error counts of the exact sums (tests/surfel_reference.py)
            exact = S.oracle(pts, nrm, rho, o, d, t_min=0.0, window=window, min_cos=min_cos)
            hit = ref[0] >= 0
            assert np.array_equal(exact.index, ref[0]) and np.array_equal(exact.count[hit], ref[4][hit])
            for out in (got, ref):
                et, bt = S.t_err_units(out[2], exact)
                ec, bc = S.cos_err_units(out[3], exact)
                assert (et <= bt).all() and (ec <= bc).all()
    if kind == 'stack' and window > 0:
        assert (ref[4] == 64).sum() > 50           # rays at the middle blend every disk: the second walk prunes nothing either
