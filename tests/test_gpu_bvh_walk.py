"""The one tree walk (csrc/dc_bvh.h) on the GPU over trees of chosen shape: MeshBVH / SurfelBVH objects made from the arrays of
raycast_reference.build_tree -- a root that is a leaf, three leaves, and the 64-leaf comb of depth 63, deeper than any tree the Morton
build produces in the rest of the suite -- go through raycast, raycast_rays, surfel_cast_rays and mesh_closest.  The answers are the host
build's brute force and the answers of the library's own tree over the same primitives, bit for bit."""
import numpy as np
import pytest
import torch

import raycast_reference as R
import surfel_reference as S
from test_bvh_walk_host import TRI_CASES, _disk_scene, disk_trees, tri_trees

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EYE = np.eye(4)[None]


@pytest.fixture(scope='module')
def lib():
    return S.surfel_host_lib()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _host(out):
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)


def _same(got, ref, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(np.asarray(g), np.asarray(r), equal_nan=True) and np.array_equal(np.signbit(g), np.signbit(r)), (what, k)


def _mesh_bvhs(lib, case):
    """The two hand-made trees of the host suite and the library's own, as mesh.MeshBVH."""
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import MeshBVH
    out = {}
    for shape, (child, box, tri, ids, _, parent) in tri_trees(lib, case).items():
        out[shape] = MeshBVH(_dev(ids), _dev(child), _dev(parent), _dev(box), _dev(tri))
    verts = np.asarray(case.verts, dtype=np.float64)
    out['library'] = ops.bvh_build(_dev(verts), _dev(case.faces.astype(np.int32)), np.concatenate([verts.min(axis=0), verts.max(axis=0)]))
    return out


@pytest.mark.parametrize('name', ['one', 'three', 'stack'])
def test_triangle_kernels_over_given_trees(lib, name):
    from depth_correction_amd import ops
    full = TRI_CASES[name]()
    step = max(1, len(full.o) // 240)
    o, d = full.o[::step], full.d[::step]
    rays = R.Case(name, full.verts, full.faces, full.cull).rays(o, d, [len(o)], [(0.0, 0.0, 0.0)], 0.0, False)
    fan = R.Case(name, full.verts, full.faces, full.cull).raycast(d, [o[0], o[-1]], 0.0, False)
    ref_rays = R.oracle(lib, rays.verts, rays.faces, rays.o, rays.d, rays.t_min, rays.cull)
    ref_fan = R.oracle(lib, fan.verts, fan.faces, fan.o, fan.d, fan.t_min, fan.cull)
    assert (ref_rays[0] >= 0).sum() > 0.4 * len(o) and (ref_fan[0] >= 0).any()
    pts = np.concatenate([o + 0.5 * d, np.asarray(full.verts)[:40] + 0.01])
    first = {}
    for shape, bvh in _mesh_bvhs(lib, full).items():
        face, t, inc = _host(ops.raycast_rays(bvh, _dev(rays.vps), _dev(rays.dirs), rays.scan_offset, _dev(rays.poses), t_min=0.0, cull=rays.cull))
        _same((face, t), ref_rays[:2], (name, shape, 'raycast_rays'))
        f2, t2, bary = _host(ops.raycast(bvh, _dev(fan.dirs), _dev(fan.poses), _dev(fan.t_min_arg), cull=fan.cull))
        _same((f2.reshape(-1), t2.reshape(-1), bary[..., 0].reshape(-1), bary[..., 1].reshape(-1)), ref_fan, (name, shape, 'raycast'))
        near = _host(ops.mesh_closest(bvh, _dev(pts)))
        assert (near[0] >= 0).all() and np.isfinite(near[1]).all()
        for key, got in (('inc', (inc,)), ('closest', near)):
            _same(got, first.setdefault(key, got), (name, shape, key))
    # the nearest triangle against numpy over every (point, face) pair
    import mesh_reference
    ref_d = mesh_reference.brute_force(full.verts, full.faces, pts)[1]
    assert np.abs(first['closest'][1] - ref_d).max() <= 1e-12 * (1.0 + ref_d.max())


@pytest.mark.parametrize('kind', ['one', 'three', 'stack'])
def test_surfel_kernel_over_given_trees(lib, kind):
    from depth_correction_amd import ops
    from depth_correction_amd.survey import SurfelBVH
    pts, nrm, rho, o, d = _disk_scene(kind)
    off = np.array([0, len(o)], dtype=np.int64)
    bvhs = {}
    trees = disk_trees(lib, pts, nrm, rho)
    for shape, (child, box, rows, ids, _, parent) in trees.items():
        bvhs[shape] = SurfelBVH(_dev(ids), _dev(child), _dev(parent), _dev(box), _dev(rows))
    bvhs['library'] = ops.surfel_bvh_build(_dev(pts), _dev(nrm), _dev(rho), np.concatenate([pts.min(axis=0), pts.max(axis=0)]))
    for window in (0.0, 0.25):
        ref = S.host_cast_brute(lib, S.disk_rows(pts, nrm, rho), o, d, 0.0, window, 0.5)
        assert (ref[0] >= 0).sum() > 0.3 * len(o)
        for shape, bvh in bvhs.items():
            got = _host(ops.surfel_cast_rays(bvh, _dev(o), _dev(d), off, _dev(EYE), t_min=0.0, window=window, min_cos=0.5))
            _same((got[0], got[1], got[4]), (ref[0], ref[1], ref[4]), (kind, shape, window, 'first hit and count'))
            if window == 0.0:
                _same(got[2:4], ref[2:4], (kind, shape, 'window 0'))
            elif shape != 'library':             # the blend in the order of the walk: the host's walk over the same tree, bit for bit
                child, box, rows, ids = trees[shape][:4]
                _same(got, S.host_cast_walk(lib, child, box, rows, ids, o, d, 0.0, window, 0.5), (kind, shape, 'blend'))
        if kind == 'stack' and window > 0:
            assert (ref[4] == 64).sum() > 50
