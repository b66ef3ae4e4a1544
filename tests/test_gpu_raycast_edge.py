"""The BVH ray caster (csrc/dc_raycast.hip) at the places where its promises are hard to keep: ties between coincident faces, a sensor
exactly at the world origin, directions with exact zero components, rays along tessellation lines and in walls' planes, scenes at
UTM-sized coordinates, trees of unusual shape, t == t_min, scaled directions.  Every cast is compared bit for bit with the oracle
(the kernels' own test_triangle over every face in index order, built for the host: whatever the traversal does, it must return
exactly this) and, on its clear rays, with an independent numpy classifier (tests/raycast_reference.py).  The scenes are checked on
the host by tests/test_raycast_host.py."""
import numpy as np
import pytest
import torch

import raycast_reference as RR
from helpers import raycast_host_lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def host():
    return raycast_host_lib()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_BVH = {}


def _bvh(case):
    """(TriangleMesh, MeshBVH) of the case's mesh, one build per mesh."""
    from depth_correction_amd.mesh import TriangleMesh
    from depth_correction_amd.ops import bvh_build
    key = (case.verts.tobytes(), case.faces.tobytes(), case.scene_box)
    if key not in _BVH:
        mesh = TriangleMesh(case.verts, case.faces)
        if case.scene_box is None:
            bvh = mesh.on_device(DEV)[3]
        else:
            bvh = bvh_build(_dev(mesh.vertices), _dev(mesh.faces), case.scene_box)
        _BVH.clear()
        _BVH[key] = (mesh, bvh)
    return _BVH[key]


def _incidence(case, face):
    """cos of the incidence angle of the case's rays on the faces ``face`` (NaN on a miss), in numpy."""
    tri = case.verts[case.faces[np.maximum(face, 0)]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    with np.errstate(invalid='ignore'):                              # a zero direction: 0 / 0, on a miss
        c = np.abs(np.einsum('rc,rc->r', n, case.d)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(case.d, axis=1))
    return np.where(face >= 0, np.minimum(1.0, c), np.nan)


def cast(case):
    """The case on the device: (face, t, u, v) of raycast, or (face, t, None, None) of raycast_rays after its ``inc`` is compared
    with numpy: the same NaNs, cos(inc) within 1e-13 (a dozen roundings of fp64 in the cosine, contracted differently on the device;
    the angle itself is ill-conditioned at 0)."""
    from depth_correction_amd import ops
    _, bvh = _bvh(case)
    if case.api == 'raycast':
        face, t, bary = ops.raycast(bvh, _dev(case.dirs), _dev(case.poses), _dev(case.t_min_arg), cull=case.cull)
        bary = bary.cpu().numpy().reshape(-1, 2)
        return face.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1), bary[:, 0], bary[:, 1]
    dtype = torch.float32 if case.dtype == np.float32 else torch.float64
    face, t, inc = ops.raycast_rays(bvh, _dev(case.vps, dtype), _dev(case.dirs, dtype), case.scan_offset, _dev(case.poses),
                                    t_min=case.t_min_arg, cull=case.cull)
    face, t, inc = face.cpu().numpy(), t.cpu().numpy(), inc.cpu().numpy()
    ref = _incidence(case, face)
    assert np.array_equal(np.isnan(inc), np.isnan(ref))
    ok = ~np.isnan(ref)
    if ok.any():
        assert np.abs(np.cos(inc[ok]) - ref[ok]).max() <= 1e-13
    return face, t, None, None


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cull', [True, False])
@pytest.mark.parametrize('sensor', [0, 1, 2])
def test_ties(host, sensor, cull):
    """Coincident faces (two tessellations of the same walls, every face twice, index order shuffled): the lowest face index among
    equal t wins, from a sensor exactly at the origin, next to it and elsewhere, towards vertices, edge midpoints and interiors."""
    case = RR.case_ties(sensor, cull)
    face, t, u, v = cast(case)
    assert (face >= 0).all()                                          # a closed room
    _, cl = RR.verify(host, case, face, t, u, v)
    assert (cl.n_tied[~case.aimed] >= 3).all()                        # interiors: a fine face, its duplicate, the coarse face under it


# ---- zero components and grazing -------------------------------------------------------------------------------------------------------
def test_zero_components(host):
    case = RR.case_zero_components()
    assert (case.d[:6] == np.concatenate([np.eye(3), -np.eye(3)])).all()
    face, t, u, v = cast(case)
    assert (face >= 0).all()
    RR.verify(host, case, face, t, u, v)
    assert np.array_equal(t[:6], [3.0, 2.0, 1.5, 3.0, 2.0, 1.5])     # the axes from the origin, exactly


@pytest.mark.parametrize('cull', [True, False])
def test_grazing(host, cull):
    case = RR.case_grazing(cull)
    face, t, _, _ = cast(case)
    RR.verify(host, case, face, t)
    axial = np.abs(case.d).max(axis=1) == 1.0
    assert (face[axial] >= 0).all()                                   # along a tessellation line the far wall is still hit


# ---- far scenes ------------------------------------------------------------------------------------------------------------------------
_NEAR = {}


def _near(host, kind):
    """The untranslated scene, cast and verified once per kind: (faces, the classifier's clear hits, their t)."""
    if kind not in _NEAR:
        near = RR.case_far(kind, 0)
        nf, nt, _, _ = cast(near)
        _, ncl = RR.verify(host, near, nf, nt)
        _NEAR[kind] = (nf, ncl.status == RR.HIT, ncl.t)
    return _NEAR[kind]


@pytest.mark.parametrize('offset', [1, 2])
@pytest.mark.parametrize('kind', ['room', 'soup'])
def test_far_scenes(host, kind, offset):
    """The scene and its sensors translated to UTM-sized coordinates (exactly: all coordinates lie on a 2^-20 grid): the oracle on the
    translated data is met bit for bit, and nothing that the untranslated scene hits clearly is missed."""
    nf, clear, nt = _near(host, kind)
    assert clear.sum() >= 1500
    far = RR.case_far(kind, offset)
    face, t, _, _ = cast(far)
    RR.verify(host, far, face, t)
    assert (face[clear] >= 0).all() and np.abs(t[clear] / nt[clear] - 1.0).max() <= 1e-12
    if kind == 'soup':                                                # no coincident faces: the very same face
        assert np.array_equal(face[clear], nf[clear])


# ---- tree shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', RR.SHAPES)
def test_tree_shapes(host, shape):
    case = RR.case_shape(shape)
    mesh, bvh = _bvh(case)
    RR.check_bvh(bvh, mesh)
    face, t, _, _ = cast(case)
    RR.verify(host, case, face, t)
    if shape == 'degenerate':
        tri = case.verts[case.faces[face]]
        assert (face >= 0).all() and (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) > 0).all()


# ---- t_min and culling on dyadic geometry ----------------------------------------------------------------------------------------------
def test_t_min_and_culling_exact(host):
    """A wall at x = 2 that shows the ray its back and one at x = 3 that faces it, a ray along +x from the origin: every number is
    exact.  t_min = 2 excludes the hit at t = 2, the next number below 2 includes it; with culling the wall behind wins."""
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import TriangleMesh
    verts = np.array([[2.0, -1, -1], [2.0, 1, -1], [2.0, 0, 1], [3.0, -1, -1], [3.0, 1, -1], [3.0, 0, 1]])
    faces = np.array([[0, 1, 2], [3, 5, 4]])                          # normals +x (away from the ray's origin) and -x
    bvh = TriangleMesh(verts, faces).on_device(DEV)[3]
    below = np.nextafter(2.0, 0.0)
    t_min = np.array([0.0, below, 2.0, 3.0, np.nextafter(3.0, 0.0)])
    dirs = np.tile([1.0, 0.0, 0.0], (len(t_min), 1))
    pose = np.eye(4)[None]
    want = {False: ([0, 0, 1, -1, 1], [2.0, 2.0, 3.0, np.inf, 3.0]), True: ([1, 1, 1, -1, 1], [3.0, 3.0, 3.0, np.inf, 3.0])}
    for cull in (False, True):
        face, t, bary = ops.raycast(bvh, _dev(dirs), _dev(pose), _dev(t_min), cull=cull)
        face, t, bary = face.cpu().numpy()[0], t.cpu().numpy()[0], bary.cpu().numpy()[0]
        assert np.array_equal(face, want[cull][0]) and np.array_equal(t, want[cull][1]), (cull, face, t)
        of, ot, ou, ov = RR.oracle(host, verts, faces, np.zeros((len(t_min), 3)), dirs, t_min, cull)
        assert np.array_equal(face, of) and np.array_equal(_bits(t), _bits(ot))
        assert np.array_equal(_bits(bary[:, 0]), _bits(ou)) and np.array_equal(_bits(bary[:, 1]), _bits(ov))
        hit = face >= 0
        assert np.array_equal(bary[hit], np.where((face[hit] == 0)[:, None], [0.25, 0.5], [0.5, 0.25]))


# ---- direction scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_direction_scale(host, dtype):
    """raycast_rays with the directions scaled by 2^k, k = -10 .. 10: the same face and t scaled exactly; a zero direction is a miss
    with inc NaN (and the launch returns: every box test passes or fails, the tree is finite)."""
    verts, faces = RR._room()
    rng = np.random.default_rng(26)
    n = 200
    base = RR._unit(rng.normal(size=(n, 3))).astype(dtype)
    base[:6] = np.concatenate([np.eye(3), -np.eye(3)]).astype(dtype)
    base[6:9] = 0.0                                                    # zero directions
    vps = (rng.uniform(-1, 1, size=(n, 3)) * [2.5, 1.5, 1.2]).astype(dtype)
    vps[:3] = 0.0
    vps[6] = 0.0
    ks = list(range(-10, 11))
    dirs = np.concatenate([base * dtype(2.0 ** k) for k in ks])
    case = RR.Case('scale-%s' % np.dtype(dtype).name, verts, faces, True).rays(np.tile(vps, (len(ks), 1)), dirs, [len(dirs)], [(0.0, 0.0, 0.0)],
                                                                                0.0, np.tile(np.arange(n) < 9, len(ks)), dtype=dtype)
    face, t, _, _ = cast(case)
    (of, ot, _, _), _ = RR.verify(host, case, face, t)
    face, t = face.reshape(len(ks), n), t.reshape(len(ks), n)
    zero = np.arange(n)[6:9]
    assert (face[:, zero] == -1).all() and np.isinf(t[:, zero]).all()
    live = np.setdiff1d(np.arange(n), zero)
    assert (face[:, live] >= 0).all()
    k0 = ks.index(0)
    for i, k in enumerate(ks):
        assert np.array_equal(face[i], face[k0]), k
        assert np.array_equal(_bits(t[i, live] * 2.0 ** k), _bits(t[k0, live])), k


# ---- beams -----------------------------------------------------------------------------------------------------------------------------
def test_beams_on_the_tie_mesh_from_the_origin(host):
    """raycast_beams' sub-ray returns on the tie mesh from a sensor at the origin equal raycast_rays on beam_subrays' output, which
    equals the oracle."""
    from depth_correction_amd import ops
    import beam_reference as BR
    case = RR.case_ties(0, True)
    _, bvh = _bvh(case)
    S, r0, spread = 16, 2.5e-3, 6.1e-3
    pat = BR.pattern(S)
    n = 150
    dirs = case.dirs[np.r_[0:50, 700:750, 1400:1450]]
    vps = np.zeros_like(dirs)
    off, poses = [0, n], np.eye(4)[None]
    out = ops.raycast_beams(bvh, _dev(vps), _dev(dirs), off, _dev(poses), pat, r0, spread, t_min=0.0, cull=True, want_samples=True)
    sub_face, sub_t = out[3].cpu().numpy(), out[4].cpu().numpy()
    o, D = ops.beam_subrays(_dev(vps), _dev(dirs), pat, r0, spread)
    rf, rt, _ = ops.raycast_rays(bvh, o.reshape(-1, 3), D.reshape(-1, 3), [0, n * S], _dev(poses), t_min=0.0, cull=True)
    assert np.array_equal(sub_face.reshape(-1), rf.cpu().numpy()) and np.array_equal(_bits(sub_t.reshape(-1)), _bits(rt.cpu().numpy()))
    assert (sub_face >= 0).all()
    sub = RR.Case('beams', case.verts, case.faces, True).rays(o.cpu().numpy().reshape(-1, 3), D.cpu().numpy().reshape(-1, 3), [n * S],
                                                             [(0.0, 0.0, 0.0)], 0.0, True)
    RR.verify(host, sub, sub_face.reshape(-1), sub_t.reshape(-1))
