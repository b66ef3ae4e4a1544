"""LBVH build and closest-hit casting (csrc/dc_raycast.hip) against fp64 brute force, and the rendered-mesh datasets end to end."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bvh(mesh):
    return mesh.on_device(DEV)[3]


def test_bvh_structure():
    from depth_correction_amd.mesh import TriangleMesh
    rng = np.random.default_rng(1)
    c = rng.uniform(-50, 50, size=(3000, 1, 3))
    mesh = TriangleMesh((c + rng.normal(scale=0.7, size=(3000, 3, 3))).reshape(-1, 3), np.arange(9000).reshape(-1, 3))
    b = _bvh(mesh)
    n = len(mesh)
    leaf_face = b.leaf_face.cpu().numpy()
    child = b.child.cpu().numpy()
    parent = b.parent.cpu().numpy()
    box = b.node_box.cpu().numpy().astype(np.float64)
    tri = b.leaf_tri.cpu().numpy()
    assert np.array_equal(np.sort(leaf_face), np.arange(n))                          # every face in exactly one leaf
    assert np.array_equal(tri.reshape(n, 3, 3), mesh.vertices[mesh.faces[leaf_face]])
    # a tree: root 0 without parent, every other node the child of exactly one internal node, which is its parent
    assert parent[0] == -1
    kids = child.reshape(-1)
    assert np.array_equal(np.sort(kids), np.arange(1, 2 * n - 1))
    assert np.array_equal(parent[kids], np.repeat(np.arange(n - 1), 2))
    for s in (0, 1):                                                                    # parents contain their children
        assert (box[child[:, s], :3] >= box[:n - 1, :3]).all() and (box[child[:, s], 3:] <= box[:n - 1, 3:]).all()
    v = tri.reshape(n, 3, 3)
    assert (box[n - 1:, :3] <= v.min(axis=1)).all() and (box[n - 1:, 3:] >= v.max(axis=1)).all()   # leaves hold their fp64 vertices
    # every leaf reaches the root, within the traversal stack's depth of 64
    node, d = np.arange(n - 1, 2 * n - 1), 0
    while (node > 0).any():
        node = np.where(node > 0, parent[np.maximum(node, 0)], 0)
        d += 1
        assert d <= 64
    assert (node == 0).all()


def _brute_force(verts, faces, o, d, t_min, cull):
    """Möller-Trumbore in fp64 over every (ray, face): (face of the closest hit or -1, t, second-best t)."""
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    e1, e2 = v1 - v0, v2 - v0
    nrm = np.cross(e1, e2)
    R = d.shape[0]
    best_f = np.full(R, -1)
    best_t = np.full(R, np.inf)
    second = np.full(R, np.inf)
    for s in range(0, R, 128):
        dd, oo = d[s:s + 128, None, :], o[s:s + 128, None, :]
        p = np.cross(dd, e2[None])
        det = np.einsum('rfc,fc->rf', p, e1)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = 1.0 / det
            tv = oo - v0[None]
            u = np.einsum('rfc,rfc->rf', tv, p) * inv
            q = np.cross(tv, e1[None])
            v = np.einsum('rfc,rfc->rf', dd, q) * inv
            t = np.einsum('fc,rfc->rf', e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min[s:s + 128, None])
        if cull:
            ok &= np.einsum('fc,rc->rf', nrm, d[s:s + 128]) < 0
        t = np.where(ok, t, np.inf)
        order = np.argsort(t, axis=1, kind='stable')[:, :2]
        rows = np.arange(t.shape[0])
        best_t[s:s + 128] = t[rows, order[:, 0]]
        second[s:s + 128] = t[rows, order[:, 1]]
        best_f[s:s + 128] = np.where(np.isfinite(best_t[s:s + 128]), order[:, 0], -1)
    return best_f, best_t, second


@pytest.mark.parametrize('cull', [False, True])
def test_cast_matches_brute_force(cull):
    from depth_correction_amd.mesh import TriangleMesh
    from depth_correction_amd.ops import raycast
    rng = np.random.default_rng(7)
    F = 20000
    c = rng.uniform(-20, 20, size=(F, 1, 3))
    mesh = TriangleMesh((c + rng.normal(scale=0.4, size=(F, 3, 3))).reshape(-1, 3), np.arange(3 * F).reshape(-1, 3))
    P, R = 50, 2000                                                    # 100 k rays: 50 origins x 2000 directions
    poses = np.tile(np.eye(4), (P, 1, 1))
    poses[:, :3, 3] = rng.uniform(-25, 25, size=(P, 3))
    d = rng.normal(size=(R, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t_min = rng.uniform(0.0, 2.0, size=R)
    face, t, bary = raycast(_bvh(mesh), torch.as_tensor(d, device=DEV), torch.as_tensor(poses, device=DEV),
                            torch.as_tensor(t_min, device=DEV), cull=cull)
    face, t, bary = face.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1), bary.cpu().numpy().reshape(-1, 2)
    o = np.repeat(poses[:, :3, 3], R, axis=0)
    dd = np.tile(d, (P, 1))
    ref_f, ref_t, second = _brute_force(mesh.vertices, mesh.faces.astype(np.int64), o, dd, np.tile(t_min, P), cull)
    hit = ref_f >= 0
    print('cull=%s: %d of %d rays hit' % (cull, hit.sum(), hit.size))
    assert hit.sum() > 10000
    assert np.array_equal(face >= 0, hit)
    with np.errstate(invalid='ignore'):
        tie = hit & (second - ref_t <= 1e-9 * ref_t)
    assert np.array_equal(face[hit & ~tie], ref_f[hit & ~tie])
    assert np.abs(t[hit] / ref_t[hit] - 1).max() < 1e-12
    assert np.isinf(t[~hit]).all()
    # the barycentrics reproduce the hit point on the face that was hit
    tri = mesh.vertices[mesh.faces[face[hit]]]
    x = tri[:, 0] + bary[hit, :1] * (tri[:, 1] - tri[:, 0]) + bary[hit, 1:] * (tri[:, 2] - tri[:, 0])
    assert np.abs(x - (o[hit] + t[hit, None] * dd[hit])).max() < 1e-9


def test_watertight_at_shared_vertices_and_edges():
    """Rays from inside a closed, finely tessellated room aimed exactly at its vertices and edge midpoints never miss."""
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.ops import raycast
    mesh = room_mesh((3.0, 2.0, 1.5), 0.25)
    v = mesh.vertices
    f = mesh.faces
    targets = np.concatenate([v, 0.5 * (v[f[:, 0]] + v[f[:, 1]]), 0.5 * (v[f[:, 1]] + v[f[:, 2]])])
    origins = np.array([[0.0, 0.0, 0.0], [0.3, -0.7, 0.25], [-1.1, 0.4, -0.6]])
    poses = np.tile(np.eye(4), (len(origins), 1, 1))
    poses[:, :3, 3] = origins
    total = 0
    for p, o in enumerate(origins):
        d = targets - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        for cull in (True, False):
            face, t, _ = raycast(_bvh(mesh), torch.as_tensor(d, device=DEV), torch.as_tensor(poses[p:p + 1], device=DEV),
                                 torch.zeros(len(d), dtype=torch.float64, device=DEV), cull=cull)
            assert int((face < 0).sum()) == 0
            total += face.numel()
    assert total > 10000


def _room_pose(yaw=0.3, t=(0.3, -0.2, 0.1)):
    pose = np.eye(4)
    pose[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
    pose[:3, 3] = t
    return pose


def test_analytic_room_render():
    from depth_correction_amd.dataset import lidar_directions, render_lidar_cloud
    from depth_correction_amd.mesh import room_mesh
    from numpy.lib.recfunctions import structured_to_unstructured as s2u
    half = np.array([6.0, 4.0, 1.5])
    mesh = room_mesh(half, 1.0)
    size, fov, S = (16, 256), (60.0, 360.0), 16
    pose = _room_pose()
    cloud = render_lidar_cloud(mesh, pose, fov=fov, size=size, num_segments=S, device=DEV)
    assert len(cloud) == S * size[0] * (size[1] // S)
    x = s2u(cloud[['x', 'y', 'z']])
    assert (s2u(cloud[['vp_x', 'vp_y', 'vp_z']]) == 0).all()
    d, _ = lidar_directions(size=size, fov=fov, num_segments=S)
    R, o = pose[:3, :3], pose[:3, 3]
    dw = d @ R.T
    with np.errstate(divide='ignore'):
        tp = np.where(dw > 0, (half - o) / dw, (-half - o) / dw)          # distance to the wall each axis reaches
    axis = np.argmin(tp, axis=1)
    t = tp[np.arange(len(d)), axis]
    assert np.abs(np.linalg.norm(x, axis=1) / t - 1).max() < 1e-12
    # x lies along its ray
    assert np.abs(x - t[:, None] * d).max() < 1e-11
    second = np.sort(tp, axis=1)[:, 1]
    clear = second - t > 1e-9 * t                                          # rays not through a room edge
    nw = np.zeros((len(d), 3))
    nw[np.arange(len(d)), axis] = -np.sign(dw[np.arange(len(d)), axis])   # inward wall normal
    nrm = s2u(cloud[['normal_x', 'normal_y', 'normal_z']])
    assert np.abs(nrm[clear] - nw[clear] @ R).max() < 1e-12


def test_deterministic_and_batched():
    from depth_correction_amd.mesh import TriangleMesh, room_mesh
    from depth_correction_amd.ops import raycast
    from depth_correction_amd.dataset import lidar_directions, render_lidar_clouds
    rng = np.random.default_rng(3)
    F = 5000
    c = rng.uniform(-10, 10, size=(F, 1, 3))
    verts = (c + rng.normal(scale=0.5, size=(F, 3, 3))).reshape(-1, 3)
    faces = np.arange(3 * F).reshape(-1, 3)
    a, b = _bvh(TriangleMesh(verts, faces)), _bvh(TriangleMesh(verts, faces))
    for name in ('leaf_face', 'child', 'parent', 'node_box', 'leaf_tri'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    d, t_min = lidar_directions(size=(32, 256), fov=(60.0, 360.0), num_segments=8)
    poses = np.stack([_room_pose(0.1 * i, (rng.uniform(-3, 3), rng.uniform(-3, 3), 0.0)) for i in range(5)])
    args = (torch.as_tensor(np.array(d), device=DEV), torch.as_tensor(poses, device=DEV), torch.as_tensor(np.array(t_min), device=DEV))
    one = raycast(a, *args)
    two = raycast(b, *args)
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    for p in range(len(poses)):
        single = raycast(a, args[0], args[1][p:p + 1], args[2])
        for x, y in zip(one, single):
            assert torch.equal(x[p:p + 1], y)
    room = room_mesh((6.0, 4.0, 1.5), 1.0, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0))])
    batch = render_lidar_clouds(room, poses, fov=(45.0, 360.0), size=(16, 128), num_segments=8, device=DEV)
    for p in range(len(poses)):
        single = render_lidar_clouds(room, poses[p:p + 1], fov=(45.0, 360.0), size=(16, 128), num_segments=8, device=DEV)[0]
        assert np.array_equal(batch[p], single)


def _pillared_room(tmp_path):
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = tmp_path / 'pillared_room.ply'
    mesh.save_ply(str(path))
    poses = np.stack([_room_pose(0.2 * i, (-2.0 + 1.0 * i, 0.3 * math.sin(i), 0.1 * i)) for i in range(5)])
    return path, poses


def test_rendered_dataset_cache_round_trip(tmp_path):
    from depth_correction_amd.dataset import RenderedMeshDataset
    path, poses = _pillared_room(tmp_path)
    kw = dict(size=(16, 128), num_segments=8, device=DEV, cache=True, cache_dir=str(tmp_path / 'gen'))
    ds = RenderedMeshDataset(str(path), poses=poses, **kw)
    first = [c for c, _ in ds]
    assert all(len(c) == 16 * 128 for c in first)                     # a closed room: every ray hits
    again = RenderedMeshDataset(str(path), poses=poses, **kw)
    assert os.path.exists(again.cloud_path(4))
    for i, (c, p) in enumerate(again):
        assert c.dtype == RenderedMeshDataset.cloud_dtype and np.array_equal(c, first[i]) and np.array_equal(p, poses[i])
    assert np.array_equal(ds[1:3][1][0], first[2])


def test_rendered_mesh_bias_landscape_argmin(tmp_path):
    """The paper's simulation: render a room with pillars, add a ScaledPolynomial bias of known w with DepthBiasDataset, sweep the
    correction weight over a 21-point grid with ball neighbourhoods: the loss is smallest within one grid step of w."""
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.eval import eval_loss_landscape
    from depth_correction_amd.model import ScaledPolynomial
    path, poses = _pillared_room(tmp_path)
    cfg = Config(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    w_true = 0.005
    ds = RenderedMeshDataset(str(path), poses=poses, size=(64, 512), fov=(45.0, 360.0), num_segments=16, device=DEV)
    biased = DepthBiasDataset(ds, ScaledPolynomial(w=[w_true], exponent=[4.0], device=DEV), cfg=cfg)
    c0, _ = ds[0]
    c1, _ = biased[0]
    assert not np.array_equal(c0['x'], c1['x'])
    ws = np.linspace(-0.01, 0.01, 21)
    loss, count = eval_loss_landscape(cfg, torch.as_tensor(ws), test_datasets=[biased],
                                      model=ScaledPolynomial(w=[0.0], exponent=[4.0], device=DEV))
    loss = loss.cpu().numpy()
    print('landscape:', list(zip(ws.round(4), loss)))
    assert np.isfinite(loss).all()
    assert abs(ws[int(np.argmin(loss))] - w_true) <= 0.001 + 1e-12, list(zip(ws, loss))
