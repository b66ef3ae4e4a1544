"""Mesh readers, procedural meshes, the lidar ray pattern and the rendered-mesh dataset plumbing (no GPU)."""
import math
import struct

import numpy as np
import pytest


def _quad_mesh():
    """A unit cube's bottom quad and a triangle: 5 vertices, a quad and a triangle -> 3 triangles."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], dtype=np.float64)
    polys = [[0, 1, 2, 3], [0, 1, 4]]
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]])
    return v, polys, tris


def test_ply_ascii_with_extra_properties(tmp_path):
    from depth_correction_amd.mesh import load_mesh
    v, polys, tris = _quad_mesh()
    lines = ['ply', 'format ascii 1.0', 'comment made by hand', 'element vertex %d' % len(v), 'property float x', 'property float y',
             'property float z', 'property uchar red', 'element face %d' % len(polys), 'property list uchar int vertex_indices',
             'property int flags', 'element edge 1', 'property int vertex1', 'property int vertex2', 'end_header']
    lines += ['%r %r %r 7' % tuple(map(float, r)) for r in v]
    lines += ['%d %s 0' % (len(p), ' '.join(map(str, p))) for p in polys]
    lines += ['0 1']
    path = tmp_path / 'm.ply'
    path.write_text('\n'.join(lines) + '\n')
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices, v)
    assert m.faces.dtype == np.int32 and np.array_equal(m.faces, tris)


@pytest.mark.parametrize('uniform', [True, False])
def test_ply_binary(tmp_path, uniform):
    from depth_correction_amd.mesh import load_mesh
    v, polys, tris = _quad_mesh()
    if uniform:
        polys, tris = [[0, 1, 2], [0, 2, 3], [0, 1, 4]], tris
    hdr = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n'
           'property float intensity\nelement face %d\nproperty list uchar uint vertex_index\nend_header\n' % (len(v), len(polys)))
    body = b''.join(struct.pack('<dddf', *r, 0.5) for r in v)
    body += b''.join(struct.pack('<B%dI' % len(p), len(p), *p) for p in polys)
    path = tmp_path / 'm.ply'
    path.write_bytes(hdr.encode() + body)
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices, v)
    assert np.array_equal(m.faces, tris)


def test_ply_round_trip_of_a_room(tmp_path):
    from depth_correction_amd.mesh import load_mesh, room_mesh
    m = room_mesh((3.0, 2.0, 1.5), 0.7, pillars=[((1.0, 0.5, 0.0), (0.3, 0.2, 0.6))])
    for binary in (True, False):
        path = str(tmp_path / ('r%d.ply' % binary))
        m.save_ply(path, binary=binary)
        r = load_mesh(path)
        assert np.array_equal(r.vertices, m.vertices) and np.array_equal(r.faces, m.faces)


def test_obj_forms(tmp_path):
    from depth_correction_amd.mesh import load_mesh
    v, _, tris = _quad_mesh()
    text = ['# a comment', 'o thing', 'mtllib x.mtl']
    text += ['v %r %r %r' % tuple(map(float, r)) for r in v[:4]]
    text += ['vt 0 0', 'vn 0 0 1', 'f 1/1/1 2/1/1 3/1/1 4/1/1']          # quad, v/vt/vn
    text += ['v %r %r %r 1.0' % tuple(map(float, v[4]))]
    text += ['usemtl m', 's off', 'f -5//1 -4//1 -1//1']                  # negative indices, i//k
    path = tmp_path / 'm.obj'
    path.write_text('\n'.join(text) + '\n')
    m = load_mesh(str(path))
    assert np.array_equal(m.vertices, v)
    assert np.array_equal(m.faces, tris)
    path.write_text('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/2 2/2 3/2\n')
    assert np.array_equal(load_mesh(str(path)).faces, [[0, 1, 2]])


@pytest.mark.parametrize('name,content,match', [
    ('m.stl', b'solid x', 'Supported mesh formats'),
    ('m.ply', b'ply\nformat binary_big_endian 1.0\nelement vertex 0\nelement face 0\nend_header\n', 'not supported'),
    ('m.ply', b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n1 0 0\n0 1 0\n',
     'vertex and a face element'),
    ('m.ply', b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
              b'element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 5\n', 'out of range'),
    ('m.ply', b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
              b'element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n', 'malformed|ends'),
    ('m.ply', b'plx\n', 'not a PLY'),
    ('m.obj', b'v 0 0 0\nv 1 0 0\nf 1 2\n', 'at least 3'),
    ('m.obj', b'v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n', 'out of range'),
    ('m.obj', b'v 0 0\n', 'malformed'),
    ('m.obj', b'v 0 0 0\nv 1 0 0\nv 0 1 0\n', 'no faces'),
])
def test_bad_files_raise_clear_errors(tmp_path, name, content, match):
    from depth_correction_amd.mesh import load_mesh
    path = tmp_path / name
    path.write_bytes(content)
    with pytest.raises(ValueError, match=match):
        load_mesh(str(path))


def _edge_use(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return e


def test_room_mesh_is_closed_and_faces_inward():
    from depth_correction_amd.mesh import room_mesh
    half = np.array([3.0, 2.0, 1.5])
    m = room_mesh(half, 0.5, pillars=[((1.0, 0.5, 0.0), (0.3, 0.2, 0.6))])
    e = _edge_use(m.faces)
    # closed and consistently oriented: every directed edge appears once, and its reverse once
    fwd = set(map(tuple, e))
    assert len(fwd) == len(e)
    assert all((b, a) in fwd for a, b in fwd)
    n = m.face_normals()
    c = m.vertices[m.faces].mean(axis=1)
    wall = (np.abs(np.abs(c) - half) < 1e-12).any(axis=1)
    axis = np.argmax(np.abs(c) / half, axis=1)
    sign = np.sign(c[np.arange(len(c)), axis])
    assert np.allclose(n[wall, axis[wall]], -sign[wall])               # inward
    pil = ~wall
    pc = c[pil] - np.array([1.0, 0.5, 0.0])
    assert (np.einsum('ij,ij->i', n[pil], pc) > 0).all()                # pillar faces outward
    assert len(m) == 2 * 2 * (12 * 8 + 12 * 6 + 8 * 6) + 2 * 2 * (2 * 3 + 1 * 3 + 2 * 1)


def test_grid_terrain_mesh_size():
    from depth_correction_amd.mesh import grid_terrain_mesh
    m = grid_terrain_mesh(40)
    assert len(m) == 2 * 40 * 40 and m.vertices.shape == (41 * 41, 3)
    assert (m.face_normals()[:, 2] > 0).all()


def _look_at_directions(size, fov, S):
    """Independent restatement: pytorch3d's look_at_rotation (z = at - eye, x = up x z, y = z x x) and a pinhole of focal
    lengths (W_s/2)/tan(F_h/2S), (H/2)/tan(F_v/2), +X left, +Y up, pixel centres at half-integers."""
    H, W = size
    Ws = int(W / S)
    fh, fv = math.radians(fov[1]), math.radians(fov[0])
    fx, fy = (Ws / 2) / math.tan(fh / S / 2), (H / 2) / math.tan(fv / 2)
    out, clip = [], []
    for i in range(S):
        a = -fh / 2 + i * (fh / S) + 1e-3
        at = np.array([math.cos(a), math.sin(a), 0.0])
        z = at / np.linalg.norm(at)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        for r in range(H):
            for c in range(Ws):
                X, Y = (Ws / 2 - (c + 0.5)) / fx, (H / 2 - (r + 0.5)) / fy
                d = X * x + Y * y + z
                d /= np.linalg.norm(d)
                out.append(d)
                clip.append(1e-3 / d.dot(z))
    return np.array(out), np.array(clip)


@pytest.mark.parametrize('size,fov,S', [((8, 24), (45.0, 360.0), 1), ((6, 64), (30.0, 360.0), 4), ((4, 512), (90.0, 360.0), 16),
                                        ((5, 50), (20.0, 120.0), 4)])
def test_lidar_directions_match_look_at(size, fov, S):
    from depth_correction_amd.dataset import lidar_directions
    d, t_min = lidar_directions(size=size, fov=fov, num_segments=S)
    ref, ref_clip = _look_at_directions(size, fov, S)
    assert d.shape == (S * size[0] * int(size[1] / S), 3)
    assert np.abs(d - ref).max() < 1e-14
    assert np.abs(t_min / ref_clip - 1).max() < 1e-13
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)


def test_lidar_directions_reject_bad_patterns():
    from depth_correction_amd.dataset import lidar_directions
    for kw in (dict(fov=(0.0, 360.0)), dict(fov=(45.0, 400.0)), dict(size=(0, 10)), dict(size=(4, 8), num_segments=16)):
        with pytest.raises(ValueError):
            lidar_directions(**kw)


def _room_file(tmp_path):
    from depth_correction_amd.mesh import room_mesh
    path = tmp_path / 'room.ply'
    room_mesh((3.0, 2.0, 1.0), 1.0).save_ply(str(path))
    return path


def test_rendered_mesh_names(tmp_path, monkeypatch):
    from depth_correction_amd import render
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import RenderedMeshDataset, create_dataset
    from depth_correction_amd.scan_io import write_poses_csv
    path = _room_file(tmp_path)
    monkeypatch.setattr(render, 'mesh_dir', lambda: str(tmp_path))
    poses = np.stack([np.eye(4)] * 12)
    poses[:, 0, 3] = np.linspace(-1, 1, 12)
    write_poses_csv(list(range(12)), poses, str(tmp_path / 'poses.csv'))
    assert RenderedMeshDataset.parse_params('n_10_size_64_512_fov_45_360'.split('_'), None, (1, 1), (1., 1.)) == \
        (10, [64, 512], [45.0, 360.0])
    assert RenderedMeshDataset.parse_params(['size', '32', '256'], 3, (1, 1), (9., 9.)) == (3, [32, 256], (9., 9.))
    ds = create_dataset('rendered_mesh/room.ply/n_10_size_32_256_fov_40_360', Config(), poses_path='poses.csv')
    assert isinstance(ds, RenderedMeshDataset)
    assert (len(ds), ds.size, ds.fov, str(ds)) == (10, (32, 256), (40.0, 360.0), 'rendered_mesh/room.ply')
    assert ds.device == Config().device
    assert np.allclose(ds.cloud_pose(3), poses[3], rtol=0, atol=1e-9)          # the CSV keeps 9 decimals
    sub = ds[2:5]
    assert len(sub) == 3 and sub.ids == [2, 3, 4] and len(ds[[0, 9]]) == 2
    assert len(RenderedMeshDataset(str(path), poses=poses[:4])) == 4
    assert len(RenderedMeshDataset('room.ply', poses=poses)) == 12
    with pytest.raises(FileNotFoundError):
        RenderedMeshDataset('rendered_mesh/missing.ply', poses=poses)
    with pytest.raises(ValueError, match='Invalid'):
        RenderedMeshDataset('other/room.ply', poses=poses)
    with pytest.raises(ValueError, match='Unsupported'):
        create_dataset('asl_laser/eth', Config())


def test_config_defaults_and_noisy_dataset_leaves_zero_bias_alone():
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import DepthBiasDataset, PlaneDataset, noisy_dataset
    cfg = Config()
    assert (cfg.depth_bias_model_class, cfg.depth_bias_model_args, cfg.depth_bias_model_kwargs) == ('ScaledPolynomial', [], {})
    ds = PlaneDataset(n_pts=100)
    assert noisy_dataset(ds, cfg) is ds
    assert noisy_dataset(ds, Config(depth_bias_model_kwargs={'w': [0.0], 'exponent': [4.0]})) is ds
    wrapped = noisy_dataset(ds, Config(depth_bias_model_kwargs={'w': [0.004], 'exponent': [4.0]}))
    assert isinstance(wrapped, DepthBiasDataset) and wrapped.target is ds
    assert float(wrapped.model.w.detach()[0, 0]) == 0.004
    assert noisy_dataset(ds, Config(depth_bias_model_class=None)) is ds


def test_depth_bias_on_the_host_with_normals():
    """DepthBiasDataset with a CPU model and clouds with normals: d / (1 - w gamma^4) along each ray (model.inverse)."""
    from numpy.lib.recfunctions import structured_to_unstructured
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.model import ScaledPolynomial
    rng = np.random.default_rng(0)
    d = rng.normal(size=(50, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    depth = rng.uniform(1, 5, size=50)
    n = rng.normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cloud = np.zeros(50, dtype=RenderedMeshDataset.cloud_dtype)
    for i, f in enumerate('xyz'):
        cloud[f] = depth * d[:, i]
        cloud['normal_' + f] = n[:, i]

    class One:
        def __getitem__(self, i):
            return cloud.copy(), np.eye(4)

        def __len__(self):
            return 1

    out, _ = DepthBiasDataset(One(), ScaledPolynomial(w=[0.01], exponent=[4.0]))[0]
    gamma = np.arccos(np.clip(np.abs(np.einsum('ij,ij->i', d, n)), None, 1.0))
    want = depth / (1 - 0.01 * gamma ** 4)
    got = structured_to_unstructured(out[['x', 'y', 'z']])
    assert np.allclose(np.linalg.norm(got, axis=1), want, rtol=1e-12)
    assert np.array_equal(structured_to_unstructured(out[['normal_x', 'normal_y', 'normal_z']]), n)


def test_mesh_cast_without_a_gpu_says_so(tmp_path):
    import torch
    from depth_correction_amd.dataset import RenderedMeshDataset, render_lidar_cloud
    from depth_correction_amd.mesh import room_mesh
    m = room_mesh((2.0, 2.0, 1.0), 1.0)
    with pytest.raises(RuntimeError, match='needs a GPU'):
        render_lidar_cloud(m, np.eye(4), size=(4, 16), num_segments=4, device='cpu')
    with pytest.raises(RuntimeError, match='needs a GPU'):
        m.on_device('cpu')
    if not torch.cuda.is_available():
        ds = RenderedMeshDataset(str(_room_file(tmp_path)), poses=np.eye(4)[None], size=(4, 16), num_segments=4)
        with pytest.raises(RuntimeError, match='needs a GPU'):
            ds[0]
