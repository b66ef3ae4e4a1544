"""Triangle meshes for the rendered-mesh datasets (the reference reads them with pytorch3d: utils.load_mesh :241-250).

``TriangleMesh`` holds float64 vertices ``[V,3]`` and int32 faces ``[F,3]`` on the host and, on demand, on a GPU together with
its LBVH (``csrc/dc_raycast.hip``).  ``load_mesh`` reads PLY (ascii, binary_little_endian) and OBJ with readers of its own
(pytorch3d, open3d and trimesh are not dependencies); polygons are fan-triangulated.  ``room_mesh`` and ``grid_terrain_mesh``
build meshes without files, for tests and benchmarks.
"""
from __future__ import annotations

import math
import os

import numpy as np

__all__ = ['TriangleMesh', 'MeshBVH', 'load_mesh', 'read_ply', 'read_obj', 'room_mesh', 'grid_terrain_mesh', 'box_mesh']


class MeshBVH(object):
    """Device arrays of ``dc_bvh_build`` (layout: include/dc_hip.h)."""

    def __init__(self, leaf_face, child, parent, node_box, leaf_tri):
        self.leaf_face, self.child, self.parent, self.node_box, self.leaf_tri = leaf_face, child, parent, node_box, leaf_tri

    @property
    def n_faces(self):
        return self.leaf_face.shape[0]


class TriangleMesh(object):
    """float64 vertices [V,3] and int32 faces [F,3] (counter-clockwise seen from the side the normal points to)."""

    def __init__(self, vertices, faces):
        v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64))
        f = np.asarray(faces)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
            raise ValueError('vertices must be a non-empty [V,3] array, got shape %s' % (v.shape,))
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError('faces must be a non-empty [F,3] array, got shape %s' % (f.shape,))
        if not np.issubdtype(f.dtype, np.integer):
            raise ValueError('faces must hold integers, got %s' % f.dtype)
        if f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError('face indices must lie in [0, %d), got [%d, %d]' % (v.shape[0], f.min(), f.max()))
        if f.shape[0] > 2 ** 30:
            raise ValueError('at most 2^30 faces, got %d' % f.shape[0])
        if not np.isfinite(v).all():
            raise ValueError('vertices must be finite')
        self.vertices = v
        self.faces = np.ascontiguousarray(f.astype(np.int32))
        self._device = {}
        self._area_cdf = {}

    def __len__(self):
        return self.faces.shape[0]

    def __repr__(self):
        return 'TriangleMesh(%d vertices, %d faces)' % (self.vertices.shape[0], self.faces.shape[0])

    @property
    def bounds(self):
        """The scene's bounding box: (lo [3], hi [3]) of the vertices."""
        return self.vertices.min(axis=0), self.vertices.max(axis=0)

    def face_normals(self):
        """normalize((v1 - v0) x (v2 - v0)) per face, float64 [F,3] (pytorch3d's faces_normals); zero for degenerate faces."""
        v = self.vertices[self.faces]
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        norm = np.linalg.norm(n, axis=1, keepdims=True)
        return np.divide(n, norm, out=np.zeros_like(n), where=norm > 0)

    def face_areas(self):
        """|(v1 - v0) x (v2 - v0)| / 2 per face, float64 [F]."""
        v = self.vertices[self.faces]
        return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)

    def area_cdf(self):
        """Inclusive prefix sum of face_areas() (numpy cumsum: one fixed order), what sample() searches."""
        return np.cumsum(self.face_areas())

    def sample(self, n, seed=135, device='cuda'):
        """``n`` points drawn from the surface with probability proportional to area (the reference's sample_points_from_meshes,
        dataset.py:450) -> (points f64 [n,3], normals f64 [n,3] = the face normals, face i32 [n]) on ``device``.  A pure function
        of (mesh, n, seed): dc_mesh_sample's formula, not pytorch3d's generator.  ``seed`` defaults to Config.random_seed's 135."""
        import torch
        from .ops import mesh_sample
        verts, faces, normals, _ = self.on_device(device)
        cdf = self._area_cdf.get(verts.device)
        if cdf is None:
            host = self.area_cdf()
            if not (np.isfinite(host[-1]) and host[-1] > 0.0):
                raise ValueError('a mesh of total area %r cannot be sampled' % float(host[-1]))
            cdf = self._area_cdf[verts.device] = torch.as_tensor(host, device=verts.device)
        face, pts = mesh_sample(verts, faces, cdf, n, seed)
        return pts, normals[face.long()], face

    def save_ply(self, path, binary=True):
        """Write the mesh as PLY (binary_little_endian or ascii): double x y z, a uchar / int list per face."""
        nv_, nf = self.vertices.shape[0], self.faces.shape[0]
        header = ('ply\nformat %s 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n'
                  'element face %d\nproperty list uchar int vertex_indices\nend_header\n'
                  % ('binary_little_endian' if binary else 'ascii', nv_, nf))
        with open(path, 'wb') as fh:
            fh.write(header.encode('ascii'))
            if binary:
                fh.write(self.vertices.astype('<f8').tobytes())
                rows = np.zeros(nf, dtype=[('n', 'u1'), ('i', '<i4', (3,))])
                rows['n'], rows['i'] = 3, self.faces
                fh.write(rows.tobytes())
            else:
                for v in self.vertices:
                    fh.write(('%r %r %r\n' % tuple(float(x) for x in v)).encode('ascii'))
                for f in self.faces:
                    fh.write(('3 %d %d %d\n' % tuple(f)).encode('ascii'))

    def on_device(self, device):
        """(vertices float64 [V,3], faces int32 [F,3], face normals float64 [F,3], MeshBVH) on ``device`` (a GPU), built once."""
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('mesh ray casting needs a GPU (device %s): depth_correction_amd has no CPU path' % device)
        if not torch.cuda.is_available():
            raise RuntimeError('mesh ray casting needs a GPU, and torch sees none: depth_correction_amd has no CPU path')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            from .ops import bvh_build
            v = torch.as_tensor(self.vertices, device=device)
            f = torch.as_tensor(self.faces, device=device)
            n = torch.as_tensor(self.face_normals(), device=device)
            lo, hi = self.bounds
            got = (v, f, n, bvh_build(v, f, np.concatenate([lo, hi])))
            self._device[device] = got
        return got


# ---- readers ------------------------------------------------------------------------------------------------------------------
def _fan(polys, n_verts, where):
    """Fan triangulation (v0, vi, vi+1) of a list of index lists; raises on short polygons and out-of-range indices."""
    if isinstance(polys, np.ndarray) and polys.ndim == 2 and polys.shape[1] >= 3:        # every polygon of one size
        k = polys.shape[1]
        f = np.stack([np.repeat(polys[:, :1], k - 2, axis=1), polys[:, 1:-1], polys[:, 2:]], axis=-1).reshape(-1, 3).astype(np.int64)
        if f.min() < 0 or f.max() >= n_verts:
            raise ValueError('%s: face index out of range [0, %d)' % (where, n_verts))
        return f
    tris = []
    for k, p in enumerate(polys):
        if len(p) < 3:
            raise ValueError('%s: face %d has %d vertices (at least 3 needed)' % (where, k, len(p)))
        for i in range(1, len(p) - 1):
            tris.append((p[0], p[i], p[i + 1]))
    if not tris:
        raise ValueError('%s: no faces' % where)
    f = np.asarray(tris, dtype=np.int64)
    if f.min() < 0 or f.max() >= n_verts:
        raise ValueError('%s: face index out of range [0, %d)' % (where, n_verts))
    return f


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_type(name, where):
    if name not in _PLY_TYPES:
        raise ValueError('%s: unknown PLY property type %r' % (where, name))
    return _PLY_TYPES[name]


def read_ply(path):
    """(vertices float64 [V,3], faces int64 [F,3]) of a PLY file: ascii or binary_little_endian, vertex x y z float or double,
    face vertex_indices / vertex_index as a list; other elements and properties are skipped, polygons fan-triangulated."""
    with open(path, 'rb') as fh:
        data = fh.read()
    where = os.path.basename(path)
    if not data.startswith(b'ply'):
        raise ValueError('%s: not a PLY file (no "ply" magic)' % where)
    end = data.find(b'end_header')
    if end < 0:
        raise ValueError('%s: PLY header has no end_header' % where)
    body_start = data.index(b'\n', end) + 1
    header = data[:end].decode('ascii', errors='replace').splitlines()
    fmt, elements = None, []
    for line in header[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property':
            if not elements:
                raise ValueError('%s: property before any element' % where)
            if tok[1] == 'list':
                elements[-1][2].append((tok[4], ('list', _ply_type(tok[2], where), _ply_type(tok[3], where))))
            else:
                elements[-1][2].append((tok[2], _ply_type(tok[1], where)))
        else:
            raise ValueError('%s: unexpected PLY header line %r' % (where, line))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError('%s: PLY format %r is not supported (ascii or binary_little_endian)' % (where, fmt))
    names = [e[0] for e in elements]
    if 'vertex' not in names or 'face' not in names:
        raise ValueError('%s: PLY needs a vertex and a face element' % where)
    if fmt == 'ascii':
        values = _ply_ascii(data[body_start:], elements, where)
    else:
        values = _ply_binary(data[body_start:], elements, where)
    vert = values['vertex']
    for c in 'xyz':
        if c not in vert:
            raise ValueError('%s: vertex element has no %r property' % (where, c))
    verts = np.stack([np.asarray(vert[c], dtype=np.float64) for c in 'xyz'], axis=1)
    face = values['face']
    key = 'vertex_indices' if 'vertex_indices' in face else ('vertex_index' if 'vertex_index' in face else None)
    if key is None:
        raise ValueError('%s: face element has no vertex_indices / vertex_index list' % where)
    return verts, _fan(face[key], verts.shape[0], where)


def _ply_ascii(body, elements, where):
    tok = body.split()
    pos, out = 0, {}
    for name, count, props in elements:
        cols = {p: [] for p, _ in props}
        if all(not isinstance(t, tuple) for _, t in props):
            width = len(props)
            if pos + width * count > len(tok):
                raise ValueError('%s: PLY body ends inside element %r' % (where, name))
            try:
                block = np.asarray(tok[pos:pos + width * count], dtype=np.float64).reshape(count, width)
            except ValueError:
                raise ValueError('%s: malformed PLY body in element %r' % (where, name))
            pos += width * count
            out[name] = {p: block[:, i] for i, (p, _) in enumerate(props)}
            continue
        try:
            for _ in range(count):
                for p, t in props:
                    if isinstance(t, tuple):
                        n = int(tok[pos])
                        cols[p].append([int(x) for x in tok[pos + 1:pos + 1 + n]])
                        if len(cols[p][-1]) != n:
                            raise IndexError
                        pos += 1 + n
                    else:
                        cols[p].append(float(tok[pos]))
                        pos += 1
        except (IndexError, ValueError):
            raise ValueError('%s: malformed PLY body in element %r' % (where, name))
        out[name] = cols
    return out


def _ply_binary(body, elements, where):
    pos, out = 0, {}
    for name, count, props in elements:
        if all(not isinstance(t, tuple) for _, t in props):
            dt = np.dtype([(p, '<' + t) for p, t in props])
            if pos + dt.itemsize * count > len(body):
                raise ValueError('%s: PLY body ends inside element %r' % (where, name))
            arr = np.frombuffer(body, dtype=dt, count=count, offset=pos)
            pos += dt.itemsize * count
            out[name] = {p: arr[p] for p, _ in props}
            continue
        # rows with lists: a fast path when every list has the length of the first one, else row by row
        cols = _ply_binary_uniform(body, pos, count, props)
        if cols is not None:
            out[name], pos = cols
            continue
        cols = {p: [] for p, _ in props}
        try:
            for _ in range(count):
                for p, t in props:
                    if isinstance(t, tuple):
                        n = int(np.frombuffer(body, dtype='<' + t[1], count=1, offset=pos)[0])
                        pos += np.dtype(t[1]).itemsize
                        cols[p].append(np.frombuffer(body, dtype='<' + t[2], count=n, offset=pos).astype(np.int64).tolist())
                        pos += n * np.dtype(t[2]).itemsize
                    else:
                        cols[p].append(float(np.frombuffer(body, dtype='<' + t, count=1, offset=pos)[0]))
                        pos += np.dtype(t).itemsize
        except ValueError:
            raise ValueError('%s: PLY body ends inside element %r' % (where, name))
        out[name] = cols
    return out


def _ply_binary_uniform(body, pos, count, props):
    fields, lists = [], []
    first = pos
    for p, t in props:
        if isinstance(t, tuple):
            if first + np.dtype(t[1]).itemsize > len(body):
                return None
            n = int(np.frombuffer(body, dtype='<' + t[1], count=1, offset=first)[0])
            fields += [(p + '__n', '<' + t[1]), (p, '<' + t[2], (n,))] if n else [(p + '__n', '<' + t[1])]
            lists.append((p, n))
            first += np.dtype(t[1]).itemsize + n * np.dtype(t[2]).itemsize
        else:
            fields.append((p, '<' + t))
            first += np.dtype(t).itemsize
    dt = np.dtype(fields)
    if count == 0 or pos + dt.itemsize * count > len(body):
        return None
    arr = np.frombuffer(body, dtype=dt, count=count, offset=pos)
    for p, n in lists:
        if not (arr[p + '__n'] == n).all():
            return None
    cols = {}
    for p, t in props:
        if isinstance(t, tuple):
            n = dict(lists)[p]
            cols[p] = arr[p].astype(np.int64).reshape(count, n) if n else [[] for _ in range(count)]
        else:
            cols[p] = arr[p]
    return cols, pos + dt.itemsize * count


def read_obj(path):
    """(vertices float64 [V,3], faces int64 [F,3]) of a Wavefront OBJ file: ``v`` and ``f`` lines (``i``, ``i/j``, ``i/j/k``,
    ``i//k``; negative indices count back from the last vertex read); polygons fan-triangulated, other lines skipped."""
    where = os.path.basename(path)
    verts, polys = [], []
    with open(path, 'r', errors='replace') as fh:
        for num, line in enumerate(fh, 1):
            tok = line.split()
            if not tok:
                continue
            try:
                if tok[0] == 'v':
                    verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                elif tok[0] == 'f':
                    poly = []
                    for t in tok[1:]:
                        i = int(t.split('/')[0])
                        if i == 0:
                            raise ValueError
                        poly.append(i - 1 if i > 0 else len(verts) + i)
                    polys.append(poly)
            except (IndexError, ValueError):
                raise ValueError('%s:%d: malformed OBJ line %r' % (where, num, line.rstrip()))
    if not verts:
        raise ValueError('%s: no vertices' % where)
    return np.asarray(verts, dtype=np.float64), _fan(polys, len(verts), where)


def load_mesh(path):
    """TriangleMesh of a .ply or .obj file (utils.load_mesh of the reference, :241-250)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.ply':
        v, f = read_ply(path)
    elif ext == '.obj':
        v, f = read_obj(path)
    else:
        raise ValueError('Supported mesh formats are *.obj or *.ply, got %s' % path)
    return TriangleMesh(v, f)


# ---- procedural meshes ----------------------------------------------------------------------------------------------------------
def _merge(parts):
    """One mesh of (vertices, faces) parts, vertices with identical coordinates merged (so that shared edges are shared)."""
    verts = np.concatenate([v for v, _ in parts])
    offs = np.cumsum([0] + [v.shape[0] for v, _ in parts[:-1]])
    faces = np.concatenate([f + o for (_, f), o in zip(parts, offs)])
    uniq, inv = np.unique(verts, axis=0, return_inverse=True)
    return uniq, inv.reshape(-1)[faces]


def _box_faces(center, half, cell, inward):
    """The six sides of an axis-aligned box as cell-sized quads (2 triangles each), normals inward or outward."""
    c, h = np.asarray(center, np.float64), np.asarray(half, np.float64)
    ticks = [np.linspace(c[a] - h[a], c[a] + h[a], max(1, int(math.ceil(2 * h[a] / cell))) + 1) for a in range(3)]
    parts = []
    for a in range(3):
        u, v = [b for b in range(3) if b != a]
        for side in (-1.0, 1.0):
            gu, gv = np.meshgrid(ticks[u], ticks[v], indexing='ij')
            pts = np.zeros(gu.shape + (3,))
            pts[..., u], pts[..., v], pts[..., a] = gu, gv, c[a] + side * h[a]
            nu, nv = gu.shape
            idx = np.arange(nu * nv).reshape(nu, nv)
            q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
            tri = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])
            # (u, v, a) is a right-handed cycle of axes iff v == (u + 1) % 3: then (q10 - q00) x (q11 - q00) points along +a
            sign = 1.0 if v == (u + 1) % 3 else -1.0
            if (sign * side > 0) == inward:           # normal along +side*a is outward: flip when inward is asked, and vice versa
                tri = tri[:, ::-1]
            parts.append((pts.reshape(-1, 3), tri))
    return parts


def box_mesh(center, half_extents, cell=None, inward=False):
    """Closed axis-aligned box (outward normals unless ``inward``), sides tessellated into ``cell``-sized quads."""
    cell = float(cell) if cell else 2.0 * float(np.max(half_extents))
    return TriangleMesh(*_merge(_box_faces(center, half_extents, cell, inward)))


def room_mesh(half_extents=(10.0, 7.0, 2.0), cell=1.0, pillars=()):
    """A closed box room centred at the origin with inward-facing normals, walls tessellated into ``cell``-sized quads (shared
    vertices, so the surface is watertight), and optional box pillars ``(center, half_extents)`` with outward faces."""
    parts = _box_faces((0.0, 0.0, 0.0), half_extents, float(cell), inward=True)
    for center, half in pillars:
        parts += _box_faces(center, half, float(cell), inward=False)
    return TriangleMesh(*_merge(parts))


def grid_terrain_mesh(n, extent=200.0, amplitude=3.0):
    """Height field z = amplitude sin(x / 7) cos(y / 11) on an n x n grid of cells over [-extent/2, extent/2]^2: 2 n^2 triangles
    with upward normals."""
    t = np.linspace(-extent / 2.0, extent / 2.0, n + 1)
    x, y = np.meshgrid(t, t, indexing='ij')
    z = amplitude * np.sin(x / 7.0) * np.cos(y / 11.0)
    verts = np.stack([x, y, z], -1).reshape(-1, 3)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])
    return TriangleMesh(verts, faces)
