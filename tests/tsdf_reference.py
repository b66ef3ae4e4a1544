"""numpy oracle of the surface reconstruction: TSDF fusion of rays and surface-nets extraction, written from the rule of DESIGN
"Surface reconstruction" (not from the kernels) and vectorised over rays, so that 2 10^4 rays take seconds.

numpy rounds every product and sum on its own, which is the rule's arithmetic; the sums are int64, so `np.add.at` in any order gives
the bits the device's atomics give.

Volume: minimum corner `origin`, voxel size a, dims (nx, ny, nz); voxel (ix, iy, iz) has the linear index (ix ny + iy) nz + iz and the
centre origin + (i + 0.5) a; truncation tau, step h = a / 2, K = ceil(tau / h).
"""
import math

import numpy as np

ONE = 2.0 ** 20
MAX_CARVE = 2.0 ** 30


def k_steps(trunc, voxel):
    return int(math.ceil(trunc / (voxel / 2.0)))


class Volume:
    def __init__(self, origin, dims, voxel, trunc=None):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.dims = tuple(int(n) for n in dims)
        self.voxel = float(voxel)
        self.trunc = 3.0 * self.voxel if trunc is None else float(trunc)
        v = self.dims[0] * self.dims[1] * self.dims[2]
        self.sum = np.zeros(v, np.int64)
        self.count = np.zeros(v, np.int32)
        self.stats = np.zeros(4, np.int64)       # rays used, rays skipped, samples outside the grid, visits

    def centre(self, axis, i):
        return self.origin[axis] + (i.astype(np.float64) + 0.5) * self.voxel


def integrate(vol, vps, dirs, depth, pose=None, mask=None, min_depth=0.0, max_range=None, carve_from=None):
    """Adds the rays (sensor frame; f32 or f64, widened exactly) to ``vol``; vps may be one row for all rays."""
    dirs = np.asarray(dirs).astype(np.float64).reshape(-1, 3)
    n = dirs.shape[0]
    vps = np.broadcast_to(np.asarray(vps).astype(np.float64).reshape(-1, 3), (n, 3))
    d = np.asarray(depth).astype(np.float64).reshape(n)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0
    with np.errstate(all='ignore'):
        if pose is not None:
            T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
            o = np.stack([((T[r, 0] * vps[:, 0] + T[r, 1] * vps[:, 1]) + T[r, 2] * vps[:, 2]) + T[r, 3] for r in range(3)], axis=1)
            u = np.stack([(T[r, 0] * dirs[:, 0] + T[r, 1] * dirs[:, 1]) + T[r, 2] * dirs[:, 2] for r in range(3)], axis=1)
        else:
            o, u = vps, dirs
        max_range = np.inf if max_range is None else float(max_range)
        finite = np.isfinite(o).all(axis=1) & np.isfinite(u).all(axis=1) & np.isfinite(d)
        use = keep & finite & ~(d <= min_depth) & ~(d > max_range)
        vol.stats[0] += int(use.sum())
        vol.stats[1] += int(n - use.sum())
        o, u, d = o[use], u[use], d[use]
        m = d.shape[0]
        a, tau, og = vol.voxel, vol.trunc, vol.origin
        h = a / 2.0
        K = k_steps(tau, a)
        k_lo = np.full(m, -K, np.int64)
        if carve_from is not None and carve_from >= 0.0:
            c = np.minimum(np.floor((d - float(carve_from)) / h), MAX_CARVE)
            k_lo = -np.maximum(K, np.where(c > 0.0, c, 0.0).astype(np.int64))
        last = np.full(m, -1, np.int64)
        nx, ny, nz = vol.dims
        for k in range(int(k_lo.min()) if m else 0, K + 1):
            t = d + float(k) * h
            act = np.nonzero((k >= k_lo) & (t > 0.0))[0]
            if act.size == 0:
                continue
            ta = t[act]
            g = [np.floor(((o[act, ax] + ta * u[act, ax]) - og[ax]) / a) for ax in range(3)]
            inside = (g[0] >= 0) & (g[0] < nx) & (g[1] >= 0) & (g[1] < ny) & (g[2] >= 0) & (g[2] < nz)
            vol.stats[2] += int((~inside).sum())
            act = act[inside]
            i = [gg[inside].astype(np.int64) for gg in g]
            v = (i[0] * ny + i[1]) * nz + i[2]
            new = v != last[act]
            act, v, i = act[new], v[new], [ii[new] for ii in i]
            last[act] = v
            c = [vol.centre(ax, i[ax]) for ax in range(3)]
            s = d[act] - ((u[act, 0] * (c[0] - o[act, 0]) + u[act, 1] * (c[1] - o[act, 1])) + u[act, 2] * (c[2] - o[act, 2]))
            add = s >= -tau
            q = np.rint(np.minimum(s[add], tau) / tau * ONE).astype(np.int64)
            np.add.at(vol.sum, v[add], q)
            np.add.at(vol.count, v[add], 1)
            vol.stats[3] += int(add.sum())
    return vol


def values(vol, min_count=1):
    """f = sum / (count 2^20) as [nx, ny, nz], NaN where unobserved."""
    obs = vol.count >= min_count
    f = np.full(vol.sum.shape, np.nan)
    f[obs] = vol.sum[obs].astype(np.float64) / (vol.count[obs].astype(np.float64) * ONE)
    return f.reshape(vol.dims)


EDGES = ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))


def extract(vol, min_count=1):
    """(vertices f64 [Nv,3], faces int32 [Nf,3]) of the surface nets on the lattice of voxel centres."""
    nx, ny, nz = vol.dims
    obs = (vol.count >= min_count).reshape(vol.dims)
    ins = (vol.sum < 0).reshape(vol.dims)
    f = np.nan_to_num(values(vol, min_count))

    def corner(arr, c):
        bx, by, bz = c & 1, (c >> 1) & 1, c >> 2
        return arr[bx:nx - 1 + bx, by:ny - 1 + by, bz:nz - 1 + bz]

    all_obs = np.ones((nx - 1, ny - 1, nz - 1), bool)
    n_in = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        all_obs &= corner(obs, c)
        n_in += corner(ins, c)
    active = all_obs & (n_in > 0) & (n_in < 8)
    acc = np.zeros(active.shape + (3,))
    cnt = np.zeros(active.shape)
    with np.errstate(all='ignore'):
        for ea, eb in EDGES:
            cross = active & (corner(ins, ea) != corner(ins, eb))
            fa, fb = corner(f, ea), corner(f, eb)
            r = fa / (fa - fb)
            for ax in range(3):
                ca, cb = float((ea >> ax) & 1), float((eb >> ax) & 1)
                acc[..., ax] = np.where(cross, acc[..., ax] + (ca + r * (cb - ca)), acc[..., ax])
            cnt += cross
        xyz = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing='ij'), axis=-1).astype(np.float64)
        vert = vol.origin + ((xyz + 0.5) + acc / cnt[..., None]) * vol.voxel
    vertices = np.ascontiguousarray(vert[active])                  # C order of the cells = ascending cell index
    ids = np.full(active.shape, -1, np.int64)
    ids[active] = np.arange(vertices.shape[0])
    idp = np.full((nx + 1, ny + 1, nz + 1), -1, np.int64)           # idp[cell + 1]; cells that do not exist hold -1
    idp[1:nx, 1:ny, 1:nz] = ids
    dims = (nx, ny, nz)

    def around(off):
        return idp[tuple(slice(1 + o, 1 + o + n) for o, n in zip(off, dims))]

    emit = np.zeros(dims + (3,), bool)
    quads = np.zeros(dims + (3, 4), np.int64)
    for e in range(3):
        b, c = (e + 1) % 3, (e + 2) % 3
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        lo[e], hi[e] = slice(0, dims[e] - 1), slice(1, dims[e])
        lo, hi = tuple(lo), tuple(hi)
        cross = np.zeros(dims, bool)
        cross[lo] = obs[lo] & obs[hi] & (ins[lo] != ins[hi])
        q = []
        for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            off = [0, 0, 0]
            off[b], off[c] = db, dc
            q.append(around(off))
        q = np.stack(q, axis=-1)
        emit[..., e] = cross & (q >= 0).all(axis=-1)
        quads[..., e, :] = np.where(ins[..., None], q, q[..., ::-1])
    quads = quads[emit]                                             # C order = ascending (index of q, e)
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, faces


# ---- mesh properties used by the tests -------------------------------------------------------------------------------------------
def face_normals(vertices, faces):
    a, b, c = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    return np.cross(b - a, c - a)


def is_closed_manifold(faces):
    """Every directed edge occurs once and its reverse occurs once."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * (int(faces.max()) + 1) + e[:, 1]
    rev = e[:, 1] * (int(faces.max()) + 1) + e[:, 0]
    return np.unique(key).size == key.size and np.array_equal(np.sort(key), np.sort(rev))


def euler_characteristic(vertices, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64), axis=1)
    return vertices.shape[0] - np.unique(e, axis=0).shape[0] + faces.shape[0]
