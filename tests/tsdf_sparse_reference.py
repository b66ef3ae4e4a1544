"""numpy oracle of the sparse TSDF volumes: block table, slots, pool, stats and surface-nets extraction, written from the rule of DESIGN
"Sparse TSDF volumes" (not from the kernels or the package) and vectorised over rays.

Lattice: origin og, voxel size a, truncation tau, h = a / 2, K = ceil(tau / h); a sample at p lies in voxel i = floor((p - og) / a), any
integer, with the centre og + (i + 0.5) a.  Voxel i lies in block b = i >> 3 at the local index ((lx 8) + ly) 8 + lz; blocks are valid in
[-2^20, 2^20) and have the key ((bx + 2^20) << 42) | ((by + 2^20) << 21) | (bz + 2^20).  keys [n_blocks] ascend, slots [n_blocks] are the
pool slots, the pool is sum int64 [capacity, 512] and count int32 [capacity, 512].

``DenseWindow`` anchors this oracle to tests/tsdf_reference.py: a dense Volume with the SAME origin whose box is [0, hi), read at the
indices [lo, hi) -- the indices are offset, never the origin, whose shift would round.
"""
import math

import numpy as np

import tsdf_reference as R

ONE = 2.0 ** 20
B = 8
BV = 512
RANGE = 2 ** 20
STATS = 5                     # rays used, rays skipped, samples outside, visits, visits dropped


def k_steps(trunc, voxel):
    return int(math.ceil(trunc / (voxel / 2.0)))


def block_key(b):
    """uint64 keys of the block coordinates b int64 [..., 3]."""
    b = np.asarray(b, np.int64) + RANGE
    return (b[..., 0].astype(np.uint64) << np.uint64(42)) | (b[..., 1].astype(np.uint64) << np.uint64(21)) | b[..., 2].astype(np.uint64)


def key_block(keys):
    keys = np.asarray(keys, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(keys >> np.uint64(42)).astype(np.int64), ((keys >> np.uint64(21)) & m).astype(np.int64), (keys & m).astype(np.int64)],
                    axis=-1) - RANGE


class SparseVolume:
    def __init__(self, voxel, trunc=None, origin=(0.0, 0.0, 0.0), capacity=64):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.voxel = float(voxel)
        self.trunc = 3.0 * self.voxel if trunc is None else float(trunc)
        self.capacity = int(capacity)
        self.keys = np.zeros(0, np.uint64)
        self.slots = np.zeros(0, np.int32)
        self.sum = np.zeros((self.capacity, BV), np.int64)
        self.count = np.zeros((self.capacity, BV), np.int32)
        self.stats = np.zeros(STATS, np.int64)
        self.info = np.zeros(2, np.int64)

    @property
    def n_blocks(self):
        return self.keys.shape[0]

    def grow(self, capacity):
        """The same table and pool with room for ``capacity`` blocks."""
        assert capacity >= self.capacity
        s, c = np.zeros((capacity, BV), np.int64), np.zeros((capacity, BV), np.int32)
        s[:self.capacity], c[:self.capacity] = self.sum, self.count
        self.sum, self.count, self.capacity = s, c, int(capacity)

    def find(self, keys):
        """Positions of ``keys`` in the table, -1 where missing."""
        keys = np.asarray(keys, np.uint64)
        pos = np.searchsorted(self.keys, keys)
        ok = pos < self.n_blocks
        ok[ok] = self.keys[pos[ok]] == keys[ok]
        return np.where(ok, pos, -1)

    def window(self, lo, dims):
        """(sum, count) [nx, ny, nz] of the voxels lo .. lo + dims; a voxel without a block holds 0."""
        idx = np.stack(np.meshgrid(*[np.arange(l, l + n) for l, n in zip(lo, dims)], indexing='ij'), axis=-1).reshape(-1, 3).astype(np.int64)
        pos = self.find(block_key(idx >> 3))
        local = ((idx[:, 0] & 7) * B + (idx[:, 1] & 7)) * B + (idx[:, 2] & 7)
        s, c = np.zeros(idx.shape[0], np.int64), np.zeros(idx.shape[0], np.int32)
        have = pos >= 0
        s[have] = self.sum[self.slots[pos[have]], local[have]]
        c[have] = self.count[self.slots[pos[have]], local[have]]
        return s.reshape(dims), c.reshape(dims)


def visits(vol, vps, dirs, depth, pose=None, mask=None, min_depth=0.0, max_range=None, **_):
    """The sample loop of every ray: (tally [used, skipped, outside], ray index, voxel int64 [m, 3], q int64 [m]) of the visits that add,
    in ascending k."""
    dirs = np.asarray(dirs).astype(np.float64).reshape(-1, 3)
    n = dirs.shape[0]
    vps = np.broadcast_to(np.asarray(vps).astype(np.float64).reshape(-1, 3), (n, 3))
    d = np.asarray(depth).astype(np.float64).reshape(n)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0
    tally = np.zeros(3, np.int64)
    out_ray, out_vox, out_q = [], [], []
    with np.errstate(all='ignore'):
        if pose is not None:
            T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
            o = np.stack([((T[r, 0] * vps[:, 0] + T[r, 1] * vps[:, 1]) + T[r, 2] * vps[:, 2]) + T[r, 3] for r in range(3)], axis=1)
            u = np.stack([(T[r, 0] * dirs[:, 0] + T[r, 1] * dirs[:, 1]) + T[r, 2] * dirs[:, 2] for r in range(3)], axis=1)
        else:
            o, u = vps, dirs
        max_range = np.inf if max_range is None else float(max_range)
        use = keep & np.isfinite(o).all(axis=1) & np.isfinite(u).all(axis=1) & np.isfinite(d) & ~(d <= min_depth) & ~(d > max_range)
        tally[0], tally[1] = int(use.sum()), int(n - use.sum())
        ray = np.nonzero(use)[0]
        o, u, d = o[use], u[use], d[use]
        m = d.shape[0]
        a, tau, og = vol.voxel, vol.trunc, vol.origin
        h = a / 2.0
        K = k_steps(tau, a)
        last = np.full((m, 3), np.iinfo(np.int64).min, np.int64)
        lim = float(RANGE * B)
        for k in range(-K, K + 1):
            t = d + float(k) * h
            act = np.nonzero(t > 0.0)[0]
            if act.size == 0:
                continue
            g = np.stack([np.floor(((o[act, ax] + t[act] * u[act, ax]) - og[ax]) / a) for ax in range(3)], axis=1)
            inside = ((g >= -lim) & (g < lim)).all(axis=1)
            tally[2] += int((~inside).sum())
            act, i = act[inside], g[inside].astype(np.int64)
            new = (i != last[act]).any(axis=1)
            act, i = act[new], i[new]
            last[act] = i
            c = og + (i.astype(np.float64) + 0.5) * a
            s = d[act] - ((u[act, 0] * (c[:, 0] - o[act, 0]) + u[act, 1] * (c[:, 1] - o[act, 1])) + u[act, 2] * (c[:, 2] - o[act, 2]))
            add = s >= -tau
            out_ray.append(ray[act[add]])
            out_vox.append(i[add])
            out_q.append(np.rint(np.minimum(s[add], tau) / tau * ONE).astype(np.int64))
    if not out_ray:
        return tally, np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    return tally, np.concatenate(out_ray), np.concatenate(out_vox), np.concatenate(out_q)


def allocate(vol, **rays):
    """Admits the wanted blocks in ascending key order into the slots n_blocks, n_blocks + 1, ... until the capacity."""
    _, _, vox, _ = visits(vol, **rays)
    want = np.unique(block_key(vox >> 3))
    want = want[vol.find(want) < 0]
    admit = want[:max(0, vol.capacity - vol.n_blocks)]
    keys = np.concatenate([vol.keys, admit])
    slots = np.concatenate([vol.slots, np.arange(vol.n_blocks, vol.n_blocks + admit.size, dtype=np.int32)])
    order = np.argsort(keys, kind='stable')
    vol.keys, vol.slots = keys[order], slots[order]
    vol.info[:] = vol.n_blocks, want.size - admit.size
    return vol


def ray_blocks(vol, **rays):
    """The most distinct blocks the adding visits of any one ray meet."""
    _, ray, vox, _ = visits(vol, **rays)
    if ray.size == 0:
        return 0
    pairs = np.unique(np.stack([ray.astype(np.uint64), block_key(vox >> 3)], axis=1), axis=0)
    return int(np.bincount(pairs[:, 0].astype(np.int64)).max())


def integrate(vol, **rays):
    tally, _, vox, q = visits(vol, **rays)
    pos = vol.find(block_key(vox >> 3))
    have = pos >= 0
    local = ((vox[:, 0] & 7) * B + (vox[:, 1] & 7)) * B + (vox[:, 2] & 7)
    np.add.at(vol.sum, (vol.slots[pos[have]], local[have]), q[have])
    np.add.at(vol.count, (vol.slots[pos[have]], local[have]), 1)
    vol.stats += [tally[0], tally[1], tally[2], q.size, int((~have).sum())]
    return vol


def fuse(vol, **rays):
    """allocate, growing the pool until nothing is refused, then integrate."""
    allocate(vol, **rays)
    while vol.info[1] > 0:
        vol.grow(max(2 * vol.capacity, vol.capacity + int(vol.info[1])))
        allocate(vol, **rays)
    return integrate(vol, **rays)


class DenseWindow(R.Volume):
    """The dense oracle's volume over the index box [0, hi) of the same lattice (same origin), read at [lo, hi)."""

    def __init__(self, sparse, lo, dims):
        self.lo = tuple(int(v) for v in lo)
        assert min(self.lo) >= 0
        R.Volume.__init__(self, sparse.origin, tuple(l + n for l, n in zip(self.lo, dims)), sparse.voxel, sparse.trunc)

    def read(self):
        sl = tuple(slice(l, None) for l in self.lo)
        return self.sum.reshape(self.dims)[sl], self.count.reshape(self.dims)[sl]


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def _gather(vol, arrays, fill):
    """Per block in key order, the values of ``arrays`` [capacity-like, 8, 8, 8] (indexed by position) at the local points -1 .. 8: [P,
    10, 10, 10], ``fill`` where the block is missing."""
    P = vol.n_blocks
    b = key_block(vol.keys)
    out = [np.full((P, 10, 10, 10), f, a.dtype) for a, f in zip(arrays, fill)]
    rng = {-1: (slice(0, 1), slice(7, 8)), 0: (slice(1, 9), slice(0, 8)), 1: (slice(9, 10), slice(0, 1))}
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                nb = b + (dx, dy, dz)
                ok = ((nb >= -RANGE) & (nb < RANGE)).all(axis=1)
                pos = np.full(P, -1, np.int64)
                if ok.any():
                    pos[ok] = vol.find(block_key(nb[ok]))
                have = pos >= 0
                dst = (rng[dx][0], rng[dy][0], rng[dz][0])
                src = (rng[dx][1], rng[dy][1], rng[dz][1])
                for o, a in zip(out, arrays):
                    o[(have,) + dst] = a[(pos[have],) + src]
    return out


def extract(vol, min_count=1):
    """(vertices f64 [Nv,3], faces int32 [Nf,3]): vertices ascend in (block key, local cell), faces in (block key of q, local q, e)."""
    P = vol.n_blocks
    if P == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    s = vol.sum[vol.slots].reshape(P, B, B, B)
    c = vol.count[vol.slots].reshape(P, B, B, B)
    obs_b = c >= min_count
    f_b = np.zeros(s.shape)
    f_b[obs_b] = s[obs_b].astype(np.float64) / (c[obs_b].astype(np.float64) * ONE)
    obs, ins, f = _gather(vol, [obs_b, s < 0, f_b], [False, False, 0.0])

    def corner(arr, k):
        """arr at the corner k of the cells 0 .. 7 (local points; index + 1 in the gathered arrays)."""
        bx, by, bz = k & 1, (k >> 1) & 1, k >> 2
        return arr[:, 1 + bx:9 + bx, 1 + by:9 + by, 1 + bz:9 + bz]

    all_obs = np.ones((P, 8, 8, 8), bool)
    n_in = np.zeros((P, 8, 8, 8), np.int64)
    for k in range(8):
        all_obs &= corner(obs, k)
        n_in += corner(ins, k)
    active = all_obs & (n_in > 0) & (n_in < 8)
    acc = np.zeros(active.shape + (3,))
    cnt = np.zeros(active.shape)
    with np.errstate(all='ignore'):
        for ea, eb in R.EDGES:
            cross = active & (corner(ins, ea) != corner(ins, eb))
            fa, fb = corner(f, ea), corner(f, eb)
            r = fa / (fa - fb)
            for ax in range(3):
                ca, cb = float((ea >> ax) & 1), float((eb >> ax) & 1)
                acc[..., ax] = np.where(cross, acc[..., ax] + (ca + r * (cb - ca)), acc[..., ax])
            cnt += cross
        loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing='ij'), axis=-1)
        xyz = (key_block(vol.keys)[:, None, None, None, :] * 8 + loc[None]).astype(np.float64)
        vert = vol.origin + ((xyz + 0.5) + acc / cnt[..., None]) * vol.voxel
    vertices = np.ascontiguousarray(vert[active])
    ids = np.full(active.shape, -1, np.int64)
    ids[active] = np.arange(vertices.shape[0])
    idg, = _gather(vol, [ids], [-1])                                 # ids of the cells -1 .. 8 around each block
    emit = np.zeros((P, 8, 8, 8, 3), bool)
    quads = np.zeros((P, 8, 8, 8, 3, 4), np.int64)
    own = (slice(None), slice(1, 9), slice(1, 9), slice(1, 9))
    for e in range(3):
        b_, c_ = (e + 1) % 3, (e + 2) % 3
        nxt = [slice(None), slice(1, 9), slice(1, 9), slice(1, 9)]
        nxt[1 + e] = slice(2, 10)
        nxt = tuple(nxt)
        cross = obs[own] & obs[nxt] & (ins[own] != ins[nxt])
        q = []
        for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            sl = [slice(None), slice(1, 9), slice(1, 9), slice(1, 9)]
            sl[1 + b_] = slice(1 + db, 9 + db)
            sl[1 + c_] = slice(1 + dc, 9 + dc)
            q.append(idg[tuple(sl)])
        q = np.stack(q, axis=-1)
        emit[..., e] = cross & (q >= 0).all(axis=-1)
        quads[..., e, :] = np.where(ins[own][..., None], q, q[..., ::-1])
    quads = quads[emit]
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, faces


def canonical_mesh(vertices, faces):
    """The mesh with its vertex rows sorted lexicographically, its faces renumbered and sorted: equal meshes give equal arrays."""
    vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    order = np.lexsort((vertices[:, 2], vertices[:, 1], vertices[:, 0]))
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    f = rank[faces] if faces.size else faces
    if f.size:
        f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    return vertices[order], f
