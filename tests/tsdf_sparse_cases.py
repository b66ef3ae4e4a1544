"""The designed cases of the sparse TSDF volumes, shared by the host tests (host build against oracle, hand-written figures) and the GPU
tests (device against oracle).  Unit voxels at the origin, tau = 2 (h = 0.5, K = 4); rays run along +z through voxel centres, as in
tests/tsdf_cases.py, so that the figures can be written by hand.

An integration case is (name, capacity, steps); a step is (kind, payload):
    ('fuse', batch)        allocate then integrate, at the capacity as it is (no growth)
    ('allocate', batch)    allocate alone
    ('integrate', batch)   integrate alone
    ('grow', capacity)     the same table and pool with more room
and a batch is a dict of tsdf_cases.batch without carving.  After every step the whole state is compared: keys, slots, n_blocks, sum,
count, stats, info.

An extraction case is (name, volume, blocks, min_count): blocks = [(block coordinate, sum [8,8,8], count [8,8,8])] in the order of their
slots.
"""
import numpy as np

import tsdf_cases as D
import tsdf_sparse_reference as S

VOLUME = dict(voxel=1.0, trunc=2.0, origin=(0.0, 0.0, 0.0))
Q = 2 ** 20
EDGE = 2 ** 23                                           # the first voxel index out of range


def z_ray(depth, x=1.5, y=1.5, z0=0.0, **kw):
    return D.z_ray(depth, x=x, y=y, z0=z0, **kw)


def many_rays(n, dtype=np.float64):
    """n distinct rays along +z over a 16 x 16 voxel patch (2 x 2 blocks), ending at three depths."""
    j = np.arange(n)
    vps = np.stack([0.5 + j % 16, 0.5 + (j // 16) % 16, np.zeros(n)], axis=1)
    return D.batch(vps, np.tile([[0.0, 0.0, 1.0]], (n, 1)), 4.5 + 0.25 * (j % 3), dtype=dtype)


def three_blocks():
    return D.batch([[1.5, 1.5, 0.0], [9.5, 1.5, 0.0], [17.5, 1.5, 0.0]], [[0.0, 0.0, 1.0]] * 3, [4.5] * 3)


def integration_cases():
    cases = [
        ('crosses_z8', 4, [('fuse', z_ray(8.5))]),                              # voxels 6 .. 10: blocks (0,0,0) and (0,0,1)
        ('crosses_zero', 4, [('fuse', z_ray(4.5, z0=-6.0))]),                   # voxels -4 .. 0: voxel -1 is block -1, local 7
        ('below_minus_tau_alone', 4, [('fuse', z_ray(6.0))]),                   # voxel 8 meets s = -2.5: block (0,0,1) is not wanted
        ('new_keys_sort_first', 4, [('fuse', z_ray(4.5)), ('fuse', z_ray(4.5, x=-1.5, z0=-6.0))]),
        ('capacity_2_of_3', 2, [('fuse', three_blocks()), ('grow', 3), ('allocate', three_blocks())]),
        ('allocate_twice', 4, [('allocate', z_ray(8.5)), ('allocate', z_ray(8.5)), ('integrate', z_ray(8.5))]),
        ('one_block_queried_around', 4, [('fuse', z_ray(4.5)), ('integrate', D.batch([[-1.5, 1.5, 0.0], [9.5, 1.5, 0.0]], [[0.0, 0.0, 1.0]] * 2,
                                                                                      [4.5, 4.5]))]),
        ('edge_of_the_range', 4, [('fuse', z_ray(4.5, z0=float(EDGE - 4)))]),   # voxels 2^23 - 2, 2^23 - 1 kept, from 2^23 on outside
        ('lowest_block', 4, [('fuse', z_ray(4.5, z0=float(-EDGE - 5)))]),      # the end point at -2^23 - 0.5: the samples below -2^23 outside
    ]
    for n in (0, 1, 65, 257):
        cases.append(('rays_%d' % n, 8, [('fuse', many_rays(n))]))
    cases.append(('rays_65_f32', 8, [('fuse', many_rays(65, np.float32))]))
    for name, _, batches in D.integration_cases():
        if any(b['carve_from'] is not None for b in batches):
            continue
        cases.append(('dense_' + name, 8, [('fuse', b) for b in batches]))
    return cases


def dense_twins():
    """{sparse case name: the dense case's batches} of the designed dense rays, which lie in block (0, 0, 0) of the same lattice."""
    return {'dense_' + name: batches for name, _, batches in D.integration_cases() if all(b['carve_from'] is None for b in batches)}


def _filled(value=Q, count=1):
    return np.full((8, 8, 8), value, np.int64), np.full((8, 8, 8), count, np.int32)


def extraction_cases():
    cases = [('empty', VOLUME, [], 1)]
    # the voxel (7, 7, 7) of block (0, 0, 0) alone inside: the cell at local (7, 7, 7) has its corners in eight blocks
    eight = []
    for b in [(1, 1, 1), (0, 1, 0), (1, 0, 0), (0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)]:      # slots are not in key order
        s, c = _filled()
        if b == (0, 0, 0):
            s[7, 7, 7] = -Q // 2
        eight.append((b, s, c))
    cases.append(('corner_cell_in_eight_blocks', VOLUME, eight, 1))
    cases.append(('corner_cell_one_block_missing', VOLUME, [e for e in eight if e[0] != (1, 1, 1)], 1))
    # the voxel (8, 8, 3) inside: the edge (8, 8, 2) -> (8, 8, 3) has its four cells in four blocks
    four = []
    for b in [(1, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0)]:
        s, c = _filled()
        if b == (1, 1, 0):
            s[0, 0, 3] = -Q // 4
        four.append((b, s, c))
    cases.append(('edge_cells_in_four_blocks', dict(voxel=0.25, trunc=0.75, origin=(-1.0, 0.5, 2.0)), four, 1))
    # counts 2 in the blocks with x = 0 and 1 in the others: min_count = 2 leaves only what lies well inside the former
    two = [(b, s, np.full((8, 8, 8), 2 if b[0] == 0 else 1, np.int32)) for b, s, _ in eight]
    two = [(b, s * c, c) for b, s, c in two]
    two[3][1][3, 3, 3] = -Q
    cases.append(('min_count_1', VOLUME, two, 1))
    cases.append(('min_count_2', VOLUME, two, 2))
    rng = np.random.default_rng(9)
    blocks = [(-1, -1, -1), (0, -1, -1), (-1, 0, 0), (0, 0, 0), (0, 0, -1), (-1, 0, -1), (1, 0, 0)]
    rnd = [(b, rng.integers(-Q, Q, (8, 8, 8)).astype(np.int64), rng.integers(0, 4, (8, 8, 8)).astype(np.int32)) for b in blocks]
    cases.append(('random', dict(voxel=0.1, trunc=0.3, origin=(0.05, -0.02, 0.01)), rnd, 1))
    cases.append(('random_min_count_2', dict(voxel=0.1, trunc=0.3, origin=(0.05, -0.02, 0.01)), rnd, 2))
    return cases


# ---- what the host and the GPU tests do with a case ----------------------------------------------------------------------------------
def step_both(got, want, kind, payload):
    """One step of a case on the implementation ``got`` (allocate / integrate / grow) and on the oracle."""
    if kind == 'grow':
        got.grow(payload)
        want.grow(payload)
        return
    if kind in ('fuse', 'allocate'):
        got.allocate(payload)
        S.allocate(want, **payload)
    if kind in ('fuse', 'integrate'):
        got.integrate(payload)
        S.integrate(want, **payload)


def assert_invariant(want):
    """A block is in the table iff one of its voxels has count > 0 (no drop); the table ascends and the slots are a permutation."""
    assert want.stats[4] == 0
    assert (np.diff(want.keys.astype(object)) > 0).all()
    assert sorted(want.slots.tolist()) == list(range(want.n_blocks))
    used = want.count.sum(axis=1) > 0
    assert used[:want.n_blocks].all() and not used[want.n_blocks:].any()
    assert want.count.sum() == want.stats[3]


# ---- a random posed scene ----------------------------------------------------------------------------------------------------------
def random_scans(offset=(0.0, 0.0, 0.0)):
    """Two organised 16 x 64 scans as tests/test_gpu_tsdf.py builds them (posed, masked, with NaN rows and infinite depths), moved by
    ``offset``."""
    rng = np.random.default_rng(20)
    el = np.deg2rad(np.linspace(-40.0, 40.0, 16))[:, None]
    az = np.deg2rad(np.arange(64) * 360.0 / 64)[None, :]
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
    scans = []
    for s, (rpy, t) in enumerate((((0.05, -0.1, 0.3), (0.2, -0.1, 0.05)), ((-0.2, 0.15, -1.1), (-0.7, 0.6, -0.2)))):
        depth = 0.2 + 1.4 * rng.random(dirs.shape[0])
        depth[rng.integers(0, depth.size, 5)] = np.nan
        depth[rng.integers(0, depth.size, 3)] = np.inf
        d = dirs.copy()
        d[rng.integers(0, depth.size, 4), 1] = np.nan
        vps = np.tile(np.array([[0.01, -0.02, 0.03]]) * (s + 1), (dirs.shape[0], 1))
        mask = (np.arange(depth.size) % 11 != 3).astype(np.uint8)
        cr, sr, cp, sp, cy, sy = np.cos(rpy[0]), np.sin(rpy[0]), np.cos(rpy[1]), np.sin(rpy[1]), np.cos(rpy[2]), np.sin(rpy[2])
        T = np.eye(4)
        T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
            np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        T[:3, 3] = np.asarray(t) + np.asarray(offset)
        scans.append(D.batch(vps, d, depth, pose=T, mask=mask, min_depth=0.25, max_range=1.5))
    return scans


RANDOM = dict(voxel=0.1, trunc=0.3, origin=(0.013, -0.021, 0.007))
WINDOW_OFFSET = (2.8, 2.1, 1.9)              # the scene moved to non-negative indices, for the dense window
WINDOW = ((2, 1, 2), (47, 45, 33))           # lo, dims
