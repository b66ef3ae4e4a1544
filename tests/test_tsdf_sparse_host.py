"""Sparse TSDF volumes on the host (no GPU): the rules of csrc/dc_tsdf_sparse_math.h through their host build (libdc_hostcheck.so, the
header the kernels inline) against tests/tsdf_sparse_reference.py, bit for bit on keys, slots, n_blocks, sum, count, stats, info, vertices
and faces, after every step of the designed cases of tests/tsdf_sparse_cases.py; hand-written figures; the oracle anchored to the dense
oracle tests/tsdf_reference.py on a window of a random posed scene; the invariant (a block is in the table iff one of its voxels has
count > 0); ray order; and the bound of blocks per ray that sizes the candidate buffer.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cases as D  # noqa: E402
import tsdf_reference as R  # noqa: E402
import tsdf_sparse_cases as C  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
from tsdf_sparse_cases import RANDOM, WINDOW, WINDOW_OFFSET, assert_invariant, random_scans, step_both  # noqa: E402

Q = 2 ** 20


def host_lib():
    """libdc_hostcheck.so with the sparse volume's exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_tsdf_sparse_allocate'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    rays = [vp, vp, vp, ci, i64, vp, vp, vp, f64, f64, ci, f64, f64, i64]
    lib.dc_host_tsdf_sparse_allocate.argtypes = rays + [vp, vp, vp, vp, vp]
    lib.dc_host_tsdf_sparse_integrate.argtypes = rays + [vp, vp, vp, vp, vp, vp]
    lib.dc_host_tsdf_sparse_extract.argtypes = [vp, vp, i64, vp, vp, vp, f64, ci, i64, i64, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostVolume:
    """The table and pool as host arrays, driven through the host build."""

    def __init__(self, lib, voxel, trunc, origin, capacity):
        self.lib, self.voxel, self.trunc, self.capacity = lib, float(voxel), float(trunc), int(capacity)
        self.origin = np.asarray(origin, np.float64).reshape(3)
        self.keys = np.zeros(capacity, np.uint64)
        self.slots = np.zeros(capacity, np.int32)
        self.n_blocks = np.zeros(1, np.int64)
        self.sum = np.zeros((capacity, 512), np.int64)
        self.count = np.zeros((capacity, 512), np.int32)
        self.stats = np.zeros(5, np.int64)
        self.info = np.zeros(2, np.int64)
        self.max_ray_blocks = np.zeros(1, np.int64)

    def _rays(self, b, k=None):
        n = b['dirs'].shape[0]
        dt = b['dirs'].dtype
        self._keep = (np.ascontiguousarray(np.broadcast_to(b['vps'], (n, 3)), dtype=dt), np.ascontiguousarray(b['dirs']),
                      np.ascontiguousarray(b['depth'], dtype=dt), None if b['mask'] is None else np.ascontiguousarray(b['mask'], dtype=np.uint8),
                      None if b['pose'] is None else np.ascontiguousarray(b['pose'], dtype=np.float64))
        vps, dirs, depth, mask, pose = self._keep
        return (_p(vps), _p(dirs), _p(depth), 0 if dt == np.float32 else 1, n, _p(mask), _p(pose), _p(self.origin), self.voxel, self.trunc,
                S.k_steps(self.trunc, self.voxel) if k is None else k, b['min_depth'], np.inf if b['max_range'] is None else b['max_range'], self.capacity)

    def allocate(self, b):
        assert self.lib.dc_host_tsdf_sparse_allocate(*self._rays(b), _p(self.keys), _p(self.slots), _p(self.n_blocks), _p(self.info),
                                                     _p(self.max_ray_blocks)) == 0

    def integrate(self, b):
        assert self.lib.dc_host_tsdf_sparse_integrate(*self._rays(b), _p(self.keys), _p(self.slots), _p(self.n_blocks), _p(self.sum),
                                                      _p(self.count), _p(self.stats)) == 0

    def grow(self, capacity):
        for name in ('keys', 'slots', 'sum', 'count'):
            old = getattr(self, name)
            new = np.zeros((capacity,) + old.shape[1:], old.dtype)
            new[:self.capacity] = old
            setattr(self, name, new)
        self.capacity = int(capacity)

    def extract(self, min_count=1):
        tot = np.zeros(2, np.int64)
        args = (_p(self.keys), _p(self.slots), int(self.n_blocks[0]), _p(self.sum), _p(self.count), _p(self.origin), self.voxel, min_count)
        assert self.lib.dc_host_tsdf_sparse_extract(*args, 0, 0, None, None, _p(tot)) == 0
        v, f = np.zeros((int(tot[0]), 3)), np.zeros((int(tot[1]), 3), np.int32)
        assert self.lib.dc_host_tsdf_sparse_extract(*args, len(v), len(f), _p(v), _p(f), _p(tot)) == 0
        assert tot.tolist() == [len(v), len(f)]
        return v, f


def assert_same_state(got, want, what=''):
    n = want.n_blocks
    assert int(got.n_blocks[0]) == n, what
    assert np.array_equal(got.keys[:n], want.keys) and np.array_equal(got.slots[:n], want.slots), what
    assert np.array_equal(got.sum, want.sum) and np.array_equal(got.count, want.count), what
    assert got.stats.tolist() == want.stats.tolist(), what
    assert got.info.tolist() == want.info.tolist(), what


def run_case(lib, capacity, steps, check=True):
    got, want = HostVolume(lib, capacity=capacity, **C.VOLUME), S.SparseVolume(capacity=capacity, **C.VOLUME)
    for j, (kind, payload) in enumerate(steps):
        step_both(got, want, kind, payload)
        if check:
            assert_same_state(got, want, (j, kind))
    return got, want


INTEGRATION = {name: rest for name, *rest in C.integration_cases()}
EXTRACTION = {name: rest for name, *rest in C.extraction_cases()}


def block(vol, b):
    """(sum, count) [8,8,8] of the block at the coordinate b of an oracle-shaped volume."""
    pos = int(np.searchsorted(vol.keys[:int(np.ravel(vol.n_blocks)[0])], S.block_key(np.array(b))))
    assert vol.keys[pos] == S.block_key(np.array(b))
    return vol.sum[vol.slots[pos]].reshape(8, 8, 8), vol.count[vol.slots[pos]].reshape(8, 8, 8)


@pytest.mark.parametrize('name', sorted(INTEGRATION))
def test_host_equals_oracle_after_every_step(lib, name):
    capacity, steps = INTEGRATION[name]
    _, want = run_case(lib, capacity, steps)
    rays = sum(p['dirs'].shape[0] for kind, p in steps if kind in ('fuse', 'integrate'))
    assert want.stats[0] + want.stats[1] == rays


def test_two_blocks_by_hand(lib):
    """d = 8.5 along z through (1.5, 1.5): s = 2, 1, 0, -1, -2 in the voxels z = 6 .. 10, that is local 6, 7 of block (0,0,0) and local
    0, 1, 2 of block (0,0,1)."""
    got, want = run_case(lib, *INTEGRATION['crosses_z8'])
    assert int(got.n_blocks[0]) == 2 and got.slots[:2].tolist() == [0, 1] and got.info.tolist() == [2, 0]
    assert S.key_block(got.keys[:2]).tolist() == [[0, 0, 0], [0, 0, 1]]
    s0, c0 = block(got, (0, 0, 0))
    s1, c1 = block(got, (0, 0, 1))
    assert s0[1, 1].tolist() == [0, 0, 0, 0, 0, 0, Q, Q // 2] and c0[1, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert s1[1, 1].tolist() == [0, -Q // 2, -Q, 0, 0, 0, 0, 0] and c1[1, 1].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert got.stats.tolist() == [1, 0, 0, 5, 0] and got.count.sum() == 5
    assert_invariant(want)


def test_negative_indices_by_hand(lib):
    """From z = -6 with d = 4.5: s = 2, 1, 0, -1 in the voxels -4 .. -1 (block -1, local 4 .. 7) and s = -2 in voxel 0 (block 0, local 0)."""
    got, want = run_case(lib, *INTEGRATION['crosses_zero'])
    assert S.key_block(got.keys[:2]).tolist() == [[0, 0, -1], [0, 0, 0]]
    sm, cm = block(got, (0, 0, -1))
    s0, c0 = block(got, (0, 0, 0))
    assert sm[1, 1].tolist() == [0, 0, 0, 0, Q, Q // 2, 0, -Q // 2] and cm[1, 1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert s0[1, 1].tolist() == [-Q, 0, 0, 0, 0, 0, 0, 0] and c0[1, 1, 0] == 1 and c0.sum() == 1
    assert_invariant(want)


def test_a_visit_below_minus_tau_allocates_nothing(lib):
    got, want = run_case(lib, *INTEGRATION['below_minus_tau_alone'])            # voxels 4 .. 7 add; voxel 8 (block (0,0,1)) meets s = -2.5
    assert int(got.n_blocks[0]) == 1 and S.key_block(got.keys[:1]).tolist() == [[0, 0, 0]]
    s0, c0 = block(got, (0, 0, 0))
    assert s0[1, 1].tolist() == [0, 0, 0, 0, 3 * Q // 4, Q // 4, -Q // 4, -3 * Q // 4] and c0[1, 1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert got.stats.tolist() == [1, 0, 0, 4, 0]
    assert_invariant(want)


def test_new_keys_before_old_ones(lib):
    got, want = run_case(lib, *INTEGRATION['new_keys_sort_first'])
    assert S.key_block(got.keys[:3]).tolist() == [[-1, 0, -1], [-1, 0, 0], [0, 0, 0]]
    assert got.slots[:3].tolist() == [1, 2, 0]
    assert block(got, (0, 0, 0))[1][1, 1].tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    assert block(got, (-1, 0, -1))[1][6, 1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]      # x = -1.5 is voxel -2: local 6
    assert_invariant(want)


def test_capacity_two_of_three(lib):
    capacity, steps = INTEGRATION['capacity_2_of_3']
    got, want = run_case(lib, capacity, steps[:1])
    assert got.info.tolist() == [2, 1] and S.key_block(got.keys[:2]).tolist() == [[0, 0, 0], [1, 0, 0]]
    assert got.stats.tolist() == [3, 0, 0, 15, 5] and got.count.sum() == 10
    got, want = run_case(lib, capacity, steps)
    assert got.info.tolist() == [3, 0] and S.key_block(got.keys[:3]).tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0]]
    assert got.slots[:3].tolist() == [0, 1, 2] and got.count.sum() == 10


def test_allocate_is_idempotent(lib):
    capacity, steps = INTEGRATION['allocate_twice']
    once, _ = run_case(lib, capacity, steps[:1])
    twice, want = run_case(lib, capacity, steps[:2])
    for name in ('keys', 'slots', 'n_blocks', 'sum', 'count', 'info'):
        assert np.array_equal(getattr(once, name), getattr(twice, name)), name
    assert_invariant(run_case(lib, capacity, steps)[1])


def test_lookups_below_and_above_the_only_key(lib):
    got, _ = run_case(lib, *INTEGRATION['one_block_queried_around'])
    assert int(got.n_blocks[0]) == 1 and got.stats.tolist() == [3, 0, 0, 15, 10] and got.count.sum() == 5


def test_the_ends_of_the_block_range(lib):
    got, want = run_case(lib, *INTEGRATION['edge_of_the_range'])
    assert S.key_block(got.keys[:1]).tolist() == [[0, 0, 2 ** 20 - 1]] and int(got.n_blocks[0]) == 1
    assert got.stats.tolist() == [1, 0, 6, 2, 0]
    s, c = block(got, (0, 0, 2 ** 20 - 1))
    assert s[1, 1].tolist() == [0, 0, 0, 0, 0, 0, Q, Q // 2] and c[1, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    got, want = run_case(lib, *INTEGRATION['lowest_block'])
    assert S.key_block(got.keys[:1]).tolist() == [[0, 0, -2 ** 20]] and got.stats.tolist() == [1, 0, 5, 2, 0]
    s, c = block(got, (0, 0, -2 ** 20))
    assert s[1, 1].tolist() == [-Q // 2, -Q, 0, 0, 0, 0, 0, 0]
    assert int(got.keys[0]) == (2 ** 20 << 42) | (2 ** 20 << 21) and int(S.block_key(np.array([2 ** 20 - 1] * 3))) == 2 ** 63 - 1


def test_empty_and_skipped(lib):
    got, _ = run_case(lib, *INTEGRATION['rays_0'])
    assert int(got.n_blocks[0]) == 0 and got.stats.tolist() == [0] * 5 and got.info.tolist() == [0, 0]
    got, _ = run_case(lib, *INTEGRATION['dense_skipped_rays'])
    assert got.stats.tolist() == [1, 6, 0, 5, 0]
    a, _ = run_case(lib, *INTEGRATION['dense_f32'])
    b, _ = run_case(lib, *INTEGRATION['dense_f64_of_f32'])
    assert a.stats[3] > 0
    for name in ('keys', 'slots', 'n_blocks', 'sum', 'count', 'stats'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('name', sorted(C.dense_twins()))
def test_designed_dense_rays_give_the_dense_sums(lib, name):
    """Block (0, 0, 0) of the lattice is the dense cases' 4 x 4 x 8 grid and more: inside the grid the sums are the dense oracle's."""
    got, want = run_case(lib, *INTEGRATION[name])
    dense = R.Volume(**D.GRID)
    for b in C.dense_twins()[name]:
        R.integrate(dense, **b)
    s, c = want.window((0, 0, 0), D.GRID['dims'])
    assert np.array_equal(s.ravel(), dense.sum) and np.array_equal(c.ravel(), dense.count)
    assert dense.count.sum() > 0


# ---- a random posed scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def random_scene(lib):
    """(host volume, oracle volume, scans) of the random scene around the origin, fused with growth from capacity 8."""
    scans = random_scans()
    got, want = HostVolume(lib, capacity=8, **RANDOM), S.SparseVolume(capacity=8, **RANDOM)
    for b in scans:
        got.allocate(b)
        S.allocate(want, **b)
        while want.info[1] > 0:
            assert got.info.tolist() == want.info.tolist()
            cap = max(2 * want.capacity, want.capacity + int(want.info[1]))
            got.grow(cap)
            want.grow(cap)
            got.allocate(b)
            S.allocate(want, **b)
        got.integrate(b)
        S.integrate(want, **b)
    return got, want, scans


def test_random_scene_host_equals_oracle(lib, random_scene):
    got, want, _ = random_scene
    assert_same_state(got, want)
    assert_invariant(want)
    b = S.key_block(want.keys)
    assert (b.min(axis=0) < 0).all() and (b.max(axis=0) >= 0).all()             # blocks with a negative coordinate on every axis
    assert want.stats[1] > 150 and want.stats[3] > 5000 and want.n_blocks > 8
    for min_count in (1, 2):
        v, f = got.extract(min_count)
        wv, wf = S.extract(want, min_count)
        assert v.shape == wv.shape and f.shape == wf.shape and len(wv) > 100 and len(wf) > 50
        assert np.array_equal(v, wv) and np.array_equal(f, wf)


def test_oracle_is_anchored_to_the_dense_oracle():
    """The sparse oracle read on the index window [lo, lo + n) equals tsdf_reference.integrate into a Volume on that window, with the
    SAME origin and offset indices; and its mesh is the dense mesh of the window, whose outermost voxel layer is unobserved."""
    scans = random_scans(WINDOW_OFFSET)
    want = S.SparseVolume(capacity=8, **RANDOM)
    lo, dims = WINDOW
    dense = S.DenseWindow(want, lo, dims)
    for b in scans:
        S.fuse(want, **b)
        R.integrate(dense, **b)
    s, c = want.window(lo, dims)
    ds, dc = dense.read()
    assert c.sum() > 5000 and np.array_equal(s, ds) and np.array_equal(c, dc)
    assert c.sum() == want.count.sum()                                          # the window holds the whole scene
    shell = np.ones(dims, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert c[shell].sum() == 0
    win = R.Volume(want.origin, dims, want.voxel, want.trunc)                   # the window's voxels as a dense volume of their own:
    win.sum[:], win.count[:] = s.ravel(), c.ravel()                             # extracted in lattice coordinates, then placed
    win.origin = np.zeros(3)
    win.voxel = 1.0
    for min_count in (1, 2):
        wv, wf = S.extract(want, min_count)
        lv, lf = R.extract(win, min_count)
        # dense vertex = 0 + ((x + 0.5) + m) 1; the sparse one og + (((x + lo) + 0.5) + m) a: compare the connectivity and the cells
        assert len(wv) == len(lv) > 100 and len(wf) == len(lf) > 50
        cells_s = np.floor((wv - want.origin) / want.voxel - 0.5 + 1e-9).astype(np.int64)
        cells_d = np.floor(lv - 0.5 + 1e-9).astype(np.int64) + np.array(lo)
        order_s, order_d = np.lexsort(cells_s.T[::-1]), np.lexsort(cells_d.T[::-1])
        assert np.array_equal(cells_s[order_s], cells_d[order_d])
        rs, rd = np.empty(len(wv), np.int64), np.empty(len(lv), np.int64)
        rs[order_s], rd[order_d] = np.arange(len(wv)), np.arange(len(lv))
        fs, fd = rs[wf], rd[lf]
        assert np.array_equal(fs[np.lexsort(fs.T[::-1])], fd[np.lexsort(fd.T[::-1])])


def test_ray_order_does_not_change_a_byte(lib, random_scene):
    got, _, scans = random_scene
    again = HostVolume(lib, capacity=got.capacity, **RANDOM)
    for s, b in enumerate(scans):
        perm = np.random.default_rng(s).permutation(b['dirs'].shape[0])
        b = dict(b, vps=b['vps'][perm], dirs=b['dirs'][perm], depth=b['depth'][perm], mask=b['mask'][perm])
        again.allocate(b)
        again.integrate(b)
    for name in ('keys', 'slots', 'n_blocks', 'sum', 'count', 'stats', 'info'):
        assert np.array_equal(getattr(again, name), getattr(got, name)), name


def test_blocks_per_ray_fit_the_candidate_share(lib, random_scene):
    """Every ray gets 2K + 1 candidate keys; the most distinct blocks one ray wants (host build and oracle agree) stays within it, and
    within the tighter 4 + floor(sqrt(3) K / 8) of DESIGN."""
    _, _, scans = random_scene
    for voxel, trunc in ((0.1, 0.3), (0.02, 0.3), (0.05, 0.9)):
        K = S.k_steps(trunc, voxel)
        got = HostVolume(lib, voxel, trunc, RANDOM['origin'], 4096)
        want = S.SparseVolume(voxel, trunc, RANDOM['origin'], 4096)
        most = 0
        for b in scans:
            got.allocate(b)
            assert int(got.max_ray_blocks[0]) == S.ray_blocks(want, **b)
            most = max(most, int(got.max_ray_blocks[0]))
        print('K = %d: at most %d blocks per ray (share %d, bound %d)' % (K, most, 2 * K + 1, 4 + int(np.sqrt(3.0) * K / 8)))
        assert 1 < most <= min(2 * K + 1, 4 + int(np.sqrt(3.0) * K / 8))


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def extraction_volumes(lib, volume, blocks):
    """(host volume, oracle volume) holding ``blocks`` in the order of their slots, with the table sorted by key."""
    cap = max(1, len(blocks)) + 1
    got, want = HostVolume(lib, capacity=cap, **volume), S.SparseVolume(capacity=cap, **volume)
    keys = np.array([int(S.block_key(np.array(b))) for b, _, _ in blocks], np.uint64)
    order = np.argsort(keys, kind='stable')
    want.keys, want.slots = keys[order], order.astype(np.int32)
    for slot, (_, s, c) in enumerate(blocks):
        want.sum[slot], want.count[slot] = s.ravel(), c.ravel()
    got.keys[:len(blocks)], got.slots[:len(blocks)], got.n_blocks[0] = want.keys, want.slots, len(blocks)
    got.sum[:], got.count[:] = want.sum, want.count
    return got, want


@pytest.mark.parametrize('name', sorted(EXTRACTION))
def test_host_extraction_equals_oracle(lib, name):
    volume, blocks, min_count = EXTRACTION[name]
    got, want = extraction_volumes(lib, volume, blocks)
    v, f = got.extract(min_count)
    wv, wf = S.extract(want, min_count)
    assert v.shape == wv.shape and f.shape == wf.shape, name
    assert np.array_equal(v, wv) and np.array_equal(f, wf), name
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(v))


def test_extraction_across_blocks_by_hand(lib):
    def mesh(name):
        volume, blocks, min_count = EXTRACTION[name]
        return S.extract(extraction_volumes(lib, volume, blocks)[1], min_count)
    v, f = mesh('empty')
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # one inside voxel at (7, 7, 7) with f = -1/2 among f = 1: eight cells, six edges; the closed surface around the voxel
    v, f = mesh('corner_cell_in_eight_blocks')
    assert v.shape == (8, 3) and f.shape == (12, 3)
    assert R.is_closed_manifold(f) and R.euler_characteristic(v, f) == 2
    centre = np.full(3, 7.5)
    assert (np.einsum('ij,ij->i', R.face_normals(v, f), v[f].mean(axis=1) - centre) > 0).all()
    # r = f_a / (f_a - f_b) = (1/2) / (3/2) = 1/3 from the inside corner: every vertex lies 1/9 of a voxel from the centre per axis
    assert np.allclose(np.abs(v - centre), 1.0 / 9.0, atol=1e-12)
    assert (v[-1] > 7.5).all()                                                 # it comes last: ascending (key, local cell)
    # without block (1, 1, 1) the cell (7, 7, 7) has an unobserved corner: its vertex and the faces that used it are gone
    v2, f2 = mesh('corner_cell_one_block_missing')
    assert v2.shape == (7, 3) and f2.shape == (6, 3)
    assert {tuple(r) for r in v2.tolist()} == {tuple(r) for r in v[:-1].tolist()}
    # the voxel (8, 8, 3) inside: its two z edges have their four cells in four blocks each
    v, f = mesh('edge_cells_in_four_blocks')
    assert v.shape == (8, 3) and f.shape == (12, 3) and R.is_closed_manifold(f)
    v1, f1 = mesh('min_count_1')
    v2, f2 = mesh('min_count_2')
    # min_count = 2 leaves the voxel (3, 3, 3) whole and, of the voxel (7, 7, 7), the four cells at x = 6 and the one edge towards -x
    assert len(v1) == 16 and len(f1) == 24 and len(v2) == 12 and len(f2) == 14


def test_refused_arguments(lib):
    b = C.z_ray(4.5)
    for bad in (dict(voxel=0.0), dict(trunc=0.0), dict(trunc=np.nan), dict(origin=(np.inf, 0.0, 0.0))):
        got = HostVolume(lib, capacity=4, **dict(C.VOLUME, **bad))
        rays = got._rays(b, 4)
        assert lib.dc_host_tsdf_sparse_allocate(*rays, _p(got.keys), _p(got.slots), _p(got.n_blocks), _p(got.info), None) == -1, bad
        assert lib.dc_host_tsdf_sparse_integrate(*rays, _p(got.keys), _p(got.slots), _p(got.n_blocks), _p(got.sum), _p(got.count),
                                                 _p(got.stats)) == -1, bad
        assert got.count.sum() == 0 and got.stats.sum() == 0 and int(got.n_blocks[0]) == 0
    tot = np.zeros(2, np.int64)
    got = HostVolume(lib, capacity=1, **C.VOLUME)
    assert lib.dc_host_tsdf_sparse_extract(_p(got.keys), _p(got.slots), 2 ** 31 // 1536 + 1, _p(got.sum), _p(got.count), _p(got.origin), 1.0, 1,
                                           0, 0, None, None, _p(tot)) == -4


def test_python_layer_without_a_gpu():
    from depth_correction_amd.config import Config
    from depth_correction_amd.reconstruction import SparseTsdfVolume, reconstruct
    assert Config().recon_sparse is False
    with pytest.raises(RuntimeError, match='no CPU path'):
        SparseTsdfVolume(0.1, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        reconstruct([], [], 0.1, sparse=True, device='cpu')
