"""Sparse TSDF volumes on the GPU: dc_tsdf_sparse_* through ops and reconstruction.SparseTsdfVolume against the numpy oracle
tests/tsdf_sparse_reference.py and against the dense TsdfVolume, bit for bit -- the designed cases of tests/tsdf_sparse_cases.py step by
step, a random posed scene with blocks at negative coordinates, the same scene on a window of a dense volume with the same origin (pool
and mesh), growth from one block, a fixed pool that drops, ray order, two clusters 20 000 voxels apart that no dense box holds, and the
layers above: reconstruct(sparse=True), eval_recon with cfg.recon_sparse.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cases as D  # noqa: E402
import tsdf_reference as R  # noqa: E402
import tsdf_sparse_cases as C  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
from tsdf_sparse_cases import RANDOM, WINDOW, WINDOW_OFFSET, assert_invariant, random_scans, step_both  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def up(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)), device=DEV)


class DeviceVolume:
    """The table and pool as device tensors, driven through ops: the shape of test_tsdf_sparse_host.HostVolume."""

    def __init__(self, voxel, trunc, origin, capacity):
        self.voxel, self.trunc, self.origin, self.capacity = float(voxel), float(trunc), tuple(origin), int(capacity)
        kw = dict(device=DEV)
        self.t = dict(keys=torch.zeros(capacity, dtype=torch.int64, **kw), slots=torch.zeros(capacity, dtype=torch.int32, **kw),
                      n_blocks=torch.zeros(1, dtype=torch.int64, **kw), sum=torch.zeros((capacity, 512), dtype=torch.int64, **kw),
                      count=torch.zeros((capacity, 512), dtype=torch.int32, **kw), stats=torch.zeros(5, dtype=torch.int64, **kw),
                      info=torch.zeros(2, dtype=torch.int64, **kw))

    def _rays(self, b):
        n, dt = b['dirs'].shape[0], b['dirs'].dtype
        args = (self.origin, self.voxel, self.trunc, up(np.broadcast_to(b['vps'], (n, 3)), dt), up(b['dirs']), up(b['depth'], dt))
        kw = dict(pose=None if b['pose'] is None else up(b['pose'], np.float64), mask=None if b['mask'] is None else up(b['mask'], np.uint8),
                  min_depth=b['min_depth'], max_range=b['max_range'])
        return args, kw

    def allocate(self, b):
        from depth_correction_amd import ops
        args, kw = self._rays(b)
        ops.tsdf_sparse_allocate(self.t['keys'], self.t['slots'], self.t['n_blocks'], self.t['info'], *args, **kw)

    def integrate(self, b):
        from depth_correction_amd import ops
        args, kw = self._rays(b)
        ops.tsdf_sparse_integrate(self.t['keys'], self.t['slots'], self.t['n_blocks'], self.t['sum'], self.t['count'], self.t['stats'], *args, **kw)

    def grow(self, capacity):
        for name in ('keys', 'slots', 'sum', 'count'):
            old = self.t[name]
            new = torch.zeros((capacity,) + tuple(old.shape[1:]), dtype=old.dtype, device=DEV)
            new[:self.capacity] = old
            self.t[name] = new
        self.capacity = int(capacity)

    def extract(self, min_count=1):
        from depth_correction_amd import ops
        v, f = ops.tsdf_sparse_extract(self.t['keys'], self.t['slots'], int(self.t['n_blocks'].item()), self.t['sum'], self.t['count'], self.origin,
                                       self.voxel, min_count=min_count)
        assert v.dtype == torch.float64 and f.dtype == torch.int32
        return v.cpu().numpy(), f.cpu().numpy()

    def host(self, name):
        a = self.t[name].cpu().numpy()
        return a.astype(np.uint64) if name == 'keys' else a


def assert_same_state(got, want, what=''):
    n = want.n_blocks
    assert int(got.host('n_blocks')[0]) == n, what
    assert np.array_equal(got.host('keys')[:n], want.keys) and np.array_equal(got.host('slots')[:n], want.slots), what
    assert np.array_equal(got.host('sum'), want.sum) and np.array_equal(got.host('count'), want.count), what
    assert got.host('stats').tolist() == want.stats.tolist(), what
    assert got.host('info').tolist() == want.info.tolist(), what


INTEGRATION = {name: rest for name, *rest in C.integration_cases()}
EXTRACTION = {name: rest for name, *rest in C.extraction_cases()}


@pytest.mark.parametrize('name', sorted(INTEGRATION))
def test_designed_integration_cases(name):
    capacity, steps = INTEGRATION[name]
    got, want = DeviceVolume(capacity=capacity, **C.VOLUME), S.SparseVolume(capacity=capacity, **C.VOLUME)
    for j, (kind, payload) in enumerate(steps):
        step_both(got, want, kind, payload)
        assert_same_state(got, want, (name, j, kind))


@pytest.mark.parametrize('name', sorted(EXTRACTION))
def test_designed_extraction_cases(name):
    volume, blocks, min_count = EXTRACTION[name]
    cap = len(blocks) + 2
    got, want = DeviceVolume(capacity=cap, **volume), S.SparseVolume(capacity=cap, **volume)
    keys = np.array([int(S.block_key(np.array(b))) for b, _, _ in blocks], np.uint64)
    order = np.argsort(keys, kind='stable')
    want.keys, want.slots = keys[order], order.astype(np.int32)
    for slot, (_, s, c) in enumerate(blocks):
        want.sum[slot], want.count[slot] = s.ravel(), c.ravel()
    got.t['keys'][:len(blocks)] = up(want.keys.astype(np.int64))
    got.t['slots'][:len(blocks)] = up(want.slots)
    got.t['n_blocks'][0] = len(blocks)
    got.t['sum'].copy_(up(want.sum))
    got.t['count'].copy_(up(want.count))
    v, f = got.extract(min_count)
    wv, wf = S.extract(want, min_count)
    assert v.shape == wv.shape and f.shape == wf.shape, (name, v.shape, wv.shape, f.shape, wf.shape)
    assert np.array_equal(v, wv) and np.array_equal(f, wf), name


# ---- the random posed scene --------------------------------------------------------------------------------------------------------
def cloud_of(b, dtype=None):
    from depth_correction_amd.depth_cloud import DepthCloud
    dt = b['dirs'].dtype if dtype is None else dtype
    n = b['dirs'].shape[0]
    return DepthCloud(up(np.broadcast_to(b['vps'], (n, 3)), dt), up(b['dirs'], dt), up(b['depth'], dt).reshape(n, 1))


def integrate_scan(vol, b, dtype=None):
    return vol.integrate(cloud_of(b, dtype), pose=b['pose'], mask=up(b['mask']), min_depth=b['min_depth'], max_range=b['max_range'])


def sparse_volume(**kw):
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    return SparseTsdfVolume(RANDOM['voxel'], trunc=RANDOM['trunc'], origin=RANDOM['origin'], device=DEV, **kw)


def as_dtype(b, dt):
    return dict(b, vps=b['vps'].astype(dt), dirs=b['dirs'].astype(dt), depth=b['depth'].astype(dt))


def assert_volume_equals_oracle(vol, want):
    n = want.n_blocks
    assert vol.n_blocks == n
    coords, slots = vol.blocks()
    assert np.array_equal(coords.cpu().numpy(), S.key_block(want.keys)) and np.array_equal(slots.cpu().numpy(), want.slots)
    assert np.array_equal(vol._keys[:n].cpu().numpy().astype(np.uint64), want.keys)
    m = min(vol.capacity, want.capacity)
    assert n <= m
    assert np.array_equal(vol._sum[:m].cpu().numpy(), want.sum[:m]) and np.array_equal(vol._count[:m].cpu().numpy(), want.count[:m])
    assert int(vol._count[m:].sum()) == 0 and int(want.count[m:].sum()) == 0
    assert list(vol.stats().values()) == want.stats.tolist() + [n]


@pytest.fixture(scope='module')
def random_scene():
    """{dtype: (device volume, oracle)} of the scene around the origin, computed once and left unchanged."""
    out = {}
    for dt in (np.float32, np.float64):
        vol, want = sparse_volume(), S.SparseVolume(capacity=8, **RANDOM)
        for b in random_scans():
            before = want.stats.copy()
            stats = integrate_scan(vol, b, dt)
            S.fuse(want, **as_dtype(b, dt))
            assert list(stats.values()) == (want.stats - before).tolist() + [want.n_blocks]
        out[dt] = (vol, want)
    return out


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_random_scene_equals_oracle(random_scene, dt):
    vol, want = random_scene[dt]
    print('random scene %s: %s, %d bytes' % (dt.__name__, vol.stats(), vol.nbytes))
    b = S.key_block(want.keys)
    assert (b.min(axis=0) < 0).all() and (b.max(axis=0) >= 0).all()             # blocks with a negative coordinate on every axis
    assert want.stats[1] > 150 and want.stats[3] > 5000 and want.n_blocks > 50
    assert_volume_equals_oracle(vol, want)
    assert_invariant(want)


@pytest.mark.parametrize('min_count', [1, 2])
def test_random_scene_extraction_equals_oracle(random_scene, min_count):
    vol, want = random_scene[np.float64]
    v, f = vol.extract(min_count)
    wv, wf = S.extract(want, min_count)
    assert tuple(v.shape) == wv.shape and tuple(f.shape) == wf.shape and len(wv) > 100 and len(wf) > 50
    assert np.array_equal(v.cpu().numpy(), wv) and np.array_equal(f.cpu().numpy(), wf)
    assert wf.min() >= 0 and wf.max() < len(wv)


def test_positive_octant_equals_the_dense_volume(random_scene):
    """The dense TsdfVolume with the same origin holds the indices >= 0 only: on them the pools agree (the rest of the scene is outside
    the dense box and inside the sparse lattice)."""
    from depth_correction_amd.reconstruction import TsdfVolume
    vol, _ = random_scene[np.float64]
    dims = (20, 18, 14)
    dense = TsdfVolume(RANDOM['origin'], dims, RANDOM['voxel'], trunc=RANDOM['trunc'], device=DEV)
    for b in random_scans():
        dense.integrate(cloud_of(b), pose=b['pose'], mask=up(b['mask']), min_depth=b['min_depth'], max_range=b['max_range'])
    s, c = vol.window((0, 0, 0), dims)
    assert int(c.sum()) > 1000 and dense.stats()['samples_outside'] > 1000
    assert torch.equal(s, dense.sums()) and torch.equal(c, dense.counts())


@pytest.fixture(scope='module')
def moved_scene():
    """(sparse volume, dense volume, dense oracle, scans) of the scene moved to non-negative indices: the dense box [0, hi) has the same
    origin and holds every voxel the scene writes."""
    from depth_correction_amd.reconstruction import TsdfVolume
    lo, dims = WINDOW
    hi = tuple(l + n for l, n in zip(lo, dims))
    scans = random_scans(WINDOW_OFFSET)
    vol = sparse_volume()
    dense = TsdfVolume(RANDOM['origin'], hi, RANDOM['voxel'], trunc=RANDOM['trunc'], device=DEV)
    oracle = R.Volume(RANDOM['origin'], hi, RANDOM['voxel'], RANDOM['trunc'])
    for b in scans:
        integrate_scan(vol, b)
        dense.integrate(cloud_of(b), pose=b['pose'], mask=up(b['mask']), min_depth=b['min_depth'], max_range=b['max_range'])
        R.integrate(oracle, **b)
    return vol, dense, oracle, scans


def test_window_and_mesh_equal_the_dense_volume(moved_scene):
    vol, dense, oracle, _ = moved_scene
    lo, dims = WINDOW
    s, c = vol.window(lo, dims)
    sl = tuple(slice(l, None) for l in lo)
    assert int(c.sum()) > 5000
    assert torch.equal(s, dense.sums()[sl]) and torch.equal(c, dense.counts()[sl])
    # the window holds the whole scene and its outermost layer is unobserved: the dense box's missing boundary cells do not matter
    assert int(c.sum()) == int(vol._count.sum()) == int(dense.counts().sum()) and oracle.stats[2] == 0
    shell = torch.ones(dims, dtype=torch.bool, device=DEV)
    shell[1:-1, 1:-1, 1:-1] = False
    assert int(c[shell].sum()) == 0
    for min_count in (1, 2):
        ov, of = R.extract(oracle, min_count)
        assert len(ov) > 100 and np.unique(ov, axis=0).shape[0] == len(ov)     # the dense oracle's vertex rows are distinct
        dv, df = dense.extract(min_count)
        sv, sf = vol.extract(min_count)
        want_v, want_f = S.canonical_mesh(dv.cpu().numpy(), df.cpu().numpy())
        got_v, got_f = S.canonical_mesh(sv.cpu().numpy(), sf.cpu().numpy())
        assert np.array_equal(want_v, S.canonical_mesh(ov, of)[0])
        assert got_v.shape == want_v.shape and got_f.shape == want_f.shape
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)


def test_growth_from_one_block(moved_scene, monkeypatch):
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    large, _, _, scans = moved_scene
    monkeypatch.setattr(SparseTsdfVolume, 'INITIAL_BLOCKS', 1)
    vol = sparse_volume()
    assert vol.capacity == 1
    for b in scans:
        stats = integrate_scan(vol, b)
        assert stats['visits_dropped'] == 0
    assert vol.capacity >= vol.n_blocks == large.n_blocks > 50
    lo, dims = WINDOW
    for a, b in zip(vol.window(lo, dims), large.window(lo, dims)):
        assert torch.equal(a, b)
    for a, b in zip(vol.blocks(), large.blocks()):
        assert torch.equal(a, b)
    for a, b in zip(vol.extract(), large.extract()):
        assert torch.equal(a, b) and a.shape[0] > 50
    assert vol.stats() == large.stats()


def test_fixed_capacity_reports_the_drops(moved_scene):
    _, _, _, scans = moved_scene
    vol, want = sparse_volume(max_blocks=10), S.SparseVolume(capacity=10, **RANDOM)
    for b in scans:
        stats = integrate_scan(vol, b)
        S.allocate(want, **b)
        S.integrate(want, **b)
        assert stats['blocks'] == want.n_blocks
    assert vol.capacity == 10 and vol.n_blocks == 10 and want.info[1] > 0
    assert_volume_equals_oracle(vol, want)
    st = vol.stats()
    assert st['visits_dropped'] == want.stats[4] > 1000 and st['visits'] - st['visits_dropped'] == int(vol._count.sum())
    with pytest.raises(ValueError, match='carve'):
        vol.integrate(cloud_of(scans[0]), carve_from=0.5)


def test_ray_order_and_repetition_do_not_change_a_bit(moved_scene):
    vol, _, _, scans = moved_scene
    for trial in range(2):
        again = sparse_volume()
        for s, b in enumerate(scans):
            if trial:
                perm = np.random.default_rng(s).permutation(b['dirs'].shape[0])
                b = dict(b, vps=b['vps'][perm], dirs=b['dirs'][perm], depth=b['depth'][perm], mask=b['mask'][perm])
            integrate_scan(again, b)
        for name in ('_keys', '_slots', '_n_blocks', '_sum', '_count', '_stats'):
            assert torch.equal(getattr(again, name), getattr(vol, name)), (trial, name)


def test_empty_cloud_and_reset():
    from depth_correction_amd.depth_cloud import DepthCloud
    vol = sparse_volume()
    empty = DepthCloud(torch.zeros((0, 3), dtype=torch.float64, device=DEV), torch.zeros((0, 3), dtype=torch.float64, device=DEV),
                       torch.zeros((0, 1), dtype=torch.float64, device=DEV))
    assert vol.integrate(empty) == dict(rays_used=0, rays_skipped=0, samples_outside=0, visits=0, visits_dropped=0, blocks=0)
    v, f = vol.extract()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    with pytest.raises(ValueError, match='no surface'):
        vol.extract_mesh()
    integrate_scan(vol, random_scans()[0])
    assert vol.n_blocks > 0 and vol.nbytes == vol.capacity * (8 + 4 + 512 * 12)
    vol.reset()
    assert vol.n_blocks == 0 and int(vol._count.sum()) == 0 and vol.stats()['rays_used'] == 0
    s, c = vol.window((-4, -4, -4), (8, 8, 8))
    assert int(c.sum()) == 0


def test_two_clusters_twenty_thousand_voxels_apart():
    """Two small scans 20 000 voxels apart on x (and 400 on y and z): the dense box of both has 2^31 voxels or more and is refused; the
    sparse volume holds a few dozen blocks, and each cluster equals the dense oracle of its own window.

    The voxel size is 1/8 m and the origin 0, so that the far window's corner L a is a double, p - L a is exact for every sample p
    beyond it (L a is a multiple of p's unit in the last place), the division by a is exact, and the centres (L + i + 0.5) a are
    doubles: the dense oracle at the origin L a is the lattice's own arithmetic, not an approximation of it."""
    from depth_correction_amd.reconstruction import SparseTsdfVolume, TsdfVolume
    a, tau = 0.125, 0.375
    shift = np.array([20000, 400, 400])
    jx, jy = [g.ravel() for g in np.meshgrid(np.arange(24), np.arange(24), indexing='ij')]
    dirs = np.tile([[0.0, 0.0, 1.0]], (jx.size, 1))
    depth = (8.0 + 0.11 * jx - 0.07 * jy) * a                                   # a tilted plane seen along +z, two rays per voxel and axis
    vol = SparseTsdfVolume(a, trunc=tau, device=DEV)
    windows = []
    for k in (0, 1):
        base = shift * k
        vps = (base + np.stack([2.2 + 0.5 * jx, 2.1 + 0.5 * jy, np.full(jx.size, 1.2)], axis=1)) * a
        b = D.batch(vps, dirs, depth)
        stats = vol.integrate(cloud_of(b))
        assert stats['visits_dropped'] == 0 and stats['samples_outside'] == 0
        dense = R.Volume(base * a, (16, 16, 24), a, tau)
        R.integrate(dense, **b)
        assert dense.stats[2] == 0 and dense.stats[3] > 300
        windows.append((tuple(int(v) for v in base), dense))
    lo, hi = np.array([2.2, 2.1, 1.2]) * a, (shift + np.array([13.7, 13.6, 1.2 + 12])) * a
    with pytest.raises(ValueError, match='2\\^31'):
        TsdfVolume.from_bounds(lo, hi, a, trunc=tau, device=DEV)
    print('two clusters: %d blocks, %d bytes' % (vol.n_blocks, vol.nbytes))
    assert 4 <= vol.n_blocks <= 48
    total = 0
    for base, dense in windows:
        s, c = vol.window(base, dense.dims)
        assert np.array_equal(s.cpu().numpy().ravel(), dense.sum) and np.array_equal(c.cpu().numpy().ravel(), dense.count)
        total += int(dense.count.sum())
    assert total == int(vol._count.sum())
    v, f = vol.extract()
    assert v.shape[0] > 20 and f.shape[0] > 20
    assert float(v[:, 0].max() - v[:, 0].min()) > 19990 * a


def test_arguments_are_checked():
    from depth_correction_amd import ops
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    with pytest.raises(ValueError):
        SparseTsdfVolume(0.0, device=DEV)
    with pytest.raises(ValueError):
        SparseTsdfVolume(0.1, max_blocks=0, device=DEV)
    vol = sparse_volume(max_blocks=4)
    c = cloud_of(random_scans()[0])
    t = (vol._keys, vol._slots, vol._n_blocks)
    rule = (vol.origin, vol.voxel_size, vol.trunc)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_allocate(*t, vol._info, vol.origin, vol.voxel_size, 0.0, c.vps, c.dirs, c.depth)
    with pytest.raises((ValueError, TypeError)):
        ops.tsdf_sparse_allocate(vol._keys, vol._slots.long(), vol._n_blocks, vol._info, *rule, c.vps, c.dirs, c.depth)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*t, vol._sum[:3], vol._count, vol._stats, *rule, c.vps, c.dirs, c.depth)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_integrate(*t, vol._sum, vol._count, vol._stats, *rule, c.vps, c.dirs, c.depth[:-1])
    with pytest.raises(ValueError):
        ops.tsdf_sparse_extract(vol._keys, vol._slots, 5, vol._sum, vol._count, vol.origin, vol.voxel_size)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_extract(vol._keys, vol._slots, 0, vol._sum, vol._count, vol.origin, vol.voxel_size, min_count=0)
    assert int(vol._count.sum()) == 0 and vol.n_blocks == 0


# ---- the layers above, on the small rendered room of the dense test -------------------------------------------------------------------
ROOM_POSES = [(0.2 * i, (-2.0 + 1.3 * i, 0.3 * math.sin(i), 0.1 * i)) for i in range(4)]


def _pose(yaw, t):
    from depth_correction_amd.dataset import euler_matrix
    T = euler_matrix(0.0, 0.0, yaw)
    T[:3, 3] = t
    return np.asarray(T, dtype=np.float64)


@pytest.fixture(scope='module')
def room(tmp_path_factory):
    from depth_correction_amd.dataset import RenderedMeshDataset
    from depth_correction_amd.mesh import room_mesh
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5, pillars=[((2.0, 1.0, 0.0), (0.4, 0.4, 1.0)), ((-2.5, -1.5, 0.0), (0.5, 0.3, 1.0))])
    path = str(tmp_path_factory.mktemp('recon_sparse') / 'pillared_room.ply')
    mesh.save_ply(path)
    ds = RenderedMeshDataset(path, poses=np.stack([_pose(yaw, t) for yaw, t in ROOM_POSES]), size=(16, 256), fov=(45.0, 360.0), num_segments=16,
                             device=DEV)
    return ds, mesh


def test_reconstruct_sparse_equals_the_dense_path(room):
    from depth_correction_amd.metrics import reconstruction_accuracy
    from depth_correction_amd.reconstruction import SparseTsdfVolume, reconstruct
    ds, gt = room
    clouds, poses = zip(*[(c, p) for c, p in ds])
    mesh, vol = reconstruct(clouds, poses, 0.1, sparse=True, device=DEV)
    assert isinstance(vol, SparseTsdfVolume) and vol.origin == (0.0, 0.0, 0.0) and vol.stats()['visits_dropped'] == 0
    assert len(mesh.vertices) > 1000 and len(mesh.faces) > 1000 and mesh.faces.min() >= 0 and mesh.faces.max() < len(mesh.vertices)
    acc = reconstruction_accuracy(mesh, gt, n_samples=20000, max_dist=0.2)
    print('sparse room: %d blocks, %d bytes, %d vertices, %d faces; accuracy %s' % (vol.n_blocks, vol.nbytes, len(mesh.vertices), len(mesh.faces),
                                                                                    acc['accuracy']))
    assert all(math.isfinite(acc[p][k]) for p in ('accuracy', 'completeness') for k in ('mean', 'rms', 'median', 'max'))
    for kw in (dict(bounds=((-1, -1, -1), (1, 1, 1))), dict(carve_from=0.5)):
        with pytest.raises(ValueError, match='sparse'):
            reconstruct(clouds, poses, 0.1, sparse=True, device=DEV, **kw)
    # the dense path in a box that no sample leaves, and a sparse volume on that box's lattice: the same mesh
    lo, hi = gt.bounds
    dense_mesh, dense = reconstruct(clouds, poses, 0.1, bounds=(lo - 0.5, hi + 0.5), device=DEV)
    assert dense.stats()['samples_outside'] == 0
    twin = SparseTsdfVolume(0.1, origin=dense.origin, device=DEV)
    for c, p in zip(clouds, poses):
        twin.integrate(c, pose=p)
    s, c = twin.window((0, 0, 0), dense.dims)
    assert torch.equal(s, dense.sums()) and torch.equal(c, dense.counts()) and int(c.sum()) == int(twin._count.sum())
    twin_mesh = twin.extract_mesh()
    want_v, want_f = S.canonical_mesh(dense_mesh.vertices, dense_mesh.faces)
    got_v, got_f = S.canonical_mesh(twin_mesh.vertices, twin_mesh.faces)
    assert np.unique(want_v, axis=0).shape[0] == len(want_v)
    assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    print('dense room: %d voxels, %d bytes; sparse twin: %d blocks, %d bytes' % (np.prod(dense.dims), 12 * np.prod(dense.dims), twin.n_blocks,
                                                                                 twin.nbytes))


def test_eval_recon_sparse(room, tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_recon
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    ds, _ = room
    cfg = Config(device=DEV, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25, recon_sparse=True,
                 recon_eval_csv=str(tmp_path / 'recon.csv'), recon_eval_samples=20000, recon_eval_max_dist=0.2)
    res = eval_recon(cfg, test_datasets=[ds], model=None)[0]
    assert isinstance(res['volume'], SparseTsdfVolume) and len(res['mesh']) > 100      # (the clouds are grid-filtered at 0.1 m first)
    assert math.isfinite(res['accuracy']['mean']) and 0.0 < res['coverage'] <= 1.0
    lines = open(cfg.recon_eval_csv).read().splitlines()
    assert len(lines) == 1 and len(lines[0].split(' ')) == 12 and lines[0].split(' ')[0] == str(ds)
    parts = lines[0].split(' ')
    assert int(parts[1]) == res['mesh'].vertices.shape[0] and int(parts[2]) == len(res['mesh'])
    cfg.recon_carve_from = 0.5
    with pytest.raises(ValueError, match='sparse'):
        eval_recon(cfg, test_datasets=[ds], model=None)
