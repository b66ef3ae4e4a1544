"""Ray casting the fused volume on the GPU: dc_tsdf_sparse_cast_rays through ops.tsdf_sparse_cast_rays against the numpy oracle
(tests/tsdf_cast_reference.py, the naive march) and the hand-computed designed cases that tests/test_tsdf_cast_host.py runs through the
host build -- face, t, normal, phi and status to the bit, inc through cos(inc) within 1e-13, with and without skipping --, the launch
tails, the random posed scene with and without own tables, the cast next to the mesh cast on a rendered room (measured, not gated),
and metrics.depth_bias / eval_bias against the fused volume."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cast_reference as C  # noqa: E402
import tsdf_loss_reference as L  # noqa: E402
import tsdf_sparse_reference as S  # noqa: E402
from test_tsdf_cast_host import check_designed, check_refinement, check_skipping, designed_volumes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_tables = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def tables(vol):
    """The oracle volume on the device as ops.TsdfTables (once per volume)."""
    from depth_correction_amd import ops
    if id(vol) not in _tables:
        cap = vol.capacity
        keys, slots = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        keys[:vol.n_blocks], slots[:vol.n_blocks] = vol.keys.view(np.int64), vol.slots
        _tables[id(vol)] = (vol, ops.TsdfTables(_t(keys), _t(slots), _t(np.array([vol.n_blocks], np.int64)), _t(vol.sum), _t(vol.count),
                                                vol.origin, vol.voxel, vol.trunc))
    return _tables[id(vol)][1]


def own_tables(owns):
    from depth_correction_amd import ops
    keys, slots, ptr, sm, cnt = L.own_tables(owns)
    return ops.TsdfOwnTables(_t(keys.view(np.int64)), _t(slots), _t(ptr), _t(sm), _t(cnt))


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def device_cast(vol, own, vps, dirs, offset, poses, mask=None, **kw):
    from depth_correction_amd import ops
    return host(ops.tsdf_sparse_cast_rays(tables(vol), _t(vps), _t(dirs), offset, _t(np.asarray(poses, np.float64).reshape(-1, 4, 4)),
                                          mask=None if mask is None else _t(np.asarray(mask).astype(np.uint8)), own=own, **kw))


def device_one(vol, vps, dirs, mask, **kw):
    return device_cast(vol, None, vps, dirs, [0, len(dirs)], C.IDENTITY, mask=mask, **kw)


# ---- 1. designed volumes -------------------------------------------------------------------------------------------------------------
def test_designed_rays_device_equals_oracle_and_hand():
    check_designed(device_one)


def test_refinement_device_equals_oracle():
    check_refinement(device_one)


def test_skipping_device_equals_naive_march():
    check_skipping(device_one)


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_launch_tails(n):
    """n copies of four designed rays in turn (a hit, an oblique hit, BEHIND, SKIPPED), f32 and f64 rays."""
    vols = designed_volumes()
    cases = [c for c in C.ray_cases() if c['name'] in ('wall, +x', 'wall, dir (1, 1, 0)', 'wall, -x from behind', 'dir = 0')]
    assert len(cases) == 4
    pick = np.arange(n) % 4
    vps = np.array([cases[k]['vp'] for k in pick], np.float64).reshape(-1, 3)
    dirs = np.array([cases[k]['dir'] for k in pick], np.float64).reshape(-1, 3)
    for dt in (np.float64, np.float32):                                   # the cases' numbers are fp32 numbers
        got = device_cast(vols['WALL'], None, vps.astype(dt), dirs.astype(dt), [0, n], C.IDENTITY, **C.DEFAULT_KW)
        assert got['t'].shape == (n,) and got['normal'].shape == (n, 3)
        for i in range(n):
            C.assert_hand({k: v[i:i + 1] for k, v in got.items()}, cases[pick[i]])


def test_arguments():
    from depth_correction_amd import ops
    vol = designed_volumes()['WALL']
    tb = tables(vol)
    vps, dirs, P = _t(np.array([[14.25, 2.0, 2.0]])), _t(np.array([[1.0, 0.0, 0.0]])), _t(C.IDENTITY)
    for kw in (dict(t_min=-1.0), dict(t_min=3.0, t_max=3.0), dict(t_max=math.inf), dict(step=0.0), dict(step=2.5), dict(step=2.0 ** -30),
               dict(refine=-1), dict(min_count=0)):
        with pytest.raises(ValueError):
            ops.tsdf_sparse_cast_rays(tb, vps, dirs, [0, 1], P, **kw)
    with pytest.raises(TypeError):
        ops.tsdf_sparse_cast_rays(vol, vps, dirs, [0, 1], P)
    with pytest.raises(TypeError):
        ops.tsdf_sparse_cast_rays(tb, vps, dirs, [0, 1], P, own=tb)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_cast_rays(tb, vps, dirs, [0, 2], P)
    out = ops.tsdf_sparse_cast_rays(tb, vps, dirs, [0, 1], P, t_max=10.0, step=0.5)
    again = ops.tsdf_sparse_cast_rays(tb, vps, dirs, [0, 1], P, t_max=10.0, step=0.5, out=out)
    assert again is out and host(out)['t'][0] == 2.25


# ---- 2. the random posed scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_random_scene_device_equals_oracle(dtype):
    sc = C.random_scene(dtype)
    assert sc['counts'][C.HIT] * 3 >= sc['n'] and min(sc['counts'][k] for k in (C.MISS, C.BEHIND, C.SKIPPED)) >= 1, sc['counts']
    own = own_tables(sc['owns'])
    for (min_count, with_own), want in sc['oracle'].items():
        for skip in (True, False):
            run = lambda: device_cast(sc['total'], own if with_own else None, sc['vps'], sc['dirs'], sc['offset'], sc['poses'], mask=sc['mask'],
                                      min_count=min_count, skip=skip, **sc['rule'])
            got, again = run(), run()
            C.assert_equal(got, want, (dtype, min_count, with_own, skip), samples='samples_read' if skip else 'samples')
            for k in got:
                assert np.array_equal(got[k], again[k], equal_nan=True), k
    first = sc['oracle'][(1, False)]
    print('random scene %s: %d rays, status counts %s, LOST %d; samples per ray naive %.1f, read %.1f'
          % (dtype, sc['n'], sc['counts'], sc['counts'][C.LOST], first['samples'].mean(), first['samples_read'].mean()))


def _clouds(scans, dtype=torch.float64):
    from depth_correction_amd.depth_cloud import DepthCloud
    return [DepthCloud(vps=_t(c['vps'], dtype), dirs=_t(c['dirs'], dtype), depth=_t(c['depth'], dtype).reshape(-1, 1),
                       inc_angles=_t(c['inc'], dtype).reshape(-1, 1), mask=_t(np.asarray(c['lmask'], bool))) for c in scans]


def test_own_tables_equal_the_refused_volumes():
    """TsdfTarget on the device: scan s cast against total minus own s equals the cast against leave_one_out_volumes()[s]."""
    from depth_correction_amd import loss as DL, ops
    scans, poses = L.box_scene(rows=24, cols=96)
    clouds = _clouds(scans)
    target = DL.TsdfTarget(0.1, trunc=0.3, leave_one_out=True, refresh_every=0).refresh(clouds, _t(poses, torch.float64))
    off = np.concatenate([[0], np.cumsum([len(c['depth']) for c in scans])])
    vps, dirs = torch.cat([c.vps for c in clouds]).contiguous(), torch.cat([c.dirs for c in clouds]).contiguous()
    P = _t(poses, torch.float64)
    got = host(ops.tsdf_sparse_cast_rays(target.tables, vps, dirs, off, P, t_max=7.0, own=target.own))
    hits = 0
    for s, volume in enumerate(target.leave_one_out_volumes()):
        a, b = int(off[s]), int(off[s + 1])
        want = host(volume.raycast(vps[a:b], dirs[a:b], poses=P[s:s + 1], t_max=7.0))
        for k in ('t', 'phi', 'normal', 'inc', 'status'):
            assert np.array_equal(got[k][a:b], want[k], equal_nan=True), (s, k)
        hit = want['status'] == C.HIT
        hits += int(hit.sum())
        # the table positions differ between the two volumes: the faces name the same blocks
        assert torch.equal(volume._keys[_t(want['face'][hit]).long()], target.total._keys[_t(got['face'][a:b][hit]).long()]), s
    assert hits > 2000


# ---- 3. against the mesh -------------------------------------------------------------------------------------------------------------
def _read_volume(volume):
    n = volume.n_blocks
    v = S.SparseVolume(volume.voxel_size, trunc=volume.trunc, origin=volume.origin, capacity=volume.capacity)
    v.keys, v.slots = volume._keys[:n].cpu().numpy().view(np.uint64), volume._slots[:n].cpu().numpy()
    v.sum, v.count = volume._sum.cpu().numpy(), volume._count.cpu().numpy()
    return v


def _quantiles(x):
    return ' '.join('%.4g' % v for v in np.quantile(x, [0.05, 0.25, 0.5, 0.75, 0.95])) if x.size else 'none'


def test_room_cast_next_to_the_mesh_cast(tmp_path):
    """A box room rendered at 16 x 256 rays a scan, fused at the ground-truth poses at 0.4 m (voxels that ray density can fill): one scan's own rays against the volume of
    the other scans (device against the oracle on the pool the device fused) and against the mesh.  The differences are printed: they
    are the measurement (DESIGN), nothing here is held to a bar of this test's making."""
    from depth_correction_amd import ops
    from depth_correction_amd.dataset import RenderedMeshDataset, euler_matrix
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    mesh = room_mesh((6.0, 4.0, 1.5), 0.5)
    path = str(tmp_path / 'room.ply')
    mesh.save_ply(path)
    poses = []
    for i in range(4):
        T = np.asarray(euler_matrix(0.0, 0.0, 0.2 * i), np.float64)
        T[:3, 3] = (-2.0 + 1.3 * i, 0.3 * math.sin(i), 0.1 * i)
        poses.append(T)
    ds = RenderedMeshDataset(path, poses=np.stack(poses), size=(16, 256), fov=(45.0, 360.0), num_segments=16, device=DEV)
    from depth_correction_amd.depth_cloud import DepthCloud
    clouds, poses = zip(*[(c if isinstance(c, DepthCloud) else DepthCloud.from_structured_array(c, dtype=np.float64, device=DEV),
                           np.asarray(p, np.float64)) for c, p in ds])
    s = 1
    others = SparseTsdfVolume(0.4, device=DEV)
    for k, (c, p) in enumerate(zip(clouds, poses)):
        if k != s:
            others.integrate(c, pose=p)
    cloud = clouds[s]
    got = host(others.raycast_cloud(cloud, pose=poses[s], t_max=8.0))
    vps = cloud.vps.reshape(-1, 3).expand(len(cloud), 3).cpu().numpy()
    dirs, mask = cloud.dirs.cpu().numpy(), None if cloud.mask is None else cloud.mask.cpu().numpy()
    want = C.cast(_read_volume(others), None, vps, dirs, [0, len(cloud)], poses[s][None], t_max=8.0, step=0.2, mask=mask)
    C.assert_equal(got, want, 'room', samples='samples_read')
    bvh = mesh.on_device(torch.device(DEV))[3]
    face, t, inc = ops.raycast_rays(bvh, _t(vps.astype(dirs.dtype)), cloud.dirs.contiguous(), [0, len(cloud)], _t(poses[s][None]))
    t_mesh, inc_mesh = t.cpu().numpy(), inc.cpu().numpy()
    both = (got['status'] == C.HIT) & (face.cpu().numpy() >= 0)
    counts = [int((got['status'] == k).sum()) for k in range(5)]
    print('room, voxel 0.4 m, %d rays: status HIT/SKIPPED/MISS/BEHIND/LOST %s, HIT share %.3f, both hit %d'
          % (len(cloud), counts, counts[0] / len(cloud), int(both.sum())))
    print('t_tsdf - t_mesh [m] quantiles 5/25/50/75/95 %%: %s; mean %.4g, rms %.4g'
          % (_quantiles(got['t'][both] - t_mesh[both]), (got['t'][both] - t_mesh[both]).mean(), np.sqrt(((got['t'][both] - t_mesh[both]) ** 2).mean())))
    print('inc_tsdf - inc_mesh [rad] quantiles 5/25/50/75/95 %%: %s; rms %.4g'
          % (_quantiles(got['inc'][both] - inc_mesh[both]), np.sqrt(((got['inc'][both] - inc_mesh[both]) ** 2).mean())))
    assert counts[0] > 0


# ---- 4. depth bias against the fused volume ------------------------------------------------------------------------------------------
# The bar of the recovered weight: the oracle's own w moves by `spread` over random summation orders of its two sums; the device adds
# the same terms in its block order (a factor 16 of the spread of 8 orders), and its angle comes from acos01, one unit in the last place
# from the oracle's arccos: x = inc^2 enters both sums, as x y and x^2, so w moves by at most 8 x 2^-52 |w| (16 with the products).
def _w_bar(ref):
    return 16.0 * ref['spread'] + 16.0 * 2.0 ** -52 * abs(ref['before']['w'])


def test_depth_bias_against_the_fused_volume():
    from depth_correction_amd import loss as DL
    from depth_correction_amd.metrics import depth_bias, fit_bias
    from depth_correction_amd.model import ScaledPolynomial
    ref = C.bias_oracle()
    before, after = ref['before'], ref['after']
    # the oracle first: the generating model leaves a smaller mean |r|, and the fit is attenuated (printed, not gated)
    assert np.abs(after['r']).mean() < np.abs(before['r']).mean()
    clouds = _clouds(ref['scans'])
    model = ScaledPolynomial(w=[L.TRUE_W], exponent=[2.0], device=DEV)
    runs = []
    for _ in range(2):
        target = DL.TsdfTarget(C.BIAS_VOXEL, trunc=C.BIAS_TRUNC, leave_one_out=True, refresh_every=0)
        runs.append(depth_bias(clouds, ref['poses'], target, model=model, tsdf_max_range=ref['t_max']))
        torch.cuda.synchronize()
    res = runs[0]
    assert torch.equal(runs[0]['before']['out'], runs[1]['before']['out']) and torch.equal(runs[0]['after']['out'], runs[1]['after']['out'])
    # before: the volumes fused from the depths as measured are the oracle's to the bit, and so is the cast
    got = dict(status=res['status'].cpu().numpy(), face=res['face'].cpu().numpy(), t=res['t'].cpu().numpy())
    assert np.array_equal(got['status'], before['hit']['status']) and np.array_equal(got['face'], before['hit']['face'])
    assert np.array_equal(got['t'], before['hit']['t'])
    assert res['before']['totals']['used'] == int(before['used'].sum())
    # the same residuals d - t to the bit, added in another order: one rounding a term at the most on either side
    assert abs(res['before']['overall']['mean_abs'] - np.abs(before['r']).mean()) <= \
        2 * (before['r'].size + 2) * 2.0 ** -53 * np.abs(before['r']).max()
    # before and after (whose volumes are fused from the depths the device's model corrects: not the oracle's bits): the totals are
    # consistent with the cast's own status -- every ray is in the mask, so used = HIT and used + left out = rays
    for part, st in (('before', 'status'), ('after', 'status_after')):
        status = res[st].cpu().numpy()
        tot = res[part]['totals']
        left_out = int((status != C.HIT).sum())
        assert tot['rays'] == len(status) and tot['used'] == tot['hits'] == int((status == C.HIT).sum()), part
        assert tot['used'] + left_out == tot['rays'], part
    fit = fit_bias(res, 'ScaledPolynomial', [2.0])
    w = float(fit['w_true_angles'][0])
    print('fit against the own volume: w %.15g (oracle %.15g, |diff| %.3g, bar %.3g); generating w %.3g: attenuation %.3f; mean |r| before '
          '%.5f m, after %.5f m' % (w, before['w'], abs(w - before['w']), _w_bar(ref), L.TRUE_W, before['w'] / L.TRUE_W,
                                    res['before']['overall']['mean_abs'], res['after']['overall']['mean_abs']))
    assert abs(w - before['w']) <= _w_bar(ref)
    assert res['after']['overall']['mean_abs'] < res['before']['overall']['mean_abs']
    # a SparseTsdfVolume as the truth: no exclusion, one cast for before and after
    plain = depth_bias(clouds, ref['poses'], target.total, model=model, tsdf_max_range=ref['t_max'])
    assert 'status' in plain and 'status_after' not in plain and plain['after'] is not None
    assert plain['before']['totals']['used'] > res['before']['totals']['used']


def test_eval_bias_against_tsdf(tmp_path, capsys):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_bias
    from test_gpu_bias import _room_setup
    cfg, biased, model, poses = _room_setup(tmp_path, [0.05], [2.0])
    cfg.bias_eval_against = 'tsdf'
    cfg.bias_eval_csv, cfg.bias_eval_curve_csv = str(tmp_path / 'bias.csv'), str(tmp_path / 'curve.csv')
    path = str(tmp_path / 'cfg.yaml')
    cfg.to_yaml(path)
    back = Config().from_yaml(path)
    assert (back.bias_eval_against, back.bias_eval_tsdf_voxel_size, back.bias_eval_tsdf_trunc, back.bias_eval_tsdf_min_count,
            back.bias_eval_tsdf_leave_one_out, back.bias_eval_tsdf_step, back.bias_eval_tsdf_max_range) == ('tsdf', 0.1, None, 1, True, None, None)
    res = eval_bias(cfg, test_datasets=[biased], model=model)[0]
    out = capsys.readouterr().out
    assert 'Depth bias on' in out and 'supervised ScaledPolynomial fit' in out
    tot = res['before']['totals']
    in_mask = torch.ones_like(res['status'], dtype=torch.bool) if res['mask'] is None else res['mask']
    assert tot['used'] > 1000 and tot['hits'] == int(((res['status'] == C.HIT) & in_mask).sum().item()) and tot['used'] <= tot['hits']
    assert 'status_after' in res and 't_after' in res and 'face_after' in res and 'inc_after' in res
    line = open(cfg.bias_eval_csv).read().split()
    assert int(line[1]) == tot['used'] and len(line) == 11
    assert len(open(cfg.bias_eval_curve_csv).read().splitlines()) == 1 + res['bins']
    with capsys.disabled():
        print('\neval_bias against tsdf: used %d of %d, mean |r| before %.5f m, after %.5f m, w at true angles %s (generating 0.05)'
              % (tot['used'], tot['rays'], res['before']['overall']['mean_abs'], res['after']['overall']['mean_abs'], res['fit']['w_true_angles']))
    cfg.bias_eval_against = 'volume'
    with pytest.raises(ValueError, match='bias_eval_against'):
        eval_bias(cfg, test_datasets=[biased], model=model)
