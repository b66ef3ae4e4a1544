"""Range-image neighbourhoods on the MI355X (csrc/dc_rangeimage.hip, depth_correction_amd/range_image.py) against the numpy
restatement tests/rangeimage_reference.py: projection and organise (winner rule, ties, rejected rows, sizes around a block), window
features against the fp64 closed form with dc_features_fwd on the same table as the yardstick, a room that is exactly planar, the
scan-shadow mask against dc_shadow_filter, and the Python entry points."""
import numpy as np
import pytest
import torch

import rangeimage_reference as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS = {torch.float32: float(np.finfo(np.float32).eps), torch.float64: float(np.finfo(np.float64).eps)}


def npy(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype)


# ---- 1. projection and organise ------------------------------------------------------------------------------------------------
def _collision_cloud(np_dtype):
    """~3 000 points on an 8 x 32 grid: many per pixel, exact depth ties, NaN / zero / out-of-fov rows, the seam points."""
    rng = np.random.default_rng(11)
    base = (rng.normal(size=(700, 3)) * np.array([4.0, 4.0, 1.2])).astype(np_dtype).astype(np.float64)
    scale = rng.choice([1.0, 2.0, 4.0], size=(700, 1))               # powers of two: same direction, depths that tie exactly
    seam = np.array([[1, 0, 0], [-1, 0.0, 0], [-1, -0.0, 0], [0, 1, 0], [0, -1, 0], [2, 2, 0], [3, 0, 3]], dtype=np.float64)
    bad = np.array([[np.nan, 1, 1], [0, 0, 0], [1, np.inf, 0], [0.1, 0.07, 5.0], [0.13, 0.1, -7.0]])
    pts = np.concatenate([base * scale, base, seam, base * scale, bad, base, base * 2.0, seam])
    pts = pts[rng.permutation(len(pts))]
    return pts.astype(np_dtype), len(base)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_projection_and_organize(dtype):
    from depth_correction_amd import range_image as ri
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    H, W, up, down = 8, 32, 45.0, -45.0
    grid = ri.SphericalGrid(H, W, up, down)
    pts_all, _ = _collision_cloud(np_dtype)
    assert 2900 < len(pts_all) < 3600
    wide = pts_all.astype(np.float64)                               # the device widens the rows before it projects them
    # the band rule: no random point within 1e-9 pixel of a pixel edge (the designed seam points sit ON edges, decided exactly)
    on_edge = ref.near_pixel_edge(wide, H, W, up, down)
    designed = (np.nan_to_num(wide) == np.rint(np.nan_to_num(wide))).all(axis=1)          # (integer coordinates: only the designed rows)
    assert not (on_edge & ~designed).any()
    for clamp in (True, False):
        for n in (len(pts_all), 0, 1, 255, 256, 257):
            pts = pts_all[:n]
            want_pix, depth = ref.pixel_rule(wide[:n], H, W, up, down, clamp=clamp)
            want_idx, want_rng = ref.winners(want_pix, depth, H * W)
            src, pix_sorted, compact = ref.organize(want_idx)
            pixel, index_image, range_image = ri.project(dev(pts.reshape(n, 3)), grid, clamp=clamp)
            assert np.array_equal(npy(pixel), want_pix), (clamp, n)
            assert np.array_equal(npy(index_image).ravel(), want_idx), (clamp, n)
            assert np.array_equal(npy(range_image).ravel(), want_rng.astype(np_dtype)), (clamp, n)
            cloud = ri.organize(dev(pts.reshape(n, 3)), grid, clamp=clamp, want_index=True)
            assert len(cloud) == len(src)
            assert np.array_equal(npy(cloud.source_index), src) and np.array_equal(npy(cloud.pixel), pix_sorted)
            assert np.array_equal(npy(cloud.index_image).ravel(), compact)
            assert cloud.depth.dtype == dtype and cloud.depth.shape == (len(src), 1)
            if n:
                # the fields are DepthCloud.from_points' of the winners
                x = pts[src].astype(np_dtype)
                d = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
                assert np.array_equal(npy(cloud.depth)[:, 0], d)
                assert np.array_equal(npy(cloud.dirs), x / d[:, None])
                assert np.array_equal(npy(cloud.points), d[:, None] * (x / d[:, None]))
                assert not npy(cloud.vps).any()
            if n == len(pts_all):
                assert len(src) > 0.75 * H * W
                ties = sum(1 for p in range(H * W) if want_idx[p] >= 0 and (depth[want_pix == p] == want_rng[p]).sum() > 1)
                assert ties > H * W // 2                             # the lower index had to win in most pixels
                assert (want_pix < 0).sum() >= (3 if clamp else 5)
                # two runs are bit-identical
                again = ri.organize(dev(pts), grid, clamp=clamp, want_index=True)
                for f in ('vps', 'dirs', 'depth', 'points', 'pixel', 'index_image', 'source_index'):
                    assert torch.equal(getattr(cloud, f), getattr(again, f)), f
                p2, i2, r2 = ri.project(dev(pts), grid, clamp=clamp)
                assert torch.equal(p2, pixel) and torch.equal(i2, index_image) and torch.equal(r2, range_image)
                # a zero viewpoint row changes nothing; a depth bound rejects the near rows
                p3, i3, _ = ri.project(dev(pts), grid, vps=torch.zeros((1, 3), dtype=dtype, device=DEV), clamp=clamp)
                assert torch.equal(p3, pixel) and torch.equal(i3, index_image)
                p4, _, _ = ri.project(dev(pts), grid, clamp=clamp, min_depth=3.0)
                assert np.array_equal(npy(p4), ref.pixel_rule(wide, H, W, up, down, clamp=clamp, min_depth=3.0)[0])


def test_organize_of_an_h_by_w_array_needs_no_projection():
    """dc_range_from_grid: row-major order is the pixel order, validity is finite and depth > min_depth."""
    from depth_correction_amd import range_image as ri
    H, W = 5, 37
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(H, W, 3)) * 3.0
    pts[0, 0] = np.nan
    pts[2, 5] = 0.0
    pts[4, 36] = [np.inf, 0, 0]
    pts[3, 3] = [0.5, 0, 0]
    cloud = ri.organize(dev(pts), ri.SphericalGrid(H, W, 45, -45), min_depth=1.0, want_index=True)
    d = np.linalg.norm(pts.reshape(-1, 3), axis=1)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(pts.reshape(-1, 3)).all(axis=1) & (d > 1.0)
    assert not ok[[0, 2 * W + 5, 4 * W + 36, 3 * W + 3]].any()
    want = np.nonzero(ok)[0]
    assert np.array_equal(npy(cloud.pixel), want) and np.array_equal(npy(cloud.source_index), want)
    compact = np.full(H * W, -1)
    compact[want] = np.arange(len(want))
    assert np.array_equal(npy(cloud.index_image).ravel(), compact)
    x = pts.reshape(-1, 3)[want]
    dd = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    assert np.array_equal(npy(cloud.depth)[:, 0], dd) and np.array_equal(npy(cloud.dirs), x / dd[:, None])
    with pytest.raises(ValueError):
        ri.organize(dev(pts), ri.SphericalGrid(H, W + 1, 45, -45))


# ---- 2. features ---------------------------------------------------------------------------------------------------------------
WINDOWS = [(1, 1), (2, 2), (3, 3), (1, 4), (0, 3), (5, 5)]           # (5, 5) in float64 is past the staged form's LDS budget: direct form


def _synthetic_image(H, W, fill, seed):
    """An organised cloud made by hand: a point per occupied pixel along the pixel's (jittered) direction at a smooth depth."""
    rng = np.random.default_rng(seed)
    occupied = rng.random(H * W) < fill
    pix = np.nonzero(occupied)[0].astype(np.int32)
    r, c = pix // W, pix % W
    yaw = (2.0 * (c + 0.5 + 0.6 * (rng.random(len(pix)) - 0.5)) / W - 1.0) * np.pi
    pitch = (1.0 - (r + 0.5 + 0.6 * (rng.random(len(pix)) - 0.5)) / H) * (np.pi / 4) - np.pi / 8
    depth = 3.0 + 0.4 * np.sin(3.0 * yaw) + 0.3 * np.cos(5.0 * pitch) + 0.02 * rng.normal(size=len(pix))
    d = np.stack([np.cos(pitch) * np.cos(yaw), -np.cos(pitch) * np.sin(yaw), np.sin(pitch)], axis=1)
    index_image = np.full(H * W, -1, dtype=np.int32)
    index_image[pix] = np.arange(len(pix), dtype=np.int32)
    return d * depth[:, None], pix, index_image


def _errors(got, want, nvalid, dtype):
    """Largest error of every compared field: mean relative to |mean|, cov and eigvals relative to the largest eigenvalue, normals and
    incidence angles absolute; eigen-quantities only where nvalid >= 3."""
    lam2 = np.maximum(want['eigvals'][:, 2], np.finfo(np.float64).tiny)
    full = nvalid >= 3
    out = {}
    out['mean'] = float(np.max(np.abs(npy(got['mean']).astype(np.float64) - want['mean']).max(axis=1) / np.abs(want['mean']).max(axis=1), initial=0.0))
    multi = nvalid >= 2
    out['cov'] = float(np.max((np.abs(npy(got['cov']).astype(np.float64) - want['cov']).reshape(-1, 9).max(axis=1) / lam2)[multi], initial=0.0))
    out['eigvals'] = float(np.max((np.abs(npy(got['eigvals']).astype(np.float64) - want['eigvals']).max(axis=1) / lam2)[full], initial=0.0))
    out['normals'] = float(np.max(np.abs(npy(got['normals']).astype(np.float64) - want['normals']).max(axis=1)[full], initial=0.0))
    out['inc_angles'] = float(np.max(np.abs(npy(got['inc_angles']).astype(np.float64) - want['inc_angles'])[:, 0][full], initial=0.0))
    return out


def _check_against_yardstick(new, old, want, nvalid, dtype, tag):
    """The new kernel may err at most 2 x what dc_features_fwd errs on the same table (it shares the arithmetic: only the summation
    order may differ), with a floor of 4 ulp of the dtype (relative to the largest eigenvalue for cov / eigvals)."""
    e_new, e_old = _errors(new, want, nvalid, dtype), _errors(old, want, nvalid, dtype)
    print('%s errors new / dc_features_fwd: %s' % (tag, ', '.join('%s %.2e / %.2e' % (f, e_new[f], e_old[f]) for f in e_new)))
    for f in e_new:
        assert e_new[f] <= max(2.0 * e_old[f], 4.0 * EPS[dtype]), (tag, f, e_new[f], e_old[f])
    return e_new, e_old


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('wrap', [True, False])
@pytest.mark.parametrize('size', [(16, 128), (13, 70), (3, 5)])
def test_window_features(size, wrap, dtype):
    from depth_correction_amd import ops, range_image as ri
    H, W = size
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    grid = ri.SphericalGrid(H, W, 22.5, -22.5, wrap=wrap)
    x, pix, index_image = _synthetic_image(H, W, 0.7 if H > 3 else 0.8, seed=H * W)
    x = x.astype(np_dtype)
    dirs = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np_dtype)
    xd, dd, pd, id_ = dev(x), dev(dirs), dev(pix), dev(index_image.reshape(H, W))
    x64, d64 = x.astype(np.float64), dirs.astype(np.float64)
    checked = 0
    for ah, aw in WINDOWS:
        if not ref.window_ok(H, W, ah, aw):
            with pytest.raises(RuntimeError, match='invalid argument'):
                ops.image_features_fwd(xd, dd, pd, id_, grid, (ah, aw), r=0.5)
            continue
        for r in ((0.5, None) if (ah, aw) == (1, 1) else (0.5,)):
            table = ref.neighbor_table(x64, pix, index_image, H, W, wrap, ah, aw, r)
            want = ref.features(x64, d64, table)
            new = ops.image_features_fwd(xd, dd, pd, id_, grid, (ah, aw), r=r)
            assert np.array_equal(npy(new['neighbors']), table), (ah, aw, r)
            assert np.array_equal(npy(new['nvalid']), want['nvalid']), (ah, aw, r)
            old = ops.features_fwd(xd, dev(table), dirs=dd)
            _check_against_yardstick(new, old, want, want['nvalid'], dtype, '%dx%d wrap=%d %s window (%d,%d) r=%s' % (H, W, wrap, np_dtype.__name__, ah, aw, r))
            checked += 1
            if r == 0.5 and (ah, aw) == (2, 2):                      # (the gate is not idle)
                assert (table >= 0).sum() < (ref.neighbor_table(x64, pix, index_image, H, W, wrap, ah, aw, None) >= 0).sum()
    assert checked >= (2 if H == 3 else 7)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_window_gate_is_inclusive_and_empty_images(dtype):
    """A neighbour exactly r = 0.5 away is a member, one ulp farther is not (coordinates exactly representable); an image with every
    pixel empty; a window that is the whole row."""
    from depth_correction_amd import ops, range_image as ri
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    H, W = 3, 5
    grid = ri.SphericalGrid(H, W, 45, -45, wrap=True)
    x = np.array([[2.0, 0, 0], [2.5, 0, 0], [np.nextafter(np_dtype(2.5), np_dtype(3.0)), 0, 0], [2.0, 0.5, 0], [2.0, 0.25, 0.25]], dtype=np_dtype)
    pix = np.array([1 * W + 1, 1 * W + 2, 1 * W + 3, 2 * W + 2, 0 * W + 2], dtype=np.int32)
    order = np.argsort(pix)
    x, pix = x[order], pix[order]
    index_image = np.full(H * W, -1, dtype=np.int32)
    index_image[pix] = np.arange(len(pix))
    dirs = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np_dtype)
    xd, dd, pd, id_ = dev(x), dev(dirs), dev(pix), dev(index_image.reshape(H, W))
    for window in ((1, 1), (1, 2), (0, 2)):
        table = ref.neighbor_table(x.astype(np.float64), pix, index_image, H, W, True, window[0], window[1], 0.5)
        new = ops.image_features_fwd(xd, dd, pd, id_, grid, window, r=0.5)
        assert np.array_equal(npy(new['neighbors']), table)
    # the row of the point at (2, 0, 0): (2.5, 0, 0) is in, its one-ulp neighbour is out
    table = ref.neighbor_table(x.astype(np.float64), pix, index_image, H, W, True, 1, 2, 0.5)
    i0 = int(np.nonzero((x == np.array([2.0, 0, 0], dtype=np_dtype)).all(axis=1))[0][0])
    i_on = int(np.nonzero(x[:, 0] == np_dtype(2.5))[0][0])
    i_off = int(np.nonzero(x[:, 0] > np_dtype(2.5))[0][0])
    assert i_on in table[i0] and i_off not in table[i0]
    got = npy(ops.image_features_fwd(xd, dd, pd, id_, grid, (1, 2), r=0.5)['neighbors'])
    assert i_on in got[i0] and i_off not in got[i0]
    # every pixel empty
    e = ops.image_features_fwd(xd[:0], dd[:0], pd[:0], torch.full((H, W), -1, dtype=torch.int32, device=DEV), grid, (1, 1), r=0.5)
    assert e['mean'].shape == (0, 3) and e['neighbors'].shape == (0, 9) and e['nvalid'].shape == (0,)


# ---- 3. a room that is exactly planar ------------------------------------------------------------------------------------------
ROOM = dict(rows=16, cols=128, fov_up=22.5, fov_down=-22.5)


@pytest.fixture(scope='module')
def room():
    from depth_correction_amd import range_image as ri
    pts, wall, normals = ref.room_scan(**ROOM)
    H, W = ROOM['rows'], ROOM['cols']
    pix, _ = ref.pixel_rule(pts, H, W, ROOM['fov_up'], ROOM['fov_down'])
    assert np.array_equal(pix, np.arange(H * W))                    # every ray returns to its own pixel
    assert not ref.near_pixel_edge(pts, H, W, ROOM['fov_up'], ROOM['fov_down']).any()
    grid = ri.SphericalGrid(H, W, ROOM['fov_up'], ROOM['fov_down'])
    return dict(points=pts, wall=wall, normals=normals, grid=grid, H=H, W=W)


def test_planar_room_normals_and_incidence(room):
    from depth_correction_amd import ops, range_image as ri
    H, W, grid = room['H'], room['W'], room['grid']
    cloud = ri.organize(dev(room['points']), grid)
    assert len(cloud) == H * W and np.array_equal(npy(cloud.pixel), np.arange(H * W))
    x, dirs = npy(cloud.points), npy(cloud.dirs)
    wall = room['wall']
    full = np.zeros(H * W, dtype=bool)
    for p in range(H * W):
        slots = ref.window_slots(H, W, True, p // W, p % W, 2, 2)
        full[p] = (slots >= 0).all() and (wall[slots] == wall[p]).all()
    print('pixels with a full 5 x 5 window on one wall: %.3f' % full.mean())
    assert full.mean() >= 0.5                                       # (61 % in this scene)
    true_n = room['normals'][wall]
    true_inc = np.arccos(np.minimum(np.abs((dirs * true_n).sum(axis=1)), 1.0))
    table = ref.neighbor_table(x, npy(cloud.pixel), npy(cloud.index_image).ravel(), H, W, True, 2, 2, None)
    ri.image_features(cloud, (2, 2), r=None)
    assert np.array_equal(npy(cloud.neighbors), table)
    old = ops.features_fwd(cloud.points, dev(table), dirs=cloud.dirs)
    e = {}
    for name, f in (('new', dict(normals=cloud.normals, inc_angles=cloud.inc_angles)), ('old', old)):
        e[name] = (float(np.abs(npy(f['normals']) - true_n)[full].max()), float(np.abs(npy(f['inc_angles'])[:, 0] - true_inc)[full].max()))
    print('planar room: normal / incidence error new %.2e / %.2e, dc_features_fwd %.2e / %.2e' % (e['new'] + e['old']))
    floor = 4.0 * EPS[torch.float64]
    assert e['new'][0] <= max(2.0 * e['old'][0], floor) and e['new'][1] <= max(2.0 * e['old'][1], floor)
    assert e['old'][0] < 1e-9 and e['old'][1] < 1e-7                # the yardstick itself finds the walls


# ---- 4. shadow -----------------------------------------------------------------------------------------------------------------
def test_image_shadow_mask_equals_shadow_filter(room):
    from depth_correction_amd import ops, range_image as ri
    from depth_correction_amd.filters import _shadow_bounds
    from depth_correction_amd.nearest_neighbors import ball_angle_to_distance
    H, W, grid = room['H'], room['W'], room['grid']
    alpha, bounds = 0.06, [0.3, float('inf')]
    r = float(ball_angle_to_distance(torch.as_tensor(alpha)))
    lo, hi, _ = _shadow_bounds(bounds)
    window = ri.shadow_window(grid, alpha)
    pts = room['points']
    depth = np.linalg.norm(pts, axis=1)
    rng = np.random.default_rng(5)
    moved = rng.choice(H * W, 200, replace=False)
    pulled = pts.copy()
    pulled[moved] = pts[moved] / depth[moved, None] * (depth[moved] - 0.3)[:, None]          # 0.3 m towards the sensor
    outcomes = []
    for name, scan in (('room', pts), ('pulled', pulled)):
        cloud = ri.organize(dev(scan), grid)
        assert np.array_equal(npy(cloud.pixel), np.arange(H * W))
        nbrs = ref.direction_neighbors(npy(cloud.dirs), r)
        holds, dr, dc = ref.window_holds(nbrs, npy(cloud.pixel).astype(np.int64), W, H, True, 1, 2)
        print('%s: direction neighbours per point %.2f, within +-%d rows and +-%d columns; window %s' % (name, nbrs.sum(axis=1).mean(), dr, dc, window))
        assert holds and window[0] >= 1 and window[1] >= 2          # every direction neighbour lies in the window Python chose
        got = ri.image_shadow_mask(cloud, alpha, bounds)
        want = ops.shadow_filter(cloud.points, cloud.vps, cloud.dirs, r, lo, hi)
        assert torch.equal(got, want), name
        assert torch.equal(ri.image_shadow_mask(cloud, alpha, bounds, window=(1, 2)), want)
        near = nbrs[moved].any(axis=0)
        outcomes.append((int((~npy(got))[near].sum()), int(npy(got)[near].sum())))
    print('removed / kept among the neighbours of the moved points: %s' % (outcomes,))
    assert outcomes[1][0] >= 20 and outcomes[1][1] >= 20
    with pytest.raises(ValueError):
        ri.shadow_window(ri.SphericalGrid(128, 1024, 45, -45), 0.1)  # more than 121 slots


# ---- 5. API --------------------------------------------------------------------------------------------------------------------
def _image_cfg(**kw):
    from depth_correction_amd.config import Config
    base = dict(local_nn_type='image', image_size=[ROOM['rows'], ROOM['cols']], image_fov=[ROOM['fov_up'], ROOM['fov_down']], image_window=[2, 2],
                nn_r=0.5, float_type='float64', device=DEV, log_filters=False, shadow_neighborhood_angle=0.06,
                shadow_angle_bounds=[0.3, float('inf')])
    base.update(kw)
    return Config(**base)


def test_api_image_neighbourhoods_from_three_inputs(room):
    from numpy.lib.recfunctions import unstructured_to_structured
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.online import correct_cloud
    from depth_correction_amd.preproc import local_feature_cloud
    H, W = room['H'], room['W']
    pts = room['points'].copy()
    depth = np.linalg.norm(pts, axis=1)
    moved = np.random.default_rng(5).choice(H * W, 200, replace=False)
    pts[moved] = pts[moved] / depth[moved, None] * (depth[moved] - 0.3)[:, None]
    cfg = _image_cfg()
    inputs = dict(device_rows=dev(pts), ndarray=pts, grid_array=unstructured_to_structured(pts, names=['x', 'y', 'z']).reshape(H, W))
    clouds = {k: local_feature_cloud(v, cfg) for k, v in inputs.items()}
    a = clouds['device_rows']
    assert 0 < len(a) < H * W                                        # the shadow mask removed rays
    assert a.mask is not None and 0 < int(a.mask.sum()) < len(a)
    assert a.neighbors.shape == (len(a), 25) and a.grid.rows == H
    for k in ('ndarray', 'grid_array'):
        for f in ('vps', 'dirs', 'depth', 'points', 'mean', 'cov', 'eigvals', 'eigvecs', 'normals', 'inc_angles', 'mask', 'neighbors', 'pixel',
                  'index_image', 'nvalid'):
            assert torch.equal(getattr(a, f), getattr(clouds[k], f)), (k, f)
    # pixel / index_image are consistent and the table is the window's
    idx = npy(a.index_image).ravel()
    assert np.array_equal(idx[npy(a.pixel)], np.arange(len(a))) and (idx >= 0).sum() == len(a)
    table = ref.neighbor_table(npy(a.points), npy(a.pixel), idx, H, W, True, 2, 2, 0.5)
    assert np.array_equal(npy(a.neighbors), table)
    # without the shadow filter every pixel survives
    b = local_feature_cloud(dev(pts), _image_cfg(shadow_angle_bounds=[]))
    assert len(b) == H * W
    # correct_cloud: the model applied to that cloud's own incidence angles and mask
    w, e = [1e-3, 2e-3], [2.0, 4.0]
    model = ScaledPolynomial(w=w, exponent=e, device=DEV)
    for k, v in inputs.items():
        c = correct_cloud(v, model, cfg)
        g = npy(a.inc_angles)[:, 0]
        want = np.where(npy(a.mask), npy(a.depth)[:, 0] * (1.0 - (w[0] * g ** e[0] + w[1] * g ** e[1])), npy(a.depth)[:, 0])
        np.testing.assert_allclose(npy(c.depth)[:, 0], want, rtol=1e-13, atol=0)
        np.testing.assert_allclose(npy(c.points), npy(c.vps) + npy(c.depth) * npy(c.dirs), rtol=1e-15, atol=1e-15)


def test_api_default_neighbourhoods_are_untouched(room):
    """With the default local_nn_type the outputs of local_feature_cloud are bit-equal to what they are without any of the new
    attributes on the configuration."""
    from depth_correction_amd.config import Config
    from depth_correction_amd.preproc import local_feature_cloud
    kw = dict(nn_k=10, nn_r=None, float_type='float64', device=DEV, shadow_neighborhood_angle=0.06, shadow_angle_bounds=[0.3, float('inf')])
    cfg = Config(**kw)
    assert cfg.local_nn_type == 'ball' and cfg.image_size == [128, 1024] and cfg.image_fov == [45., -45.] and cfg.image_wrap is True
    assert cfg.image_window == [2, 2]
    assert Config().from_dict(__import__('yaml').safe_load(cfg.to_yaml())).local_nn_type == 'ball'
    bare = Config(**kw)
    for name in ('local_nn_type', 'image_size', 'image_fov', 'image_wrap', 'image_window'):
        delattr(bare, name)
    raw = dev(room['points'])
    a, b = local_feature_cloud(raw, cfg), local_feature_cloud(raw, bare)
    assert not hasattr(a, 'pixel') and len(a) > 0
    for f in ('vps', 'dirs', 'depth', 'points', 'mean', 'cov', 'eigvals', 'eigvecs', 'normals', 'inc_angles', 'mask', 'neighbors'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    with pytest.raises(ValueError):
        local_feature_cloud(raw, Config(local_nn_type='image', image_size=[16, 128], image_fov=[22.5, -22.5], image_window=[6, 6], device=DEV))


def test_select_keeps_pixel_and_index_image_consistent(room):
    from depth_correction_amd import range_image as ri
    H, W, grid = room['H'], room['W'], room['grid']
    cloud = ri.organize(dev(room['points']), grid)
    ri.image_features(cloud, (1, 1), r=0.5)
    keep = torch.as_tensor(np.random.default_rng(1).random(len(cloud)) < 0.6, device=DEV)
    sub = ri.select(cloud, keep)
    assert ri.is_organized(sub) and sub.index_image is None and len(sub) == int(keep.sum())
    assert torch.equal(sub.pixel, cloud.pixel[keep]) and torch.equal(sub.points, cloud.points[keep]) and torch.equal(sub.eigvals, cloud.eigvals[keep])
    idx = npy(ri.index_image(sub)).ravel()
    assert np.array_equal(idx[npy(sub.pixel)], np.arange(len(sub))) and (idx >= 0).sum() == len(sub)
    assert not ri.is_organized(cloud[keep])                         # plain slicing loses the attributes
    # the range image of the survivors and its inverse at the pixel centres
    pixel, index_image, range_image = ri.project(sub, grid)
    assert np.array_equal(npy(pixel), npy(sub.pixel)) and np.array_equal(npy(index_image).ravel(), idx)
    back = ri.depth_to_points(range_image, grid)
    p2, _, _ = ri.project(back, grid)
    assert np.array_equal(npy(p2), npy(sub.pixel))                  # a pixel centre projects to its own pixel
    np.testing.assert_allclose(npy(back.norm(dim=1)), npy(sub.depth)[:, 0], rtol=1e-14)
