"""Finite-beam rendering on the GPU: dc_beam_subrays and dc_raycast_beams stage by stage against raycast_rays on the emitted sub-rays
and the numpy restatement of the reduction (tests/beam_reference.py), the per-beam invariants, an analytic tilted plane, a depth
edge, and the rendered dataset end to end through depth_bias / fit_bias."""
import math

import numpy as np
import pytest
import torch

import beam_reference as R
from helpers import slam_pose
from test_beam_host import R0, SPREAD, beams_for_subrays, check_subrays

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -52
T_MIN = 0.05


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bvh(verts, faces):
    from depth_correction_amd.mesh import TriangleMesh
    return TriangleMesh(verts, faces).on_device(DEV)[3]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. sub-rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('S', [1, 4, 16, 64])
def test_subrays(S, dtype):
    from depth_correction_amd import ops
    vps, dirs = beams_for_subrays()
    vps_d, dirs_d = _dev(vps, dtype), _dev(dirs, dtype)
    pat = R.pattern(S)
    o, D = ops.beam_subrays(vps_d, dirs_d, pat, R0, SPREAD)
    assert o.shape == D.shape == (len(dirs), S, 3) and o.dtype == D.dtype == torch.float64
    # fp32 inputs are converted exactly: the reference takes the same values
    check_subrays(o.cpu().numpy(), D.cpu().numpy(), vps_d.double().cpu().numpy(), dirs_d.double().cpu().numpy(), pat)
    bad = _dev([[0, 0, 0], [float('nan'), 1, 0], [float('inf'), 0, 0]], dtype)
    o, D = ops.beam_subrays(torch.zeros_like(bad), bad, pat, R0, SPREAD)
    assert torch.isnan(o).all() and torch.isnan(D).all()
    o, D = ops.beam_subrays(vps_d[:0], dirs_d[:0], pat, R0, SPREAD)
    assert o.shape == (0, S, 3) and D.shape == (0, S, 3)


# ---- 2. stage by stage ----------------------------------------------------------------------------------------------------------------
COUNTS = (300, 0, 500, 1, 400)


@pytest.fixture(scope='module')
def scene():
    """The triangle soup and five scans of beams: random rotations, view points N(0, 0.3), directions that are not unit."""
    verts, faces, rng = R.soup(33, 6000, 15.0, 0.5)
    n = sum(COUNTS)
    poses = np.stack([slam_pose(rng.uniform(-math.pi, math.pi), rng.normal(scale=0.5, size=3), roll=rng.uniform(-math.pi, math.pi),
                                pitch=rng.uniform(-1.0, 1.0)) for _ in COUNTS])
    vps = rng.normal(scale=0.3, size=(n, 3))
    dirs = rng.normal(size=(n, 3)) * rng.uniform(0.3, 4.0, size=(n, 1))
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    return dict(bvh=_bvh(verts, faces), vps=_dev(vps), dirs=_dev(dirs), off=off, poses=_dev(poses), n=n)


def _cast(scene, S, cull, weight, detection='quantile', tau=None, min_hits=1, want_samples=True):
    from depth_correction_amd import ops
    out = ops.raycast_beams(scene['bvh'], scene['vps'], scene['dirs'], scene['off'], scene['poses'], R.pattern(S), R0, SPREAD, t_min=T_MIN,
                            cull=cull, weight=weight, detection=detection, tau=tau, min_hits=min_hits, want_samples=want_samples)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize('weight', ['uniform', 'lambert'])
@pytest.mark.parametrize('cull', [True, False])
@pytest.mark.parametrize('S', [1, 16, 64])
def test_stage_by_stage(scene, S, cull, weight):
    """The sub-ray returns are raycast_rays' on the emitted sub-rays, bit for bit; the weights are the pattern's (uniform) or the cosine
    of that call's incidence angle (lambert); the reduction is beam_reference.reduce of those returns.

    The lambert bar is 4 ulp with the ulp taken at the scale of the weights, 2^-52: |w - cos(inc)| <= 4 * 2^-52.  The weight is the
    cosine c itself; the reference cos(arccos(c)) goes through an angle rounded to fp64 in [0, pi/2], which alone moves its cosine by
    up to sin(inc) ulp(inc) / 2 = 2^-53 near grazing incidence, whatever the size of c.  Measured on the MI355X: 0.50 x 2^-52 in all
    six cases; counted in spacings of cos(inc) itself the same differences are 9 to 126 (at small cosines), all of it the rounding of
    the reference's angle."""
    from depth_correction_amd import ops
    n, pat = scene['n'], R.pattern(S)
    face, depth, n_hits, sub_face, sub_t, sub_w = _cast(scene, S, cull, weight)
    # the sub-rays, cast one by one
    o, D = ops.beam_subrays(scene['vps'], scene['dirs'], pat, R0, SPREAD)
    rf, rt, rinc = ops.raycast_rays(scene['bvh'], o.reshape(-1, 3), D.reshape(-1, 3), scene['off'] * S, scene['poses'], t_min=T_MIN, cull=cull)
    rf, rt, rinc = rf.cpu().numpy().reshape(n, S), rt.cpu().numpy().reshape(n, S), rinc.cpu().numpy().reshape(n, S)
    assert np.array_equal(sub_face, rf) and np.array_equal(_bits(sub_t), _bits(rt))
    hit = rf >= 0
    if weight == 'uniform':
        assert np.array_equal(sub_w, np.where(hit, pat[None, :, 2], 0.0))
    else:
        err = np.abs(sub_w[hit] - pat[None, :, 2].repeat(n, 0)[hit] * np.cos(rinc[hit]))
        print('lambert: max |w - cos(inc)| = %.3g (%.2f x 2^-52; %.1f spacings of cos(inc))'
              % (err.max(), err.max() / EPS, (err / np.spacing(np.cos(rinc[hit]))).max()))
        assert (err <= 4 * EPS).all() and (sub_w[~hit] == 0.0).all()
        assert (sub_w[hit] > 0).all() and (sub_w[hit] <= 1.0).all()
    # what the test needs to see
    full, none = n_hits == S, n_hits == 0
    partial = ~full & ~none
    many_faces = np.array([len(set(sub_face[i][sub_face[i] >= 0])) > 1 for i in range(n)])
    print('S %d cull %d %s: no hit %.1f %%, partial %.1f %%, full %.1f %%, hit beams on several faces %.1f %%'
          % (S, cull, weight, 100 * none.mean(), 100 * partial.mean(), 100 * full.mean(), 100 * many_faces[~none].mean()))
    if S == 16:
        assert none.mean() >= 0.10 and partial.mean() >= 0.10 and full.mean() >= 0.10 and many_faces[~none].mean() >= 0.05
    # the reduction
    assert np.array_equal(n_hits, hit.sum(axis=1))
    lo = np.where(hit, sub_t, np.inf).min(axis=1)
    hi = np.where(hit, sub_t, -np.inf).max(axis=1)
    for tau in (1.0 / S, 0.5, 1.0):
        f, d, h, sf, st, sw = _cast(scene, S, cull, weight, tau=tau)
        assert np.array_equal(sf, sub_face) and np.array_equal(_bits(st), _bits(sub_t)) and np.array_equal(_bits(sw), _bits(sub_w))
        f_ref, d_ref, h_ref = R.reduce(sub_face, sub_t, sub_w, R.QUANTILE, tau, 1)
        assert np.array_equal(h, h_ref) and np.array_equal(f, f_ref) and np.array_equal(_bits(d), _bits(d_ref)), tau
        assert np.array_equal(f < 0, none) and np.isinf(d[none]).all()
        if weight == 'uniform' and tau != 0.5:                  # 3. the first return is the nearest hit, the last the farthest
            assert np.array_equal(_bits(d[~none]), _bits((lo if tau < 1.0 else hi)[~none]))
    f, d, h = _cast(scene, S, cull, weight, detection='mean', want_samples=False)
    f_ref, d_ref, h_ref = R.reduce(sub_face, sub_t, sub_w, R.MEAN, 0.5, 1)
    assert np.array_equal(h, h_ref) and np.array_equal(np.isinf(d), np.isinf(d_ref)) and np.array_equal(f < 0, f_ref < 0)
    ok = np.isfinite(d_ref)
    assert (np.abs(d[ok] - d_ref[ok]) <= S * EPS * d_ref[ok]).all()
    assert np.array_equal(f[ok & (d == d_ref)], f_ref[ok & (d == d_ref)])
    assert (d[ok] >= lo[ok] * (1 - S * EPS)).all() and (d[ok] <= hi[ok] * (1 + S * EPS)).all()
    if S > 1:
        spread_out = ok & (hi > lo * (1 + 1e-9))
        assert spread_out.any() and (d[spread_out] > lo[spread_out]).all() and (d[spread_out] < hi[spread_out]).all()
    # min_hits = S turns exactly the partial bundles into misses
    f, d, h = _cast(scene, S, cull, weight, min_hits=S, want_samples=False)
    assert np.array_equal(h, n_hits) and np.array_equal(f >= 0, full) and np.array_equal(np.isfinite(d), full)
    assert np.array_equal(f[full], face[full]) and np.array_equal(_bits(d[full]), _bits(depth[full]))


# ---- 3. per-beam invariants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_one_sample_is_the_thin_ray(scene, dtype):
    """S = 1 with the pattern [(0, 0, 1)]: the beam is the ray along d from the view point."""
    from depth_correction_amd import ops
    vps, dirs = scene['vps'].to(dtype), scene['dirs'].to(dtype)
    pat = np.array([[0.0, 0.0, 1.0]])
    face, depth, n_hits = ops.raycast_beams(scene['bvh'], vps, dirs, scene['off'], scene['poses'], pat, R0, SPREAD, t_min=T_MIN, tau=1.0)
    s = dirs.double().cpu().numpy()
    dhat = _dev(s / np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None])
    rf, rt, _ = ops.raycast_rays(scene['bvh'], vps.double(), dhat, scene['off'], scene['poses'], t_min=T_MIN)
    assert torch.equal(face, rf) and torch.equal(depth, rt) and torch.equal(n_hits, (rf >= 0).int())
    assert 0.2 < (rf >= 0).double().mean() < 0.9


def test_reproducible_and_per_beam_t_min(scene):
    from depth_correction_amd import ops
    args = (scene['bvh'], scene['vps'], scene['dirs'], scene['off'], scene['poses'], R.pattern(16), R0, SPREAD)
    a = ops.raycast_beams(*args, t_min=T_MIN, weight='lambert', tau=0.5, want_samples=True)
    b = ops.raycast_beams(*args, t_min=T_MIN, weight='lambert', tau=0.5, want_samples=True)
    assert all(torch.equal(x.view(torch.int32 if x.dtype == torch.int32 else torch.int64),
                           y.view(torch.int32 if y.dtype == torch.int32 else torch.int64)) for x, y in zip(a, b))
    # a tensor of near clips, all equal, is the scalar
    c = ops.raycast_beams(*args, t_min=torch.full((scene['n'],), T_MIN, dtype=torch.float64, device=DEV), weight='lambert', tau=0.5)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], c))
    # and one beyond every hit of a beam turns that beam into a miss
    far = torch.where(torch.arange(scene['n'], device=DEV) % 2 == 0, 1e3, T_MIN).double()
    d = ops.raycast_beams(*args, t_min=far, weight='lambert', tau=0.5)
    assert (d[0][0::2] < 0).all() and torch.equal(d[0][1::2], a[0][1::2]) and torch.equal(d[1][1::2], a[1][1::2])


def test_empty_and_all_miss(scene):
    from depth_correction_amd import ops
    pat = R.pattern(16)
    z = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    out = ops.raycast_beams(scene['bvh'], z, z, [0] * 6, scene['poses'], pat, R0, SPREAD, want_samples=True)
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,), (0, 16), (0, 16), (0, 16)]
    # a scene of one small triangle far behind every beam
    tri = _bvh(np.array([[-500.0, 0, 0], [-500.0, 1, 0], [-500.0, 0, 1]]), np.array([[0, 1, 2]], dtype=np.int32))
    dirs = _dev(np.abs(np.random.default_rng(2).normal(size=(77, 3))) + 0.1)
    face, depth, n_hits, sf, st, sw = ops.raycast_beams(tri, torch.zeros_like(dirs), dirs, [0, 77], torch.eye(4, dtype=torch.float64, device=DEV)[None],
                                                        pat, R0, SPREAD, cull=False, want_samples=True)
    assert (face == -1).all() and torch.isinf(depth).all() and (n_hits == 0).all()
    assert (sf == -1).all() and torch.isinf(st).all() and (sw == 0).all()
    # beams without a direction are misses among beams that hit
    wall = _bvh(np.array([[5.0, -50, -50], [5.0, 50, -50], [5.0, 0, 80]]), np.array([[0, 1, 2]], dtype=np.int32))
    dirs = _dev([[1.0, 0, 0], [0, 0, 0], [2.0, 0.1, 0], [float('nan'), 0, 0]])
    face, depth, n_hits = ops.raycast_beams(wall, torch.zeros_like(dirs), dirs, [0, 4], torch.eye(4, dtype=torch.float64, device=DEV)[None],
                                            pat, R0, SPREAD, cull=False)
    assert face.tolist() == [0, -1, 0, -1] and n_hits.tolist() == [16, 0, 16, 0] and torch.isinf(depth[1::2]).all()


def test_refusals(scene):
    from depth_correction_amd import ops
    args = (scene['bvh'], scene['vps'], scene['dirs'], scene['off'], scene['poses'])
    with pytest.raises(ValueError):
        ops.raycast_beams(*args, R.pattern(12), R0, SPREAD)
    bad = R.pattern(4)
    bad[1, 2] = -1.0
    with pytest.raises(ValueError):
        ops.raycast_beams(*args, bad, R0, SPREAD)
    bad[1, 2] = float('nan')
    with pytest.raises(ValueError):
        ops.raycast_beams(*args, bad, R0, SPREAD)
    for kw in (dict(tau=0.0), dict(tau=1.1), dict(min_hits=0), dict(min_hits=5), dict(weight='x'), dict(detection='x'), dict(t_min=float('nan'))):
        with pytest.raises(ValueError):
            ops.raycast_beams(*args, R.pattern(4), R0, SPREAD, **kw)
    for r0, spread in ((-1.0, 0.0), (0.0, -1.0), (float('inf'), 0.0), (0.0, float('nan'))):
        with pytest.raises(ValueError):
            ops.raycast_beams(*args, R.pattern(4), r0, spread)
    # the library's own checks, behind the wrapper's
    from depth_correction_amd import _native as nv
    pat = np.ascontiguousarray(R.pattern(4))
    out = [torch.empty(4, dtype=t, device=DEV) for t in (torch.int32, torch.float64, torch.int32)]
    b, off = scene['bvh'], _dev(np.array([0, 4], dtype=np.int64))

    def raw(n_samples=4, r0=R0, spread=SPREAD, weight=0, detection=1, tau=0.5, min_hits=1, pattern=pat):
        return nv.lib().dc_raycast_beams(nv.ptr(b.child), nv.ptr(b.node_box), nv.ptr(b.leaf_tri), nv.ptr(b.leaf_face), b.n_faces,
                                         nv.ptr(scene['vps']), nv.ptr(scene['dirs']), nv.DC_F64, 4, nv.ptr(off),
                                         nv.ptr(scene['poses']), 1, pattern.ctypes.data, n_samples, r0, spread, None, 0.0, 1, weight, detection,
                                         tau, min_hits, nv.ptr(out[0]), nv.ptr(out[1]), nv.ptr(out[2]), None, None, None, nv.stream_ptr())
    assert raw() == 0
    torch.cuda.synchronize()
    for kw in (dict(n_samples=3), dict(n_samples=0), dict(r0=-1.0), dict(spread=float('inf')), dict(weight=2), dict(detection=2),
               dict(tau=0.0), dict(tau=float('nan')), dict(min_hits=0), dict(min_hits=5), dict(pattern=np.ascontiguousarray(bad))):
        assert raw(**kw) == nv.DC_ERR_ARG, kw


# ---- 4. analytic plane ----------------------------------------------------------------------------------------------------------------
def test_tilted_plane():
    """One large triangle through (10, 0, 0), its normal tilted by gamma from the beam about three azimuths: every sub-ray's t is the
    plane's, and the first return comes early by an amount that grows with the tilt."""
    from depth_correction_amd import ops
    S, pat = 16, R.pattern(16)
    eye = torch.eye(4, dtype=torch.float64, device=DEV)[None]
    dirs = _dev([[1.0, 0.0, 0.0]])
    vps = torch.zeros_like(dirs)
    o, D = (x.cpu().numpy()[0] for x in ops.beam_subrays(vps, dirs, pat, R0, SPREAD))
    for alpha in (0.3, 2.0, 4.4):
        rel = []
        for gamma in (0, 15, 30, 45, 60, 75):
            g = math.radians(gamma)
            nrm = np.array([math.cos(g), math.sin(g) * math.cos(alpha), math.sin(g) * math.sin(alpha)])
            u = np.cross(nrm, [0.3, -0.5, 0.8])
            u /= np.linalg.norm(u)
            v = np.cross(nrm, u)
            p0 = np.array([10.0, 0.0, 0.0])
            tri = np.stack([p0 + 900.0 * u, p0 - 450.0 * u + 780.0 * v, p0 - 450.0 * u - 780.0 * v])
            nn = np.cross(tri[1] - tri[0], tri[2] - tri[0])             # the plane of the vertices as they are stored
            want = (nn @ tri[0] - o @ nn) / (D @ nn)
            bvh = _bvh(tri, np.array([[0, 1, 2]], dtype=np.int32))
            res = {}
            for name, kw in (('first', dict(tau=1.0 / S)), ('median', dict(tau=0.5)), ('last', dict(tau=1.0)), ('mean', dict(detection='mean'))):
                face, depth, n_hits, sf, st, sw = ops.raycast_beams(bvh, vps, dirs, [0, 1], eye, pat, R0, SPREAD, cull=False, want_samples=True, **kw)
                assert n_hits.item() == S and face.item() == 0 and (sf == 0).all()
                assert np.abs(st.cpu().numpy()[0] - want).max() <= 1e-12 * want.max()
                res[name] = depth.item()
            t0 = want[0]
            assert abs(t0 - 10.0) <= 1e-11
            if gamma == 0:
                assert all(abs(d - t0) <= 1e-12 * t0 for d in res.values()), res
            else:
                assert res['first'] < res['median'] < res['last'] and res['first'] < res['mean'] < res['last']
            rel.append((res['first'] - t0) / t0)
        print('azimuth %.1f: first-return relative error %s' % (alpha, np.array2string(np.array(rel), precision=3)))
        assert all(r < 0 for r in rel[1:]) and all(b < a for a, b in zip(rel[:-1], rel[1:])), rel


# ---- 5. a depth edge ------------------------------------------------------------------------------------------------------------------
def test_depth_edge():
    """A wall at 5 m that ends at y = 0 in front of a wall at 6 m, a beam centred on the step: the first return is the near wall, the
    last the far one, the mean a mixed point between them."""
    from depth_correction_amd import ops
    S, pat = 64, R.pattern(64)
    verts = np.array([[5.0, -10, -10], [5.0, 0, -10], [5.0, 0, 10], [5.0, -10, 10],
                      [6.0, -10, -10], [6.0, 10, -10], [6.0, 10, 10], [6.0, -10, 10]])
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)
    bvh = _bvh(verts, faces)
    dirs = _dev([[1.0, 0.0, 0.0]])
    eye = torch.eye(4, dtype=torch.float64, device=DEV)[None]
    res = {}
    for name, kw in (('first', dict(tau=1.0 / S)), ('last', dict(tau=1.0)), ('mean', dict(detection='mean'))):
        face, depth, n_hits, sf, st, sw = ops.raycast_beams(bvh, torch.zeros_like(dirs), dirs, [0, 1], eye, pat, R0, SPREAD, cull=False,
                                                            want_samples=True, **kw)
        assert n_hits.item() == S
        res[name] = (depth.item(), face.item())
    near, far = int((sf < 2).sum()), int((sf >= 2).sum())
    assert near + far == S and near >= S // 4 and far >= S // 4
    assert abs(res['first'][0] - 5.0) <= 1e-3 and res['first'][1] in (0, 1)
    assert abs(res['last'][0] - 6.0) <= 1e-3 and res['last'][1] in (2, 3)
    assert res['first'][0] < res['mean'][0] < res['last'][0]


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------
SIZE, FOV, SEGMENTS = (16, 256), (45.0, 360.0), 16


def _room(tmp_path):
    from depth_correction_amd.mesh import room_mesh
    path = str(tmp_path / 'room.ply')
    room_mesh().save_ply(path)
    return path, slam_pose(0.3, (0.3, -0.2, 0.1))[None]


def _dataset(path, poses, **kw):
    from depth_correction_amd.render import RenderedMeshDataset
    return RenderedMeshDataset(path, poses=poses, size=SIZE, fov=FOV, num_segments=SEGMENTS, device=DEV, **kw)


def test_one_sample_renders_the_thin_scan(tmp_path):
    from depth_correction_amd.render import BeamModel
    path, poses = _room(tmp_path)
    thin = _dataset(path, poses)[0][0]
    one = _dataset(path, poses, beam=BeamModel(samples=1))[0][0]
    assert len(thin) == len(one) > 0.9 * SIZE[0] * SIZE[1]
    for f in thin.dtype.names:
        assert np.abs(thin[f] - one[f]).max() <= 1e-9, f


def test_rendered_beams_carry_a_bias_that_grows_with_the_angle(tmp_path):
    """The default BeamModel (16 samples, first return) over the room: no beam is longer than its axis, the mean relative error falls
    from bin to bin of the true incidence angle, and the supervised fit of a ScaledPolynomial takes part of it away."""
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.metrics import depth_bias, fit_bias, fitted_model
    from depth_correction_amd.render import BeamModel
    path, poses = _room(tmp_path)
    ds = _dataset(path, poses, beam=BeamModel())
    cloud = DepthCloud.from_structured_array(ds[0][0], dtype=np.float64, device=DEV)
    assert cloud.depth.dtype == torch.float64
    cloud.update_incidence_angles()                     # from the rendered normals: the estimated angles of the second system
    mesh = ds.get_mesh()
    res = depth_bias([cloud], poses, mesh, fit_class='ScaledPolynomial', fit_exponent=[2.0, 4.0])
    d, t, face = res['before']['depth'].cpu().numpy(), res['t'].cpu().numpy(), res['face'].cpu().numpy()
    used = (face >= 0) & np.isfinite(t) & (d > 0)
    assert res['before']['totals']['used'] == used.sum() > 0.9 * len(d)
    r = d[used] - t[used]
    print('rays %d, used %d, max r / d = %.3g eps' % (len(d), used.sum(), (r / d[used]).max() / EPS))
    assert (r <= 4 * EPS * d[used]).all()
    count, rel_mean = res['before']['count'].cpu().numpy(), res['before']['rel_mean'].cpu().numpy()
    big = count >= 100
    print('bins with >= 100 rays: %s\nmean rho: %s' % (np.flatnonzero(big), np.array2string(rel_mean[big], precision=3)))
    assert big.sum() >= 8 and (rel_mean[big] < 0).all() and (np.diff(rel_mean[big]) < 0).all()
    fit = fit_bias(res, 'ScaledPolynomial', [2.0, 4.0])
    assert fit['message'] is None
    after = depth_bias([cloud], poses, mesh, model=fitted_model(fit, 'true_angles', device=DEV))['after']
    print('fit %s: rms of rho %.3e -> %.3e' % (fit['w_true_angles'], res['before']['overall']['rel_rms'], after['overall']['rel_rms']))
    assert after['totals']['used'] == used.sum() and after['overall']['rel_rms'] < res['before']['overall']['rel_rms']


def test_cache_round_trip_with_a_beam(tmp_path):
    import os
    from depth_correction_amd.render import BeamModel
    path, poses = _room(tmp_path)
    kw = dict(cache=True, cache_dir=str(tmp_path / 'gen'))
    beam = BeamModel(samples=8, tau=0.5)
    first = _dataset(path, poses, beam=beam, **kw)
    a = first[0][0]
    assert os.path.exists(first.cloud_path(0))
    again = _dataset(path, poses, beam=BeamModel(samples=8, tau=0.5), **kw)
    again.get_mesh = lambda: (_ for _ in ()).throw(AssertionError('the cache was not read'))
    b = again[0][0]
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # a thin-ray dataset over the same mesh and poses has files of its own
    thin = _dataset(path, poses, **kw)
    assert not os.path.exists(thin.cloud_path(0))
    c = thin[0][0]
    assert os.path.exists(thin.cloud_path(0)) and thin.cloud_path(0) != first.cloud_path(0)
    assert len(c) != len(a) or c.tobytes() != a.tobytes()
    assert c.tobytes() == _dataset(path, poses)[0][0].tobytes()
