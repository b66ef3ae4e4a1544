"""Surface reconstruction on the host (no GPU): the rules of csrc/dc_tsdf_math.h through their host build (libdc_hostcheck.so, the header
the kernels inline) against tests/tsdf_reference.py, bit for bit on sum, count, stats, vertices and faces, on the designed cases of
tests/tsdf_cases.py; hand-written figures for the designed rays; then properties of the oracle on two analytic scenes.

Figures of the analytic scenes (voxel 0.1, truncation 0.3): plane at incidence <= 45 degrees, 1750 vertices, worst 0.227 voxel from the
plane; sphere of radius 0.5 from 14 viewpoints, 536 vertices, worst 0.252 voxel from the sphere.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cases as C  # noqa: E402
import tsdf_reference as R  # noqa: E402

Q = 2 ** 20


def host_lib():
    """libdc_hostcheck.so with the surface reconstruction's exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_tsdf_integrate'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_tsdf_integrate.argtypes = [vp, vp, vp, ci, i64, vp, vp, vp, f64, ci, ci, ci, f64, ci, f64, f64, f64, vp, vp, vp]
    lib.dc_host_tsdf_extract.argtypes = [vp, vp, vp, f64, ci, ci, ci, ci, i64, i64, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_integrate(lib, vol, b):
    """One batch of tsdf_cases into the oracle-shaped volume ``vol`` through the host build; returns the status."""
    n = b['dirs'].shape[0]
    dt = b['dirs'].dtype
    vps = np.ascontiguousarray(np.broadcast_to(b['vps'], (n, 3)), dtype=dt)
    dirs, depth = np.ascontiguousarray(b['dirs']), np.ascontiguousarray(b['depth'], dtype=dt)
    mask = None if b['mask'] is None else np.ascontiguousarray(b['mask'], dtype=np.uint8)
    pose = None if b['pose'] is None else np.ascontiguousarray(b['pose'], dtype=np.float64)
    return lib.dc_host_tsdf_integrate(_p(vps), _p(dirs), _p(depth), 0 if dt == np.float32 else 1, n, _p(mask), _p(pose), _p(vol.origin), vol.voxel,
                                      *vol.dims, vol.trunc, R.k_steps(vol.trunc, vol.voxel), b['min_depth'],
                                      np.inf if b['max_range'] is None else b['max_range'], -1.0 if b['carve_from'] is None else b['carve_from'],
                                      _p(vol.sum), _p(vol.count), _p(vol.stats))


def host_extract(lib, vol, min_count=1):
    tot = np.zeros(2, np.int64)
    args = (_p(vol.sum), _p(vol.count), _p(vol.origin), vol.voxel, *vol.dims, min_count)
    assert lib.dc_host_tsdf_extract(*args, 0, 0, None, None, _p(tot)) == 0
    v, f = np.zeros((int(tot[0]), 3)), np.zeros((int(tot[1]), 3), np.int32)
    assert lib.dc_host_tsdf_extract(*args, len(v), len(f), _p(v), _p(f), _p(tot)) == 0
    assert tot.tolist() == [len(v), len(f)]
    return v, f


def run_case(lib, volume, batches):
    """(host volume, oracle volume) after all batches."""
    got, want = R.Volume(**volume), R.Volume(**volume)
    for b in batches:
        assert host_integrate(lib, got, b) == 0
        R.integrate(want, **b)
    return got, want


def assert_same_volume(got, want, what=''):
    assert np.array_equal(got.sum, want.sum), what
    assert np.array_equal(got.count, want.count), what
    assert got.stats.tolist() == want.stats.tolist(), what


INTEGRATION = {name: (vol, batches) for name, vol, batches in C.integration_cases()}
EXTRACTION = {name: rest for name, *rest in C.extraction_cases()}


def column(vol, x=1, y=1):
    return vol.sum.reshape(vol.dims)[x, y].tolist(), vol.count.reshape(vol.dims)[x, y].tolist()


@pytest.mark.parametrize('name', sorted(INTEGRATION))
def test_host_integration_equals_oracle(lib, name):
    got, want = run_case(lib, *INTEGRATION[name])
    assert_same_volume(got, want, name)
    assert want.stats[0] + want.stats[1] == sum(b['dirs'].shape[0] for b in INTEGRATION[name][1])


def test_designed_ray_by_hand(lib):
    """The axis-parallel ray through the voxel centres (1.5, 1.5, z + 0.5) with d = 4.5, tau = 2: s = 2, 1, 0, -1, -2 in the voxels z = 2 .. 6.
    s == tau gives +2^20 and s == -tau is kept; every voxel holds two samples and counts once; the sample at z = 3.0 lies on a face and
    goes to voxel 3."""
    got, _ = run_case(lib, *INTEGRATION['s_equals_tau_both_ends'])
    s, c = column(got)
    assert s == [0, 0, Q, Q // 2, 0, -Q // 2, -Q, 0]
    assert c == [0, 0, 1, 1, 1, 1, 1, 0]
    assert got.stats.tolist() == [1, 0, 0, 5]
    assert got.count.sum() == 5
    # d = 4.75: s = 2.25 in voxel 2 is clamped
    got, _ = run_case(lib, *INTEGRATION['clamp'])
    s, c = column(got)
    assert s == [0, 0, Q, 5 * Q // 8, Q // 8, -3 * Q // 8, -7 * Q // 8, 0] and c == [0, 0, 1, 1, 1, 1, 1, 0]
    # d = 5: voxel 7 is reached by the sample at z = 7.0 with s = -2.5 < -tau: dropped
    got, _ = run_case(lib, *INTEGRATION['below_minus_tau_dropped'])
    s, c = column(got)
    assert s == [0, 0, 0, 3 * Q // 4, Q // 4, -Q // 4, -3 * Q // 4, 0] and c == [0, 0, 0, 1, 1, 1, 1, 0]
    assert got.stats.tolist() == [1, 0, 0, 4]


def test_face_leaving_and_carving_by_hand(lib):
    got, _ = run_case(lib, *INTEGRATION['face_goes_up'])
    assert column(got, 2, 3)[1] == [0, 0, 1, 1, 1, 1, 1, 0] and got.count.sum() == 5
    got, _ = run_case(lib, *INTEGRATION['leaves_grid'])            # t = 5 .. 9: voxels 5, 6, 7, then three samples outside
    s, c = column(got)
    assert c == [0, 0, 0, 0, 0, 1, 1, 1] and s[5:] == [3 * Q // 4, Q // 4, -Q // 4]
    assert got.stats.tolist() == [1, 0, 3, 3]
    got, _ = run_case(lib, *INTEGRATION['carve'])                  # from t = 0.5: voxels 0 and 1 are seen free
    s, c = column(got)
    assert s == [Q, Q, Q, Q // 2, 0, -Q // 2, -Q, 0] and c == [1, 1, 1, 1, 1, 1, 1, 0]
    got, _ = run_case(lib, *INTEGRATION['behind_the_sensor'])      # o_z = 0.25, d = 1: t = 0.5 .. 3 only; voxel 3 meets s = -2.25
    s, c = column(got)
    assert c == [1, 1, 1, 0, 0, 0, 0, 0] and got.stats.tolist() == [1, 0, 0, 3]
    assert s[:3] == [3 * Q // 8, -Q // 8, -5 * Q // 8]


def test_ties_round_to_even(lib):
    got, _ = run_case(lib, *INTEGRATION['tie_to_even'])            # 0.5 -> 0
    assert column(got)[0][4] == 0 and column(got)[1][4] == 1
    got, _ = run_case(lib, *INTEGRATION['tie_to_even_odd'])        # 1.5 -> 2
    assert column(got)[0][4] == 2
    assert column(got)[0][3] == Q // 2 + 2                         # 2^19 + 1.5 -> 2^19 + 2


def test_skipped_rays(lib):
    """Of the seven rays only the first is used: NaN, infinite depth, mask 0, d == min_depth, d just above max_range, infinite dir."""
    got, want = run_case(lib, *INTEGRATION['skipped_rays'])
    assert got.stats.tolist() == [1, 6, 0, 5]
    one, _ = run_case(lib, *INTEGRATION['s_equals_tau_both_ends'])
    assert np.array_equal(got.sum, one.sum) and np.array_equal(got.count, one.count)


def test_f32_and_f64_inputs_agree(lib):
    a, _ = run_case(lib, *INTEGRATION['f32'])
    b, _ = run_case(lib, *INTEGRATION['f64_of_f32'])
    assert a.stats[3] > 0
    assert_same_volume(a, b)


def test_refused_arguments(lib):
    """Dims below 2, 2^31 voxels, a voxel size or a truncation that is not > 0: DC_ERR_ARG before anything is touched."""
    vol = R.Volume(**C.GRID)
    b = C.z_ray(4.5)
    good = dict(dims=(4, 4, 8), voxel=1.0, trunc=2.0)
    for bad in (dict(dims=(1, 4, 8)), dict(dims=(2048, 2048, 512)), dict(voxel=0.0), dict(trunc=0.0), dict(trunc=np.nan)):
        a = dict(good, **bad)
        rc = lib.dc_host_tsdf_integrate(_p(b['vps']), _p(b['dirs']), _p(b['depth']), 1, 1, None, None, _p(vol.origin), a['voxel'], *a['dims'],
                                        a['trunc'], 4, 0.0, np.inf, -1.0, _p(vol.sum), _p(vol.count), _p(vol.stats))
        assert rc == -1, bad
    assert vol.count.sum() == 0 and vol.stats.sum() == 0


def test_config_keys_and_no_cpu_path():
    """The new Config keys default to off; the reconstruction refuses a CPU device with the package's usual error."""
    from depth_correction_amd.config import Config, map_eval_csv, recon_eval_csv
    from depth_correction_amd.reconstruction import TsdfVolume, reconstruct
    cfg = Config()
    assert cfg.recon_voxel_size == 0.1 and cfg.recon_trunc is None and cfg.recon_min_count == 1 and cfg.recon_max_range is None
    assert cfg.recon_carve_from is None and cfg.recon_bounds is None and cfg.recon_poses == 'dataset' and cfg.recon_eval_csv is None
    assert cfg.recon_mesh_ply is None and cfg.recon_eval_samples == 100000 and cfg.recon_eval_max_dist is None
    assert recon_eval_csv('/tmp/log', 'val') == '/tmp/log/recon_eval_val.csv' and recon_eval_csv('', None) == 'recon_eval.csv'
    assert os.path.dirname(recon_eval_csv('/x/y', 'test')) == os.path.dirname(map_eval_csv('/x/y', 'test'))
    with pytest.raises(RuntimeError, match='no CPU path'):
        TsdfVolume((0, 0, 0), (4, 4, 4), 0.1, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        reconstruct([], [], 0.1, device='cpu')
    from depth_correction_amd.ops import tsdf_k_steps
    assert tsdf_k_steps(0.3, 0.1) == R.k_steps(0.3, 0.1) == 6 and tsdf_k_steps(2.0, 1.0) == 4 and tsdf_k_steps(2.25, 1.0) == 5


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def extraction_volume(volume, s, c):
    vol = R.Volume(**volume)
    vol.sum[:] = np.asarray(s, np.int64).ravel()
    vol.count[:] = np.asarray(c, np.int32).ravel()
    return vol


@pytest.mark.parametrize('name', sorted(EXTRACTION))
def test_host_extraction_equals_oracle(lib, name):
    volume, s, c, min_count = EXTRACTION[name]
    vol = extraction_volume(volume, s, c)
    v, f = host_extract(lib, vol, min_count)
    wv, wf = R.extract(vol, min_count)
    assert v.shape == wv.shape and f.shape == wf.shape, name
    assert np.array_equal(v, wv) and np.array_equal(f, wf), name
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(v))


def test_small_volumes_by_hand(lib):
    volume, s, c, _ = EXTRACTION['one_cell']
    v, f = R.extract(extraction_volume(volume, s, c))
    assert v.shape == (1, 3) and f.shape == (0, 3)
    assert v[0].tolist() == [0.5 + 0.5 / 3.0] * 3                       # three crossings at r = 0.5, one per axis
    volume, s, c, _ = EXTRACTION['centre_inside']
    vol = extraction_volume(volume, s, c)
    v, f = R.extract(vol)
    assert v.shape == (8, 3) and f.shape == (12, 3)
    assert R.is_closed_manifold(f) and R.euler_characteristic(v, f) == 2
    centre = vol.origin + 1.5 * vol.voxel
    n = R.face_normals(v, f)
    mid = v[f].mean(axis=1)
    assert (np.einsum('ij,ij->i', n, mid - centre) > 0).all()          # outward: the free side
    # one unobserved corner removes exactly its cells: here the cell (0, 0, 0), its vertex and the faces that used it
    volume, s, c, _ = EXTRACTION['one_corner_unobserved']
    v2, f2 = R.extract(extraction_volume(volume, s, c))
    assert v2.shape == (7, 3)
    assert f2.shape == (6, 3)                                           # the three edges at the centre towards -x, -y, -z lose their quads
    # sum == 0 is outside: the centre is no longer inside, the voxel (1, 1, 2) with sum -3 is
    volume, s, c, _ = EXTRACTION['zero_is_outside']
    vol = extraction_volume(volume, s, c)
    v3, f3 = R.extract(vol)
    assert v3.shape == (4, 3) and f3.shape == (2, 3)                    # the four cells around the edge (1,1,1)-(1,1,2); the grid ends above
    assert (v3[:, 2] > 1.5).all()


def test_linear_field_is_extracted_at_its_zero_level(lib):
    """f = (2 x + 3 y - 5 z + 1.25) / 16 in lattice coordinates: every crossing lies on the plane, so does their mean."""
    volume, s, c, _ = EXTRACTION['linear']
    vol = extraction_volume(volume, s, c)
    v, f = R.extract(vol)
    assert len(v) > 8 and len(f) > 0
    lat = (v - vol.origin) / vol.voxel - 0.5
    res = 2 * lat[:, 0] + 3 * lat[:, 1] - 5 * lat[:, 2] + 1.25
    assert np.abs(res).max() < 1e-12
    n = R.face_normals(v, f)
    assert (n @ np.array([2.0, 3.0, -5.0]) > 0).all()                   # towards growing f, the free side
    # min_count = 2 drops the voxels seen once and every cell that touches one
    v2, f2 = R.extract(vol, 2)
    assert 0 < len(v2) < len(v)
    assert {tuple(r) for r in v2.tolist()} <= {tuple(r) for r in v.tolist()}


# ---- properties of the oracle on analytic scenes -------------------------------------------------------------------------------------
def cone_rays(rng, axis, half_angle, n):
    """n unit directions within half_angle of axis."""
    axis = axis / np.linalg.norm(axis)
    a = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(axis, a)
    th = half_angle * np.sqrt(rng.random(n))
    ph = 2 * np.pi * rng.random(n)
    d = np.cos(th)[:, None] * axis + np.sin(th)[:, None] * (np.cos(ph)[:, None] * a + np.sin(ph)[:, None] * b)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def plane_scene(max_incidence_deg, seed=3):
    """A tilted plane n.x = c seen from two viewpoints; (rays per viewpoint, plane, volume)."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.2, -0.1, 1.0])
    nrm /= np.linalg.norm(nrm)
    c = 0.537
    scans = []
    for vp in (np.array([-0.4, 0.1, 2.6]), np.array([0.5, -0.3, 2.2])):
        dirs = cone_rays(rng, -nrm, np.deg2rad(max_incidence_deg), 20000)
        depth = (c - nrm @ vp) / (dirs @ nrm)
        scans.append((vp, dirs, depth))
    return scans, (nrm, c)


def test_plane_scene(lib):
    voxel = 0.1
    scans, (nrm, c) = plane_scene(45.0)
    pts = np.concatenate([vp + d[:, None] * u for vp, u, d in scans])
    for vp, u, d in scans:                                           # the scene's own preconditions
        assert (d > 0).all() and np.isfinite(d).all()
        assert (-(u @ nrm) >= np.cos(np.deg2rad(45.0)) - 1e-12).all()
        assert nrm @ vp > c
    lo, hi = pts.min(axis=0) - 0.3, pts.max(axis=0) + 0.3
    dims = tuple(int(n) for n in np.ceil((hi - lo) / voxel))
    vol = R.Volume(lo, dims, voxel, 0.3)
    for vp, u, d in scans:
        R.integrate(vol, vp[None], u, d)
    v, f = R.extract(vol)
    assert len(v) > 500 and len(f) > 500
    dist = np.abs(v @ nrm - c) / voxel
    print('plane: %d vertices, %d faces, worst %.3f voxel' % (len(v), len(f), dist.max()))
    assert dist.max() <= 1.0                                         # derived: (sqrt(3) / 2) a tan 45 = 0.87 a
    assert (R.face_normals(v, f) @ nrm > 0).all()                    # towards the sensors


def test_sphere_scene(lib):
    voxel, radius, stand_off = 0.1, 0.5, 2.0
    centre = np.array([0.03, -0.02, 0.05])
    axes = [np.array(a, float) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    axes += [np.array((sx, sy, sz), float) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    assert len(axes) == 14
    rng = np.random.default_rng(11)
    lo, hi = centre - radius - 0.35, centre + radius + 0.35
    vol = R.Volume(lo, tuple(int(n) for n in np.ceil((hi - lo) / voxel)), voxel, 0.3)
    hits = 0
    for ax in axes:
        vp = centre + stand_off * ax / np.linalg.norm(ax)
        u = cone_rays(rng, centre - vp, np.arcsin(radius / stand_off), 6000)
        b = u @ (vp - centre)
        disc = b * b - (stand_off ** 2 - radius ** 2)
        ok = disc > 0
        d = -b[ok] - np.sqrt(disc[ok])
        assert (d > 0).all() and np.allclose(np.linalg.norm(vp + d[:, None] * u[ok] - centre, axis=1), radius, atol=1e-9)
        hits += int(ok.sum())
        R.integrate(vol, vp[None], u[ok], d)
    assert hits > 50000
    v, f = R.extract(vol)
    dist = np.abs(np.linalg.norm(v - centre, axis=1) - radius) / voxel
    print('sphere: %d vertices, %d faces, worst %.3f voxel' % (len(v), len(f), dist.max()))
    assert R.is_closed_manifold(f)
    assert R.euler_characteristic(v, f) == 2
    assert (np.einsum('ij,ij->i', R.face_normals(v, f), v[f].mean(axis=1) - centre) > 0).all()
    assert dist.max() <= 1.0
