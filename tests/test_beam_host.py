"""Finite-beam rendering on the host (no GPU): the sensor model against the reference's recorded numbers, the footprint pattern, the
per-beam arithmetic of dc_beam_subrays / dc_raycast_beams through its host build (libdc_hostcheck.so, the header the kernels include)
against the numpy restatement (tests/beam_reference.py), BeamModel and the dataset's cache path, and the refusals."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import beam_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')
EPS = 2.0 ** -52
R0, SPREAD = 2.5e-3, math.tan(math.radians(0.35))


@pytest.fixture(scope='module')
def host():
    if not os.path.exists(LIB) or not hasattr(ctypes.CDLL(LIB), 'dc_host_beam_select'):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    lib.dc_host_beam_subrays.restype = None
    lib.dc_host_beam_subrays.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.dc_host_beam_select.restype = ctypes.c_int
    lib.dc_host_beam_select.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int] + \
        [ctypes.c_void_p] * 3
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- the sensor model ---------------------------------------------------------------------------------------------------------------
# recorded from the reference's sensor.py (floats in, float32 tensors out)
RECORDED = {
    'OUSTER': (22.70602035522461, 55.465021521857345,
               [0.13866256177425385, 0.13869617879390717, 0.13879698514938354, 0.14198468625545502, 0.15151463449001312]),
    'HOKUYO': (21.70244026184082, 53.01352885790784,
               [0.13253381848335266, 0.13256898522377014, 0.1326744258403778, 0.1360057294368744, 0.14592666923999786]),
}


@pytest.mark.parametrize('name', sorted(RECORDED))
def test_sensor_numbers(name):
    from depth_correction_amd import sensor as S
    sen = getattr(S.Sensors, name)
    z_r, m2, radii = RECORDED[name]
    assert float(sen.rayleight_length()) == pytest.approx(z_r, rel=1e-6)
    assert float(sen.m2) == pytest.approx(m2, rel=1e-6)
    assert float(sen.beam_propagation_factor()) == pytest.approx(m2, rel=1e-6)
    for z, w in zip([0.0, 0.5, 1.0, 5.0, 10.0], radii):
        assert float(sen.beam_radius(z)) == pytest.approx(w, rel=1e-6), z
    assert sen.rayleight_length().dtype == torch.float32 and sen.beam_radius(1.0).dtype == torch.float32


def test_sensor_api():
    from depth_correction_amd import sensor as S
    for name in ('beam_radius', 'Medium', 'Media', 'rayleight_length', 'Sensor', 'Sensors', 'beam_pattern'):
        assert name in S.__all__ and hasattr(S, name)
    assert S.Media.AIR.refractive_index == 1.000293 and S.Media.VACUUM.refractive_index == 1.0
    w0, lam = 2.5e-3, 865e-9
    assert float(S.rayleight_length(w0, lam, n=1.0)) == pytest.approx(math.pi * w0 * w0 / lam, rel=1e-6)
    assert float(S.beam_radius(3.0, w0, lam, 2.0, n=1.0)) == pytest.approx(w0 * 2.0 * math.sqrt(1 + (3.0 / (math.pi * w0 * w0 / lam)) ** 2), rel=1e-6)
    assert S.Sensor(name='x', wavelength=lam, waist_radius=w0).m2 == 1.0
    assert S.Sensor(name='x', wavelength=lam, waist_radius=w0, divergence=0.01).m2 == pytest.approx(0.01 * math.pi * w0 / lam, rel=1e-12)
    assert str(S.Sensors.OUSTER) == 'Ouster OS0'


@pytest.mark.parametrize('S', [1, 8, 16, 64])
@pytest.mark.parametrize('rho_max', [1.5, 0.7])
def test_beam_pattern(S, rho_max):
    from depth_correction_amd.sensor import beam_pattern
    got, want = beam_pattern(S, rho_max), R.pattern(S, rho_max)
    assert got.dtype == np.float64 and got.shape == (S, 3)
    assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all()
    assert (got[0] == [0.0, 0.0, 1.0]).all()
    assert (got[:, 2] == 1.0).all()
    rho = np.hypot(got[:, 0], got[:, 1])
    assert rho.max() < rho_max and (np.diff(rho) > 0).all()


def test_beam_pattern_refuses():
    from depth_correction_amd.sensor import beam_pattern
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            beam_pattern(bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            beam_pattern(16, rho_max=bad)


# ---- sub-rays -------------------------------------------------------------------------------------------------------------------------
def beams_for_subrays(seed=5):
    """1 000 random directions (not unit) plus the ones that pin the tie rule of the frame's axis, view points N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(1000, 3)) * rng.uniform(0.2, 5.0, size=(1000, 1))
    fixed = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
             [1 / math.sqrt(2), 1 / math.sqrt(2), 0], [1 / math.sqrt(3), 1 / math.sqrt(3), 1 / math.sqrt(3)]]
    dirs = np.concatenate([dirs, np.array(fixed, dtype=np.float64)])
    vps = rng.normal(scale=0.3, size=dirs.shape)
    return np.ascontiguousarray(vps), np.ascontiguousarray(dirs)


def check_subrays(o, D, vps, dirs, pat):
    """The bars of the sub-ray tests: 8 eps max(1, |v|) per component against the numpy restatement, |D . d - 1| <= 4 eps."""
    o_ref, D_ref = R.subrays(vps, dirs, pat, R0, SPREAD)
    bar = 8 * EPS * np.maximum(1.0, np.linalg.norm(vps, axis=1))[:, None, None]
    assert (np.abs(o - o_ref) <= bar).all(), np.abs(o - o_ref).max()
    assert (np.abs(D - D_ref) <= bar).all(), np.abs(D - D_ref).max()
    dhat = dirs / np.sqrt((dirs * dirs).sum(axis=1, keepdims=True))
    assert (np.abs(np.einsum('nsc,nc->ns', D, dhat) - 1.0) <= 4 * EPS).all()


@pytest.mark.parametrize('S', [1, 4, 16, 64])
def test_host_subrays(host, S):
    vps, dirs = beams_for_subrays()
    pat = np.ascontiguousarray(R.pattern(S))
    o, D = np.full((len(dirs), S, 3), np.nan), np.full((len(dirs), S, 3), np.nan)
    host.dc_host_beam_subrays(_p(vps), _p(dirs), len(dirs), _p(pat), S, R0, SPREAD, _p(o), _p(D))
    check_subrays(o, D, vps, dirs, pat)
    # sample 0 is the beam's axis from its view point
    assert (o[:, 0] == vps).all()


def test_host_subrays_tie_rule_and_bad_directions(host):
    """The frame's axis is the first smallest |d_k|: e1 = (a x d) / |a x d| for the directions with tied components; a zero or
    non-finite direction emits NaN."""
    pat = np.ascontiguousarray(np.array([[1.0, 0.0, 1.0]]))
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0]], dtype=np.float64)
    want_e1 = np.array([[0, 0, -1], [0, 0, 1], [0, -1, 0], [-1, 1, 0], [0, -1, 1]], dtype=np.float64)      # a x d with a = y, x, x, z, x
    want_e1 /= np.linalg.norm(want_e1, axis=1, keepdims=True)
    vps = np.zeros_like(dirs)
    o, D = np.zeros((len(dirs), 1, 3)), np.zeros((len(dirs), 1, 3))
    host.dc_host_beam_subrays(_p(vps), _p(dirs), len(dirs), _p(pat), 1, 1.0, 0.0, _p(o), _p(D))           # r0 = 1, px = 1: the origin is e1
    assert np.abs(o[:5, 0] - want_e1).max() <= 4 * EPS
    assert np.isnan(o[5:]).all() and np.isnan(D[5:]).all()


# ---- the reduction --------------------------------------------------------------------------------------------------------------------
def bundles(S, n=3000, seed=9):
    """Random sub-ray tables: empty, partial and full bundles, ties in t (values from a grid of few depths), unequal weights, zero
    weights and weights that are not finite (no hit)."""
    rng = np.random.default_rng(seed + S)
    p_hit = rng.choice([0.0, 0.3, 0.8, 1.0], size=(n, 1))
    hit = rng.uniform(size=(n, S)) < p_hit
    face = np.where(hit, rng.integers(0, 50, size=(n, S)), -1).astype(np.int32)
    t = np.where(rng.uniform(size=(n, 1)) < 0.5, rng.integers(1, 6, size=(n, S)) * 0.25, rng.uniform(0.5, 30.0, size=(n, S)))
    w = rng.uniform(0.0, 1.0, size=(n, S))
    w[rng.uniform(size=(n, S)) < 0.05] = 0.0
    w[rng.uniform(size=(n, S)) < 0.02] = np.nan
    uniform = rng.uniform(size=n) < 0.3
    w[uniform] = np.where(np.isnan(w[uniform]), np.nan, 1.0)
    t, w = np.where(hit, t, np.inf), np.where(hit, w, 0.0)
    return np.ascontiguousarray(face), np.ascontiguousarray(t), np.ascontiguousarray(w)


def host_select(host, face, t, w, detection, tau, min_hits):
    n, S = face.shape
    f, d, h = np.full(n, -7, dtype=np.int32), np.full(n, np.nan), np.full(n, -7, dtype=np.int32)
    rc = host.dc_host_beam_select(_p(face), _p(t), _p(w), n, S, detection, tau, min_hits, _p(f), _p(d), _p(h))
    return rc, f, d, h


@pytest.mark.parametrize('S', [1, 4, 64])
def test_host_selection(host, S):
    face, t, w = bundles(S)
    hits = ((face >= 0) & np.isfinite(w)).sum(axis=1)
    assert (hits == 0).any() and (hits == S).any() and (S == 1 or ((hits > 0) & (hits < S)).any())
    for min_hits in sorted({1, S}):
        for tau in (1.0 / S, 0.5, 1.0):
            rc, f, d, h = host_select(host, face, t, w, R.QUANTILE, tau, min_hits)
            f_ref, d_ref, h_ref = R.reduce(face, t, w, R.QUANTILE, tau, min_hits)
            assert rc == 0 and (h == h_ref).all() and (f == f_ref).all()
            assert (d.view(np.int64) == d_ref.view(np.int64)).all()
        rc, f, d, h = host_select(host, face, t, w, R.MEAN, 0.5, min_hits)
        f_ref, d_ref, h_ref = R.reduce(face, t, w, R.MEAN, 0.5, min_hits)
        assert rc == 0 and (h == h_ref).all()
        assert (np.isinf(d) == np.isinf(d_ref)).all() and ((f < 0) == (f_ref < 0)).all()
        ok = np.isfinite(d_ref)
        assert (np.abs(d[ok] - d_ref[ok]) <= S * EPS * d_ref[ok]).all()
        assert (f[ok & (d == d_ref)] == f_ref[ok & (d == d_ref)]).all()


def test_host_selection_refuses(host):
    face, t, w = bundles(4, n=8)
    for S_, det, tau, mh in ((4, 2, 0.5, 1), (4, R.QUANTILE, 0.0, 1), (4, R.QUANTILE, 1.5, 1), (4, R.QUANTILE, float('nan'), 1),
                             (4, R.MEAN, 0.5, 0), (4, R.MEAN, 0.5, 5)):
        assert host_select(host, face, t, w, det, tau, mh)[0] == -1
    three = np.ascontiguousarray(face[:, :3]), np.ascontiguousarray(t[:, :3]), np.ascontiguousarray(w[:, :3])
    assert host_select(host, *three, R.MEAN, 0.5, 1)[0] == -1


# ---- BeamModel, the cache path, refusals ----------------------------------------------------------------------------------------------
def test_beam_model():
    from depth_correction_amd.render import BeamModel
    from depth_correction_amd.sensor import Sensors, Sensor
    b = BeamModel()
    assert b.sensor is Sensors.OUSTER and b.samples == 16 and b.detection == 'quantile' and b.weight == 'uniform' and b.min_hits == 1
    assert b.tau == 1.0 / 16 and b.r0 == 2.5e-3 and b.spread == math.tan(math.radians(0.35))
    assert (b.pattern == R.pattern(16)).all() or np.abs(b.pattern - R.pattern(16)).max() < 1e-15
    c = BeamModel(sensor=Sensor(name='s', wavelength=1e-6, waist_radius=1e-3, divergence=1e-3), samples=8, tau=0.5, r0=4e-3)
    assert c.r0 == 4e-3 and c.divergence == 1e-3 and c.tau == 0.5 and c.pattern.shape == (8, 3)
    assert BeamModel(divergence=0.0).spread == 0.0
    for kw in (dict(samples=0), dict(samples=12), dict(samples=128), dict(detection='median'), dict(weight='cosine'), dict(tau=0.0),
               dict(tau=1.5), dict(min_hits=0), dict(min_hits=17), dict(r0=-1.0), dict(divergence=2.0)):
        with pytest.raises(ValueError):
            BeamModel(**kw)
    keys = {BeamModel(**kw).cache_key() for kw in (dict(), dict(samples=8), dict(detection='mean'), dict(tau=0.5), dict(weight='lambert'),
                                                   dict(min_hits=2), dict(r0=1e-3), dict(divergence=1e-3))}
    assert len(keys) == 8


def test_cache_path(tmp_path):
    """Without a beam the cache path is what it was before beams existed; with one it gains a directory naming the beam."""
    from depth_correction_amd.mesh import box_mesh
    from depth_correction_amd.render import BeamModel, RenderedMeshDataset
    path = str(tmp_path / 'box.ply')
    box_mesh((0, 0, 0), (2, 2, 2), inward=True).save_ply(path)
    poses = np.eye(4)[None]
    kw = dict(poses=poses, size=(16, 256), fov=(45.0, 360.0), num_segments=16, cache=True, cache_dir=str(tmp_path / 'gen'))
    thin = RenderedMeshDataset(path, **kw)
    want = os.path.join(str(tmp_path / 'gen'), 'rendered_mesh', 'box.ply', 'hash_%s_size_16_256_fov_45_360' % thin.hash_name,
                        'cloud_00000.bin')
    assert thin.beam is None and thin.cloud_path(0) == want
    beam = BeamModel(samples=8)
    fat = RenderedMeshDataset(path, beam=beam, **kw)
    assert fat.beam is beam and fat[0:1].beam is beam
    assert os.path.dirname(os.path.dirname(fat.cloud_path(0))) == os.path.dirname(want)
    assert os.path.basename(os.path.dirname(fat.cloud_path(0))) == beam.cache_key() and fat.cloud_path(0) != want
    assert RenderedMeshDataset(path, beam=BeamModel(samples=8, tau=1.0), **kw).cloud_path(0) != fat.cloud_path(0)
    with pytest.raises(TypeError):
        RenderedMeshDataset(path, beam='ouster', **kw)


def test_refusals_without_a_gpu():
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import MeshBVH
    z = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.beam_subrays(z, z, R.pattern(4), R0, SPREAD)
    bvh = MeshBVH(torch.zeros(1, dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                  torch.zeros((1, 6)), torch.zeros((1, 9), dtype=torch.float64))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.raycast_beams(bvh, z, z, [0, 4], torch.eye(4, dtype=torch.float64)[None], R.pattern(4), R0, SPREAD)
