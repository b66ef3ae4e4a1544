"""The ray cast against the fused volume on the host (no GPU): the rule of csrc/dc_tsdf_cast_math.h through its host build
(libdc_hostcheck.so: the header the kernel inlines, run ray after ray) against the numpy oracle tests/tsdf_cast_reference.py, which
marches every sample, and against the hand-computed values of its designed cases.  face, t, normal, phi and status are held to the bit,
inc through cos(inc) within 1e-13 (the bar of tests/test_gpu_raycast_edge.py), with and without skipping of absent blocks.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdf_cast_reference as C  # noqa: E402
import tsdf_loss_reference as L  # noqa: E402

DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}               # DC_F32 / DC_F64


def host_lib():
    """libdc_hostcheck.so with the cast's export (rebuilt when the library at hand predates it)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_tsdf_sparse_cast_rays'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_tsdf_sparse_cast_rays.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, f64, f64, ci, vp, vp, vp, ci, i64,
                                                  vp, vp, ci, f64, f64, f64, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_cast(lib, total, owns, vps, dirs, scan_offset, poses, t_min=0.0, t_max=100.0, step=None, refine=2, min_count=1, mask=None, skip=True,
              rc=0):
    """dc_host_tsdf_sparse_cast_rays -> the dict of the outputs (numpy)."""
    dirs = np.ascontiguousarray(dirs).reshape(-1, 3)
    vps = np.ascontiguousarray(np.asarray(vps).astype(dirs.dtype)).reshape(-1, 3)
    n = dirs.shape[0]
    keys, slots = np.ascontiguousarray(total.keys, np.uint64), np.ascontiguousarray(total.slots, np.int32)
    own_args = (None, None, None, 0, 0, None, None)
    if owns is not None:
        ok, osl, optr, osum, ocnt = L.own_tables(owns)
        own_args = (_p(ok) if ok.size else _p(osum), _p(osl) if osl.size else _p(osum), _p(optr), ok.size, osum.shape[0], _p(osum), _p(ocnt))
    off = np.ascontiguousarray(scan_offset, np.int64)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    m8 = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    out = dict(face=np.full(n, 7, np.int32), t=np.full(n, 7.0), inc=np.full(n, 7.0), normal=np.full((n, 3), 7.0), phi=np.full(n, 7.0),
               status=np.full(n, 7, np.uint8), samples=np.full(n, 7, np.int32))
    got = lib.dc_host_tsdf_sparse_cast_rays(
        _p(keys), _p(slots), _p(np.array([total.n_blocks], np.int64)), total.capacity, _p(total.sum), _p(total.count), *own_args,
        _p(np.ascontiguousarray(total.origin, np.float64)), total.voxel, total.trunc, min_count, _p(vps), _p(dirs), _p(m8), DTYPES[dirs.dtype],
        n, _p(off), _p(P), P.shape[0], t_min, t_max, total.voxel / 2.0 if step is None else step, refine, int(skip), _p(out['face']),
        _p(out['t']), _p(out['inc']), _p(out['normal']), _p(out['phi']), _p(out['status']), _p(out['samples']))
    assert got == rc, got
    return out


@functools.lru_cache(maxsize=None)
def designed_volumes():
    return C.volumes()


def oracle_one(vol, vps, dirs, mask, **kw):
    return C.cast(vol, None, vps, dirs, [0, len(dirs)], C.IDENTITY, mask=mask, **kw)


@functools.lru_cache(maxsize=None)
def skip_oracle():
    """The oracle's naive march of the three long rays, once."""
    vols = designed_volumes()
    return tuple(C.run_case(oracle_one, vols, case, **C.SKIP_KW) for case in C.skip_cases())


def check_designed(cast_one):
    """Every single-ray case through ``cast_one(volume, vps, dirs, mask, skip=..., **rule)``: the hand values, the oracle, both marches."""
    vols = designed_volumes()
    seen = set()
    for case in C.ray_cases():
        want = C.run_case(oracle_one, vols, case)
        C.assert_hand(want, case)                                          # the oracle itself holds the hand values
        for skip in (True, False):
            got = C.run_case(functools.partial(cast_one, skip=skip), vols, case)
            C.assert_hand(got, case)
            C.assert_equal(got, want, (case['name'], skip), samples='samples_read' if skip else 'samples')
        seen.add(case['status'])
    assert seen == {C.HIT, C.SKIPPED, C.MISS, C.BEHIND, C.LOST}


def check_refinement(cast_one):
    """The bent field: refine 0, 1, 2, 4 to the bit, and |phi| does not grow from 0 to 2 rounds."""
    vols = designed_volumes()
    phi = {}
    for refine in C.REFINES:
        case = dict(C.BEND_RAY, name='bend, refine %d' % refine, kw=dict(refine=refine))
        want = C.run_case(oracle_one, vols, case)
        assert want['status'][0] == C.HIT
        for skip in (True, False):
            got = C.run_case(functools.partial(cast_one, skip=skip), vols, case)
            C.assert_equal(got, want, (case['name'], skip), samples='samples_read' if skip else 'samples')
        phi[refine] = abs(float(want['phi'][0]))
    assert phi[0] > 0.0 and phi[0] >= phi[1] >= phi[2], phi
    assert len({want_t for want_t in phi.values()}) > 1, phi               # the field is not linear along this ray


def check_skipping(cast_one):
    """200 absent blocks in front of the wall: both marches equal the oracle's naive one, and skipping reads a fraction of the samples."""
    vols = designed_volumes()
    for case, want in zip(C.skip_cases(), skip_oracle()):
        C.assert_hand(want, case)
        fast = C.run_case(functools.partial(cast_one, skip=True), vols, case, **C.SKIP_KW)
        slow = C.run_case(functools.partial(cast_one, skip=False), vols, case, **C.SKIP_KW)
        C.assert_hand(fast, case)
        C.assert_equal(fast, want, (case['name'], 'skip'), samples='samples_read')
        C.assert_equal(slow, want, (case['name'], 'naive'), samples='samples')
        naive = int(want['samples'][0])
        assert naive > 3000, naive
        assert int(fast['samples'][0]) <= naive
        if case['name'] == 'axis':
            # an absent block holds 16 naive samples at step a / 2; a jump spends at most 2 look-ups and no voxel read on it
            assert 4 * int(fast['samples'][0]) <= naive, (int(fast['samples'][0]), naive)


# ---- 1. designed volumes -------------------------------------------------------------------------------------------------------------
def _host_one(lib):
    return lambda vol, vps, dirs, mask, **kw: host_cast(lib, vol, None, vps, dirs, [0, len(dirs)], C.IDENTITY, mask=mask, **kw)


def test_designed_rays_host_equals_oracle_and_hand(lib):
    check_designed(_host_one(lib))


def test_refinement_host_equals_oracle(lib):
    check_refinement(_host_one(lib))


def test_skipping_host_equals_naive_march(lib):
    check_skipping(_host_one(lib))


def test_arguments_host(lib):
    vol = designed_volumes()['WALL']
    vps, dirs = np.array([[14.25, 2.0, 2.0]]), np.array([[1.0, 0.0, 0.0]])
    bad = [dict(t_min=-1.0), dict(t_min=3.0, t_max=3.0), dict(t_max=np.inf), dict(t_min=np.nan), dict(step=0.0), dict(step=2.5),
           dict(step=2.0 ** -30, t_max=100.0), dict(refine=-1), dict(min_count=0)]
    for kw in bad:
        host_cast(lib, vol, None, vps, dirs, [0, 1], C.IDENTITY, rc=-1, **dict(C.DEFAULT_KW, **kw))
    out = host_cast(lib, vol, None, vps[:0], dirs[:0], [0, 0], C.IDENTITY, **C.DEFAULT_KW)           # no ray is legal
    assert out['t'].shape == (0,)


# ---- 2. the random posed scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_random_scene_host_equals_oracle(lib, dtype):
    sc = C.random_scene(dtype)
    assert sc['counts'][C.HIT] * 3 >= sc['n'] and min(sc['counts'][k] for k in (C.MISS, C.BEHIND, C.SKIPPED)) >= 1, sc['counts']
    for (min_count, with_own), want in sc['oracle'].items():
        owns = sc['owns'] if with_own else None
        for skip in (True, False):
            got = host_cast(lib, sc['total'], owns, sc['vps'], sc['dirs'], sc['offset'], sc['poses'], mask=sc['mask'], min_count=min_count,
                            skip=skip, **sc['rule'])
            C.assert_equal(got, want, (dtype, min_count, with_own, skip), samples='samples_read' if skip else 'samples')


def test_own_tables_equal_refused_volumes_host(lib):
    """The cast with the scan's own volume taken out equals the cast against the explicitly re-fused other scans."""
    sc = C.random_scene('float64')
    want = host_cast(lib, sc['total'], sc['owns'], sc['vps'], sc['dirs'], sc['offset'], sc['poses'], mask=sc['mask'], **sc['rule'])
    ns = len(sc['offset']) - 1
    for s in range(ns):
        a, b = sc['offset'][s], sc['offset'][s + 1]
        others = sc['fuse']([k for k in range(ns) if k != s])
        got = host_cast(lib, others, None, sc['vps'][a:b], sc['dirs'][a:b], [0, b - a], sc['poses'][s:s + 1], mask=sc['mask'][a:b], **sc['rule'])
        # the table positions differ between the two volumes: the face is compared through the block it names
        for k in ('t', 'phi', 'normal', 'status'):
            assert np.array_equal(got[k], want[k][a:b], equal_nan=True), (s, k)
        hit = got['status'] == C.HIT
        assert np.array_equal(others.keys[got['face'][hit]], sc['total'].keys[want['face'][a:b][hit]]), s


# ---- 3. eval_bias' plumbing ----------------------------------------------------------------------------------------------------------
def test_config_and_truth_of_eval_bias(tmp_path):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import _bias_truth, eval_bias
    from depth_correction_amd.loss import TsdfTarget
    from depth_correction_amd.model import BaseModel

    class MeshOnly(object):
        def __iter__(self):
            return iter(())

        def get_mesh(self):
            return 'the mesh'

    cfg = Config(device='cpu')
    assert (cfg.bias_eval_tsdf_voxel_size, cfg.bias_eval_tsdf_trunc, cfg.bias_eval_tsdf_min_count, cfg.bias_eval_tsdf_leave_one_out,
            cfg.bias_eval_tsdf_step, cfg.bias_eval_tsdf_max_range) == (0.1, None, 1, True, None, None)
    assert cfg.bias_eval_against == 'auto' and _bias_truth(MeshOnly(), 'm', cfg) == 'the mesh'           # 'auto' never chooses 'tsdf'
    cfg.bias_eval_against, cfg.bias_eval_tsdf_voxel_size, cfg.bias_eval_tsdf_trunc, cfg.bias_eval_tsdf_min_count = 'tsdf', 0.2, 0.5, 2
    cfg.bias_eval_tsdf_leave_one_out, cfg.bias_eval_tsdf_step, cfg.bias_eval_tsdf_max_range = False, 0.05, 30.0
    path = str(tmp_path / 'cfg.yaml')
    cfg.to_yaml(path)
    assert Config().from_yaml(path).to_dict() == cfg.to_dict() == cfg.copy().to_dict()
    truth = _bias_truth(MeshOnly(), 'm', cfg)
    assert isinstance(truth, TsdfTarget) and (truth.voxel_size, truth.trunc, truth.min_count, truth.leave_one_out, truth.refresh_every) == \
        (0.2, 0.5, 2, False, 0) and truth.total is None
    with pytest.raises(RuntimeError, match='needs a GPU'):                # 'tsdf' gets as far as a mesh dataset does
        eval_bias(cfg, test_datasets=[MeshOnly()], model=BaseModel())
    cfg.bias_eval_against = 'volume'
    with pytest.raises(ValueError, match='bias_eval_against'):
        eval_bias(cfg, test_datasets=[MeshOnly()], model=BaseModel())
