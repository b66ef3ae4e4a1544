"""Host side of the supervised cloud loss (csrc/dc_cloudloss_math.h, loss.cloud_loss, survey.SurveyCloud, Config): the per-point term
of the kernel in its host build against numpy, the numpy closed form of tests/cloudloss_reference.py against central differences at
frozen correspondences -- which pins the reference before the GPU tests hold the kernel to it --, the properties of the test scene
the GPU tests rely on, and the configuration surface.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cloudloss_reference as C
import meshloss_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')


@pytest.fixture(scope='module')
def host():
    import __graft_entry__ as ge
    if not os.path.exists(HOSTLIB):
        ge.build()
    lib = ctypes.CDLL(HOSTLIB)
    if not hasattr(lib, 'dc_host_cloud_loss_term'):
        ge.build()
        lib = ctypes.CDLL(HOSTLIB)
    lib.dc_host_cloud_loss_term.restype = ctypes.c_double
    lib.dc_host_cloud_loss_term.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2
    return lib


def _term(lib, x, y, n, plane, squared):
    x, y, n = (np.ascontiguousarray(v, np.float64) for v in (x, y, n))
    r, g = np.zeros(1), np.zeros(3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ell = lib.dc_host_cloud_loss_term(p(x), p(y), p(n), int(plane), int(squared), p(r), p(g))
    return ell, r[0], g


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


_N = np.array([0.48, 0.48, np.sqrt(1.0 - 2.0 * 0.48 ** 2)])          # |n| = 1 to rounding
_Y = [0.5, 0.25, 0.75]
CASES = {                                                  # x, y
    'positive': ([0.7, -0.05, 1.15], _Y),
    'negative': ([0.3, 0.55, -0.05], _Y),                  # n . (x - y) < 0
    'zero': (_Y, _Y),                                      # x on y
    'in_plane': ([1.5, -0.75, 0.75], _Y),                  # off y by (1, -1, 0): r = 0.48 - 0.48 + 0 = 0 exactly, in y's plane
}


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('plane', [False, True])
@pytest.mark.parametrize('case', sorted(CASES))
def test_point_term_against_numpy(host, case, plane, squared):
    """l, r and dl/dx of the kernel's header in both forms, squared and not, at positive, negative and zero r: r and the squared
    term are the same operations as numpy's (bit-equal); the unit vector and the products with 2 one division / product per
    component (<= 4 ulp); l = 0 gives a zero gradient."""
    x, y = (np.array(v, np.float64) for v in CASES[case])
    ell, r, g = _term(host, x, y, _N, plane, squared)
    e = x - y
    if plane:
        ref_r = (_N[0] * e[0] + _N[1] * e[1]) + _N[2] * e[2]
        assert r == ref_r and ell == (ref_r * ref_r if squared else abs(ref_r))
        assert {'positive': ref_r > 0, 'negative': ref_r < 0}.get(case, ref_r == 0)
        ref_g = 2.0 * ref_r * _N if squared else np.sign(ref_r) * _N
        if ref_r == 0:
            assert ell == 0.0 and np.array_equal(g, np.zeros(3)), (case, g)
        elif squared:
            assert _ulps(g, ref_g).max() <= 4, (case, g, ref_g)
        else:
            assert np.array_equal(g, ref_g)                # +-n itself
        return
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert r == np.sqrt(d2) and ell == (d2 if squared else np.sqrt(d2))
    if case == 'zero':
        assert r == 0.0 and ell == 0.0 and np.array_equal(g, np.zeros(3))
        return
    ref_g = 2.0 * e if squared else e / np.sqrt(d2)
    assert _ulps(g, ref_g).max() <= 4, (case, g, ref_g)
    if not squared:
        assert abs(np.linalg.norm(g) - 1.0) < 1e-15


@pytest.mark.parametrize('plane', [False, True])
def test_point_term_keeps_a_nan_visible(host, plane):
    ell, r, g = _term(host, [np.nan, 0.0, 0.0], [0.0, 0.0, 0.0], _N, plane, False)
    assert np.isnan(ell) and np.isnan(r) and np.isnan(g).all()


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    return C.scene(), C.survey()


def test_scene_properties(scene):
    """What the GPU tests rely on, checked on the reference alone: the brute force's second-best d^2 exceeds its best by more than
    1e-9 extent^2 everywhere but at the hand-made tie; the hand-made points fall as designed; no matched distance lies within the bar
    of max_dist or of the 0.8 quantile."""
    (mesh, scans, poses, loss_mask), (sp, sn) = scene
    assert len(sp) > 3000 and np.allclose(np.linalg.norm(sn, axis=1), 1.0)
    kind, w, e = 'ScaledPolynomial', np.array([-0.004, 0.002]), np.array([2.0, 4.0])
    x = M.points(scans, poses, kind, w, e)['x']
    idx, d2, second = C.nearest(sp, x)
    with np.errstate(invalid='ignore'):
        close = np.isfinite(d2) & ~(second - d2 > 1e-9 * C.EXTENT ** 2)
    assert list(np.flatnonzero(close)) == [C.HAND['tie']]
    assert d2[C.HAND['tie']] == second[C.HAND['tie']] == 2.0 ** -8 + 2.0 ** -10 and idx[C.HAND['tie']] == 1
    assert idx[C.HAND['on_point']] == 0 and d2[C.HAND['on_point']] == 0.0
    assert idx[C.HAND['inside']] == 3 == idx[C.HAND['outside']]
    assert d2[C.HAND['inside']] < C.MAX_DIST ** 2 < d2[C.HAND['outside']]
    assert idx[C.HAND['nan']] == -1
    for ratio in (1.0, 0.8):
        ref = C.cloud_loss(sp, sn, scans, poses, kind, w, e, loss_mask=loss_mask, ratio=ratio)
        n_in = int(loss_mask.sum())
        assert ref['used'] + ref['gated'] + ref['trimmed'] + ref['invalid'] == n_in and ref['invalid'] == 1
        assert ref['gated'] > 1 and ref['used'] > 0.5 * n_in
        assert ref['mask'][[C.HAND['on_point'], C.HAND['tie'], C.HAND['inside']]].all() or ratio < 1.0
        assert not ref['mask'][[C.HAND['outside'], C.HAND['nan'], C.MASKED]].any()
        finite = np.isfinite(np.sqrt(d2))
        assert np.abs(np.sqrt(d2)[finite] - C.MAX_DIST).min() > C.BAR
        if ratio < 1.0:
            assert ref['trimmed'] > 0 and np.abs(ref['dist'][ref['matched']] - ref['threshold']).min() > C.BAR
        print('ratio %.1f: used %d gated %d trimmed %d invalid %d, threshold %.6f, loss %.9g'
              % (ratio, ref['used'], ref['gated'], ref['trimmed'], ref['invalid'], ref['threshold'], ref['loss']))


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('plane', [False, True])
def test_closed_form_against_central_differences(scene, plane, squared):
    """dL/dw, dL/de and dL/d[R|t] of the numpy closed form against central differences of its own loss at h = 1e-6 with the
    correspondences (and with them the used set) frozen at the unperturbed ones -- the gradient's definition.  Bound 1e-6 relative to
    the largest entry of the group, the bar of tests/test_meshloss_host.py for its closed form: the h^2 truncation and the eps / h
    rounding of central differences with headroom -- not a measurement of any kernel.  The point on its survey point (l = 0, where
    the un-squared forms have a kink) is left out of the differences, as the closed form leaves it out of the gradient."""
    (mesh, scans, poses, loss_mask), (sp, sn) = scene
    kind, w, e = 'ScaledPolynomial', np.array([-0.004, 0.002]), np.array([2.0, 4.0])
    mask = loss_mask.copy()
    mask[C.HAND['on_point']] = False
    ref = C.cloud_loss(sp, sn, scans, poses, kind, w, e, loss_mask=mask, plane=plane, squared=squared, ratio=0.8)
    frozen = np.where(ref['mask'], ref['match'], -1)

    def loss(w_=w, e_=e, P=poses):
        out = C.cloud_loss(sp, sn, scans, P, kind, w_, e_, idx=frozen, loss_mask=mask & ref['mask'], plane=plane, squared=squared)
        assert out['used'] == ref['used']
        return out['loss']

    assert loss() == ref['loss']
    h = 1e-6
    diff = lambda fun: (fun(h) - fun(-h)) / (2 * h)
    fd_w = np.array([diff(lambda s, k=k: loss(w_=w + s * np.eye(2)[k])) for k in range(2)])
    fd_e = np.array([diff(lambda s, k=k: loss(e_=e + s * np.eye(2)[k])) for k in range(2)])
    fd_T = np.zeros((len(scans), 3, 4))
    for s_ in (0, 1, 3):                                   # (scan 2 is empty: its gradient is zero by construction)
        for a in range(3):
            for b in range(4):
                def f(step, s_=s_, a=a, b=b):
                    P = poses.copy()
                    P[s_, a, b] += step
                    return loss(P=P)
                fd_T[s_, a, b] = diff(f)
    for name, got, fd in (('gw', ref['gw'], fd_w), ('ge', ref['ge'], fd_e), ('gT', ref['gT'], fd_T)):
        err = np.abs(got - fd).max() / np.abs(fd).max()
        print('plane %d squared %d %s: closed form against central differences, relative error %.3g' % (plane, squared, name, err))
        assert err <= 1e-6, (name, err)
    assert np.array_equal(ref['gT'][2], np.zeros((3, 4)))


# ---- configuration surface -----------------------------------------------------------------------------------------------------------
def test_config_accepts_cloud_loss():
    from depth_correction_amd.config import CLOUD_LOSS_DEFAULTS, Config, Loss
    from depth_correction_amd import loss as L
    assert Loss.cloud_loss == 'cloud_loss' and 'cloud_loss' in Loss
    assert 'cloud_loss' not in list(Loss) and 'cloud_loss' not in Config().eval_losses       # not part of the default sweep
    cfg = Config()
    cfg.loss = 'cloud_loss'
    assert L.loss_by_name('cloud_loss') is L.cloud_loss and 'cloud_loss' in L.__all__
    fun = L.create_loss(cfg)
    assert fun.name == 'cloud_loss' and callable(fun)
    assert CLOUD_LOSS_DEFAULTS == {'cloud_point_to_plane': True, 'cloud_squared': False, 'cloud_max_dist': None, 'cloud_inlier_ratio': 1.0}
    assert cfg.cloud_samples > 0
    assert Config.from_dict(Config(), cfg.to_dict()).cloud_samples == cfg.cloud_samples


def test_cloud_loss_argument_errors():
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd import loss as L
    from depth_correction_amd.survey import SurveyCloud
    sv = SurveyCloud(np.zeros((2, 3)) + [[0.0], [1.0]], np.tile([0.0, 0.0, 1.0], (2, 1)))
    cloud = DepthCloud(vps=torch.zeros((3, 3)), dirs=torch.eye(3), depth=torch.ones((3, 1)))
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.cloud_loss([[cloud]], [torch.eye(4)[None]], None, masks=[(sv, None)], cloud_max_dist=1.0)
    with pytest.raises(ValueError, match='at least one sequence'):
        L.cloud_loss([], None, None, masks=[])


def test_survey_masks_errors():
    from depth_correction_amd.eval import survey_masks

    class NoSurvey(object):
        pass

    with pytest.raises(ValueError, match='no surveyed cloud'):
        survey_masks([NoSurvey()], ['bare'], [[]])

    class Own(object):
        pass
    from depth_correction_amd.survey import SurveyCloud
    own = Own()
    own.survey = SurveyCloud(np.zeros((1, 3)), np.array([[0.0, 0.0, 2.0]]))
    (sv, mask), = survey_masks([own], ['own'], [[]])
    assert sv is own.survey and mask is None


def test_survey_cloud_construction(tmp_path):
    from depth_correction_amd.survey import SurveyCloud
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    nrm = np.tile([0.0, 3.0, 4.0], (5, 1))
    nrm[1, 0], nrm[3, 2] = np.nan, np.inf
    with pytest.warns(UserWarning, match='dropped 2 of 5'):
        sv = SurveyCloud.from_points(pts, nrm)
    assert len(sv) == 3 and sv.n_dropped == 2 and sv.points.dtype == torch.float64 and sv.normals.dtype == torch.float64
    assert np.array_equal(sv.points.numpy(), pts[[0, 2, 4]].astype(np.float64))
    assert np.allclose(sv.normals.numpy(), [[0.0, 0.6, 0.8]] * 3, atol=1e-16)
    assert '2 dropped' in repr(sv)
    with pytest.raises(ValueError, match='shape'):
        SurveyCloud(pts, nrm[:4])
    with pytest.raises(ValueError, match='finite'):
        SurveyCloud(np.array([[np.nan, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match='zero'):
        SurveyCloud(np.zeros((1, 3)), np.zeros((1, 3)))
    with pytest.raises(RuntimeError, match='GPU'):
        sv.on_device('cpu')
    # the structured .npz layout with normals goes through scan_io's reader
    arr = np.zeros(4, dtype=[(k, 'f4') for k in ('x', 'y', 'z', 'normal_x', 'normal_y', 'normal_z')])
    arr['x'], arr['normal_z'] = np.arange(4), 1.0
    np.savez(str(tmp_path / 'survey.npz'), cloud=arr)
    sv2 = SurveyCloud.from_file(str(tmp_path / 'survey.npz'))
    assert len(sv2) == 4 and np.array_equal(sv2.points[:, 0].numpy(), np.arange(4.0)) and np.array_equal(sv2.normals[:, 2].numpy(), np.ones(4))
