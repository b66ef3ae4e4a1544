"""The supervised cloud loss on the MI355X (csrc/dc_cloudloss.hip, ops.cloud_loss, loss.cloud_loss, train() with cfg.loss =
'cloud_loss', metrics.map_accuracy on a survey) against the numpy closed form of tests/cloudloss_reference.py, which
tests/test_cloudloss_host.py holds to central differences.

Scene and hand-made points: cloudloss_reference's header (scans of 300, 1, 0 and 129 points, a survey of about 4000 points).

Bars, all from reference quantities (nothing is tuned to the kernel):
  points       bar = 2^-40 x extent, the bar of tests/test_gpu_meshdist.py, for |x - reference x| and every distance and residual
  indices      equal to the brute force's wherever its second-best d^2 exceeds its best by more than 1e-9 x extent^2 (the reference
               alone excludes nothing but the hand-made tie: tests/test_cloudloss_host.py and test 1 here check it on the CPU)
  threshold    equal to np.quantile of the DEVICE's matched distances (the equality tests/test_gpu_slam_parity.py holds dc_quantile
               to), hence within bar of the reference's; the used set equal (no reference distance lies within bar of it)
  loss         bar, against the closed form, whose correspondences are then the device's
  gradients    cloudloss_reference.grad_bounds: 2^-40 sum |a_j|, plus sum |a_j| 2 bar / l_j for the point form, 2 bar per component
               times the coefficient for the squared forms, nothing more for the plane form
  bit equality idx_out / dist_out against ops.knn on the fp64 points of ops.points_fwd; two calls, whatever ran in between."""
import math
import os
import re

import numpy as np
import pytest
import torch

import cloudloss_reference as C
import meshloss_reference as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NP_DTYPES = {'float32': np.float32, 'float64': np.float64}
W_MODEL = {'ScaledPolynomial': ([-0.004, 0.002], [2.0, 4.0]), 'Polynomial': ([0.003, -0.001], [2.0, 4.0]), 'InvCos': ([1e-4], [0.0]),
           None: (None, None)}
_cache = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


class Scene(object):
    """The reference scene on the device in one cloud dtype: PointSet, scan_ptr, poses12, the loss mask, the survey and its grid."""

    def __init__(self, dtype, lmask=None, seed=11, sizes=C.SIZES):
        from depth_correction_amd import ops
        from depth_correction_amd.survey import SurveyCloud
        self.mesh, self.scans, self.poses, self.loss_mask = C.scene(dtype=NP_DTYPES[dtype], seed=seed, sizes=sizes)
        if lmask is not None:
            off = 0
            for c in self.scans:
                c['lmask'] = c['lmask'] & lmask[off:off + len(c['depth'])]
                off += len(c['depth'])
        cat = lambda k: np.concatenate([c[k] for c in self.scans])
        self.ps = ops.PointSet(_t(cat('vps')), _t(cat('dirs')), _t(cat('depth')), _t(cat('inc')), _t(cat('lmask')))
        self.sizes = [len(c['depth']) for c in self.scans]
        self.n = sum(self.sizes)
        self.scan_ptr = _t(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64))
        self.poses12 = _t(self.poses[:, :3, :].reshape(-1, 12))
        self.sp, self.sn = C.survey()
        self.survey = SurveyCloud(self.sp, self.sn)
        assert self.survey.n_dropped == 0 and np.array_equal(self.survey.points.numpy(), self.sp)
        self.sd = self.survey.on_device(DEV)
        self.mask = _t(self.loss_mask)

    def model(self, kind):
        w, e = W_MODEL[kind]
        return (kind, None, None) if kind is None else (kind, _t(w, torch.float64), _t(e, torch.float64))

    def run(self, kind=None, w=None, e=None, **kw):
        from depth_correction_amd import ops
        kw.setdefault('max_dist', C.MAX_DIST)
        kw.setdefault('mask', self.mask)
        out = ops.cloud_loss(self.sd, self.ps, self.scan_ptr, self.poses12, kind, w, e, **kw)
        torch.cuda.synchronize()
        return out

    def reference(self, kind, **kw):
        wv, ev = W_MODEL[kind]
        return C.cloud_loss(self.sp, self.sn, self.scans, self.poses, kind, wv, ev, loss_mask=self.loss_mask, **kw)

    def points64(self, kind, w, e):
        """The same fields in fp64 through the un-fused point kernel."""
        from depth_correction_amd import ops
        f64 = lambda t: None if t is None else t.double().contiguous()
        sid = torch.repeat_interleave(torch.arange(len(self.sizes), device=DEV), _t(np.array(self.sizes))).to(torch.int32).contiguous()
        ps64 = ops.PointSet(f64(self.ps.vps), f64(self.ps.dirs), f64(self.ps.depth), f64(self.ps.inc), self.ps.lmask, sid)
        return ops.points_fwd(ps64, self.poses12, kind, w, e)


def _scene(dtype, sizes=C.SIZES):
    if (dtype, sizes) not in _cache:
        _cache[dtype, sizes] = Scene(dtype, sizes=sizes)
    return _cache[dtype, sizes]


def _split(out, nt, ns):
    o = out.cpu().numpy()
    return dict(loss=o[0], used=o[1], gated=o[2], trimmed=o[3], invalid=o[4], threshold=o[5], gw=o[6:6 + nt], ge=o[6 + nt:6 + 2 * nt],
                gT=o[6 + 2 * nt:].reshape(ns, 3, 4))


COUNTS = ('used', 'gated', 'trimmed', 'invalid')


def _check_gradients(got, ref, plane, squared, what, with_e):
    bounds = C.grad_bounds(ref, plane=plane, squared=squared)
    print('%s: loss %.12g (reference %.12g, |diff| %.3g, bar %.3g)' % (what, got['loss'], ref['loss'], abs(got['loss'] - ref['loss']), C.BAR))
    assert abs(got['loss'] - ref['loss']) <= C.BAR, (what, got['loss'], ref['loss'])
    assert tuple(got[k] for k in COUNTS) == tuple(ref[k] for k in COUNTS), what
    for name in ('gw', 'ge', 'gT'):
        want = ref[name] if (name != 'ge' or with_e) else np.zeros_like(ref['ge'])
        if not want.size:
            assert not got[name].size
            continue
        err = np.abs(got[name] - want)
        worst = np.unravel_index(int(np.argmax(err - bounds[name])), err.shape)
        print('%s: %s largest |diff| %.3g (its bound %.3g, largest entry %.3g)' % (what, name, err[worst], bounds[name][worst], np.abs(want).max()))
        assert (err <= bounds[name]).all(), (what, name, worst, got[name][worst], want[worst], err[worst], bounds[name][worst])
    if ref['used']:
        assert np.abs(ref['gT']).max() > 0


# ---- 1. per-point outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_per_point_outputs(dtype):
    """idx_out / dist_out bit-equal to ops.knn(survey, 1, r = max_dist, query = ops.points_fwd(...)) gated by the mask; the index equal
    to the brute force's wherever it decides clearly; the hand-made tie to the lower index; the residual against numpy."""
    from depth_correction_amd import ops
    sc = _scene(dtype)
    kind, w, e = sc.model('ScaledPolynomial')
    out, idx, dist, resid = sc.run(kind, w, e, want_points=True)
    ref = sc.reference(kind)
    x64 = sc.points64(kind, w, e)
    d2, i2 = ops.knn(sc.sd.points, 1, r=C.MAX_DIST, query=x64)
    torch.cuda.synchronize()
    finite = np.isfinite(ref['x']).all(axis=1)
    assert np.abs(x64.cpu().numpy()[finite] - ref['x'][finite]).max() <= C.BAR
    keep = sc.mask & (i2[:, 0] >= 0)
    assert torch.equal(idx, torch.where(keep, i2[:, 0], torch.full_like(i2[:, 0], -1)))
    assert torch.equal(dist, torch.where(keep, d2[:, 0], torch.full_like(d2[:, 0], float('inf'))))
    # against the brute force: on the CPU, the reference alone leaves out nothing but the hand-made tie
    bf_idx, bf_d2, bf_second = C.nearest(sc.sp, ref['x'])
    with np.errstate(invalid='ignore'):
        clear = bf_second - bf_d2 > 1e-9 * C.EXTENT ** 2
    assert list(np.flatnonzero(finite & ~clear)) == [C.HAND['tie']] and (finite & ~clear).mean() <= 0.01
    got = idx.cpu().numpy()
    used = ref['mask']
    assert np.array_equal(got >= 0, used)
    assert np.array_equal(got[used & clear], bf_idx[used & clear])
    assert got[C.HAND['tie']] == 1 and bf_idx[C.HAND['tie']] == 1                       # survey points 1 and 2 tie: the lower index
    assert got[C.HAND['on_point']] == 0 and dist[C.HAND['on_point']].item() == 0.0 and resid[C.HAND['on_point']].item() == 0.0
    assert got[C.HAND['inside']] == 3 and got[C.HAND['outside']] == -1 and got[C.HAND['nan']] == -1 and got[C.MASKED] == -1
    d, r = dist.cpu().numpy(), resid.cpu().numpy()
    print('%s: distances %.3g .. %.3g m, largest |dist - brute force| %.3g m, |resid - reference| %.3g m (bar %.3g m)'
          % (dtype, d[used].min(), d[used].max(), np.abs(d[used] - ref['dist'][used]).max(), np.abs(r[used] - ref['r'][used]).max(), C.BAR))
    assert np.abs(d[used] - ref['dist'][used]).max() <= C.BAR and np.abs(r[used] - ref['r'][used]).max() <= C.BAR
    assert np.isinf(d[~used]).all() and np.isnan(r[~used]).all()


# ---- 2. status counts, the threshold, the used set ----------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio', [1.0, 0.8])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_status_counts_and_used_set(dtype, ratio):
    sc = _scene(dtype)
    kind, w, e = sc.model('ScaledPolynomial')
    ref = sc.reference(kind, ratio=ratio)
    # on the CPU: no reference distance within the bar of the gate or of the threshold
    assert np.abs(ref['dist'][ref['matched']] - C.MAX_DIST).min() > C.BAR
    if ratio < 1.0:
        assert np.abs(ref['dist'][ref['matched']] - ref['threshold']).min() > C.BAR
    out, idx, dist, _ = sc.run(kind, w, e, inlier_ratio=ratio, want_points=True)
    got = _split(out, 2, len(sc.sizes))
    print('%s ratio %.1f: used %d gated %d trimmed %d invalid %d threshold %.12g (reference %.12g)'
          % ((dtype, ratio) + tuple(got[k] for k in COUNTS) + (got['threshold'], ref['threshold'])))
    assert tuple(got[k] for k in COUNTS) == tuple(ref[k] for k in COUNTS)
    assert got['invalid'] == 1 and got['gated'] >= 2 and (got['trimmed'] > 0) == (ratio < 1.0)
    if ratio < 1.0:
        full = sc.run(kind, w, e, want_points=True)[2].cpu().numpy()              # every matched distance
        assert got['threshold'] == np.quantile(full[np.isfinite(full)], ratio)
        assert abs(got['threshold'] - ref['threshold']) <= C.BAR
    else:
        assert math.isinf(got['threshold'])
    assert np.array_equal(idx.cpu().numpy() >= 0, ref['mask'])
    assert np.array_equal(idx.cpu().numpy(), ref['idx'])


# ---- 3. loss and gradients -------------------------------------------------------------------------------------------------------
CASES = {
    'none_plane': dict(kind=None),
    'none_point_trim': dict(kind=None, plane=False, inlier_ratio=0.8),
    'sp_plane': dict(kind='ScaledPolynomial'),
    'sp_plane_squared': dict(kind='ScaledPolynomial', squared=True),
    'sp_plane_trim': dict(kind='ScaledPolynomial', inlier_ratio=0.8),
    'sp_point': dict(kind='ScaledPolynomial', plane=False),
    'sp_point_squared_trim': dict(kind='ScaledPolynomial', plane=False, squared=True, inlier_ratio=0.8),
    'sp_point_trim_exponent': dict(kind='ScaledPolynomial', plane=False, inlier_ratio=0.8, want_exponent=True),
    'poly_plane_squared_trim_exponent': dict(kind='Polynomial', squared=True, inlier_ratio=0.8, want_exponent=True),
    'poly_point': dict(kind='Polynomial', plane=False),
    'invcos_plane_trim': dict(kind='InvCos', inlier_ratio=0.8),
    'invcos_point_squared': dict(kind='InvCos', plane=False, squared=True),
    'local_mask_plane': dict(kind='ScaledPolynomial', local_mask=True),
    # 513 points in scan 0: five blocks on the finishing kernel's four chains, so chain 0 adds two rows (float64 only)
    'five_blocks': dict(kind='ScaledPolynomial', sizes=(513, 0, 1)),
}


@pytest.mark.parametrize('case,dtype', [(c, d) for d in ('float32', 'float64') for c in sorted(CASES) if 'sizes' not in CASES[c]]
                         + [('five_blocks', 'float64')])
def test_loss_and_gradients(dtype, case):
    """out against the closed form: loss, the four counts, dL/dw, dL/de, dL/d[R|t] of every scan (the empty scan's is zero).  The
    closed form's correspondences are the brute force's, asserted equal to the device's first."""
    cfg = dict(CASES[case])
    rng = np.random.default_rng(5)
    sizes = cfg.pop('sizes', C.SIZES)
    sc = Scene(dtype, lmask=rng.random(C.N_ALL) < 0.7) if cfg.pop('local_mask', False) else _scene(dtype, sizes)
    kind, w, e = sc.model(cfg.pop('kind'))
    plane, squared, want_e = cfg.get('plane', True), cfg.get('squared', False), cfg.get('want_exponent', False)
    out, idx, dist, resid = sc.run(kind, w, e, want_points=True, **cfg)
    ref = sc.reference(kind, plane=plane, squared=squared, ratio=cfg.get('inlier_ratio', 1.0))
    assert ref['mask'][:sizes[0]].any() and ref['mask'][-sizes[-1]:].any()       # the first and the last scan have used points
    assert np.array_equal(idx.cpu().numpy(), ref['idx'])
    nt = 0 if kind is None else len(W_MODEL[kind][0])
    got = _split(out, nt, len(sc.sizes))
    _check_gradients(got, ref, plane, squared, '%s %s' % (dtype, case), want_e)
    assert not got['gT'][sizes.index(0)].any()                         # the empty scan
    if case == 'local_mask_plane':                                     # uncorrected points: no weight gradient of theirs
        lm = np.concatenate([c['lmask'] for c in sc.scans])
        assert not ref['terms']['gw'][~lm].any() and ref['terms']['gw'][lm].any()


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_whatever_ran_between():
    sc, other = _scene('float32'), Scene('float64', seed=23)
    kind, w, e = sc.model('ScaledPolynomial')
    kw = dict(want_points=True, inlier_ratio=0.8, want_exponent=True)
    a = sc.run(kind, w, e, **kw)
    b = sc.run(kind, w, e, **kw)
    other.run(*other.model('Polynomial'), squared=True, plane=False)
    sc.run(kind, w * 1.5, e, inlier_ratio=0.5)                         # the same workspace and grid, other values
    c = sc.run(kind, w, e, **kw)
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t          # (NaN residuals of unused points compare as bits)
    for x, y, z in zip(a, b, c):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))
    assert torch.isnan(a[3]).any() and not torch.isnan(a[0]).any()


# ---- 5. arguments and degenerate inputs --------------------------------------------------------------------------------------------
def test_argument_contract():
    from depth_correction_amd import ops
    sc = _scene('float64')
    for bad in (None, float('nan'), float('inf'), 0.0, -1.0):
        with pytest.raises(ValueError, match='max_dist'):
            sc.run(max_dist=bad)
    with pytest.raises(ValueError, match='inlier_ratio'):
        sc.run(inlier_ratio=1.5)
    with pytest.raises(ValueError, match='scan_ptr'):
        ops.cloud_loss(sc.sd, sc.ps, _t(np.array([0, 5, 3, sc.n], np.int64)), sc.poses12[:3].contiguous(), max_dist=1.0)
    # no points at all: NaN loss, zero counts and gradients, an infinite threshold; a sequence of empty scans is legal
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
    empty = ops.PointSet(None, z(0, 3), z(0), z(0))
    kind, w, e = sc.model('ScaledPolynomial')
    out = ops.cloud_loss(sc.sd, empty, _t(np.zeros(3, np.int64)), sc.poses12[:2].contiguous(), kind, w, e, max_dist=1.0, inlier_ratio=0.8)
    out = out.cpu().numpy()
    assert out.shape == (6 + 4 + 24,) and math.isnan(out[0]) and math.isinf(out[5]) and not out[1:5].any() and not out[6:].any()
    # every point gated: NaN loss, zero gradients, a NaN threshold (the quantile of nothing), no error
    o3 = sc.run(kind, w, e, max_dist=1e-9, inlier_ratio=0.8, mask=sc.mask & _t(np.arange(sc.n) != C.HAND['on_point'])).cpu().numpy()
    assert math.isnan(o3[0]) and o3[1] == 0 and o3[2] == sc.n - 3 and o3[3] == 0 and o3[4] == 1 and math.isnan(o3[5]) and not o3[6:].any()


# ---- 6. autograd surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('plane', [True, False])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_autograd_surface_against_unfused_composition(dtype, plane):
    """loss.cloud_loss with a model and per-pose corrections requiring grad, trimmed at 0.8: loss, w.grad and pose_deltas.grad of the
    fused call equal those of the un-fused torch composition (fused=False) and the closed form within test 3's bounds -- the
    corrections' through the Jacobian of the corrected poses, |dT/ddelta| times the bound of dL/dT."""
    from depth_correction_amd import loss as L
    from depth_correction_amd.config import Config, PoseCorrection
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.eval import create_corrected_poses
    from depth_correction_amd.model import ScaledPolynomial
    sc = _scene(dtype)
    tdt = getattr(torch, dtype)
    clouds = [DepthCloud(vps=_t(c['vps']), dirs=_t(c['dirs']), depth=_t(c['depth']).reshape(-1, 1), inc_angles=_t(c['inc']).reshape(-1, 1),
                         mask=_t(c['lmask'])) for c in sc.scans]
    cfg = Config(device=DEV, float_type=dtype, pose_correction=PoseCorrection.pose)
    poses0 = _t(sc.poses, tdt)
    rng = np.random.default_rng(9)
    delta0 = rng.normal(scale=0.01, size=(len(clouds), 6))
    wv, ev = W_MODEL['ScaledPolynomial']
    kw = dict(cloud_point_to_plane=plane, cloud_max_dist=C.MAX_DIST, cloud_inlier_ratio=0.8)
    res = {}
    for fused in (True, False):
        model = ScaledPolynomial(w=list(wv), exponent=list(ev), device=DEV)
        deltas = _t(delta0, torch.float64).requires_grad_(True)       # (fp64 corrections: both forms see the same poses)
        poses_upd = create_corrected_poses([poses0.double()], [deltas], cfg)
        loss, loss_clouds = L.cloud_loss([clouds], poses_upd, model, masks=[(sc.survey, sc.mask)], fused=fused, **kw)
        loss.backward()
        torch.cuda.synchronize()
        res[fused] = (loss.item(), model.w.grad.cpu().numpy().reshape(-1), deltas.grad.cpu().numpy(), poses_upd[0].detach().cpu().numpy())
        assert len(loss_clouds) == 1 and len(loss_clouds[0]) == sc.n
    ref = C.cloud_loss(sc.sp, sc.sn, sc.scans, res[True][3], 'ScaledPolynomial', wv, ev, loss_mask=sc.loss_mask, plane=plane, ratio=0.8)
    # on the CPU: at these poses too the reference decides every correspondence, the gate and the threshold clearly
    _, bd2, bsec = C.nearest(sc.sp, ref['x'])
    with np.errstate(invalid='ignore'):
        assert (bsec - bd2 > 1e-9 * C.EXTENT ** 2)[np.isfinite(bd2)].all()
    assert np.abs(ref['dist'][ref['matched']] - C.MAX_DIST).min() > C.BAR and np.abs(ref['dist'][ref['matched']] - ref['threshold']).min() > C.BAR
    bounds = C.grad_bounds(ref, plane=plane)
    print('%s plane %d: fused %.12g, un-fused %.12g, closed form %.12g' % (dtype, plane, res[True][0], res[False][0], ref['loss']))
    assert abs(res[True][0] - res[False][0]) <= C.BAR and abs(res[True][0] - ref['loss']) <= C.BAR
    assert (np.abs(res[True][1] - res[False][1]) <= bounds['gw']).all(), (res[True][1], res[False][1], bounds['gw'])
    assert (np.abs(res[True][1] - ref['gw']) <= bounds['gw']).all()
    assert np.abs(res[True][1]).max() > 0
    d = _t(delta0, torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: create_corrected_poses([poses0.double()], [v], cfg)[0][:, :3, :], d)
    J = J.cpu().numpy()                                                # [S,3,4,S,6]
    S = len(clouds)
    bound_d = np.stack([(bounds['gT'][s][:, :, None] * np.abs(J[s, :, :, s, :])).sum(axis=(0, 1)) for s in range(S)])
    bound_d += 2.0 ** -40 * np.stack([(np.abs(ref['gT'][s])[:, :, None] * np.abs(J[s, :, :, s, :])).sum(axis=(0, 1)) for s in range(S)])
    want_d = np.stack([(ref['gT'][s][:, :, None] * J[s, :, :, s, :]).sum(axis=(0, 1)) for s in range(S)])
    err = np.abs(res[True][2] - res[False][2])
    print('%s plane %d: pose corrections, largest |fused - un-fused| %.3g (bound there %.3g)' % (dtype, plane, err.max(), bound_d.reshape(-1)[err.argmax()]))
    assert (err <= bound_d).all(), (err, bound_d)
    assert (np.abs(res[True][2] - want_d) <= bound_d).all()
    assert not res[True][2][2].any() and np.abs(res[True][2]).max() > 0


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def _pose(yaw, t):
    T = np.eye(4)
    T[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


def test_train_end_to_end(tmp_path, capsys):
    """train() with cfg.loss = 'cloud_loss' on two rendered sequences of the room (3 poses x 16 x 64 rays each) whose depths are
    biased by ScaledPolynomial(W_TRUE), against the surveys the datasets sample from their mesh: the run completes and writes
    best.yaml, the training loss falls, and the weights move from zero toward the generating ones (w . W_TRUE > 0: the direction
    only, no distance)."""
    from depth_correction_amd.config import Config, PoseCorrection
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.survey import SurveyCloud
    from depth_correction_amd.train import train
    path = tmp_path / 'room.ply'
    M.room().save_ply(str(path))
    cfg = Config(device=DEV, float_type='float64', min_depth=0.3, max_depth=25.0, grid_res=0.05, nn_k=0, nn_r=0.6, loss='cloud_loss',
                 n_opt_iters=30, lr=1e-3, log_dir=str(tmp_path / 'model'), pose_correction=PoseCorrection.none, cloud_samples=20000,
                 model_kwargs={'w': [0.0, 0.0], 'exponent': list(M.E_TRUE)})
    cfg.loss_kwargs = dict(cfg.loss_kwargs, cloud_max_dist=0.3, cloud_inlier_ratio=0.9)
    gt = ScaledPolynomial(w=list(M.W_TRUE), exponent=list(M.E_TRUE), device=DEV)
    seqs = []
    for q in range(2):
        poses = np.stack([_pose(0.3 * i + q, (-2.0 + 1.2 * i, 0.4 * q - 0.5, 0.1 * i)) for i in range(3)])
        ds = RenderedMeshDataset(str(path), poses=poses, size=(16, 64), fov=(45.0, 360.0), num_segments=8, device=DEV)
        seqs.append(DepthBiasDataset(ds, gt, cfg=cfg))
    sv = seqs[0].get_survey(cfg.cloud_samples)
    assert isinstance(sv, SurveyCloud) and len(sv) == 20000 and seqs[0].get_survey(cfg.cloud_samples) is sv
    os.makedirs(cfg.log_dir)
    capsys.readouterr()
    best = train(cfg, train_datasets=seqs, val_datasets=[])
    text = capsys.readouterr().out
    losses = [float(m) for m in re.findall(r'^It\. \d+: train loss: (-?[0-9.]+|nan)', text, flags=re.M)]
    assert len(losses) == 30 and os.path.exists(os.path.join(cfg.log_dir, 'best.yaml')) and best is not None
    trained = ScaledPolynomial(w=[0.0, 0.0], exponent=list(M.E_TRUE), device=DEV)
    trained.load_state_dict(torch.load(best.model_state_dict))
    wt = trained.w.detach().cpu().numpy().reshape(-1)
    print('train loss: first %.9f, last %.9f; trained w %s (generating %s)' % (losses[0], losses[-1], wt, M.W_TRUE))
    assert losses[-1] < losses[0]
    assert float(np.dot(wt, M.W_TRUE)) > 0.0


def test_sharded_training_is_refused(monkeypatch, tmp_path):
    from depth_correction_amd import train as T
    from depth_correction_amd.config import Config
    monkeypatch.setattr(T, '_sharding', lambda cfg: (0, 2, True))
    with pytest.raises(NotImplementedError, match='cloud_loss'):
        T.train(Config(device=DEV, loss='cloud_loss', log_dir=str(tmp_path)), train_datasets=[], val_datasets=[])


# ---- 8. map accuracy against a survey ---------------------------------------------------------------------------------------------
def test_map_accuracy_against_survey():
    """metrics.map_accuracy(points, survey) = the numpy statistics of the brute-force nearest-point distances (each within the bar;
    n exact), signed_mean NaN, no completeness_mean; point_to_cloud_distance's indices are the brute force's."""
    from depth_correction_amd import metrics
    sc = _scene('float64')
    kind, w, e = sc.model('ScaledPolynomial')
    ref = sc.reference(kind)
    finite = np.isfinite(ref['x']).all(axis=1)
    pts = _t(ref['x'][finite])
    res = metrics.map_accuracy(pts, sc.survey, inlier_ratio=0.8)
    idx, d2, second = C.nearest(sc.sp, ref['x'][finite])
    d = np.sqrt(d2)
    thr = np.quantile(d, 0.8)
    want = dict(n=float(len(d)), mean=d.mean(), rms=np.sqrt((d * d).mean()), median=np.quantile(d, 0.5), trimmed_mean=d[d <= thr].mean(),
                max=d.max())
    print('map accuracy against the survey: %s' % {k: res[k] for k in want})
    assert res['n'] == want['n'] and math.isnan(res['signed_mean']) and 'completeness_mean' not in res
    for k in ('mean', 'rms', 'median', 'trimmed_mean', 'max'):
        assert abs(res[k] - want[k]) <= C.BAR, (k, res[k], want[k])
    dist, got_idx, closest = metrics.point_to_cloud_distance(pts, sc.survey, return_closest=True)
    clear = second - d2 > 1e-9 * C.EXTENT ** 2
    assert np.array_equal(got_idx.cpu().numpy()[clear], idx[clear]) and np.array_equal(closest.cpu().numpy()[clear], sc.sp[idx[clear]])
    assert np.abs(dist.cpu().numpy() - d).max() <= C.BAR
    gated = metrics.point_to_cloud_distance(pts, sc.survey, max_dist=C.MAX_DIST)
    assert np.array_equal(np.isfinite(gated.cpu().numpy()), d2 < C.MAX_DIST ** 2)
