"""The supervised mesh loss on the MI355X (csrc/dc_meshloss.hip, ops.mesh_loss, loss.mesh_loss, train() with cfg.loss = 'mesh_loss')
against the numpy closed form of tests/meshloss_reference.py, which tests/test_meshloss_host.py holds to central differences.

Scene and sizes: meshloss_reference's header (scans of 300, 1, 0 and 129 points on the 380-face pillared room).

Bars, all from reference quantities (nothing is tuned to the kernel):
  distances    bar = 2^-40 x extent, the bar of tests/test_gpu_meshdist.py (its header gives the reason); faces where the brute
               force's second-best distance exceeds its best by more than 1e-9 x extent
  loss         bar, against the closed form evaluated at the DEVICE's faces (after the per-point check has held: no near-tie list)
  gradients    per entry sum_j a_j: 2^-40 sum |a_j| + sum |a_j| 2 bar / r_j (meshloss_reference.grad_bounds: fp64 summation of
               <= 1e3 terms, and the conditioning of (x - c) / r at small r; squared: 2 bar per component times the coefficient)
  bit equality per-point outputs against ops.mesh_closest on the fp64 points of ops.points_fwd; every output across leaf hints;
               two calls, whatever ran in between."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_reference as R
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
    """The reference scene on the device in one cloud dtype: PointSet, scan_ptr, poses12, the mesh's tree."""

    def __init__(self, dtype, lmask=None, seed=11, sizes=M.SIZES):
        from depth_correction_amd import ops
        self.mesh, self.scans, self.poses = M.scene(sizes=sizes, dtype=NP_DTYPES[dtype], seed=seed)
        if lmask is not None:
            off = 0
            for c in self.scans:
                c['lmask'] = lmask[off:off + len(c['depth'])]
                off += len(c['depth'])
        cat = lambda k: np.concatenate([c[k] for c in self.scans])
        self.ps = ops.PointSet(_t(cat('vps')), _t(cat('dirs')), _t(cat('depth')), _t(cat('inc')), _t(cat('lmask')))
        self.sizes = [len(c['depth']) for c in self.scans]
        self.n = sum(self.sizes)
        self.scan_ptr = _t(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64))
        self.poses12 = _t(self.poses[:, :3, :].reshape(-1, 12))
        self.bvh = self.mesh.on_device(DEV)[3]

    def model(self, kind):
        w, e = W_MODEL[kind]
        return (kind, None, None) if kind is None else (kind, _t(w, torch.float64), _t(e, torch.float64))

    def run(self, kind=None, w=None, e=None, **kw):
        from depth_correction_amd import ops
        out = ops.mesh_loss(self.bvh, self.ps, self.scan_ptr, self.poses12, kind, w, e, **kw)
        torch.cuda.synchronize()
        return out


def _scene(dtype, sizes=M.SIZES):
    if (dtype, sizes) not in _cache:
        _cache[dtype, sizes] = Scene(dtype, sizes=sizes)
    return _cache[dtype, sizes]


def _split(out, nt, ns):
    o = out.cpu().numpy()
    return dict(loss=o[0], used=o[1], gated=o[2], invalid=o[3], gw=o[4:4 + nt], ge=o[4 + nt:4 + 2 * nt],
                gT=o[4 + 2 * nt:].reshape(ns, 3, 4))


def _check_gradients(got, ref, squared, what, with_e):
    bounds = M.grad_bounds(ref, squared=squared)
    print('%s: loss %.12g (reference %.12g, |diff| %.3g, bar %.3g)' % (what, got['loss'], ref['loss'], abs(got['loss'] - ref['loss']), M.BAR))
    assert abs(got['loss'] - ref['loss']) <= M.BAR, (what, got['loss'], ref['loss'])
    assert (got['used'], got['gated'], got['invalid']) == (ref['used'], ref['gated'], ref['invalid']), what
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
    """dist_out against the brute force, face_out where the brute force decides clearly, and face / dist / closest bit-equal to
    ops.mesh_closest on the points ops.points_fwd gives for the same fields in fp64."""
    from depth_correction_amd import ops
    sc = _scene(dtype)
    kind, w, e = sc.model('ScaledPolynomial')
    out, face, dist, closest = sc.run(kind, w, e, want_points=True)
    ref = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, *W_MODEL[kind])
    bf_face, bf_dist, second = R.brute_force(sc.mesh.vertices, sc.mesh.faces, ref['x'])
    d = dist.cpu().numpy()
    print('%s: distances %.3g .. %.3g m, largest |dist - brute force| %.3g m (bar %.3g m)' % (dtype, bf_dist.min(), bf_dist.max(), np.abs(d - bf_dist).max(), M.BAR))
    assert np.abs(d - bf_dist).max() <= M.BAR
    clear = second - bf_dist > 1e-9 * M.EXTENT
    assert clear.mean() > 0.9
    assert np.array_equal(face.cpu().numpy()[clear], bf_face[clear])
    # the same fields in fp64 through the un-fused kernels
    f64 = lambda t: None if t is None else t.double().contiguous()
    sid = torch.repeat_interleave(torch.arange(len(sc.sizes), device=DEV), _t(np.array(sc.sizes))).to(torch.int32).contiguous()
    ps64 = ops.PointSet(f64(sc.ps.vps), f64(sc.ps.dirs), f64(sc.ps.depth), f64(sc.ps.inc), sc.ps.lmask, sid)
    x64 = ops.points_fwd(ps64, sc.poses12, kind, w, e)
    f2, d2, c2 = ops.mesh_closest(sc.bvh, x64)
    torch.cuda.synchronize()
    assert np.abs(x64.cpu().numpy() - ref['x']).max() <= M.BAR
    assert torch.equal(face, f2) and torch.equal(dist, d2) and torch.equal(closest, c2)
    assert int(out[1]) == sc.n and int(out[2]) == 0 and int(out[3]) == 0


# ---- 2. loss and gradients -------------------------------------------------------------------------------------------------------
CASES = {
    'none': dict(kind=None),
    'scaled_polynomial': dict(kind='ScaledPolynomial'),
    'scaled_polynomial_squared': dict(kind='ScaledPolynomial', squared=True),
    'polynomial': dict(kind='Polynomial'),
    'invcos': dict(kind='InvCos'),
    'exponent_grad': dict(kind='ScaledPolynomial', want_exponent=True),
    'exponent_grad_squared': dict(kind='Polynomial', want_exponent=True, squared=True),
    'local_mask': dict(kind='ScaledPolynomial', local_mask=True),
    'loss_mask': dict(kind='ScaledPolynomial', loss_mask=True),
    # 1025 points in scan 0: nine blocks on the finishing kernel's eight chains, so chain 0 adds two rows (float64 only)
    'nine_blocks': dict(kind='ScaledPolynomial', sizes=(1025, 0, 1)),
}


@pytest.mark.parametrize('case,dtype', [(c, d) for d in ('float32', 'float64') for c in sorted(CASES) if 'sizes' not in CASES[c]]
                         + [('nine_blocks', 'float64')])
def test_loss_and_gradients(dtype, case):
    """out against the closed form at the device's own faces: loss, the three counts, dL/dw, dL/de, dL/d[R|t] of every scan (the
    empty scan's is zero)."""
    cfg = dict(CASES[case])
    rng = np.random.default_rng(5)
    sizes = cfg.pop('sizes', M.SIZES)
    n = sum(sizes)
    sc = Scene(dtype, lmask=rng.random(n) < 0.7) if cfg.pop('local_mask', False) else _scene(dtype, sizes)
    loss_mask = rng.random(n) < 0.6 if cfg.pop('loss_mask', False) else None
    kind, w, e = sc.model(cfg.pop('kind'))
    squared, want_e = cfg.get('squared', False), cfg.get('want_exponent', False)
    out, face, dist, closest = sc.run(kind, w, e, want_points=True, mask=None if loss_mask is None else _t(loss_mask), **cfg)
    wv, ev = W_MODEL[kind]
    # the per-point outputs hold first (test 1's bars), then the closed form at these faces
    bf = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev, loss_mask=loss_mask, squared=squared)
    used = bf['mask']
    assert used[:sizes[0]].any() and used[-sizes[-1]:].any()           # the first and the last scan have used points
    assert np.abs(dist.cpu().numpy()[used] - bf['r'][used]).max() <= M.BAR
    assert (face.cpu().numpy()[~used] == -1).all()
    ref = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev, face=face.cpu().numpy(), loss_mask=loss_mask, squared=squared)
    nt = 0 if kind is None else len(wv)
    got = _split(out, nt, len(sc.sizes))
    _check_gradients(got, ref, squared, '%s %s' % (dtype, case), want_e)
    assert not got['gT'][sizes.index(0)].any()                         # the empty scan
    if case == 'local_mask':                                           # uncorrected points: no weight gradient of theirs
        lm = np.concatenate([c['lmask'] for c in sc.scans])
        assert not ref['terms']['gw'][~lm].any() and ref['terms']['gw'][lm].any()
    if loss_mask is not None:
        assert got['used'] == loss_mask.sum() < n


# ---- 3. hint invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_hint_never_changes_a_bit(dtype):
    sc = _scene(dtype)
    kind, w, e = sc.model('ScaledPolynomial')
    base = sc.run(kind, w, e, want_points=True, want_exponent=True)
    nf = sc.bvh.n_faces
    carried = torch.full((sc.n,), -1, dtype=torch.int32, device=DEV)
    first = sc.run(kind, w * 1.01, e, leaf_hint=carried, want_points=True, want_exponent=True)       # slightly different weights
    # the written-back hint is the winning leaf: its face is the face reported
    assert (carried >= 0).all() and torch.equal(sc.bvh.leaf_face[carried.long()], first[1])
    rng = np.random.default_rng(3)
    hints = {'carried': carried.clone(),
             'permuted': _t(rng.permutation(nf)[rng.integers(0, nf, size=sc.n)].astype(np.int32)),
             'garbage': _t(np.resize(np.array([-1, nf, 2 ** 31 - 1, -7, nf + 5], np.int32), sc.n))}
    for name, hint in hints.items():
        got = sc.run(kind, w, e, leaf_hint=hint, want_points=True, want_exponent=True)
        for a, b, what in zip(got, base, ('out', 'face', 'dist', 'closest')):
            assert torch.equal(a, b), (name, what)
        assert torch.equal(sc.bvh.leaf_face[hint.long()], base[1]), name       # every hint comes back as the winning leaf


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_whatever_ran_between():
    sc, other = _scene('float32'), Scene('float64', seed=23)
    kind, w, e = sc.model('ScaledPolynomial')
    a = sc.run(kind, w, e, want_points=True)
    b = sc.run(kind, w, e, want_points=True)
    other.run(*other.model('Polynomial'), squared=True)
    c = sc.run(kind, w, e, want_points=True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---- 5. gate and invalid points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_gate_and_invalid_points(dtype):
    from depth_correction_amd import ops
    sc = _scene(dtype)
    kind, w, e = sc.model('ScaledPolynomial')
    wv, ev = W_MODEL[kind]
    full = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev)
    md = float(np.median(full['r']))
    assert np.abs(full['r'] - md).min() > M.BAR                        # fixed seeds: no distance within the bar of the gate
    out, face, dist, closest = sc.run(kind, w, e, max_dist=md, want_points=True)
    ref = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev, max_dist=md)
    keep = ref['mask']
    assert 0 < keep.sum() < sc.n and np.array_equal(face.cpu().numpy() >= 0, keep)
    assert np.isinf(dist.cpu().numpy()[~keep]).all() and np.isnan(closest.cpu().numpy()[~keep]).all()
    ref = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev, face=np.where(keep, face.cpu().numpy(), 0), max_dist=md)
    got = _split(out, 2, len(sc.sizes))
    assert (got['used'], got['gated'], got['invalid']) == (keep.sum(), sc.n - keep.sum(), 0)
    _check_gradients(got, ref, False, '%s gated' % dtype, False)      # gated points contribute nothing
    # rows with a NaN / inf depth are counted invalid and contribute nothing
    depth = sc.ps.depth.clone()
    bad = [0, 5, 299, 300, 301, sc.n - 1]                              # (300: the one-point scan)
    depth[bad[0::2]] = float('nan')
    depth[bad[1::2]] = float('inf')
    ps = ops.PointSet(sc.ps.vps, sc.ps.dirs, depth, sc.ps.inc, sc.ps.lmask)
    out2, face2, _, _ = ops.mesh_loss(sc.bvh, ps, sc.scan_ptr, sc.poses12, kind, w, e, want_points=True)
    loss_mask = np.ones(sc.n, bool)
    loss_mask[bad] = False
    ref2 = M.mesh_loss(sc.mesh, sc.scans, sc.poses, kind, wv, ev, face=np.maximum(face2.cpu().numpy(), 0), loss_mask=loss_mask)
    got2 = _split(out2, 2, len(sc.sizes))
    assert (got2['used'], got2['gated'], got2['invalid']) == (sc.n - len(bad), 0, len(bad))
    assert (face2.cpu().numpy()[bad] == -1).all()
    ref2['invalid'] = len(bad)                                         # (the reference left them out through its mask)
    _check_gradients(got2, ref2, False, '%s invalid rows' % dtype, False)
    assert not got2['gT'][1].any()                                     # the one-point scan's only point is invalid
    # every point gated: NaN loss, zero gradients, no error
    hint = torch.zeros((sc.n,), dtype=torch.int32, device=DEV)
    out3 = sc.run(kind, w, e, max_dist=1e-9, leaf_hint=hint)
    o3 = out3.cpu().numpy()
    assert math.isnan(o3[0]) and o3[1] == 0 and o3[2] == sc.n and o3[3] == 0 and not o3[4:].any()
    assert (hint == -1).all()


def test_argument_contract():
    from depth_correction_amd import ops
    sc = _scene('float64')
    with pytest.raises(ValueError, match='NaN'):
        sc.run(max_dist=float('nan'))
    with pytest.raises(ValueError, match='scan_ptr'):
        ops.mesh_loss(sc.bvh, sc.ps, _t(np.array([0, 5, 3, sc.n], np.int64)), sc.poses12[:3].contiguous())
    # no points at all: NaN loss, zero counts and gradients; a sequence of empty scans is legal
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
    empty = ops.PointSet(None, z(0, 3), z(0), z(0))
    kind, w, e = sc.model('ScaledPolynomial')
    out = ops.mesh_loss(sc.bvh, empty, _t(np.zeros(3, np.int64)), sc.poses12[:2].contiguous(), kind, w, e).cpu().numpy()
    assert out.shape == (4 + 4 + 24,) and math.isnan(out[0]) and not out[1:].any()


# ---- 6. autograd surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_autograd_surface_against_unfused_composition(dtype):
    """loss.mesh_loss with a model and per-pose corrections requiring grad: w.grad and pose_deltas.grad of the fused call equal
    those of the un-fused torch composition (fused=False) within test 2's bounds -- the corrections' through the Jacobian of the
    corrected poses, |dT/ddelta| times the bound of dL/dT."""
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
    res = {}
    for fused in (True, False):
        model = ScaledPolynomial(w=list(wv), exponent=list(ev), device=DEV)
        deltas = _t(delta0, torch.float64).requires_grad_(True)       # (fp64 corrections: both forms see the same poses)
        poses_upd = create_corrected_poses([poses0.double()], [deltas], cfg)
        loss, loss_clouds = L.mesh_loss([clouds], poses_upd, model, masks=[(sc.mesh, None)], fused=fused)
        loss.backward()
        torch.cuda.synchronize()
        res[fused] = (loss.item(), model.w.grad.cpu().numpy().reshape(-1), deltas.grad.cpu().numpy(), poses_upd[0].detach().cpu().numpy())
        assert len(loss_clouds) == 1 and len(loss_clouds[0]) == sc.n
    ref = M.mesh_loss(sc.mesh, sc.scans, res[True][3], 'ScaledPolynomial', wv, ev)
    bounds = M.grad_bounds(ref)
    print('%s: fused %.12g, un-fused %.12g, closed form %.12g' % (dtype, res[True][0], res[False][0], ref['loss']))
    assert abs(res[True][0] - res[False][0]) <= M.BAR and abs(res[True][0] - ref['loss']) <= M.BAR
    assert (np.abs(res[True][1] - res[False][1]) <= bounds['gw']).all(), (res[True][1], res[False][1], bounds['gw'])
    assert (np.abs(res[True][1] - ref['gw']) <= bounds['gw']).all()
    # dL/ddelta_s[k] = sum_ab dL/dT_s[a,b] dT_s[a,b]/ddelta_s[k]
    d = _t(delta0, torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: create_corrected_poses([poses0.double()], [v], cfg)[0][:, :3, :], d)
    J = J.cpu().numpy()                                                # [S,3,4,S,6]
    S = len(clouds)
    bound_d = np.stack([(bounds['gT'][s][:, :, None] * np.abs(J[s, :, :, s, :])).sum(axis=(0, 1)) for s in range(S)])
    bound_d += 2.0 ** -40 * np.stack([(np.abs(ref['gT'][s])[:, :, None] * np.abs(J[s, :, :, s, :])).sum(axis=(0, 1)) for s in range(S)])
    want_d = np.stack([(ref['gT'][s][:, :, None] * J[s, :, :, s, :]).sum(axis=(0, 1)) for s in range(S)])
    err = np.abs(res[True][2] - res[False][2])
    print('%s: pose corrections, largest |fused - un-fused| %.3g (bound there %.3g)' % (dtype, err.max(), bound_d.reshape(-1)[err.argmax()]))
    assert (err <= bound_d).all(), (err, bound_d)
    assert (np.abs(res[True][2] - want_d) <= bound_d).all()
    assert not res[True][2][2].any() and np.abs(res[True][2]).max() > 0


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def _pose(yaw, t):
    T = np.eye(4)
    T[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


def _train_lines(cfg, train_datasets, capsys):
    from depth_correction_amd.train import train
    capsys.readouterr()
    best = train(cfg, train_datasets=train_datasets, val_datasets=[])
    out = capsys.readouterr().out
    losses = [float(m) for m in re.findall(r'^It\. \d+: train loss: (-?[0-9.]+|nan)', out, flags=re.M)]
    return best, losses


def test_train_end_to_end(tmp_path, capsys):
    """train() with cfg.loss = 'mesh_loss' on two rendered sequences of the room (3 poses x 16 x 64 rays each) biased by the scene's
    weights: the run completes and writes best.yaml, the training loss falls, and eval_loss with the trained model is below eval_loss
    with zero weights.  Then per-pose corrections from 1 cm of seeded pose noise: the loss falls.  (No magnitude is asserted.)"""
    from depth_correction_amd.config import Config, PoseCorrection
    from depth_correction_amd.dataset import DepthBiasDataset, NoisyPoseDataset, RenderedMeshDataset
    from depth_correction_amd.eval import eval_loss
    from depth_correction_amd.model import ScaledPolynomial
    path = tmp_path / 'room.ply'
    M.room().save_ply(str(path))
    mk = lambda d, **kw: Config(device=DEV, float_type='float64', min_depth=0.3, max_depth=25.0, grid_res=0.05, nn_k=0, nn_r=0.6,
                                loss='mesh_loss', n_opt_iters=30, lr=1e-3, log_dir=str(d),
                                model_kwargs={'w': [0.0, 0.0], 'exponent': list(M.E_TRUE)}).from_dict(kw)
    cfg = mk(tmp_path / 'model', pose_correction=PoseCorrection.none)
    gt = ScaledPolynomial(w=list(M.W_TRUE), exponent=list(M.E_TRUE), device=DEV)
    seqs = []
    for q in range(2):
        poses = np.stack([_pose(0.3 * i + q, (-2.0 + 1.2 * i, 0.4 * q - 0.5, 0.1 * i)) for i in range(3)])
        ds = RenderedMeshDataset(str(path), poses=poses, size=(16, 64), fov=(45.0, 360.0), num_segments=8, device=DEV)
        seqs.append(DepthBiasDataset(ds, gt, cfg=cfg))
    os.makedirs(cfg.log_dir)
    best, losses = _train_lines(cfg, seqs, capsys)
    report = ['model only: first %.9f, last %.9f' % (losses[0], losses[-1])]      # (printed at the end: _train_lines drains capsys)
    assert len(losses) == 30 and os.path.exists(os.path.join(cfg.log_dir, 'best.yaml')) and best is not None
    assert losses[-1] < losses[0]
    trained = ScaledPolynomial(w=[0.0, 0.0], exponent=list(M.E_TRUE), device=DEV)
    trained.load_state_dict(torch.load(best.model_state_dict))
    zero = ScaledPolynomial(w=[0.0, 0.0], exponent=list(M.E_TRUE), device=DEV)
    after, before = eval_loss(cfg, test_datasets=seqs, model=trained).item(), eval_loss(cfg, test_datasets=seqs, model=zero).item()
    report.append('eval_loss: zero weights %.9f, trained %.9f' % (before, after))
    assert after < before
    # per-pose corrections against noisy poses, on the plain loop
    cfg2 = mk(tmp_path / 'pose', pose_correction=PoseCorrection.pose, loop_batch=1)
    os.makedirs(cfg2.log_dir)
    noisy = [NoisyPoseDataset(ds, noise=0.01, mode='pose') for ds in seqs]
    _, losses2 = _train_lines(cfg2, noisy, capsys)
    print('\n'.join(report + ['model and poses: first %.9f, last %.9f' % (losses2[0], losses2[-1])]))
    assert len(losses2) == 30 and losses2[-1] < losses2[0]


def test_sharded_training_is_refused(monkeypatch, tmp_path):
    from depth_correction_amd import train as T
    from depth_correction_amd.config import Config
    monkeypatch.setattr(T, '_sharding', lambda cfg: (0, 2, True))
    with pytest.raises(NotImplementedError, match='mesh_loss'):
        T.train(Config(device=DEV, loss='mesh_loss', log_dir=str(tmp_path)), train_datasets=[], val_datasets=[])
