"""Loss landscape over the model weights (eval.landscape_clouds / eval_loss_landscape, dc_sequence_landscape) against a per-weight
loop of eval_loss_clouds, and the reference's eval_loss / eval_loss_all."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cfg(float_type='float64', radius=False, **kw):
    from depth_correction_amd.config import Config
    nn = dict(nn_k=0, nn_r=0.25) if radius else dict(nn_k=10, nn_r=0.0)
    base = dict(device=DEV, float_type=float_type, min_depth=1.0, max_depth=25.0, grid_res=0.1, **nn)
    base.update(kw)
    return Config(**base)


def _datasets(name):
    from depth_correction_amd.dataset import KittiLikeDataset, RoomBoxDataset
    if name == 'room':
        return [RoomBoxDataset(n_pts=20000, n_poses=3)]
    return [KittiLikeDataset(n_poses=3, n_rings=32, n_azimuth=512)]


def _setup(cfg, name='room'):
    from depth_correction_amd.eval import _load_test_sequences
    from depth_correction_amd.preproc import establish_neighborhoods
    clouds, poses = _load_test_sequences(cfg, _datasets(name))
    ns = [establish_neighborhoods(clouds=c, poses=p, cfg=cfg) for c, p in zip(clouds, poses)]
    return clouds, poses, ns


def _model(P):
    from depth_correction_amd.model import ScaledPolynomial
    if P == 1:
        return ScaledPolynomial(w=[0.0], exponent=[4.0], device=DEV)
    return ScaledPolynomial(w=[0.0, 0.0], exponent=[2.0, 4.0], device=DEV)


def _weights(P):
    if P == 1:
        return torch.linspace(-0.01, 0.01, 21, dtype=torch.float64)
    g = torch.linspace(-0.004, 0.004, 5, dtype=torch.float64)
    return torch.stack(torch.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)


def _loop(clouds, poses, deltas, masks, ns, model, weights, cfg, plane=False, with_max=False):
    from depth_correction_amd.eval import _model_with_weights, eval_loss_clouds
    from depth_correction_amd.loss import create_loss
    loss_fun = create_loss(cfg)
    w = weights.reshape(weights.shape[0], -1)
    out, cnt, lmax = [], [], []
    with torch.no_grad():
        for row in w:
            loss, views, _, _ = eval_loss_clouds(clouds, poses, deltas, list(masks), ns, _model_with_weights(model, row), loss_fun, cfg)
            out.append(float(loss))
            cnt.append(float(sum(len(v.loss) if plane else float(v.count) for v in views)))
            if not plane:          # the largest pointwise loss that counts (bounds what one point on an eigenvalue bound moves)
                ls = [v.loss[v.mask] if v.mask is not None else v.loss for v in views]
                lmax.append(max((float(l.max()) if l.numel() else 0.0) for l in ls))
    if with_max:
        return np.array(out), np.array(cnt), np.array(lmax)
    return np.array(out), np.array(cnt)


def _fixed_deltas(poses, cfg):
    """Non-zero, fixed pose corrections (PoseCorrection.pose)."""
    g = torch.Generator().manual_seed(5)
    return [(1e-3 * torch.randn((len(p), 6), generator=g, dtype=torch.float64)).to(device=DEV, dtype=p.dtype) for p in poses]


def _given_masks(clouds, poses, ns, cfg):
    from depth_correction_amd.preproc import compute_neighborhood_features, global_cloud, global_cloud_mask
    out = []
    for c, p, nn in zip(clouds, poses, ns):
        g = compute_neighborhood_features(cloud=global_cloud(clouds=c, model=None, poses=p), neighborhoods=nn, cfg=cfg)
        out.append(global_cloud_mask(g, g.mask, cfg))
    return out


def _check(cfg, clouds, poses, deltas, masks, ns, P):
    from depth_correction_amd.eval import landscape_clouds, landscape_paths
    model, weights = _model(P), _weights(P)
    before = landscape_paths['kernel']
    loss, count = landscape_clouds(clouds, poses, deltas, masks, ns, model, weights, cfg)
    assert landscape_paths['kernel'] == before + 1
    ref, ref_cnt, lmax = _loop(clouds, poses, deltas, masks, ns, model, weights, cfg, with_max=True)
    loss, count = loss.cpu().numpy(), count.cpu().numpy()
    rel = np.abs(loss - ref) / np.abs(ref)
    if cfg.float_type == 'float64':
        assert rel.max() < 1e-9, (rel.max(), loss, ref)
        assert np.array_equal(count, ref_cnt), (count, ref_cnt)
    else:
        # float32: the loop decides the eigenvalue bounds on float32 eigenvalues of float32 points, the kernel on fp64 moments, so a
        # point that sits on a bound can fall on either side (masks of None only).  Rows with equal counts hold the 1e-5 bar; a row
        # whose count differs moves its sum by at most the flipped points' losses (observed maxima printed with -s)
        dcnt = np.abs(count - ref_cnt)
        same = dcnt == 0
        print('float32 landscape: max rel loss %.3g over %d equal-count rows, max rel count %.3g'
              % (rel[same].max() if same.any() else 0.0, same.sum(), (dcnt / ref_cnt).max()))
        assert rel[same].max() < 1e-5 if same.any() else True, (rel, loss, ref)
        assert (dcnt / ref_cnt).max() <= 1e-4, (count, ref_cnt)
        if masks[0] is not None:
            assert same.all(), (count, ref_cnt)
        dsum = np.abs(loss * count - ref * ref_cnt)
        assert (dsum <= dcnt * lmax + 1e-5 * np.abs(ref * ref_cnt)).all(), (dsum, dcnt, lmax)
    return loss


@pytest.mark.parametrize('float_type', ['float64', 'float32'])
@pytest.mark.parametrize('radius', [False, True])
@pytest.mark.parametrize('loss,kw', [('min_eigval_loss', dict(normalization=True, sqrt=False)),
                                     ('min_eigval_loss', dict(normalization=False, sqrt=True)),
                                     ('trace_loss', dict(normalization=False, sqrt=False))])
@pytest.mark.parametrize('given_masks', [False, True])
@pytest.mark.parametrize('dataset', ['room', 'kitti'])
def test_ball_landscape_matches_loop(float_type, radius, loss, kw, given_masks, dataset):
    cfg = _cfg(float_type, radius, loss=loss)
    cfg.loss_kwargs = dict(cfg.loss_kwargs, **kw)
    clouds, poses, ns = _setup(cfg, dataset)
    masks = _given_masks(clouds, poses, ns, cfg) if given_masks else [None] * len(clouds)
    for P in (1, 2):
        _check(cfg, clouds, poses, [None] * len(clouds), masks, ns, P)


@pytest.mark.parametrize('float_type', ['float64', 'float32'])
def test_ball_landscape_with_pose_corrections(float_type):
    from depth_correction_amd.config import PoseCorrection
    cfg = _cfg(float_type, pose_correction=PoseCorrection.pose)
    clouds, poses, ns = _setup(cfg, 'room')
    deltas = _fixed_deltas(poses, cfg)
    for P in (1, 2):
        _check(cfg, clouds, poses, deltas, [None], ns, P)


def test_landscape_deterministic_and_edges():
    from depth_correction_amd.eval import eval_loss_clouds, landscape_clouds
    from depth_correction_amd.loss import create_loss
    cfg = _cfg('float32')
    clouds, poses, ns = _setup(cfg, 'room')
    model, weights = _model(2), _weights(2)
    a = landscape_clouds(clouds, poses, [None], [None], ns, model, weights, cfg)
    b = landscape_clouds(clouds, poses, [None], [None], ns, model, weights, cfg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # W = 1 equals eval_loss_clouds
    m1 = _model(1)
    with torch.no_grad():
        ref, *_ = eval_loss_clouds(clouds, poses, [None], [None], ns, m1, create_loss(cfg), cfg)
    one, _ = landscape_clouds(clouds, poses, [None], [None], ns, m1, torch.zeros((1,), dtype=torch.float64), cfg)
    assert abs(one.item() - ref.item()) <= 1e-5 * abs(ref.item())
    # W = 4096 in chunks: the same values as the rows computed alone
    big = torch.linspace(-0.02, 0.02, 4096, dtype=torch.float64)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lb, cb = landscape_clouds(clouds, poses, [None], [None], ns, m1, big, cfg)
    assert torch.cuda.max_memory_allocated() - base < 256 * 2 ** 20
    assert lb.shape == (4096,) and torch.isfinite(lb).all()
    sel = [0, 127, 128, 2047, 4095]
    ls, _ = landscape_clouds(clouds, poses, [None], [None], ns, m1, big[sel], cfg)
    assert torch.equal(ls, lb[sel])
    # an all-false mask: nan, like the loop
    empty = [torch.zeros((sum(len(c) for c in clouds[0]),), dtype=torch.bool, device=DEV)]
    le, ce = landscape_clouds(clouds, poses, [None], empty, ns, m1, big[:3], cfg)
    assert torch.isnan(le).all() and (ce == 0).all()
    ref_e, _ = _loop(clouds, poses, [None], empty, ns, m1, big[:3], cfg)
    assert np.isnan(ref_e).all()
    with pytest.raises(ValueError):
        landscape_clouds(clouds, poses, [None], [None], ns, model, torch.zeros((4,), dtype=torch.float64), cfg)


def _no_kernel_model():
    from depth_correction_amd.model import ScaledPolynomial

    class NoKernel(ScaledPolynomial):
        kernel_kind = None
    return NoKernel(w=[0.0], exponent=[4.0], device=DEV)


@pytest.mark.parametrize('case', ['inlier_ratio', 'inlier_max_loss', 'skip_nans', 'nn_scale', 'vp_dispersion_to_depth2', 'linear',
                                  'no_kernel_kind', 'icp'])
def test_landscape_fallbacks_equal_loop(case):
    from depth_correction_amd.eval import _model_with_weights, eval_loss_clouds, landscape_clouds, landscape_paths
    from depth_correction_amd.loss import create_loss
    from depth_correction_amd.model import Linear
    cfg = _cfg('float64')
    model, weights = _model(1), _weights(1)[::5]
    if case == 'inlier_ratio':
        cfg.loss_kwargs = dict(cfg.loss_kwargs, inlier_ratio=0.5)
    elif case == 'inlier_max_loss':
        cfg.loss_kwargs = dict(cfg.loss_kwargs, inlier_max_loss=0.05)
    elif case == 'skip_nans':
        cfg.loss_kwargs = dict(cfg.loss_kwargs, skip_nans=True)
    elif case == 'nn_scale':
        cfg.nn_scale = 0.5
    elif case == 'vp_dispersion_to_depth2':
        cfg.vp_dispersion_to_depth2_bounds = [0.0, 1.0]
    elif case == 'linear':
        model = Linear(device=DEV)
        weights = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.01, 0.0], [0.99, 0.0, 0.01]], dtype=torch.float64)
    elif case == 'no_kernel_kind':
        model = _no_kernel_model()
        base = torch.cat([p.detach().reshape(-1).double().cpu() for p in model.parameters()])
        weights = base.repeat(3, 1)
        weights[1, 0] += 0.005
        weights[2, 0] -= 0.005
    elif case == 'icp':
        cfg.loss = 'icp_loss'
    clouds, poses, ns = _setup(cfg, 'room')
    masks = [None]
    if case == 'icp':
        from depth_correction_amd.train import _icp_masks
        masks = _icp_masks(clouds, poses, cfg.loss_kwargs['icp_inlier_ratio'])
    before = dict(landscape_paths)
    loss, count = landscape_clouds(clouds, poses, [None], masks, ns, model, weights, cfg)
    assert landscape_paths['loop'] == before.get('loop', 0) + 1 and landscape_paths['kernel'] == before.get('kernel', 0)
    with torch.no_grad():
        for j, row in enumerate(weights.reshape(weights.shape[0], -1)):
            ref, views, *_ = eval_loss_clouds(clouds, poses, [None], list(masks), ns, _model_with_weights(model, row), create_loss(cfg), cfg)
            assert float(loss[j]) == float(ref) or (np.isnan(float(ref)) and np.isnan(float(loss[j])))
    # the count behind every mean (the ICP loss is a mean over scan pairs, not points: nan)
    if case == 'icp':
        assert torch.isnan(count).all()
    else:
        assert torch.isfinite(count).all() and (count > 0).all(), count


def test_landscape_loss_offset_fails_like_the_loop():
    """loss_offset takes the loop, so an evaluation eval_loss_clouds cannot do fails in the same way."""
    from depth_correction_amd.eval import eval_loss_clouds, landscape_clouds
    from depth_correction_amd.loss import create_loss
    cfg = _cfg('float64', loss_offset=True)
    clouds, poses, ns = _setup(cfg, 'room')
    model = _model(1)
    with pytest.raises(Exception) as loop_err, torch.no_grad():
        eval_loss_clouds(clouds, poses, [None], [None], ns, model, create_loss(cfg), cfg)
    with pytest.raises(type(loop_err.value)):
        landscape_clouds(clouds, poses, [None], [None], ns, model, _weights(1)[:2], cfg)


def test_plane_landscape_argmin():
    """The loss-landscape experiment on the room with plane neighbourhoods: a +0.004 bias, the minimum within one step of -0.004,
    through the plane kernel, every row equal to eval_loss_clouds."""
    from test_gpu_planes import _plane_cfg, _room_global
    from depth_correction_amd.eval import landscape_clouds, landscape_paths
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.preproc import establish_neighborhoods
    clouds, poses, g, _ = _room_global(bias=0.004)
    cfg = _plane_cfg(loss='min_eigval_loss')
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    ws = np.linspace(-0.01, 0.01, 21)
    model = ScaledPolynomial(w=[0.0], exponent=[4.0], device=DEV)
    before = landscape_paths['kernel']
    loss, count = landscape_clouds([clouds], [poses], [None], [None], [planes], model, torch.as_tensor(ws), cfg)
    assert landscape_paths['kernel'] == before + 1
    loss = loss.cpu().numpy()
    assert abs(ws[int(np.argmin(loss))] + 0.004) <= 0.001 + 1e-12, list(zip(ws, loss))
    assert (count.cpu().numpy() == len(planes)).all()
    ref, ref_cnt = _loop([clouds], [poses], [None], [None], [planes], model, torch.as_tensor(ws), cfg, plane=True)
    rel = np.abs(loss - ref) / np.abs(ref)
    print('plane landscape: max rel loss %.3g' % rel.max())
    assert rel.max() < 1e-9, (rel.max(), loss, ref)
    assert np.array_equal(count.cpu().numpy(), ref_cnt)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('loss,kw', [('min_eigval_loss', dict(normalization=True, sqrt=False)),
                                     ('min_eigval_loss', dict(normalization=False, sqrt=True)),
                                     ('trace_loss', dict(sqrt=False))])
@pytest.mark.parametrize('P', [1, 2])
def test_plane_landscape_matches_loop(dtype, loss, kw, P):
    from test_gpu_planes import _plane_cfg, _room_global
    from depth_correction_amd.eval import landscape_clouds, landscape_paths
    from depth_correction_amd.model import Polynomial, ScaledPolynomial
    from depth_correction_amd.preproc import establish_neighborhoods
    clouds, poses, g, _ = _room_global(bias=0.004, dtype=dtype)
    cfg = _plane_cfg(loss=loss, float_type='float64' if dtype == np.float64 else 'float32')
    cfg.loss_kwargs = dict(cfg.loss_kwargs, **kw)
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    model = (ScaledPolynomial if P == 1 else Polynomial)(w=[0.0] * P, exponent=[4.0] if P == 1 else [2.0, 4.0], device=DEV)
    weights = _weights(P) * (1.0 if P == 1 else 0.01)
    mask = torch.ones((len(planes),), dtype=torch.bool, device=DEV)
    mask[1] = False
    for masks in ([None], [mask]):
        before = landscape_paths['kernel']
        out, count = landscape_clouds([clouds], [poses], [None], masks, [planes], model, weights, cfg)
        assert landscape_paths['kernel'] == before + 1
        ref, ref_cnt = _loop([clouds], [poses], [None], masks, [planes], model, weights, cfg, plane=True)
        rel = np.abs(out.cpu().numpy() - ref) / np.abs(ref)
        print('plane landscape %s: max rel loss %.3g' % (np.dtype(dtype).name, rel.max()))
        assert rel.max() < (1e-9 if dtype == np.float64 else 1e-5), (rel.max(), out, ref)
        assert np.array_equal(count.cpu().numpy(), ref_cnt)


def test_eval_loss_from_config(tmp_path):
    from depth_correction_amd.eval import _load_test_sequences, eval_loss, eval_loss_clouds, eval_loss_landscape
    from depth_correction_amd.loss import create_loss
    from depth_correction_amd.model import load_model
    from depth_correction_amd.preproc import establish_neighborhoods
    csv = tmp_path / 'eval.csv'
    cfg = _cfg('float64', test_names=['plane'], loss_eval_csv=str(csv), min_depth=0.5, model_class='ScaledPolynomial',
               model_kwargs={'w': [0.002], 'exponent': [4.0]})
    loss, ns = eval_loss(cfg, return_neighborhood=True)
    again = eval_loss(cfg, test_ns=ns)
    assert float(loss) == float(again)
    from depth_correction_amd.dataset import create_dataset
    clouds, poses = _load_test_sequences(cfg, [create_dataset('plane', cfg)])
    ns2 = [establish_neighborhoods(clouds=clouds[0], poses=poses[0], cfg=cfg)]
    with torch.no_grad():
        ref, *_ = eval_loss_clouds(clouds, poses, [None], [None], ns2, load_model(cfg=cfg), create_loss(cfg), cfg)
    assert float(loss) == float(ref)
    lines = csv.read_text().splitlines()
    assert lines == ['plane %.9f' % float(loss)] * 2
    ls, _ = eval_loss_landscape(cfg, torch.tensor([0.002, 0.0], dtype=torch.float64), test_ns=ns)
    assert abs(ls[0].item() - float(loss)) <= 1e-9 * abs(float(loss))


def test_eval_loss_plane_config_runs():
    from depth_correction_amd.config import NeighborhoodType
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.eval import eval_loss
    cfg = _cfg('float64', nn_type=NeighborhoodType.plane, ransac_dist_thresh=0.03, min_valid_neighbors=250, max_neighborhoods=6,
               grid_res=0.2, min_depth=0.0, max_depth=float('inf'))
    loss = eval_loss(cfg, test_datasets=[RoomBoxDataset(n_pts=20000, n_poses=3)])
    assert torch.isfinite(torch.as_tensor(loss))


def test_eval_loss_all_writes_one_file_per_loss_and_subset(tmp_path):
    from depth_correction_amd.eval import eval_loss_all
    cfg = _cfg('float64', train_names=['plane'], test_names=['plane'], log_dir=str(tmp_path), min_depth=0.5,
               eval_losses=['min_eigval_loss', 'trace_loss'])
    eval_loss_all(cfg)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ['loss_eval_min_eigval_loss_test.csv', 'loss_eval_min_eigval_loss_train.csv',
                     'loss_eval_trace_loss_test.csv', 'loss_eval_trace_loss_train.csv']
    for p in tmp_path.iterdir():
        name, value = p.read_text().split()
        assert name == 'plane' and np.isfinite(float(value))
