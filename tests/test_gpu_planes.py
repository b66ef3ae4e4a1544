"""Plane neighbourhoods on the GPU: RANSAC and DBSCAN against numpy / scipy restatements, the room's six walls, the plane
features, losses and gradients against a float64 torch restatement of preproc.py:218-243, and the loss-landscape / train()
end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _two_planes(n=20000, seed=7):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-5, 5, size=(n // 2, 2))
    p1 = np.stack([a[:, 0], a[:, 1], 0.01 * rng.normal(size=len(a))], 1)                 # z = 0
    b = rng.uniform(-3, 3, size=(n // 3, 2))
    p2 = np.stack([2.0 + 0.01 * rng.normal(size=len(b)), b[:, 0], 1.5 + b[:, 1]], 1)      # x = 2
    c = rng.uniform(-5, 5, size=(n - len(p1) - len(p2), 3))
    return np.concatenate([p1, p2, c])


def _np_plane(p0, p1, p2):
    u, v = p1 - p0, p2 - p0
    c = np.cross(u, v)
    nc = np.sqrt(c @ c)
    if not nc > 1e-12 * np.sqrt(u @ u) * np.sqrt(v @ v):
        return None
    n = c / nc
    return n, -(n @ p0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_ransac_round_matches_numpy(dtype):
    from depth_correction_amd import segmentation as S
    x = torch.tensor(_two_planes(), dtype=dtype, device=DEV)
    xd = x.double().cpu().numpy()
    n, H, thr, seed = len(xd), 200, 0.03, 135
    rem = torch.arange(n, dtype=torch.int32, device=DEV)
    bufs = dict(hyp=torch.empty((H, 4), dtype=torch.float64, device=DEV), anchor=torch.empty((H, 3), dtype=torch.float64, device=DEV),
                valid=torch.empty((H,), dtype=torch.int32, device=DEV), counts=torch.empty((H,), dtype=torch.int32, device=DEV),
                best=torch.empty((2,), dtype=torch.int32, device=DEV))
    h_gpu, c_gpu = S._ransac_round(x, rem, seed, 0, H, thr, bufs)
    counts = bufs['counts'].cpu().numpy()
    want = np.full(H, -1)
    for h in range(H):
        j = S.ransac_sample(seed, 0, h, n)
        pl = _np_plane(*xd[list(j)]) if len(set(j)) == 3 else None
        if pl is None:
            continue
        r = np.abs(xd @ pl[0] + pl[1])
        want[h] = int((r <= thr).sum())
        border = int((np.abs(r - thr) < 1e-12).sum())
        assert border <= 1e-3 * n, (h, border)                    # at most 0.1 % of the points may lie on the border at all
        assert abs(int(counts[h]) - want[h]) <= border, (h, counts[h], want[h])
    assert h_gpu == int(np.argmax(want)) and c_gpu == want.max()
    # refit: least-squares plane of the inliers, largest component positive, inliers selected again
    params, mask = S._refit(x, rem, thr, bufs)
    j = S.ransac_sample(seed, 0, h_gpu, n)
    n0, d0 = _np_plane(*xd[list(j)])
    inl = xd[np.abs(xd @ n0 + d0) <= thr]
    cen = inl.mean(0)
    _, V = np.linalg.eigh(np.cov((inl - cen).T))
    nn = V[:, 0] * np.sign(V[np.argmax(np.abs(V[:, 0])), 0])
    ref = np.concatenate([nn, [-(nn @ cen)]])
    np.testing.assert_allclose(params.cpu().numpy(), ref, rtol=0, atol=1e-10)
    r = np.abs(xd @ ref[:3] + ref[3])
    sel = mask.cpu().numpy().astype(bool)
    diff = sel != (r <= thr)
    assert diff.sum() <= 1e-3 * n and (not diff.any() or np.all(np.abs(r[diff] - thr) < 1e-12))


def test_dbscan_matches_ckdtree():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    from depth_correction_amd.segmentation import dbscan
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(0, 2, size=(1500, 2)), np.zeros((1500, 1))], 1)
    b = np.concatenate([rng.uniform(4, 5, size=(600, 2)), np.zeros((600, 1))], 1)
    noise = np.concatenate([rng.uniform(-3, 8, size=(200, 2)), np.zeros((200, 1))], 1)
    x = np.concatenate([a, b, noise])
    eps = 0.12
    labels, lbl, size = dbscan(torch.tensor(x, device=DEV), eps)
    nb = cKDTree(x).query_ball_point(x, eps)
    core = np.array([len(r) >= 10 for r in nb])
    rows, cols = [], []
    for i, r in enumerate(nb):
        if core[i]:
            for j in r:
                if core[j]:
                    rows.append(i)
                    cols.append(j)
    _, comp = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(len(x), len(x))), directed=False)
    first = {}
    for i in range(len(x)):
        if core[i] and comp[i] not in first:
            first[comp[i]] = i
    want = np.full(len(x), -1)
    for i in range(len(x)):
        if core[i]:
            want[i] = first[comp[i]]
        else:
            ls = [first[comp[j]] for j in nb[i] if core[j]]
            want[i] = min(ls) if ls else -1
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    u, c = np.unique(want[want >= 0], return_counts=True)
    k = np.flatnonzero(c == c.max())[0]
    assert (lbl, size) == (int(u[k]), int(c[k]))


def _room_global(n_pts=20000, n_poses=4, bias=None, dtype=np.float64):
    """Grid-filtered global cloud of the room (and its local clouds / poses); ``bias``: ScaledPolynomial weight of a depth
    bias d (1 - bias gamma^4) applied with the true wall normals."""
    from depth_correction_amd.dataset import RoomBoxDataset, _structured
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.filters import filter_grid
    from depth_correction_amd.preproc import global_cloud
    ds = RoomBoxDataset(n_pts=n_pts, n_poses=n_poses)
    clouds, poses, raw = [], [], []
    for s in range(n_poses):
        arr, pose = ds[s]
        xyz = np.stack([arr[f] for f in 'xyz'], 1).astype(np.float64)
        if bias is not None:
            g = xyz + pose[:3, 3]
            axis = np.argmax(np.abs(g) / ds.half, axis=1)
            r = np.linalg.norm(xyz, axis=1, keepdims=True)
            cosg = np.abs(xyz[np.arange(len(xyz)), axis]) / r[:, 0]
            gam = np.arccos(np.clip(cosg, 0, 1))
            xyz = xyz * (1.0 - bias * gam ** 4)[:, None]
        arr = _structured(xyz.astype(dtype))
        c = DepthCloud.from_structured_array(arr, dtype=dtype, device=DEV)
        c = filter_grid(c, grid_res=0.2, keep='random', rng=np.random.default_rng(s))
        raw.append((arr, pose))
        clouds.append(c)
        poses.append(pose)
    poses = torch.as_tensor(np.stack(poses).astype(dtype), device=DEV)
    return clouds, poses, global_cloud(clouds=clouds, poses=poses), raw


def _plane_cfg(**kw):
    from depth_correction_amd.config import Config, NeighborhoodType
    base = dict(nn_type=NeighborhoodType.plane, ransac_dist_thresh=0.03, min_valid_neighbors=250, max_neighborhoods=6, grid_res=0.2,
                num_ransac_iters=500, device=DEV)
    base.update(kw)
    return Config(**base)


def test_room_six_walls_deterministic():
    from depth_correction_amd.preproc import establish_neighborhoods
    _, _, g, _ = _room_global()
    cfg = _plane_cfg()
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    planes2 = establish_neighborhoods(cloud=g, cfg=cfg)
    assert len(planes) == 6
    assert torch.equal(planes.params, planes2.params)
    assert all(torch.equal(a, b) for a, b in zip(planes.indices, planes2.indices))
    half = np.array([10.0, 7.0, 2.0])
    walls = [(k, s) for k in range(3) for s in (-1.0, 1.0)]
    x = g.to_points().detach().double().cpu().numpy()
    seen = set()
    for p, idx in zip(planes.params.cpu().numpy(), planes.indices):
        n, d = p[:3], p[3]
        k = int(np.argmax(np.abs(n)))
        assert abs(n[k]) > 0.9999
        s = -np.sign(d / n[k])
        assert abs(abs(d) - half[k]) < 0.01, (p, half[k])
        seen.add((k, s))
        # every point near the wall (within 1 cm of it) and more than 5 cm from its edges is in this plane
        others = [a for a in range(3) if a != k]
        near = (np.abs(x[:, k] - s * half[k]) <= 0.01)
        for a in others:
            near &= np.abs(x[:, a]) < half[a] - 0.05
        got = np.zeros(len(x), dtype=bool)
        got[idx.cpu().numpy()] = True
        miss = near & ~got
        # (the far ends of the floor and ceiling are seen at grazing angles from every view point: a few sparse points there are
        #  DBSCAN noise, not members of the largest cluster -- at most 0.5 %)
        assert miss.sum() <= 0.005 * near.sum(), (int(miss.sum()), int(near.sum()), p, x[miss][:5])
    assert seen == set(walls)


def _ref_loss(raw, poses, deltas, params, indices, w, e, kind, loss, sqrt, normalization):
    """float64 torch on the CPU: global cloud with corrected poses, preproc.py:218-243, loss.py:216-294."""
    from depth_correction_amd.transform import corrected_poses
    # float32 clouds: the corrected poses and the global cloud are held in float32 on the device; the restatement rounds the
    # same values (with an identity gradient) so that both sides differentiate the same numbers
    r32 = (lambda v: v + (v.float().double() - v).detach()) if raw[0].dirs.dtype == torch.float32 else (lambda v: v)
    P = r32(corrected_poses(poses, deltas)) if deltas is not None else poses
    vps, dirs, depth = [], [], []
    for c, T in zip(raw, P):
        d0 = c.dirs.detach().double().cpu()
        dirs.append(r32(d0 @ T[:3, :3].t()))
        vps.append(T[:3, 3].expand(len(d0), 3))
        depth.append(c.depth.detach().double().cpu().reshape(-1, 1))
    vps, dirs, depth = torch.cat(vps), torch.cat(dirs), torch.cat(depth)
    covs = []
    for p, idx in zip(params, indices):
        idx = torch.as_tensor(idx).long()
        dd, vv, rr = dirs[idx], vps[idx], depth[idx]
        inc = torch.arccos((dd @ p[:3]).abs().clamp(max=1.0)).unsqueeze(-1)
        b = torch.pow(inc, e) @ w.t()
        if kind == 'ScaledPolynomial':
            rr = rr * (1.0 - b)
        elif kind == 'Polynomial':
            rr = rr - b
        xx = vv + rr * dd
        covs.append(torch.cov(xx.t(), correction=1))
    cov = torch.stack(covs)
    lam = torch.linalg.eigh(cov)[0]
    if loss == 'min_eigval_loss':
        l = lam[:, 0] / lam.sum(-1).clamp(min=1e-6) if normalization else lam[:, 0]
    else:
        l = cov.diagonal(dim1=-2, dim2=-1).sum(-1)
    l = torch.relu(l)
    if sqrt:
        l = torch.sqrt(l)
    return l.mean(), cov, lam


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kind', ['ScaledPolynomial', 'Polynomial', 'tensor'])
@pytest.mark.parametrize('loss,sqrt,normalization', [('min_eigval_loss', False, False), ('min_eigval_loss', True, True),
                                                     ('trace_loss', False, False), ('trace_loss', True, False)])
def test_plane_features_loss_and_gradients(dtype, kind, loss, sqrt, normalization):
    from depth_correction_amd import model as M
    from depth_correction_amd.config import PoseCorrection
    from depth_correction_amd.eval import create_corrected_poses
    from depth_correction_amd.loss import min_eigval_loss, trace_loss
    from depth_correction_amd.preproc import compute_neighborhood_features, establish_neighborhoods, global_cloud
    clouds, poses, g, raw = _room_global(n_pts=8000, dtype=dtype)
    cfg = _plane_cfg(pose_correction=PoseCorrection.sequence, float_type='float64' if dtype == np.float64 else 'float32')
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    assert len(planes) >= 4
    w0, e0 = [[2e-3, -1e-3]], [[2.0, 4.0]]
    if kind == 'tensor':
        class Tensor(M.ScaledPolynomial):
            kernel_kind = None
        model, rkind = Tensor(w=w0[0], exponent=e0[0], device=DEV), 'ScaledPolynomial'
    else:
        model, rkind = getattr(M, kind)(w=w0[0], exponent=e0[0], device=DEV), kind
    deltas = torch.tensor([[1e-3, -2e-3, 1e-3, 1e-3, 2e-3, -1e-3]], dtype=poses.dtype, device=DEV, requires_grad=True)
    P = create_corrected_poses([poses], [deltas], cfg)[0]
    gc = global_cloud(clouds=clouds, poses=P)
    feat = compute_neighborhood_features(cloud=gc, model=model, neighborhoods=planes, cfg=cfg)
    fun = min_eigval_loss if loss == 'min_eigval_loss' else trace_loss
    kw = dict(sqrt=sqrt, normalization=normalization) if loss == 'min_eigval_loss' else dict(sqrt=sqrt)
    val, _ = fun([feat], **kw)
    val.backward()
    wr = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    dr = torch.tensor(deltas.detach().cpu().numpy().astype(np.float64), requires_grad=True)
    pr = torch.tensor(poses.cpu().numpy().astype(np.float64))
    ref, cov_r, lam_r = _ref_loss(clouds, pr, dr, planes.params.cpu(), [i.cpu() for i in planes.indices], wr,
                                  torch.tensor(e0, dtype=torch.float64), rkind, loss, sqrt, normalization)
    ref.backward()
    tol = 1e-9 if dtype == np.float64 else 1e-5
    cs = cov_r.abs().max().item()
    assert (feat.cov.double().cpu() - cov_r).abs().max().item() <= tol * cs
    assert (feat.eigvals.double().cpu() - lam_r).abs().max().item() <= tol * lam_r.abs().max().item()
    assert abs(val.item() - ref.item()) <= tol * abs(ref.item())
    gw, gwr = model.w.grad.double().cpu(), wr.grad
    assert (gw - gwr).abs().max().item() <= tol * gwr.abs().max().item() + 1e-300, (gw, gwr)
    gd, gdr = deltas.grad.double().cpu(), dr.grad
    # (float32 trace loss: the trace is nearly invariant under the pose, so dL/d pose is a small remainder of large cancelling terms
    #  and inherits the float32 rounding of the global cloud at 1.5e-5 of its size: the bar is 3e-5 there)
    ptol = 3e-5 if (dtype == np.float32 and loss == 'trace_loss') else tol
    assert (gd - gdr).abs().max().item() <= ptol * gdr.abs().max().item(), (gd, gdr)


def test_loss_landscape_argmin():
    """The reference's loss-landscape experiment (loss_landscape.py): a ScaledPolynomial depth bias w = 0.004 on the room, then
    the correction weight swept over [-0.01, 0.01]: the loss is smallest within one step of -0.004."""
    from depth_correction_amd.eval import eval_loss_clouds
    from depth_correction_amd.loss import create_loss
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.preproc import establish_neighborhoods
    clouds, poses, g, raw = _room_global(bias=0.004)
    cfg = _plane_cfg(loss='min_eigval_loss')
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    local = clouds
    loss_fun = create_loss(cfg)
    ws = np.linspace(-0.01, 0.01, 21)
    vals = []
    with torch.no_grad():
        for w in ws:
            model = ScaledPolynomial(w=[float(w)], exponent=[4.0], device=DEV)
            loss, *_ = eval_loss_clouds([local], [poses], [None], [None], [planes], model, loss_fun, cfg)
            vals.append(loss.item())
    assert abs(ws[int(np.argmin(vals))] + 0.004) <= 0.001 + 1e-12, list(zip(ws, vals))


def test_train_plane_loss_decreases(tmp_path):
    from depth_correction_amd.train import train
    _, _, _, raw = _room_global(bias=0.004)
    cfg = _plane_cfg(loss='min_eigval_loss', n_opt_iters=20, lr=2e-4, log_dir=str(tmp_path), model_class='ScaledPolynomial',
                     model_kwargs={'w': [0.0], 'exponent': [4.0]}, min_depth=0.0, max_depth=float('inf'))
    seen = []

    class CB:
        def __getattr__(self, name):
            return lambda *a, **k: None

        def train_loss(self, it, model, clouds, pose_deltas, poses, masks, loss):
            seen.append(loss.item())
    train(cfg, callbacks=CB(), train_datasets=[raw], val_datasets=[])
    assert len(seen) == 20
    assert seen[-1] < seen[0], seen
