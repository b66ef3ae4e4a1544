"""The loss against the fused volume on the GPU (csrc/dc_tsdf_loss.hip): one evaluation -- loss and gradients to the weights and the
poses -- of --poses rendered H x W scans (2 cm of depth noise, a ScaledPolynomial model) of the pillared room of the other loss tools
against the sparse TSDF volume the scans themselves fuse into (loss.TsdfTarget, voxels of --voxel metres), timed in ONE process,
alternating, after a warm-up of every form:

    fused_loo   the one host call (ops.tsdf_loss) with exclusion: every scan against the volume of the other scans
    fused_all   the same without exclusion
    unfused     the composition ops.points_fwd + ops.tsdf_sparse_sample + the torch expression for l and dl/dx + ops.points_bwd
                (no exclusion: the composition would need one sample call per scan and S volumes of S - 1 scans)
    refresh     TsdfTarget.refresh, all scans only and with leave-one-out (host timer: it reads the host)
    cloud_loss  as context: one ops.cloud_loss evaluation of the same points against a survey of --survey points sampled from the mesh
                (point to plane, gated at 0.5 m, trimmed at 0.8: tools/cloudloss_bench.py's settings)
    min_eigval  as context: one pose-mode evaluation (loss, dL/dw, dL/d[R|t]) of the k = 10 min-eigenvalue loss on the same points
                (pipeline.build_sequence + SequencePlan.eval_native, what tools/pose_bench.py times)

fused_all and unfused are compared in the same run: the same used set, the loss within 16 ((n + 16) 2^-53 sum |l| + 2^-53 sum 2 |phi|
sum_a |grad_a| |x_a|) / M (the bar of tests/test_gpu_tsdf_loss.py's fused-against-un-fused test, formed on the device).  Device events,
medians of --reps.  Prints one JSON line.

With --train the tool runs train() instead, on --poses rendered --train-size scans of the same room whose depths carry the bias d / (1
- 0.05 g^2) (dataset.DepthBiasDataset; a ScaledPolynomial with one weight, exponent 2, started at 0): the wall time per iteration
with cfg.loss = 'tsdf_loss' at tsdf_refresh_every 1 and 10 (the difference of a long and a short run over the difference of their
iterations, so that the set-up drops out), and the weight --train-iters iterations reach with tsdf_loss and with min_eigval_loss.

    python tools/tsdfloss_bench.py [--poses 10] [--size 64 2048] [--voxel 0.1] [--reps 10] [--survey 200000]
    python tools/tsdfloss_bench.py --train [--train-size 32 512] [--train-iters 100] [--lr 1e-3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from meshloss_bench import _poses, _scans          # noqa: E402  (the same scans as the mesh-loss tool)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _unfused(tb, ps, poses12, kind, w, e):
    from depth_correction_amd import ops
    x = ops.points_fwd(ps, poses12, kind, w, e)
    s = ops.tsdf_sparse_sample(tb.keys, tb.slots, tb.n_blocks, tb.sum, tb.count, tb.origin, tb.voxel, tb.trunc, x)
    used = (s['flag'] == 0) & (s['dist'] < tb.trunc)
    m = used.sum()
    phi = torch.where(used, s['value'], torch.zeros_like(s['value']))
    loss = (phi * phi).sum() / m
    g = ((2.0 * phi)[:, None] * s['grad'] / m).contiguous()
    gw, ge, gT = ops.points_bwd(g, ps, poses12, kind, w, e, want_pose=True)
    return loss, used, gw, gT, x, s


ROOM = dict(size=(10.0, 7.0, 2.0), pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)), ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
TRUE_W = 0.05


def _train(args):
    """train() on the biased pillared room: time per iteration and the weight reached."""
    import tempfile
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.train import train
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'room.ply')
    room_mesh(ROOM['size'], 0.5, pillars=ROOM['pillars']).save_ply(path)
    poses = _poses(args.poses, 0.0, 3.0)
    gt = ScaledPolynomial(w=[TRUE_W], exponent=[2.0], device='cuda:0')
    runs = [0]

    def run(loss, iters, **loss_kwargs):
        runs[0] += 1
        cfg = Config(device='cuda:0', float_type='float64', min_depth=0.3, max_depth=25.0, grid_res=0.05, nn_k=0, nn_r=0.25, loss=loss,
                     n_opt_iters=iters, lr=args.lr, log_dir=os.path.join(tmp, 'run%d' % runs[0]), model_kwargs={'w': [0.0], 'exponent': [2.0]})
        cfg.loss_kwargs = dict(cfg.loss_kwargs, tsdf_voxel_size=args.voxel, **loss_kwargs)
        ds = DepthBiasDataset(RenderedMeshDataset(path, poses=poses, size=tuple(args.train_size), fov=(45.0, 360.0), num_segments=args.segments,
                                                  device='cuda:0'), gt, cfg=cfg)
        os.makedirs(cfg.log_dir)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train(cfg, train_datasets=[ds], val_datasets=[])
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        last = sorted((f for f in os.listdir(cfg.log_dir) if f.endswith('_state_dict.pth')), key=lambda f: os.path.getmtime(os.path.join(cfg.log_dir, f)))
        w = torch.load(os.path.join(cfg.log_dir, last[-1]))['w'].reshape(-1).tolist() if last else None
        return seconds, w
    out = dict(tool='tsdfloss_bench --train', poses=args.poses, size=list(args.train_size), voxel=args.voxel, iters=args.train_iters, lr=args.lr,
               true_w=TRUE_W)
    short = 20
    run('tsdf_loss', 4, tsdf_refresh_every=1)                        # warm-up of the process (library load, first launches)
    for every in (1, 10):
        t_short, _ = run('tsdf_loss', short, tsdf_refresh_every=every)
        t_long, w = run('tsdf_loss', args.train_iters, tsdf_refresh_every=every)
        out['tsdf_refresh_%d' % every] = dict(ms_per_iteration=(t_long - t_short) * 1e3 / (args.train_iters - short), w_of_best_iteration=w,
                                              seconds=[t_short, t_long])
    t_short, _ = run('min_eigval_loss', short)
    t_long, w = run('min_eigval_loss', args.train_iters)
    out['min_eigval_loss'] = dict(ms_per_iteration=(t_long - t_short) * 1e3 / (args.train_iters - short), w_of_best_iteration=w,
                                  seconds=[t_short, t_long])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--survey', type=int, default=200000, help='points of the survey of the cloud_loss context row')
    ap.add_argument('--train', action='store_true', help='run train() on the biased room instead of the evaluations')
    ap.add_argument('--train-size', type=int, nargs=2, default=(32, 512))
    ap.add_argument('--train-iters', type=int, default=100)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--voxel', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tsdfloss_bench needs a GPU')
    if args.train:
        return _train(args)
    from depth_correction_amd import ops
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.loss import TsdfTarget
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    out = dict(tool='tsdfloss_bench', poses=args.poses, size=list(args.size), voxel=args.voxel, reps=args.reps)
    room = room_mesh(ROOM['size'], 0.5, pillars=ROOM['pillars'])
    kind = 'ScaledPolynomial'
    w = torch.tensor([-0.004, 0.002], dtype=torch.float64, device=dev)
    e = torch.tensor([2.0, 4.0], dtype=torch.float64, device=dev)
    model = ScaledPolynomial(w=w.tolist(), exponent=e.tolist(), device=dev)
    _, _, normals, bvh = room.on_device(dev)
    poses = torch.as_tensor(_poses(args.poses, 0.0, 3.0), device=dev)
    ps, scan_ptr = _scans(room, bvh, normals, poses, dirs, tmin, dev)
    poses12 = poses[:, :3, :].reshape(-1, 12).contiguous()
    ptr = scan_ptr.tolist()
    clouds = [DepthCloud(vps=torch.zeros((b - a, 3), dtype=torch.float64, device=dev), dirs=ps.dirs[a:b], depth=ps.depth[a:b].reshape(-1, 1),
                         inc_angles=ps.inc[a:b].reshape(-1, 1)) for a, b in zip(ptr, ptr[1:])]
    targets = {}
    for name, loo in (('all', False), ('loo', True)):
        t = TsdfTarget(args.voxel, leave_one_out=loo, refresh_every=0)
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.refresh(clouds, poses, model)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        targets[name] = t
        out['refresh_%s_ms' % name] = float(np.median(times))
    tgt = targets['loo']
    out['points'], out['blocks'] = ps.n, tgt.total.n_blocks
    out['own_blocks'] = int(tgt.own.keys.shape[0])
    ws = ops.tsdf_loss_workspace(ps.n, args.poses, 2, dev)
    forms = {
        'fused_loo': lambda **kw: ops.tsdf_loss(tgt.tables, ps, scan_ptr, poses12, kind, w, e, own=tgt.own, ws=ws, **kw),
        'fused_all': lambda **kw: ops.tsdf_loss(tgt.tables, ps, scan_ptr, poses12, kind, w, e, ws=ws, **kw),
        'unfused': lambda: _unfused(tgt.tables, ps, poses12, kind, w, e),
    }
    # context: the supervised cloud loss and the k = 10 min-eigenvalue loss (pose mode) on the same points
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.survey import SurveyCloud
    sd = SurveyCloud.from_mesh(room, args.survey, seed=135, device=dev).on_device(dev).reserve(ps.n)
    cws = ops.cloud_loss_workspace(ps.n, args.poses, 2, dev)
    forms['cloud_loss'] = lambda: ops.cloud_loss(sd, ps, scan_ptr, poses12, kind, w, e, plane=True, max_dist=0.5, inlier_ratio=0.8, ws=cws)
    local = (ps.dirs * ps.depth[:, None]).float().cpu().numpy()
    plan, info = build_sequence([local[a:b] for a, b in zip(ptr, ptr[1:])], poses.cpu().numpy(), k=10, dtype=torch.float32, device=dev)
    res = torch.zeros((2 + 4 + 12 * plan.n_scans,), dtype=torch.float64, device=dev)
    P = plan.poses12(info['poses'])
    forms['min_eigval'] = lambda: plan.eval_native(w, e, P, res, want_grad=True, want_pose=True)
    out['survey_points'], out['min_eigval_k'] = sd.n, 10
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in forms}
    for rep in range(args.reps):
        for k, fn in forms.items():
            ts[k].append(_event_ms(fn))
    for k, v in ts.items():
        out['%s_ms' % k], out['%s_min_ms' % k] = float(np.median(v)), float(np.min(v))
    out['fused_all_over_unfused'] = out['fused_all_ms'] / out['unfused_ms']
    out['cloud_loss_used'] = int(forms['cloud_loss']()[1])
    # the two forms at the timed size
    o, value, flag, x = forms['fused_all'](want_points=True)
    loss_u, used_u, gw_u, gT_u, x_u, s = _unfused(tgt.tables, ps, poses12, kind, w, e)
    n, m = ps.n, float(o[1])
    phi = torch.where(used_u, s['value'], torch.zeros_like(s['value']))
    reach = (s['grad'].abs() * x_u.abs()).sum(dim=1)
    bar = 16 * 2.0 ** -53 * ((n + 16) * float((phi * phi).sum()) + float((2.0 * phi.abs() * reach).sum())) / m
    out['loss'], out['loss_diff'], out['loss_bar'] = float(o[0]), abs(float(o[0]) - float(loss_u)), bar
    out['used'], out['gated'], out['unobserved'], out['invalid'] = (int(v) for v in o[1:5].tolist())
    out['used_equal'] = bool(torch.equal(flag == 0, used_u))
    out['x_equal'] = bool(torch.equal(x, x_u))
    out['grad_w_rel_diff'] = float((o[5:7] - gw_u).abs().max() / gw_u.abs().max())
    out['grad_pose_rel_diff'] = float((o[9:].reshape(-1, 3, 4) - gT_u).abs().max() / gT_u.abs().max())
    o_loo = forms['fused_loo']()
    out['loss_loo'], out['used_loo'] = float(o_loo[0]), int(o_loo[1])
    assert out['loss_diff'] <= out['loss_bar'] and out['used_equal'], out
    print(json.dumps(out))


if __name__ == '__main__':
    main()
