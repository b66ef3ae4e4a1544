"""The supervised mesh loss on the GPU (csrc/dc_meshloss.hip): one evaluation -- loss and gradients to the weights and the poses --
of --poses rendered H x W scans (2 cm of depth noise, a ScaledPolynomial model) against a >= 1 M-triangle grid_terrain_mesh and
against a pillared room_mesh, timed three ways in ONE process, alternating, after a warm-up of every shape:

    cold    the fused call (ops.mesh_loss) with the leaf hint reset to -1
    warm    the fused call with the hint carried from the previous call at weights 1 % away (what consecutive Adam steps do)
    unfused the composition ops.points_fwd + ops.mesh_closest + the torch expression for l and dl/dx + ops.points_bwd

and the time per iteration of train() with cfg.loss = 'mesh_loss' on the room.  The fused and the un-fused form are compared at the
timed size in the same run (loss within 2^-40 x extent, faces equal).  Medians of --reps synchronised runs.  Prints one JSON line.

    python tools/meshloss_bench.py [--n 710] [--poses 10] [--size 64 2048] [--reps 10] [--train-iters 40]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/meshloss_bench.py --reps 3 --train-iters 0      # kernel times
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# launches per evaluation: the fused call is its walk kernel and its finishing kernel; the composition is dc_points_fwd,
# dc_mesh_closest, dc_points_bwd's two, and the elementwise / reduction kernels of the torch expression below (counted from it)
LAUNCHES = {'fused': 2, 'unfused_native': 4, 'unfused_torch': 9}


def _poses(n, height, spread):
    out = []
    for i in range(n):
        yaw = 0.37 * i
        p = np.eye(4)
        p[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
        p[:3, 3] = (spread * math.cos(1.3 * i), spread * math.sin(0.7 * i), height)
        out.append(p)
    return np.stack(out)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _scans(mesh, bvh, normals, poses, dirs, tmin, dev):
    """Sensor-frame fields of the rays that hit, scan-major: (PointSet with scan ids, scan_ptr)."""
    from depth_correction_amd import ops
    face, t, _ = ops.raycast(bvh, dirs, poses, tmin)
    hit = face >= 0
    gen = torch.Generator(device=dev).manual_seed(135)
    depth = (t + 0.02 * torch.randn(t.shape, dtype=torch.float64, device=dev, generator=gen))[hit].contiguous()
    d = dirs[None].expand(poses.shape[0], -1, -1)[hit].contiguous()
    world = torch.einsum('pij,rj->pri', poses[:, :3, :3], dirs)[hit]
    inc = torch.acos((world * normals[face[hit].long()]).sum(dim=-1).abs().clamp(max=1.0)).contiguous()
    sizes = hit.sum(dim=1).tolist()
    scan_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), device=dev)
    return ops.PointSet(None, d, depth, inc, None, ops.scan_ids(sizes, dev)), scan_ptr


def _unfused(bvh, ps, poses12, kind, w, e):
    from depth_correction_amd import ops
    x = ops.points_fwd(ps, poses12, kind, w, e)
    face, dist, closest = ops.mesh_closest(bvh, x)
    used = face >= 0
    m = used.sum()
    diff = torch.where(used[:, None], x - closest, torch.zeros_like(x))
    r = torch.where(used, dist, torch.zeros_like(dist))
    loss = r.sum() / m
    g = (diff / torch.where(r > 0, r, torch.ones_like(r))[:, None] / m).contiguous()
    gw, ge, gT = ops.points_bwd(g, ps, poses12, kind, w, e, want_pose=True)
    return loss, face, gw, gT


def _train_ms_per_iter(room, iters, size, dev):
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import DepthBiasDataset, RenderedMeshDataset
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.train import train
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'room.ply')
    room.save_ply(path)
    cfg = Config(device=str(dev), float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25, loss='mesh_loss',
                 lr=1e-3, log_dir=os.path.join(tmp, 'log'), model_kwargs={'w': [0.0, 0.0], 'exponent': [2.0, 4.0]})
    ds = RenderedMeshDataset(path, poses=_poses(4, 0.0, 3.0), size=size, fov=(45.0, 360.0), num_segments=16, device=str(dev))
    ds = DepthBiasDataset(ds, ScaledPolynomial(w=[-0.01, 0.004], exponent=[2.0, 4.0], device=dev), cfg=cfg)
    out = {}
    for n_it in (3, 3, 3 + iters):                   # a warm-up run (one-time costs: the tree, the first launches), then the
                                                     # difference of two runs, which leaves the set-up (clouds, neighbourhoods) out
        cfg.n_opt_iters = n_it
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train(cfg, train_datasets=[ds], val_datasets=[])
        torch.cuda.synchronize()
        out[n_it] = (time.perf_counter() - t0) * 1e3
    return (out[3 + iters] - out[3]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--train-iters', type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('meshloss_bench needs a GPU')
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    out = dict(tool='meshloss_bench', poses=args.poses, size=list(args.size), reps=args.reps, launches=LAUNCHES)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    kind = 'ScaledPolynomial'
    w0 = torch.tensor([-0.004, 0.002], dtype=torch.float64, device=dev)
    w1, e = (w0 * 1.01).contiguous(), torch.tensor([2.0, 4.0], dtype=torch.float64, device=dev)
    scenes = []
    for name, mesh, height, spread in (('terrain', grid_terrain_mesh(args.n), 8.0, 60.0), ('room', room, 0.0, 3.0)):
        _, _, normals, bvh = mesh.on_device(dev)
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        ps, scan_ptr = _scans(mesh, bvh, normals, poses, dirs, tmin, dev)
        poses12 = poses[:, :3, :].reshape(-1, 12).contiguous()
        hint = torch.full((ps.n,), -1, dtype=torch.int32, device=dev)
        ws = ops.mesh_loss_workspace(ps.n, args.poses, 2, dev)
        fused = lambda w, hint=hint, bvh=bvh, ps=ps, scan_ptr=scan_ptr, poses12=poses12, ws=ws: ops.mesh_loss(
            bvh, ps, scan_ptr, poses12, kind, w, e, leaf_hint=hint, ws=ws)
        scenes.append((name, mesh, bvh, ps, scan_ptr, poses12, hint, fused))
    for name, mesh, bvh, ps, scan_ptr, poses12, hint, fused in scenes:      # warm-up of every shape before any is timed
        fused(w0)
        _unfused(bvh, ps, poses12, kind, w0, e)
    torch.cuda.synchronize()
    for name, mesh, bvh, ps, scan_ptr, poses12, hint, fused in scenes:
        ts = {'cold': [], 'warm': [], 'unfused': []}
        for rep in range(args.reps):
            def cold():
                hint.fill_(-1)
                fused(w0)
            ts['cold'].append(_timed(cold))                         # leaves the hint of w0 behind
            ts['warm'].append(_timed(lambda: fused(w1)))             # ... carried to weights 1 % away
            ts['unfused'].append(_timed(lambda: _unfused(bvh, ps, poses12, kind, w1, e)))
        res = {'faces': len(mesh), 'points': ps.n}
        for k, v in ts.items():
            res['%s_ms' % k], res['%s_min_ms' % k] = float(np.median(v)), float(np.min(v))
        res['cold_over_unfused'], res['warm_over_unfused'] = res['cold_ms'] / res['unfused_ms'], res['warm_ms'] / res['unfused_ms']
        res['warm_over_cold'] = res['warm_ms'] / res['cold_ms']
        # the two forms at the timed size
        o, face, dist, _ = ops.mesh_loss(bvh, ps, scan_ptr, poses12, kind, w1, e, leaf_hint=hint, want_points=True)
        loss_u, face_u, gw_u, gT_u = _unfused(bvh, ps, poses12, kind, w1, e)
        extent = float(np.max(mesh.bounds[1] - mesh.bounds[0]))
        res['loss'], res['loss_diff'], res['loss_bar'] = float(o[0]), abs(float(o[0]) - float(loss_u)), 2.0 ** -40 * extent
        res['faces_equal'] = bool(torch.equal(face, face_u))
        res['grad_w_rel_diff'] = float((o[4:6] - gw_u).abs().max() / gw_u.abs().max())
        res['grad_pose_rel_diff'] = float((o[8:].reshape(-1, 3, 4) - gT_u).abs().max() / gT_u.abs().max())
        assert res['loss_diff'] <= res['loss_bar'] and res['faces_equal'], res
        out[name] = res
    if args.train_iters > 0:
        out['train_room_ms_per_iter'] = _train_ms_per_iter(room, args.train_iters, (64, 512), dev)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
