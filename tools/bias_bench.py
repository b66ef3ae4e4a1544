"""Depth bias against the mesh on the GPU (csrc/dc_raycast.hip dc_raycast_rays, csrc/dc_bias.hip): (a) the cast of measured rays next to
dc_raycast on identical rays (--poses poses x --size pattern, vps = 0) against a >= 1 M-triangle grid_terrain_mesh, a pillared
room_mesh and the 12-triangle room of tools/render_bench.py; (b) the same hits as measured rays in the order filter_grid leaves them (grid 0.1 m, keep='random') next to the same
rays in pattern order and after a Morton sort of their end points (the sort's own cost beside it); (c) dc_bias_accumulate on the
rays of (a) with 18 bins and 2 terms; (d) a whole eval_bias on the room of tools/slam_bench.py (--eval-poses scans of --eval-size).
Median, min and max of --reps synchronised runs in a warm process.  Prints one JSON line.

    python tools/bias_bench.py [--n 710] [--poses 10] [--size 128 2048] [--reps 20] [--eval-poses 20] [--eval-size 64 2048]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bias_bench.py --reps 3 --eval-poses 0      # kernel times
"""
import argparse
import contextlib
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def _poses(n, height, spread):
    out = []
    for i in range(n):
        yaw = 0.37 * i
        p = np.eye(4)
        p[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
        p[:3, 3] = (spread * math.cos(1.3 * i), spread * math.sin(0.7 * i), height)
        out.append(p)
    return np.stack(out)


def _eval_bench(args, dev):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_bias
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.render import DepthBiasDataset, RenderedMeshDataset
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from slam_bench import _poses as slam_poses
    mesh = room_mesh((8.0, 5.0, 2.0), 0.5, pillars=[((2.0, 2.5, 0.0), (0.4, 0.4, 1.5)), ((-2.5, -2.5, 0.0), (0.5, 0.3, 1.5)),
                                                    ((0.5, -1.0, 0.0), (0.3, 0.3, 1.5))])
    path = os.path.join(tempfile.mkdtemp(), 'bench_room.ply')
    mesh.save_ply(path)
    cfg = Config(device=dev, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.1, nn_k=0, nn_r=0.25)
    model = ScaledPolynomial(w=[0.02, 0.01], exponent=[2.0, 4.0], device=dev)
    ds = DepthBiasDataset(RenderedMeshDataset(path, poses=slam_poses(args.eval_poses), size=tuple(args.eval_size), fov=(45.0, 360.0),
                                              num_segments=16, device=dev), model, cfg=cfg)
    items = [(c, p) for c, p in ds]                       # rendering and biasing are the dataset's cost, not the evaluation's

    class Cached(object):
        def get_mesh(self):
            return ds.get_mesh()

        def __iter__(self):
            return iter(items)

        def __str__(self):
            return 'bench_room'

    ts, res = [], None
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):          # eval_bias prints its line per sequence: this tool prints one JSON line
            res = eval_bias(cfg, test_datasets=[Cached()], model=model)[0]
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    b, a, fit = res['before'], res['after'], res['fit']
    return dict(scans=args.eval_poses, size=list(args.eval_size), rays=int(b['totals']['rays']), used=int(b['totals']['used']),
                eval_bias_ms=dict(first=ts[0], median=float(np.median(ts[1:])), min=float(np.min(ts[1:])), max=float(np.max(ts[1:]))),
                rms_before=b['overall']['rms'], rms_after=a['overall']['rms'], angle_err_rms=b['overall']['angle_err_rms'],
                angle_err_rms_per_bin=[round(float(x), 5) for x in b['angle_err_rms'].cpu().tolist()],
                w_true_angles=[float(x) for x in fit['w_true_angles']], w_est_angles=[float(x) for x in fit['w_est_angles']])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(128, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--eval-poses', type=int, default=20)
    ap.add_argument('--eval-size', type=int, nargs=2, default=(64, 2048))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bias_bench needs a GPU')
    from depth_correction_amd.filters import filter_grid
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.ops import bias_accumulate, bias_out_count, bias_workspace, gather_rows, raycast, raycast_rays, spatial_order
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs1 = torch.as_tensor(np.array(d), device=dev)
    # one near clip for both entry points: dc_raycast_rays takes a scalar
    tmin = torch.full((dirs1.shape[0],), float(np.max(t_min)), dtype=torch.float64, device=dev)
    R, tmin0 = dirs1.shape[0], float(np.max(t_min))
    out = dict(tool='bias_bench', poses=args.poses, size=list(args.size), reps=args.reps)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    room12 = room_mesh((10.0, 7.0, 2.0), 100.0)                           # the 12-triangle room of tools/render_bench.py
    for name, mesh, height, spread in (('terrain', grid_terrain_mesh(args.n), 8.0, 60.0), ('room', room, 0.0, 3.0), ('room12', room12, 0.0, 3.0)):
        bvh = mesh.on_device(dev)[3]
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        P = poses.shape[0]
        dirs = dirs1.repeat(P, 1).contiguous()
        vps = torch.zeros_like(dirs)
        off = torch.arange(P + 1, dtype=torch.int64, device=dev) * R
        face, t, _ = raycast(bvh, dirs1, poses, tmin)
        face2, t2, inc = raycast_rays(bvh, vps, dirs, off, poses, t_min=tmin0)
        assert torch.equal(face.reshape(-1), face2) and torch.equal(t.reshape(-1), t2)
        # interleaved, so that a drift of the clocks or of the machine's load meets both alike
        a, b = [], []
        for _ in range(3):
            a.append(_stats_ms(lambda: raycast(bvh, dirs1, poses, tmin), args.reps))
            b.append(_stats_ms(lambda: raycast_rays(bvh, vps, dirs, off, poses, t_min=tmin0), args.reps))
        merge = lambda rs: dict(median=float(np.median([r['median'] for r in rs])), min=min(r['min'] for r in rs), max=max(r['max'] for r in rs),
                                medians=[r['median'] for r in rs])
        res = dict(faces=len(mesh), rays=int(face2.numel()), hits=int((face2 >= 0).sum()), raycast_ms=merge(a), raycast_rays_ms=merge(b))
        res['ratio'] = res['raycast_rays_ms']['median'] / res['raycast_ms']['median']
        vps32, dirs32 = vps.float(), dirs.float()
        res['raycast_rays_f32_ms'] = _stats_ms(lambda: raycast_rays(bvh, vps32, dirs32, off, poses, t_min=tmin0), args.reps)
        # ---- ray order: the hits as measured rays, per scan through filter_grid ----
        kept_pattern, kept_filter, sizes = [], [], []
        for p in range(P):
            idx = torch.nonzero(face[p] >= 0).reshape(-1)
            pts = (dirs1[idx] * t[p][idx, None]).contiguous()                      # sensor frame
            sel = filter_grid(pts, 0.1, only_mask=True, keep='random', rng=np.random.default_rng(135))
            sel = torch.as_tensor(np.asarray(sel, dtype=np.int64), device=dev)
            kept_filter.append(idx[sel])
            kept_pattern.append(torch.sort(idx[sel]).values)
            sizes.append(len(sel))
        off2 = np.concatenate([[0], np.cumsum(sizes)])
        off2_dev = torch.as_tensor(off2, dtype=torch.int64, device=dev)
        cast = lambda dd: raycast_rays(bvh, torch.zeros_like(dd), dd, off2_dev, poses, t_min=tmin0)
        d_filter = torch.cat([dirs1[k] for k in kept_filter]).contiguous()
        d_pattern = torch.cat([dirs1[k] for k in kept_pattern]).contiguous()

        def morton(dd):
            parts = []
            for p in range(P):
                seg = dd[off2[p]:off2[p + 1]].contiguous()
                parts.append(gather_rows(seg, spatial_order(seg).long()) if seg.shape[0] else seg)
            return torch.cat(parts).contiguous()
        d_morton = morton(d_filter)
        res['order'] = dict(rays=int(off2[-1]), filter_grid_ms=_stats_ms(lambda: cast(d_filter), args.reps),
                            pattern_ms=_stats_ms(lambda: cast(d_pattern), args.reps), morton_ms=_stats_ms(lambda: cast(d_morton), args.reps),
                            morton_sort_ms=_stats_ms(lambda: morton(d_filter), args.reps))
        # ---- accumulate on the rays of (a) ----
        gen = torch.Generator(device=dev).manual_seed(135)
        depth = (t.reshape(-1).nan_to_num(posinf=1.0) * (1.0 + 0.02 * inc.nan_to_num() ** 2)
                 + 0.01 * torch.randn(t.numel(), dtype=torch.float64, device=dev, generator=gen)).contiguous()
        est = (inc.nan_to_num() + 0.03 * torch.randn(t.numel(), dtype=torch.float64, device=dev, generator=gen)).clamp(0.0, math.pi / 2)
        mask = torch.rand(t.numel(), device=dev, generator=gen) < 0.8
        buf = torch.empty((bias_out_count(18, 2),), dtype=torch.float64, device=dev)
        ws = bias_workspace(18, 2, dev)
        acc = lambda: bias_accumulate(depth, est, mask, face2, t2, inc, 'ScaledPolynomial', [2.0, 4.0], n_bins=18, max_residual=0.5, out=buf, ws=ws)
        res['accumulate_ms'] = _stats_ms(acc, args.reps)
        res['accumulate_used'] = int(acc()[3])
        out[name] = res
    if args.eval_poses > 0:
        out['eval_bias'] = _eval_bench(args, 'cuda:0')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
