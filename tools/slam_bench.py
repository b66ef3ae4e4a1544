"""SLAM evaluation on the GPU (csrc/dc_slam.hip, slam.py): a --poses-pose sequence of --size lidar scans rendered from a room with
pillars, run through the mapper with the slam_eval.launch odometry noise.  Per scan: registration time, ICP iterations, host status
reads, map-update time and map size; launches per ICP iteration; the mean errors of SLAM and odometry.  Prints one JSON line.

    python tools/slam_bench.py [--poses 100] [--size 64 2048] [--grid-res 0.1] [--map points|tsdf]

With --map tsdf the same scene and odometry go through slam.TsdfMapper (cfg.slam_map = 'tsdf': every scan is registered against the fused
sparse TSDF volume, DESIGN "Scan-to-TSDF registration"); the JSON has the same keys, map_size_final counting blocks, added the rays fused
and grid_builds 0.

With --sweep the sequence is rendered as moving sweeps (render.SweepModel) and registered twice, by the 6-dof iteration on the raw
scans and by the sweep-aware 12-dof iteration (cfg.slam_ct, the odometry's twist as prior twist): registration time, iterations, time
and launches per iteration and the errors of both, side by side, in one JSON line.
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


def _poses(n):
    from depth_correction_amd.dataset import euler_matrix
    out = []
    for i in range(n):
        s = i / max(n - 1, 1)
        T = euler_matrix(0.0, 0.0, 0.6 * math.sin(2 * math.pi * s))
        T[:3, 3] = (-4.0 + 8.0 * s, 1.5 * math.sin(2 * math.pi * s), 0.05 * math.sin(7 * s))
        out.append(T)
    return np.stack(out)


def _sweep_compare(args):
    """The swept sequence through both registrations: dict(six_dof=..., sweep_aware=...) of medians and errors."""
    from depth_correction_amd.config import Config
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import RenderedMeshDataset, SweepModel
    from depth_correction_amd.slam import IcpMapper, mapper_input, odometry_poses, path_lengths, slam_errors
    from depth_correction_amd.sweep import motion_twist
    from depth_correction_amd.utils import delta_transform
    dev = 'cuda:0'
    mesh = room_mesh((8.0, 5.0, 2.0), 0.5, pillars=[((2.0, 2.5, 0.0), (0.4, 0.4, 1.5)), ((-2.5, -2.5, 0.0), (0.5, 0.3, 1.5)),
                                                    ((0.5, -1.0, 0.0), (0.3, 0.3, 1.5))])
    path = os.path.join(tempfile.mkdtemp(), 'bench_room.ply')
    mesh.save_ply(path)
    gt = _poses(args.poses)
    ds = RenderedMeshDataset(path, poses=gt, size=tuple(args.size), fov=(45.0, 360.0), num_segments=16, device=dev, sweep=SweepModel())
    clouds = [c for c, _ in ds]
    lengths = path_lengths(gt)
    out = dict(tool='slam_bench', sweep=True, poses=args.poses, size=list(args.size), grid_res=args.grid_res, status_every=args.status_every)
    for name, ct in (('six_dof', False), ('sweep_aware', True)):
        cfg = Config(device=dev, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=args.grid_res,
                     odom_cov=[1e-4] * 3 + [2.5e-3] * 3, slam_ct=ct)
        odom = odometry_poses(gt, cfg.odom_cov)
        mapper = IcpMapper(cfg, status_every=args.status_every)
        slam = odom.copy()
        rows = []
        for i, cloud in enumerate(clouds):
            scan = mapper.prepare(mapper_input(cloud, None, cfg))
            prior = odom[0] if i == 0 else slam[i - 1] @ delta_transform(odom[i - 1], odom[i])
            step = delta_transform(slam[i - 1], prior) if i > 0 else (delta_transform(odom[0], odom[1]) if len(clouds) > 1 else np.eye(4))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pose, info = mapper.register(scan, prior, twist=motion_twist(step))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if info['ok']:
                mapper.update(info.pop('deskewed', scan), pose, overlap=info['overlap'] if info['status'] != 'init' else None)
            slam[i] = pose
            rows.append(dict(register_ms=(t1 - t0) * 1e3, iterations=info['iterations'], status=info['status'],
                             launches=info['launches_per_iteration']))
        reg = [r for r in rows[1:] if r['iterations'] > 0]
        out[name] = dict(register_ms_median=float(np.median([r['register_ms'] for r in reg])) if reg else None,
                         iterations_median=float(np.median([r['iterations'] for r in reg])) if reg else None,
                         ms_per_iteration_median=float(np.median([r['register_ms'] / r['iterations'] for r in reg])) if reg else None,
                         launches_per_iteration=reg[0]['launches'] if reg else None,
                         failed=[i for i, r in enumerate(rows) if r['status'] in ('empty', 'too_few_pairs', 'singular', 'not_finite', 'bound')],
                         map_size_final=mapper.n_map, slam_errors=slam_errors(slam, gt, lengths))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=100)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--grid-res', type=float, default=0.1)
    ap.add_argument('--status-every', type=int, default=4)
    ap.add_argument('--map', choices=('points', 'tsdf'), default='points', help="the mapper's map (cfg.slam_map)")
    ap.add_argument('--tsdf-voxel', type=float, default=0.1, help='voxel size of the TSDF map (cfg.slam_tsdf_voxel_size)')
    ap.add_argument('--sweep', action='store_true', help='render moving sweeps and time the 6-dof and the sweep-aware registration')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('slam_bench needs a GPU')
    if args.sweep:
        print(json.dumps(_sweep_compare(args)))
        return
    from depth_correction_amd.config import Config
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import RenderedMeshDataset
    from depth_correction_amd.slam import make_mapper, mapper_input, odometry_poses, path_lengths, slam_errors
    from depth_correction_amd.utils import delta_transform
    dev = 'cuda:0'
    mesh = room_mesh((8.0, 5.0, 2.0), 0.5, pillars=[((2.0, 2.5, 0.0), (0.4, 0.4, 1.5)), ((-2.5, -2.5, 0.0), (0.5, 0.3, 1.5)),
                                                    ((0.5, -1.0, 0.0), (0.3, 0.3, 1.5))])
    path = os.path.join(tempfile.mkdtemp(), 'bench_room.ply')
    mesh.save_ply(path)
    gt = _poses(args.poses)
    ds = RenderedMeshDataset(path, poses=gt, size=tuple(args.size), fov=(45.0, 360.0), num_segments=16, device=dev)
    cfg = Config(device=dev, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=args.grid_res,
                 odom_cov=[1e-4] * 3 + [2.5e-3] * 3, slam_map=args.map, slam_tsdf_voxel_size=args.tsdf_voxel)
    clouds = [c for c, _ in ds]
    odom = odometry_poses(gt, cfg.odom_cov)
    mapper = make_mapper(cfg, status_every=args.status_every)
    launches = None
    slam = odom.copy()
    rows = []
    for i, cloud in enumerate(clouds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scan = mapper.prepare(mapper_input(cloud, None, cfg))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        prior = odom[0] if i == 0 else slam[i - 1] @ delta_transform(odom[i - 1], odom[i])
        pose, info = mapper.register(scan, prior)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        added = mapper.update(scan, pose, overlap=info['overlap'] if info['status'] != 'init' else None) if info['ok'] else 0
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        slam[i] = pose
        launches = info['launches_per_iteration']
        rows.append(dict(points=len(scan), prepare_ms=(t1 - t0) * 1e3, register_ms=(t2 - t1) * 1e3, update_ms=(t3 - t2) * 1e3,
                         iterations=info['iterations'], host_reads=info['host_reads'], status=info['status'], added=added,
                         map_size=mapper.n_map))
    lengths = path_lengths(gt)
    reg = [r for r in rows[1:] if r['iterations'] > 0]
    med = lambda k, rs=reg: float(np.median([r[k] for r in rs])) if rs else float('nan')
    iters = np.array([r['iterations'] for r in reg])
    out = dict(tool='slam_bench', map=args.map, poses=args.poses, size=list(args.size), grid_res=args.grid_res, points_per_scan=med('points', rows),
               launches_per_iteration=launches, status_every=args.status_every,
               register_ms_median=med('register_ms'), register_ms_max=float(max(r['register_ms'] for r in reg)) if reg else None,
               iterations_median=float(np.median(iters)) if len(iters) else None, iterations_max=int(iters.max()) if len(iters) else None,
               ms_per_iteration_median=float(np.median([r['register_ms'] / r['iterations'] for r in reg])) if reg else None,
               host_reads_per_iteration=float(sum(r['host_reads'] for r in reg) / max(1, iters.sum())),
               prepare_ms_median=med('prepare_ms', rows), update_ms_median=med('update_ms', rows[1:]),
               map_size_final=mapper.n_map, grid_builds=getattr(mapper, 'grid_builds', 0),
               failed=[i for i, r in enumerate(rows) if r['status'] in ('empty', 'too_few_pairs', 'singular', 'not_finite', 'bound')],
               slam_errors=slam_errors(slam, gt, lengths), odom_errors=slam_errors(odom, gt, lengths))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
