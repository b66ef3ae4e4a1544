"""Dynamic points in the map on the GPU (csrc/dc_dynamic.hip, slam.IcpMapper.update_dynamic): slam_bench's room with one box that
moves (--object: its half extents), --poses poses of --size lidar scans through the mapper with the slam_eval.launch odometry noise.
Reports the median time of update_dynamic and its split (directions, compaction, grid build, query, update), the map size and the
share of map points in range and matched, and the registration time with slam_cut_dynamic off and on.  Prints one JSON line.

    python tools/dynamic_bench.py [--poses 100] [--size 64 2048] [--object 0.4 0.4 0.8]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ('directions', 'compaction', 'grid_build', 'query', 'update')


def _poses(n):
    from depth_correction_amd.dataset import euler_matrix
    out = []
    for i in range(n):
        s = i / max(n - 1, 1)
        T = euler_matrix(0.0, 0.0, 0.6 * math.sin(2 * math.pi * s))
        T[:3, 3] = (-4.0 + 8.0 * s, 1.5 * math.sin(2 * math.pi * s), 0.05 * math.sin(7 * s))
        out.append(T)
    return np.stack(out)


def _run(clouds, odom, cfg):
    """The sequence through a mapper of cfg.  The tool drives update_dynamic itself, on every registered scan and with a
    synchronising timer that splits its stages (cfg leaves slam_compute_prob_dynamic off, so update() does not run it again)."""
    from depth_correction_amd.slam import IcpMapper, mapper_input
    from depth_correction_amd.utils import delta_transform
    mapper = IcpMapper(cfg)
    slam = odom.copy()
    rows = []
    for i, cloud in enumerate(clouds):
        scan = mapper.prepare(mapper_input(cloud, None, cfg))
        prior = odom[0] if i == 0 else slam[i - 1] @ delta_transform(odom[i - 1], odom[i])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pose, info = mapper.register(scan, prior)
        torch.cuda.synchronize()
        row = dict(register_ms=(time.perf_counter() - t0) * 1e3, iterations=info['iterations'], status=info['status'], map_size=mapper.n_map)
        slam[i] = pose
        if info['ok'] and mapper.n_map > 0:
            stamps = []

            def timer(stage):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
            timer('start')
            dyn = mapper.update_dynamic(scan, pose, timer=timer)
            if len(stamps) == len(STAGES) + 1:
                row.update({s + '_ms': (b - a) * 1e3 for s, a, b in zip(STAGES, stamps, stamps[1:])})
                row['dynamic_ms'] = (stamps[-1] - stamps[0]) * 1e3
                row.update(dyn)
        if info['ok']:
            mapper.update(scan, pose, overlap=info['overlap'] if info['status'] != 'init' else None)
        rows.append(row)
    return mapper, slam, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=100)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--object', type=float, nargs=3, default=(0.4, 0.4, 0.8), help='half extents of the box that moves')
    ap.add_argument('--grid-res', type=float, default=0.1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dynamic_bench needs a GPU')
    from depth_correction_amd.config import Config
    from depth_correction_amd.mesh import box_mesh, room_mesh
    from depth_correction_amd.render import MovingObjectDataset
    from depth_correction_amd.slam import odometry_poses, path_lengths, slam_errors
    dev = 'cuda:0'
    room = room_mesh((8.0, 5.0, 2.0), 0.5, pillars=[((2.0, 2.5, 0.0), (0.4, 0.4, 1.5)), ((-2.5, -2.5, 0.0), (0.5, 0.3, 1.5)),
                                                    ((0.5, -1.0, 0.0), (0.3, 0.3, 1.5))])
    half = tuple(args.object)
    box = box_mesh((0.0, 0.0, 0.0), half)
    gt = _poses(args.poses)
    obj = np.tile(np.eye(4), (args.poses, 1, 1))
    obj[:, :3, 3] = (5.0, -3.0, -2.0 + half[2])              # standing on the floor, off the sensor's path
    obj[args.poses // 3:, :3, 3] = (-5.5, 3.0, -2.0 + half[2])
    ds = MovingObjectDataset(room, [(box, obj)], gt, size=tuple(args.size), fov=(45.0, 360.0), num_segments=16, device=dev)
    clouds = [c for c, _ in ds]
    base = dict(device=dev, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=args.grid_res, odom_cov=[1e-4] * 3 + [2.5e-3] * 3)
    odom = odometry_poses(gt, base['odom_cov'])
    lengths = path_lengths(gt)
    med = lambda rs, k: float(np.median([r[k] for r in rs if k in r])) if any(k in r for r in rs) else None
    # 1. update_dynamic on every registered scan, split into its stages
    mapper, slam, rows = _run(clouds, odom, Config(**base))
    out = dict(tool='dynamic_bench', poses=args.poses, size=list(args.size), object=list(half), map_size_final=mapper.n_map,
               dynamic_final=mapper.n_dynamic, update_dynamic_ms_median=med(rows, 'dynamic_ms'))
    out.update({s + '_ms_median': med(rows, s + '_ms') for s in STAGES})
    timed = [r for r in rows if 'in_range' in r]
    out['in_range_share'] = float(np.mean([r['in_range'] / r['map_size'] for r in timed])) if timed else None
    out['matched_share'] = float(np.mean([r['matched'] / r['map_size'] for r in timed])) if timed else None
    out['occluded_share_of_matched'] = float(np.mean([r['occluded'] / max(r['matched'], 1) for r in timed])) if timed else None
    out['register_ms_median_cut_off'] = med([r for r in rows[1:] if r['iterations'] > 0], 'register_ms')
    out['slam_errors_cut_off'] = slam_errors(slam, gt, lengths)
    # 2. registration with the reference cloud cut at the threshold (probabilities on every scan, as above)
    mapper, slam, rows = _run(clouds, odom, Config(slam_cut_dynamic=True, **base))
    out['register_ms_median_cut_on'] = med([r for r in rows[1:] if r['iterations'] > 0], 'register_ms')
    out['slam_errors_cut_on'] = slam_errors(slam, gt, lengths)
    out['grid_builds_cut_on'] = mapper.grid_builds
    out['failed_cut_on'] = [i for i, r in enumerate(rows) if r['status'] in ('empty', 'too_few_pairs', 'singular', 'not_finite', 'bound')]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
