"""Mesh rendering on the GPU (csrc/dc_raycast.hip): LBVH build time on a >= 1 M-triangle grid_terrain_mesh, and the one-launch cast
of --poses poses x H x W lidar rays (rays/s) against that terrain and against a 12-triangle room (traversal-light).  Medians of
--reps synchronised runs in a warm process.  Prints one JSON line.

    python tools/render_bench.py [--n 710] [--poses 10] [--size 128 2048] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/render_bench.py --reps 3      # kernel times
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


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def _poses(n, height, spread):
    out = []
    for i in range(n):
        yaw = 0.37 * i
        p = np.eye(4)
        p[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
        p[:3, 3] = (spread * math.cos(1.3 * i), spread * math.sin(0.7 * i), height)
        out.append(p)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(128, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench needs a GPU')
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.ops import bvh_build, raycast
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    terrain = grid_terrain_mesh(args.n)
    verts = torch.as_tensor(terrain.vertices, device=dev)
    faces = torch.as_tensor(terrain.faces, device=dev)
    box = np.concatenate(terrain.bounds)
    build_ms, build_min = _median_ms(lambda: bvh_build(verts, faces, box), args.reps)
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    n_rays = args.poses * dirs.shape[0]
    out = dict(tool='render_bench', faces=len(terrain), bvh_build_ms=build_ms, bvh_build_min_ms=build_min, poses=args.poses,
               size=list(args.size), rays=n_rays)
    for name, mesh, height, spread in (('terrain', terrain, 8.0, 60.0), ('room12', room_mesh((10.0, 7.0, 2.0), 100.0), 0.0, 3.0)):
        bvh = mesh.on_device(dev)[3]
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        face, _, _ = raycast(bvh, dirs, poses, tmin)
        ms, mn = _median_ms(lambda: raycast(bvh, dirs, poses, tmin), args.reps)
        out.update({'%s_faces' % name: len(mesh), '%s_cast_ms' % name: ms, '%s_cast_min_ms' % name: mn,
                    '%s_mrays_per_s' % name: n_rays / ms / 1e3, '%s_hit_fraction' % name: float((face >= 0).float().mean())})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
