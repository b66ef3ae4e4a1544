"""Map accuracy on the GPU (csrc/dc_meshdist.hip): the closest-point query for (a) the points of --poses rendered H x W scans with
2 cm of Gaussian noise, (b) as many points uniform in the scene box (far from the surface: long traversals), against a
>= 1 M-triangle grid_terrain_mesh and against a pillared room_mesh, and (c) mesh.sample of --samples points.  Next to (a) the ray
cast of the same scans on the same mesh and the chamfer distance of the same points to a --samples-point sampled cloud, which
are what the numbers are read against.  Medians of --reps synchronised runs in a warm process.  Prints one JSON line.

    python tools/mesh_bench.py [--n 710] [--poses 10] [--size 128 2048] [--samples 10000000] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/mesh_bench.py --reps 3      # kernel times
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
    ap.add_argument('--samples', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mesh_bench needs a GPU')
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.metrics import chamfer_distance
    from depth_correction_amd.ops import mesh_closest, raycast
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    out = dict(tool='mesh_bench', poses=args.poses, size=list(args.size), samples=args.samples, reps=args.reps)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    for name, mesh, height, spread in (('terrain', grid_terrain_mesh(args.n), 8.0, 60.0), ('room', room, 0.0, 3.0)):
        verts, faces, _, bvh = mesh.on_device(dev)
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        face, t, _ = raycast(bvh, dirs, poses, tmin)
        cast_ms, _ = _median_ms(lambda: raycast(bvh, dirs, poses, tmin), args.reps)
        hit = face >= 0
        world_dirs = torch.einsum('pij,rj->pri', poses[:, :3, :3], dirs)
        pts = (poses[:, None, :3, 3] + t[..., None].nan_to_num(posinf=0.0) * world_dirs)[hit]
        gen = torch.Generator(device=dev).manual_seed(135)
        scan = (pts + 0.02 * torch.randn(pts.shape, dtype=torch.float64, device=dev, generator=gen)).contiguous()
        lo, hi = (torch.as_tensor(b, device=dev) for b in mesh.bounds)
        uniform = (lo + (hi - lo) * torch.rand(scan.shape, dtype=torch.float64, device=dev, generator=gen)).contiguous()
        res = {'faces': len(mesh), 'rays': int(hit.numel()), 'points': int(scan.shape[0]), 'cast_ms': cast_ms}
        for what, q in (('scan', scan), ('uniform', uniform)):
            _, dist, _ = mesh_closest(bvh, q)
            ms, mn = _median_ms(lambda: mesh_closest(bvh, q), args.reps)
            res.update({'closest_%s_ms' % what: ms, 'closest_%s_min_ms' % what: mn, 'closest_%s_mpoints_per_s' % what: q.shape[0] / ms / 1e3,
                        'closest_%s_mean_dist' % what: float(dist.mean())})
        sample_ms, sample_min = _median_ms(lambda: mesh.sample(args.samples, seed=135, device=dev), args.reps)
        cloud = mesh.sample(args.samples, seed=135, device=dev)[0]
        chamfer_ms, _ = _median_ms(lambda: chamfer_distance(scan, cloud, apply_point_reduction=False), max(3, args.reps // 3))
        res.update({'sample_ms': sample_ms, 'sample_min_ms': sample_min, 'sample_mpoints_per_s': args.samples / sample_ms / 1e3,
                    'chamfer_scan_ms': chamfer_ms})
        out[name] = res
        del cloud
    print(json.dumps(out))


if __name__ == '__main__':
    main()
