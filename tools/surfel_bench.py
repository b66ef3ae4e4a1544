"""Surfel ray casting on the GPU (csrc/dc_raycast.hip dc_surfel_bvh_build / dc_surfel_cast_rays): surveys of --samples points sampled
from the pillared room of tools/bias_bench.py and from a >= 1 M-triangle grid_terrain_mesh, every point a disk whose radius is the
distance to its --k-th nearest other point; --poses poses x --size pattern measured rays (vps = 0).  Timed: the build (radii given),
the k-NN radii beside it, the first-hit cast (window = 0), the blended cast (--window), and dc_raycast_rays of the same rays against
the mesh the survey was sampled from.  Beside the times: how many rays hit, the disks blended per ray, and the difference of the
surfel depths to the mesh's.  Median, min and max of --reps synchronised runs in a warm process.  Prints one JSON line.

    python tools/surfel_bench.py [--samples 200000 2000000] [--n 710] [--poses 10] [--size 64 2048] [--k 10] [--window 0.1] [--reps 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/surfel_bench.py --reps 3      # kernel times
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, nargs='+', default=(200000, 2000000))
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--window', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('surfel_bench needs a GPU')
    from bias_bench import _poses, _stats_ms
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.ops import knn, raycast_rays, surfel_bvh_build, surfel_cast_rays
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.survey import SurveyCloud
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs1 = torch.as_tensor(np.array(d), device=dev)
    R, tmin0 = dirs1.shape[0], float(np.max(t_min))
    out = dict(tool='surfel_bench', poses=args.poses, size=list(args.size), k=args.k, window=args.window, reps=args.reps)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    for name, mesh, height, spread in (('room', room, 0.0, 3.0), ('terrain', grid_terrain_mesh(args.n), 8.0, 60.0)):
        bvh_mesh = mesh.on_device(dev)[3]
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        P = poses.shape[0]
        dirs = dirs1.repeat(P, 1).contiguous()
        vps = torch.zeros_like(dirs)
        off = torch.arange(P + 1, dtype=torch.int64, device=dev) * R
        face, t_mesh, _ = raycast_rays(bvh_mesh, vps, dirs, off, poses, t_min=tmin0)
        res = dict(faces=len(mesh), rays=int(face.numel()), mesh_hits=int((face >= 0).sum()),
                   raycast_rays_ms=_stats_ms(lambda: raycast_rays(bvh_mesh, vps, dirs, off, poses, t_min=tmin0), args.reps))
        for m in args.samples:
            survey = SurveyCloud.from_mesh(mesh, m, device=dev).on_device(dev)
            box = torch.cat([survey.points.amin(dim=0), survey.points.amax(dim=0)]).cpu().numpy()
            radii = knn(survey.points, args.k + 1)[0][:, args.k].contiguous()
            bvh = surfel_bvh_build(survey.points, survey.normals, radii, box)
            index, t_first, _, _, _ = surfel_cast_rays(bvh, vps, dirs, off, poses, t_min=tmin0)
            _, _, t, _, count = surfel_cast_rays(bvh, vps, dirs, off, poses, t_min=tmin0, window=args.window)
            both = (index >= 0) & (face >= 0)
            diff_first, diff = (t_first - t_mesh)[both], (t - t_mesh)[both]
            near = diff_first.abs() < 0.5                    # the same surface: not a silhouette's overhang, not a gap
            r = dict(samples=m, radius_median=float(radii.median()), hits=int((index >= 0).sum()), hits_both=int(both.sum()),
                     same_surface=int(near.sum()), count_mean=float(count[index >= 0].double().mean()), count_max=int(count.max()),
                     first_minus_mesh_mean=float(diff_first[near].mean()), first_minus_mesh_rms=float(diff_first[near].square().mean().sqrt()),
                     blend_minus_mesh_mean=float(diff[near].mean()), blend_minus_mesh_rms=float(diff[near].square().mean().sqrt()),
                     knn_radii_ms=_stats_ms(lambda: knn(survey.points, args.k + 1), max(3, args.reps // 4)),
                     build_ms=_stats_ms(lambda: surfel_bvh_build(survey.points, survey.normals, radii, box), args.reps),
                     cast_first_ms=_stats_ms(lambda: surfel_cast_rays(bvh, vps, dirs, off, poses, t_min=tmin0), args.reps),
                     cast_blend_ms=_stats_ms(lambda: surfel_cast_rays(bvh, vps, dirs, off, poses, t_min=tmin0, window=args.window), args.reps))
            r['first_over_mesh'] = r['cast_first_ms']['median'] / res['raycast_rays_ms']['median']
            r['blend_over_first'] = r['cast_blend_ms']['median'] / r['cast_first_ms']['median']
            res['survey_%d' % m] = r
            del bvh, survey, radii
        out[name] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
