"""Moving-sweep rendering and de-skew on the GPU (csrc/dc_raycast.hip dc_raycast_sweep / dc_sweep_rays, csrc/dc_sweep.hip dc_deskew):
--poses poses x --size rays against a >= 1 M-triangle grid_terrain_mesh and a pillared room_mesh,
(a) dc_raycast_sweep at zero twist next to the thin dc_raycast_rays on the same rays (their results are compared: equal),
(b) dc_raycast_sweep under a twist of 0.5 m and 0.2 rad next to the composition dc_sweep_rays + dc_raycast_rays (compared: equal),
(c) dc_deskew of the resulting points next to a torch composition (per-point axis_angle_to_matrix + bmm + the translation).
Median, min and max of --reps synchronised runs in a warm process, the variants interleaved.  Prints one JSON line.

    python tools/sweep_bench.py [--n 710] [--poses 10] [--size 64 2048] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/sweep_bench.py --reps 2      # kernel times
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bias_bench import _poses, _stats_ms          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sweep_bench needs a GPU')
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.ops import deskew, raycast_rays, raycast_sweep, sweep_rays
    from depth_correction_amd.render import SweepModel, lidar_directions
    from depth_correction_amd.transform import axis_angle_to_matrix
    dev = torch.device('cuda:0')
    fov = (45.0, 360.0)
    d, t_min = lidar_directions(size=args.size, fov=fov, num_segments=args.segments)
    tau1 = SweepModel.sweep_times(d, fov, 'ccw')
    R, tmin0 = d.shape[0], float(np.max(t_min))                           # one near clip everywhere: dc_raycast_rays takes a scalar
    out = dict(tool='sweep_bench', poses=args.poses, size=list(args.size), reps=args.reps)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    merge = lambda rs: dict(median=float(np.median([r['median'] for r in rs])), min=min(r['min'] for r in rs), max=max(r['max'] for r in rs),
                            medians=[r['median'] for r in rs])
    same = lambda a, b: all(torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)) for x, y in zip(a, b))
    for name, mesh, height, spread in (('terrain', grid_terrain_mesh(args.n), 8.0, 60.0), ('room', room, 0.0, 3.0)):
        bvh = mesh.on_device(dev)[3]
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        P = poses.shape[0]
        dirs = torch.as_tensor(np.array(d), device=dev).repeat(P, 1).contiguous()
        tau = torch.as_tensor(tau1, device=dev).repeat(P).contiguous()
        vps = torch.zeros_like(dirs)
        off = torch.arange(P + 1, dtype=torch.int64, device=dev) * R
        zero = np.zeros((P, 6))
        moving = np.tile(np.array([0.4, 0.3, 0.0, 0.0, 0.0, 0.2]), (P, 1))
        thin = lambda: raycast_rays(bvh, vps, dirs, off, poses, t_min=tmin0)
        still = lambda: raycast_sweep(bvh, vps, dirs, tau, off, poses, zero, t_min=tmin0)
        fused = lambda: raycast_sweep(bvh, vps, dirs, tau, off, poses, moving, t_min=tmin0)

        def composed():
            o, D = sweep_rays(vps, dirs, tau, off, moving)
            return raycast_rays(bvh, o, D, off, poses, t_min=tmin0)
        res = dict(faces=len(mesh), rays=int(dirs.shape[0]), still_equals_thin=same(still(), thin()), fused_equals_composed=same(fused(), composed()))
        face, t, _ = fused()
        res['hits'] = int((face >= 0).sum())
        pts = (torch.where(face >= 0, t, torch.zeros_like(t))[:, None] * dirs).contiguous()
        tw_d = torch.as_tensor(moving, device=dev)
        scan = torch.arange(P, device=dev).repeat_interleave(R)

        def torch_deskew():
            Rm = axis_angle_to_matrix(tau[:, None] * tw_d[scan, 3:])
            return torch.bmm(Rm, pts[:, :, None])[:, :, 0] + tau[:, None] * tw_d[scan, :3]
        kernel_deskew = lambda: deskew(pts, tau, off, moving)
        res['deskew_max_diff_m'] = float((kernel_deskew()[0] - torch_deskew()).abs().max())
        ts = {k: [] for k in ('thin', 'still', 'fused', 'composed', 'deskew', 'torch_deskew')}
        for _ in range(3):                                                # interleaved: a drift of the machine's load meets all alike
            for k, fn in (('thin', thin), ('still', still), ('fused', fused), ('composed', composed), ('deskew', kernel_deskew),
                          ('torch_deskew', torch_deskew)):
                ts[k].append(_stats_ms(fn, args.reps))
        for k, v in ts.items():
            res[k + '_ms'] = merge(v)
        med = lambda k: res[k + '_ms']['median']
        res['rays_per_s'] = res['rays'] / (med('fused') * 1e-3)
        res['still_over_thin'] = med('still') / med('thin')
        res['fused_over_composed'] = med('fused') / med('composed')
        res['deskew_over_torch'] = med('deskew') / med('torch_deskew')
        res['sweep_rays_ms'] = _stats_ms(lambda: sweep_rays(vps, dirs, tau, off, moving), 3)
        print('%s: %s' % (name, json.dumps(res)), file=sys.stderr, flush=True)
        out[name] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
