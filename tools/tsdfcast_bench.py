"""Ray casting the fused volume on the GPU (csrc/dc_tsdf_cast.hip), on the bench room of tools/recon_bench.py: --poses rendered H x W
scans of the pillared room fused into a sparse volume at --voxel, then the room's own rays (every scan, at its pose) cast against that
volume.  Device events, medians of --reps runs in a warm process.  It reports, it does not gate:

  (a) the cast with skipping of absent blocks next to the naive march of every sample (skip=False), whose outputs must EQUAL it
      (asserted, all but the sample counts);
  (b) the composition a user has without the cast: extract_mesh + BVH build + raycast_rays on the extracted mesh -- the composition's
      cast alone, and with its set-up;
  (c) raycast_rays of the same rays against the ground-truth room, as context;
  (d) samples per ray and the status counts; t against the ground truth for the rays both hit.

Prints one JSON line.

    python tools/tsdfcast_bench.py [--poses 10] [--size 64 2048] [--voxel 0.05] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recon_bench import _cloud, _event_ms, _poses  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--voxel', type=float, default=0.05)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--t-max', type=float, default=20.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tsdfcast_bench needs a GPU')
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs1, tmin = torch.as_tensor(np.array(d), device=dev).contiguous(), torch.as_tensor(np.array(t_min), device=dev)
    poses = torch.as_tensor(_poses(args.poses, 3.0), device=dev)
    room_bvh = room.on_device(dev)[3]
    face, depth, _ = ops.raycast(room_bvh, dirs1, poses, tmin)
    depth = torch.where(face >= 0, depth, torch.full_like(depth, float('inf'))).contiguous()
    vps1 = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    vol = SparseTsdfVolume(args.voxel, device=dev)
    for p in range(args.poses):
        vol.integrate(_cloud(vps1, dirs1, depth[p]), pose=poses[p])
    rays = dirs1.shape[0]
    n = rays * args.poses
    dirs = dirs1.repeat(args.poses, 1).contiguous()
    vps = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    off = torch.arange(args.poses + 1, dtype=torch.int64, device=dev) * rays
    tables = vol.tables()
    out = dict(tool='tsdfcast_bench', poses=args.poses, size=list(args.size), rays=n, voxel=args.voxel, step=args.voxel / 2, t_max=args.t_max,
               blocks=vol.n_blocks, reps=args.reps)
    res = {}
    for skip in (True, False):
        buf = ops.tsdf_sparse_cast_rays(tables, vps, dirs, off, poses, t_max=args.t_max, skip=skip)
        ms, ms_min = _event_ms(lambda: ops.tsdf_sparse_cast_rays(tables, vps, dirs, off, poses, t_max=args.t_max, skip=skip, out=buf),
                               args.reps if skip else max(2, args.reps // 3))
        res[skip] = {k: v.clone() for k, v in buf.items()}
        key = 'cast' if skip else 'cast_naive'
        out[key + '_ms'], out[key + '_min_ms'] = ms, ms_min
        out[key + '_samples_per_ray'] = float(res[skip]['samples'].double().mean())
        out[key + '_samples_max'] = int(res[skip]['samples'].max())
    for k in ('face', 't', 'inc', 'normal', 'phi', 'status'):
        a, b = res[True][k], res[False][k]
        assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), 'skip and naive differ in ' + k
    out['equal'] = True
    out['naive_over_skip'] = out['cast_naive_ms'] / out['cast_ms']
    status = res[True]['status']
    out['status'] = {name: int((status == code).sum()) for name, code in (('hit', 0), ('skipped', 1), ('miss', 2), ('behind', 3), ('lost', 4))}
    out['mrays_per_s'] = n / out['cast_ms'] / 1e3
    # the composition without the cast: extraction, tree, mesh cast
    state = {}

    def setup():
        mesh = vol.extract_mesh()
        state['mesh'], state['bvh'] = mesh, mesh.on_device(dev)[3]

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(max(2, args.reps // 3) + 1):
        torch.cuda.synchronize()
        e0.record()
        setup()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    out['composition_setup_ms'] = float(np.median(times[1:]))
    out['composition_faces'] = len(state['mesh'])
    cast_mesh = lambda: ops.raycast_rays(state['bvh'], vps, dirs, off, poses)
    out['composition_cast_ms'], out['composition_cast_min_ms'] = _event_ms(cast_mesh, args.reps)
    out['composition_total_ms'] = out['composition_setup_ms'] + out['composition_cast_ms']
    out['cast_over_composition_cast'] = out['cast_ms'] / out['composition_cast_ms']
    out['ground_truth_cast_ms'], out['ground_truth_cast_min_ms'] = _event_ms(lambda: ops.raycast_rays(room_bvh, vps, dirs, off, poses), args.reps)
    f_gt, t_gt, inc_gt = ops.raycast_rays(room_bvh, vps, dirs, off, poses)
    both = (status == 0) & (f_gt >= 0)
    dt = (res[True]['t'][both] - t_gt[both]).cpu().numpy()
    di = (res[True]['inc'][both] - inc_gt[both]).cpu().numpy()
    q = lambda x: [float(v) for v in np.quantile(x, [0.05, 0.25, 0.5, 0.75, 0.95])] if x.size else []
    out.update(both_hit=int(both.sum()), dt_quantiles=q(dt), dt_rms=float(np.sqrt((dt ** 2).mean())) if dt.size else None,
               dinc_quantiles=q(di), dinc_rms=float(np.sqrt((di ** 2).mean())) if di.size else None)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
