"""The supervised cloud loss on the GPU (csrc/dc_cloudloss.hip): one evaluation -- loss and gradients to the weights and the poses --
of --poses rendered H x W scans (2 cm of depth noise, a ScaledPolynomial model) of a pillared room against surveys of two sizes
sampled from the room's mesh (SurveyCloud.from_mesh), point to plane, trimmed at 0.8, timed two ways in ONE process, alternating,
after a warm-up of every shape:

    fused    the one host call (ops.cloud_loss) on the survey's persistent grid
    unfused  the composition ops.points_fwd + ops.knn_grid_query on the same grid + ops.quantile + the torch expression for l and
             dl/dx + ops.points_bwd

The two forms are compared at the timed size in the same run (loss within 2^-40 x extent, correspondences equal).  Medians of --reps
synchronised runs.  Prints one JSON line.

    python tools/cloudloss_bench.py [--surveys 200000 2000000] [--poses 10] [--size 64 2048] [--reps 10]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/cloudloss_bench.py --reps 3      # kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from meshloss_bench import _poses, _scans, _timed          # noqa: E402  (the same scans as the mesh-loss tool)

MAX_DIST, RATIO = 0.5, 0.8


def _unfused(sd, ps, poses12, kind, w, e):
    from depth_correction_amd import ops
    x = ops.points_fwd(ps, poses12, kind, w, e)
    dist, idx = ops.knn_grid_query(sd.grid, x, sd.identity_pose(), 1, r=MAX_DIST)
    dist, idx = dist[:, 0].contiguous(), idx[:, 0]
    thr = ops.quantile(dist, RATIO)
    used = (idx >= 0) & (dist <= thr)
    m = used.sum()
    j = idx.clamp(min=0).long()
    nrm = sd.normals[j]
    r = ((x - sd.points[j]) * nrm).sum(dim=-1)
    r = torch.where(used, r, torch.zeros_like(r))
    loss = r.abs().sum() / m
    g = (torch.sign(r)[:, None] * nrm / m).contiguous()
    gw, ge, gT = ops.points_bwd(g, ps, poses12, kind, w, e, want_pose=True)
    return loss, torch.where(used, idx, torch.full_like(idx, -1)), gw, gT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--surveys', type=int, nargs='+', default=(200000, 2000000), help='survey sizes (points sampled from the mesh)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cloudloss_bench needs a GPU')
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.survey import SurveyCloud
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    out = dict(tool='cloudloss_bench', poses=args.poses, size=list(args.size), reps=args.reps, max_dist=MAX_DIST, inlier_ratio=RATIO)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    kind = 'ScaledPolynomial'
    w = torch.tensor([-0.004, 0.002], dtype=torch.float64, device=dev)
    e = torch.tensor([2.0, 4.0], dtype=torch.float64, device=dev)
    _, _, normals, bvh = room.on_device(dev)
    poses = torch.as_tensor(_poses(args.poses, 0.0, 3.0), device=dev)
    ps, scan_ptr = _scans(room, bvh, normals, poses, dirs, tmin, dev)
    poses12 = poses[:, :3, :].reshape(-1, 12).contiguous()
    ws = ops.cloud_loss_workspace(ps.n, args.poses, 2, dev)
    scenes = []
    for m in args.surveys:
        t0 = time.perf_counter()
        sd = SurveyCloud.from_mesh(room, m, seed=135, device=dev).on_device(dev).reserve(ps.n)
        torch.cuda.synchronize()
        fused = lambda sd=sd, **kw: ops.cloud_loss(sd, ps, scan_ptr, poses12, kind, w, e, plane=True, max_dist=MAX_DIST, inlier_ratio=RATIO,
                                                   ws=ws, **kw)
        scenes.append((m, sd, fused, (time.perf_counter() - t0) * 1e3))
    for m, sd, fused, _ in scenes:                          # warm-up of every shape before any is timed
        fused()
        _unfused(sd, ps, poses12, kind, w, e)
    torch.cuda.synchronize()
    for m, sd, fused, setup_ms in scenes:
        ts = {'fused': [], 'unfused': []}
        for rep in range(args.reps):
            ts['fused'].append(_timed(fused))
            ts['unfused'].append(_timed(lambda: _unfused(sd, ps, poses12, kind, w, e)))
        res = {'survey_points': sd.n, 'points': ps.n, 'survey_setup_ms': setup_ms}
        for k, v in ts.items():
            res['%s_ms' % k], res['%s_min_ms' % k] = float(np.median(v)), float(np.min(v))
        res['fused_over_unfused'] = res['fused_ms'] / res['unfused_ms']
        # the two forms at the timed size
        o, idx, dist, resid = fused(want_points=True)
        loss_u, idx_u, gw_u, gT_u = _unfused(sd, ps, poses12, kind, w, e)
        extent = float(np.max(room.bounds[1] - room.bounds[0]))
        res['loss'], res['loss_diff'], res['loss_bar'] = float(o[0]), abs(float(o[0]) - float(loss_u)), 2.0 ** -40 * extent
        res['used'], res['gated'], res['trimmed'] = int(o[1]), int(o[2]), int(o[3])
        res['idx_equal'] = bool(torch.equal(idx, idx_u))
        res['grad_w_rel_diff'] = float((o[6:8] - gw_u).abs().max() / gw_u.abs().max())
        res['grad_pose_rel_diff'] = float((o[10:].reshape(-1, 3, 4) - gT_u).abs().max() / gT_u.abs().max())
        assert res['loss_diff'] <= res['loss_bar'] and res['idx_equal'], res
        out['survey_%d' % m] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
