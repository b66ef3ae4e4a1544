"""Survey registration on the GPU (csrc/dc_align.hip): the map of --poses rendered H x W scans (2 cm of depth noise) of a pillared
room, moved out of the survey's frame by a known transform (2 degrees, 12 cm), registered to surveys of two sizes sampled from the
room's mesh -- --iters iterations, trimmed at 0.8, convergence checks off so that both forms run every iteration -- timed two ways
in ONE process, alternating, after a warm-up of every shape:

    native    the one host call (ops.survey_align): every iteration queued on the stream, no host read in between
    unfused   per iteration ops.knn_grid_query + ops.quantile + torch masked sums of the pair moments, one host read, the closed-form
              fit on the host (means + SVD, the reference's route) and the pose written back to the device

and the k-NN query alone (--iters queries under the start pose and under the final estimate: the search is cheaper the better the
clouds are aligned) for its share of the native iteration.  The two forms are compared
at the timed size in the same run: the registered map points agree within 2^-40 x extent.  Medians of --reps synchronised runs.
Prints one JSON line.

    python tools/align_bench.py [--surveys 200000 2000000] [--poses 10] [--size 64 2048] [--iters 30] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/align_bench.py --native-only --surveys 2000000 --reps 3    # kernel times
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from meshloss_bench import _poses, _scans, _timed          # noqa: E402  (the same scans as the mesh-loss tool)

MAX_DIST, RATIO = 0.5, 0.8


def _offset():
    a = np.array([0.3, -0.2, 1.0])
    a /= np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(math.radians(2.0)) * K + (1.0 - math.cos(math.radians(2.0))) * (K @ K)
    T[:3, 3] = (0.08, -0.07, 0.05)
    return T


def _host_fit(W, a, b, S):
    """Route A from the (uncentred) moments of the kept pairs: means, cross-covariance, SVD with the determinant fix."""
    mp, my = a / W, b / W
    H = (S - np.outer(a, b) / W).T                   # sum (y - my)(p - mp)^T
    U, _, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, my - R @ mp
    return T


def _unfused(sd, q, origins, iters):
    from depth_correction_amd import ops
    pose = torch.eye(4, dtype=torch.float64, device=q.device)
    o = origins.cpu().numpy()
    qc = q - origins[:3]
    T = np.eye(4)
    for _ in range(iters):
        dist, idx = ops.knn_grid_query(sd.grid, q, pose, 1, r=MAX_DIST)
        dist, idx = dist[:, 0].contiguous(), idx[:, 0]
        thr = ops.quantile(dist, RATIO)
        kept = ((idx >= 0) & (dist <= thr)).to(torch.float64)
        yc = (sd.points[idx.clamp(min=0).long()] - origins[3:]) * kept[:, None]
        pk = qc * kept[:, None]
        m = torch.cat([kept.sum()[None], pk.sum(dim=0), yc.sum(dim=0), (pk.t() @ yc).reshape(-1)]).cpu().numpy()   # the host read
        Tc = _host_fit(m[0], m[1:4], m[4:7], m[7:16].reshape(3, 3))      # between the centred frames
        T = np.eye(4)
        T[:3, :3] = Tc[:3, :3]
        T[:3, 3] = o[3:] + Tc[:3, 3] - Tc[:3, :3] @ o[:3]
        pose.copy_(torch.as_tensor(T))
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--surveys', type=int, nargs='+', default=(200000, 2000000), help='survey sizes (points sampled from the mesh)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--native-only', action='store_true', help='time the native form alone (for a kernel trace of it)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('align_bench needs a GPU')
    from depth_correction_amd import _native as nv
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.survey import SurveyCloud
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    out = dict(tool='align_bench', poses=args.poses, size=list(args.size), reps=args.reps, iters=args.iters, max_dist=MAX_DIST,
               inlier_ratio=RATIO)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    _, _, normals, bvh = room.on_device(dev)
    poses = torch.as_tensor(_poses(args.poses, 0.0, 3.0), device=dev)
    ps, _ = _scans(room, bvh, normals, poses, dirs, tmin, dev)
    world = ops.points_fwd(ps, poses[:, :3, :].reshape(-1, 12).contiguous(), None, None, None).to(torch.float64)
    Ti = torch.as_tensor(np.linalg.inv(_offset()), device=dev)
    q = (world @ Ti[:3, :3].t() + Ti[:3, 3]).contiguous()
    n = q.shape[0]
    extent = float(np.max(room.bounds[1] - room.bounds[0]))
    bar = 2.0 ** -40 * extent
    ws = ops.survey_align_workspace(n, dev)
    state = torch.empty((nv.DC_ALIGN_STATE_COUNT,), dtype=torch.float64, device=dev)
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    history = torch.empty((args.iters, nv.DC_ALIGN_HISTORY_COLS), dtype=torch.float64, device=dev)
    o_p = 0.5 * (q.amin(dim=0) + q.amax(dim=0))
    idx = torch.empty((n, 1), dtype=torch.int32, device=dev)
    dist = torch.empty((n, 1), dtype=torch.float64, device=dev)
    scenes = []
    for m in args.surveys:
        sd = SurveyCloud.from_mesh(room, m, seed=135, device=dev).on_device(dev).reserve(n)
        origins = torch.cat([o_p, sd.origin()]).contiguous()
        native = lambda sd=sd, origins=origins: ops.survey_align(sd, q, origins, inlier_ratio=RATIO, max_dist=MAX_DIST, n_iters=args.iters,
                                                                 state=state, status=status, history=history, ws=ws)
        scenes.append((m, sd, origins, native))
    for m, sd, origins, native in scenes:                   # warm-up of every shape before any is timed
        native()
        if not args.native_only:
            _unfused(sd, q, origins, 2)
    torch.cuda.synchronize()
    if args.native_only:
        for m, sd, origins, native in scenes:
            ts = [_timed(native) / args.iters for _ in range(args.reps)]
            out['survey_%d' % m] = {'survey_points': sd.n, 'points': n, 'native_ms_per_iter': float(np.median(ts))}
        print(json.dumps(out))
        return

    def queries(sd, pose):
        for _ in range(args.iters):
            ops.knn_grid_query(sd.grid, q, pose, 1, r=MAX_DIST, idx=idx, dist=dist)

    for m, sd, origins, native in scenes:
        native()
        final = state[:16].reshape(4, 4).clone()            # the search is cheaper the better the clouds are aligned: time both ends
        queries(sd, final)
        torch.cuda.synchronize()
        ts = {'native': [], 'unfused': [], 'query_start_pose': [], 'query_final_pose': []}
        for rep in range(args.reps):
            ts['native'].append(_timed(native) / args.iters)
            ts['unfused'].append(_timed(lambda: _unfused(sd, q, origins, args.iters)) / args.iters)
            ts['query_start_pose'].append(_timed(lambda: queries(sd, sd.identity_pose())) / args.iters)
            ts['query_final_pose'].append(_timed(lambda: queries(sd, final)) / args.iters)
        res = {'survey_points': sd.n, 'points': n}
        for k, v in ts.items():
            res['%s_ms_per_iter' % k], res['%s_min_ms_per_iter' % k] = float(np.median(v)), float(np.min(v))
        res['native_over_unfused'] = res['native_ms_per_iter'] / res['unfused_ms_per_iter']
        res['query_share_of_native'] = res['query_final_pose_ms_per_iter'] / res['native_ms_per_iter']
        # the two forms at the timed size
        native()
        torch.cuda.synchronize()
        Tn = state[:16].reshape(4, 4).cpu().numpy()
        code = status.cpu().numpy()
        Tu = _unfused(sd, q, origins, args.iters)
        qs = q[::97].cpu().numpy()
        diff = float(np.abs((qs @ Tn[:3, :3].T + Tn[:3, 3]) - (qs @ Tu[:3, :3].T + Tu[:3, 3])).max())
        back = float(np.abs(Tn @ np.linalg.inv(_offset()) - np.eye(4)).max())
        h = history.cpu().numpy()
        res.update(status=nv.ALIGN_STATUS[int(code[0])], iterations=int(code[1]), pairs=float(h[-1, 0]), rms=float(h[-1, 1]),
                   last_d_rot=float(h[-1, 3]), last_d_trans=float(h[-1, 4]), native_vs_unfused_points=diff, bar=bar,
                   distance_to_true_transform=back)
        out['survey_%d' % m] = res
    print(json.dumps(out))
    for m in args.surveys:
        res = out['survey_%d' % m]
        assert res['native_vs_unfused_points'] <= res['bar'], res


if __name__ == '__main__':
    main()
