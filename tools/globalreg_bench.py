"""Global registration on the GPU (csrc/dc_globalreg.hip, registration.register_global): the map of --poses rendered H x W scans (2 cm
of depth noise) of a pillared room, moved out of the survey's frame by 140 degrees and 3 m, registered WITHOUT a prior to surveys of
two sizes sampled from the room's mesh, with default arguments.  Timed in ONE process after a warm-up of every shape, medians of
--reps synchronised runs, the variants of a stage alternating:

    stages       voxel filter, normals, k-NN, dc_pair_spfh, dc_pair_fpfh, dc_feature_nn, dc_greg_fit, dc_greg_score (with the compaction
                 of the valid list), the M fitness queries, the refinement, and the whole call (the survey's side cached, as it is
                 from the second call on; its one-time cost is reported beside)
    matching     against torch.cdist + argmin over the same rows (fp32; another rounding and no tie rule: the share of equal indices
                 is reported)
    fit + score  against a batched torch restatement on the device: the draws in int64 arithmetic, the edge check over all K, the
                 valid triples fitted by torch.linalg.svd, the scores by chunked [V, C] distance counts

and reports the points after the filter, the share of right matches (within eps of the true position), the valid hypotheses, the
winner and its distance to the true transform.  Prints one JSON line.

    python tools/globalreg_bench.py [--surveys 200000 2000000] [--poses 10] [--size 64 2048] [--reps 5]
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

M64 = (1 << 64) - 1


def _offset():
    a = np.array([0.3, -0.2, 1.0])
    a /= np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = math.radians(140.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    T[:3, 3] = (2.0, -2.0, 1.0)                        # 3 m
    return T


def _i64(v):
    v &= M64
    return v - (1 << 64) if v >= 1 << 63 else v


def _lsr(z, s):
    """Logical shift right of int64 words."""
    return (z >> s) & ((1 << (64 - s)) - 1)


def _torch_draws(seed, K, C, dev):
    """The three draws of every hypothesis in int64 arithmetic (wrapping products, logical shifts, an unsigned remainder)."""
    h = torch.arange(K, dtype=torch.int64, device=dev)
    out = []
    for t in range(3):
        z = (_i64(seed) ^ (h << 2) ^ t) + _i64(0x9E3779B97F4A7C15)
        z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
        z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
        z = z ^ _lsr(z, 31)
        r = torch.remainder(z, C)
        out.append(torch.where(z < 0, torch.remainder(r + (1 << 64) % C, C), r))
    return torch.stack(out, dim=1)


def _torch_fit_score(P, Y, K, seed, min_edge, rho, eps, chunk=2048):
    """(valid bool [K], score int32 [K]) by batched torch operations on the device."""
    C = P.shape[0]
    j = _torch_draws(seed, K, C, P.device)
    ok = (j[:, 0] != j[:, 1]) & (j[:, 0] != j[:, 2]) & (j[:, 1] != j[:, 2])
    p, y = P[j], Y[j]                                   # [K, 3, 3]
    for a, b in ((0, 1), (1, 2), (2, 0)):
        lp, ly = (p[:, a] - p[:, b]).norm(dim=1), (y[:, a] - y[:, b]).norm(dim=1)
        ok &= (lp >= min_edge) & (lp >= rho * ly) & (ly >= rho * lp)
    rows = torch.nonzero(ok).reshape(-1)
    p, y = p[rows], y[rows]
    mp, my = p.mean(dim=1, keepdim=True), y.mean(dim=1, keepdim=True)
    H = (y - my).transpose(1, 2) @ (p - mp)
    U, s, Vt = torch.linalg.svd(H)
    d = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1))
    R = U @ D @ Vt
    t = my[:, 0] - (R @ mp.transpose(1, 2))[:, :, 0]
    good = 2.0 * (s[:, 1] + d * s[:, 2]) > 1e-12 * s.sum(dim=1)
    score = torch.full((K,), -1, dtype=torch.int32, device=P.device)
    for a in range(0, rows.shape[0], chunk):
        x = P[None] @ R[a:a + chunk].transpose(1, 2) + t[a:a + chunk, None]
        score[rows[a:a + chunk]] = ((x - Y[None]).square().sum(dim=2) <= eps * eps).sum(dim=1).to(torch.int32)
    valid = torch.zeros((K,), dtype=torch.bool, device=P.device)
    valid[rows] = good
    score[rows[~good]] = -1
    return valid, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--surveys', type=int, nargs='+', default=(200000, 2000000), help='survey sizes (points sampled from the mesh)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('globalreg_bench needs a GPU')
    from depth_correction_amd import _native as nv
    from depth_correction_amd import ops
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.registration import global_descriptors, register_cloud, register_global
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.survey import SurveyCloud
    dev = torch.device('cuda:0')
    lib, ptr, stream = nv.lib(), nv.ptr, nv.stream_ptr
    voxel, k_tab, K, n_cand, seed, rho = 0.25, 64, 2 ** 20, 16, 135, 0.9
    radius, eps, min_edge = 6 * voxel, 0.6 * voxel, 4 * voxel
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    _, _, normals, bvh = room.on_device(dev)
    poses = torch.as_tensor(_poses(args.poses, 0.0, 3.0), device=dev)
    ps, _ = _scans(room, bvh, normals, poses, dirs, tmin, dev)
    world = ops.points_fwd(ps, poses[:, :3, :].reshape(-1, 12).contiguous(), None, None, None).to(torch.float64)
    T_true = _offset()
    Ti = torch.as_tensor(np.linalg.inv(T_true), device=dev)
    q = (world @ Ti[:3, :3].t() + Ti[:3, 3]).contiguous()
    Tt = torch.as_tensor(T_true, device=dev)
    out = dict(tool='globalreg_bench', poses=args.poses, size=list(args.size), reps=args.reps, points=q.shape[0], voxel=voxel,
               n_hypotheses=K, eps=eps, min_edge=min_edge)

    def med(fn):
        return float(np.median([_timed(fn) for _ in range(args.reps)]))

    def med2(fa, fb):                                   # two variants of one stage, alternating
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(_timed(fa))
            tb.append(_timed(fb))
        return float(np.median(ta)), float(np.median(tb))

    # ---- the cloud's side, stage by stage (every stage run once before it is timed) ----
    keep = ops.voxel_filter(q, voxel, preserve_order=True)
    fp = q[keep].contiguous()
    n = fp.shape[0]

    def est_normals():
        c = DepthCloud.from_points(fp)
        c.update_all(k=10, r=None)
        return c.normals.detach().to(torch.float64).contiguous()
    fn = est_normals()
    dist, idx = ops.knn(fp, k_tab, r=radius)
    idx = torch.where(idx == torch.arange(n, dtype=torch.int32, device=dev)[:, None], torch.full_like(idx, -1), idx).contiguous()
    spfh = torch.empty((n, 33), dtype=torch.float64, device=dev)
    m = torch.empty((n,), dtype=torch.int32, device=dev)
    feat = torch.empty((n, 33), dtype=torch.float32, device=dev)
    has = torch.empty((n,), dtype=torch.int32, device=dev)
    run_spfh = lambda: nv.check(lib.dc_pair_spfh(ptr(fp), ptr(fn), n, ptr(idx), k_tab, ptr(spfh), ptr(m), stream()), 'dc_pair_spfh')
    run_fpfh = lambda: nv.check(lib.dc_pair_fpfh(ptr(fp), ptr(fn), n, ptr(idx), k_tab, ptr(spfh), ptr(feat), ptr(has), stream()), 'dc_pair_fpfh')
    run_spfh()
    run_fpfh()
    torch.cuda.synchronize()
    out['cloud'] = dict(points_after_filter=n, with_descriptor=int(has.sum()),
                        filter_ms=med(lambda: ops.voxel_filter(q, voxel, preserve_order=True)), normals_ms=med(est_normals),
                        knn_ms=med(lambda: ops.knn(fp, k_tab, r=radius)), spfh_ms=med(run_spfh), fpfh_ms=med(run_fpfh))
    for size in args.surveys:
        sv = SurveyCloud.from_mesh(room, size, seed=135, device=dev)
        sd = sv.on_device(dev)
        res = dict(survey_points=sd.n)
        res['survey_side_once_ms'] = _timed(lambda: sv.global_descriptors(dev, voxel, 64, radius))
        sp, _, sfeat, shas = sv.global_descriptors(dev, voxel, 64, radius)
        res['survey_points_after_filter'] = sp.shape[0]
        res['survey_side_again_ms'] = med(lambda: global_descriptors(sd.points, sd.normals, voxel, 64, radius))
        # matching
        midx, _ = ops.feature_nn(feat, has, sfeat, shas)
        qrows, srows = torch.nonzero(has).reshape(-1), torch.nonzero(shas).reshape(-1)

        def cdist_match():
            return srows[torch.cdist(feat[qrows], sfeat[srows]).argmin(dim=1)]
        alt = cdist_match()
        res['matching_ms'], res['matching_cdist_ms'] = med2(lambda: ops.feature_nn(feat, has, sfeat, shas), cdist_match)
        res['matching_cdist_equal_share'] = float((alt == midx[qrows].long()).double().mean())
        rows = torch.nonzero(midx >= 0).reshape(-1)
        P, Y = fp[rows].contiguous(), sp[midx[rows].long()].contiguous()
        C = P.shape[0]
        right = ((P @ Tt[:3, :3].t() + Tt[:3, 3]) - Y).norm(dim=1) <= eps
        res.update(correspondences=C, right_share=float(right.double().mean()))
        # fit and score
        origins = torch.cat([0.5 * (q.amin(dim=0) + q.amax(dim=0)), sd.origin()]).contiguous()
        valid, T = ops.greg_fit(P, Y, origins, K, seed, min_edge, rho)
        score = ops.greg_score(valid, T, P, Y, eps)
        tv, ts = _torch_fit_score(P, Y, K, seed, min_edge, rho, eps)
        res['fit_ms'] = med(lambda: ops.greg_fit(P, Y, origins, K, seed, min_edge, rho))
        res['score_ms'] = med(lambda: ops.greg_score(valid, T, P, Y, eps))
        res['fit_score_ms'], res['fit_score_torch_ms'] = med2(
            lambda: ops.greg_score(*ops.greg_fit(P, Y, origins, K, seed, min_edge, rho), P, Y, eps),
            lambda: _torch_fit_score(P, Y, K, seed, min_edge, rho, eps))
        res.update(valid=int(valid.sum()), valid_equal=bool(torch.equal(valid != 0, tv)),
                   score_equal_share=float((score == ts).double().mean()), best_score=int(score.max()))
        # the fitness queries of the candidates
        sd.reserve(n)
        cand = torch.topk(score.to(torch.int64), min(n_cand, int(valid.sum()))).indices
        Tc = T[cand].contiguous()
        i1 = torch.empty((n, 1), dtype=torch.int32, device=dev)
        d1 = torch.empty((n, 1), dtype=torch.float64, device=dev)

        def fitness():
            for c in range(Tc.shape[0]):
                ops.knn_grid_query(sd.grid, fp, Tc[c], 1, r=eps, idx=i1, dist=d1)
        fitness()
        res['fitness_ms'] = med(fitness)
        # the whole call, and the refinement alone
        reg = register_global(q, sv)
        res['whole_ms'], res['whole_coarse_only_ms'] = med2(lambda: register_global(q, sv), lambda: register_global(q, sv, refine=False))
        res['refine_ms'] = med(lambda: register_cloud(q, sv, init=reg.T_coarse, max_dist=2 * voxel))
        dT = reg.T @ np.linalg.inv(T_true)
        qs = q[::97].cpu().numpy()
        res.update(status=reg.status, hypothesis=reg.hypothesis, score=reg.score, fitness=reg.fitness, n_valid=reg.n_valid,
                   refined_status=reg.refined.status, refined_iterations=reg.refined.iterations,
                   coarse_point_error=float(np.linalg.norm((qs @ reg.T_coarse[:3, :3].T + reg.T_coarse[:3, 3])
                                                           - (qs @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).max()),
                   refined_point_error=float(np.linalg.norm((qs @ reg.T[:3, :3].T + reg.T[:3, 3])
                                                            - (qs @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).max()),
                   refined_vs_true=float(np.abs(dT - np.eye(4)).max()))
        out['survey_%d' % size] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
