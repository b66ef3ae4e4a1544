"""Plane registration on the GPU (csrc/dc_planereg.hip, registration.register_planes) on the scene of tools/globalreg_bench.py: the
map of --poses rendered H x W scans (2 cm of depth noise) of a pillared room, moved out of the survey's frame by 140 degrees and 3 m,
registered WITHOUT a prior to surveys of two sizes sampled from the room's mesh, with default arguments.  Timed in ONE process after a
warm-up of every shape, medians of --reps synchronised runs, the variants of a stage alternating:

    stages        the two plane fits (the cloud's; the survey's once, as it is cached), the triples, dc_planereg_count, the scan,
                  dc_planereg_fill, the suppression, the fitness queries of the candidates, the refinement, and the whole call
    count + fill  against a batched torch restatement of rules 1 to 5 and the score on the device (the valid triples fitted by
                  torch.linalg.svd, the translation by torch.linalg.solve) on the first --slice hypotheses, with equal valid lists
                  and equal scores ASSERTED

and reports the plane counts, the triples, the enumerated and the valid hypotheses, the winner, its fitness and the runner-up, and
the coarse and refined distance to the true transform.  Prints one JSON line.

    python tools/planereg_bench.py [--surveys 200000 2000000] [--poses 10] [--size 64 2048] [--reps 5] [--slice 4194304]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from globalreg_bench import _offset                        # noqa: E402  (the same placement as the descriptor tool)
from meshloss_bench import _poses, _scans, _timed          # noqa: E402  (the same scans as the mesh-loss tool)


def _det3(a, b, c):
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2])) \
        + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0])


def _dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _torch_hypotheses(cp, cs, sp, tri, tol, h_end, chunk=1 << 20):
    """(h int64 [V], score int64 [V]) of the hypotheses 0 .. h_end-1 by batched torch operations on the device."""
    min_det, tol_dot, cos_tol, tol_d = tol
    ps, dev = sp.shape[0], cp.device
    n, m = cp[:, :3], sp[:, :3]
    hs, scs = [], []
    for h0 in range(0, h_end, chunk):
        h = torch.arange(h0, min(h0 + chunk, h_end), dtype=torch.int64, device=dev)
        s, r = h & 7, h >> 3
        k, r = r % ps, r // ps
        j, r = r % ps, r // ps
        i, u = r % ps, r // ps
        sg = torch.stack([1.0 - 2.0 * ((s >> b) & 1).double() for b in range(3)], dim=1)
        t = tri[u].long()
        na, nb, nc, mi, mj, mk = n[t[:, 0]], n[t[:, 1]], n[t[:, 2]], m[i], m[j], m[k]
        dm = _det3(mi, mj, mk)
        ok = (i != j) & (i != k) & (j != k) & (dm.abs() >= min_det)
        ok &= ((sg[:, 0] * sg[:, 1]) * _dot3(na, nb) - _dot3(mi, mj)).abs() <= tol_dot
        ok &= ((sg[:, 0] * sg[:, 2]) * _dot3(na, nc) - _dot3(mi, mk)).abs() <= tol_dot
        ok &= ((sg[:, 1] * sg[:, 2]) * _dot3(nb, nc) - _dot3(mj, mk)).abs() <= tol_dot
        ok &= (((sg[:, 0] * sg[:, 1]) * sg[:, 2]) * _det3(na, nb, nc)) * dm > 0.0
        rows = torch.nonzero(ok).reshape(-1)
        if rows.shape[0] == 0:
            continue
        t, sg = t[rows], sg[rows]
        N = cp[t] * sg[:, :, None]                         # [V, 3, 4]: sigma (n, d)
        M = sp[torch.stack([i[rows], j[rows], k[rows]], dim=1)]
        H = M[:, :, :3].transpose(1, 2) @ N[:, :, :3]      # sum m_t (sigma n_t)^T
        U, _, Vt = torch.linalg.svd(H)
        d = torch.where(torch.linalg.det(U) * torch.linalg.det(Vt) >= 0.0, 1.0, -1.0)
        R = (U * torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1)[:, None, :]) @ Vt
        tr = torch.linalg.solve(M[:, :, :3], (N[:, :, 3] - M[:, :, 3])[:, :, None])[:, :, 0]
        fin = torch.isfinite(R).all(dim=(1, 2)) & torch.isfinite(tr).all(dim=1)
        n1 = torch.einsum('vij,qj->vqi', R, n)
        d1 = cp[None, :, 3] - torch.einsum('vqi,vi->vq', n1, tr)
        c = torch.einsum('vqi,ri->vqr', n1, m)
        agree = (c.abs() >= cos_tol) & ((torch.where(c >= 0.0, 1.0, -1.0) * d1[:, :, None] - sp[None, None, :, 3]).abs() <= tol_d)
        sc = (agree.any(dim=2) * cs[None, :]).sum(dim=1)
        hs.append(h[rows][fin])
        scs.append(sc[fin])
    if not hs:
        return torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev)
    return torch.cat(hs), torch.cat(scs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--surveys', type=int, nargs='+', default=(200000, 2000000), help='survey sizes (points sampled from the mesh)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--slice', type=int, default=1 << 22, help='hypotheses of the torch restatement')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('planereg_bench needs a GPU')
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.registration import cloud_planes, register_cloud, register_planes
    from depth_correction_amd.render import lidar_directions
    from depth_correction_amd.survey import SurveyCloud
    dev = torch.device('cuda:0')
    kw = dict(plane_voxel=0.1, distance_threshold=0.03, ransac_iters=500, cluster_eps=0.4, max_planes=32, seed=0)
    tol = (0.5, 0.05, math.cos(math.radians(3.0)), 0.05)
    voxel, n_cand, rot, trans = 0.25, 64, math.radians(5.0), 0.25
    eps = 0.6 * voxel
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev), torch.as_tensor(np.array(t_min), device=dev)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    _, _, normals, bvh = room.on_device(dev)
    poses = torch.as_tensor(_poses(args.poses, 0.0, 3.0), device=dev)
    ps_, _ = _scans(room, bvh, normals, poses, dirs, tmin, dev)
    world = ops.points_fwd(ps_, poses[:, :3, :].reshape(-1, 12).contiguous(), None, None, None).to(torch.float64)
    T_true = _offset()
    Ti = torch.as_tensor(np.linalg.inv(T_true), device=dev)
    q = (world @ Ti[:3, :3].t() + Ti[:3, 3]).contiguous()
    out = dict(tool='planereg_bench', poses=args.poses, size=list(args.size), reps=args.reps, points=q.shape[0], voxel=voxel,
               n_candidates=n_cand, **kw)

    def med(fn):
        return float(np.median([_timed(fn) for _ in range(args.reps)]))

    def med2(fa, fb):                                   # two variants of one stage, alternating
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(_timed(fa))
            tb.append(_timed(fb))
        return float(np.median(ta)), float(np.median(tb))

    def cloud_side():
        return cloud_planes(q, kw['plane_voxel'], kw['distance_threshold'], 40, kw['ransac_iters'], kw['cluster_eps'], kw['max_planes'], 0)
    cp, cs = cloud_side()
    fp = q[ops.voxel_filter(q, voxel, preserve_order=True)].contiguous()
    n = fp.shape[0]
    centre = 0.5 * (q.amin(dim=0) + q.amax(dim=0))
    out['cloud'] = dict(planes=cp.shape[0], points_after_filter=n, plane_fit_ms=med(cloud_side))
    qs = q[::97].cpu().numpy()

    def point_error(T):
        return float(np.linalg.norm((qs @ T[:3, :3].T + T[:3, 3]) - (qs @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).max())
    for size in args.surveys:
        sv = SurveyCloud.from_mesh(room, size, seed=135, device=dev)
        sd = sv.on_device(dev)
        res = dict(survey_points=sd.n)
        res['survey_plane_fit_once_ms'] = _timed(lambda: sv.planes(dev, min_support=100, **kw))
        sp, _ = sv.planes(dev, min_support=100, **kw)
        res['survey_planes'] = sp.shape[0]
        if min(cp.shape[0], sp.shape[0]) < 3:
            res['status'] = 'too_few_planes'
            out['survey_%d' % size] = res
            continue
        tri = ops.planereg_triples(cp, tol[0])
        total = tri.shape[0] * sp.shape[0] ** 3 * 8
        res.update(triples=tri.shape[0], enumerated=total, triples_ms=med(lambda: ops.planereg_triples(cp, tol[0])))
        if total == 0:
            res['status'] = 'too_few_planes'
            out['survey_%d' % size] = res
            continue
        args5 = (cp, cs, sp, tri) + tol
        counts = ops.planereg_count(*args5)
        ends = torch.cumsum(counts, dim=0, dtype=torch.int64)
        offsets, n_valid = (ends - counts).contiguous(), int(ends[-1])
        h, T, score = ops.planereg_fill(*args5, offsets, n_valid)
        res.update(valid=n_valid, blocks=counts.shape[0], count_ms=med(lambda: ops.planereg_count(*args5)),
                   scan_ms=med(lambda: int(torch.cumsum(counts, dim=0, dtype=torch.int64)[-1])),
                   fill_ms=med(lambda: ops.planereg_fill(*args5, offsets, n_valid)))
        # the kernels against the torch restatement on a slice of the enumeration
        cut = min(total, args.slice)
        hk, _, sk = ops.planereg_hypotheses(*args5, h_end=cut)
        ht, st = _torch_hypotheses(cp, cs, sp, tri, tol, cut)
        assert torch.equal(hk, ht), 'the valid lists differ: %d against %d rows' % (hk.shape[0], ht.shape[0])
        assert torch.equal(sk, st), 'the scores differ in %d rows' % int((sk != st).sum())
        res['slice'] = cut
        res['slice_valid'] = int(hk.shape[0])
        res['slice_kernels_ms'], res['slice_torch_ms'] = med2(lambda: ops.planereg_hypotheses(*args5, h_end=cut),
                                                              lambda: _torch_hypotheses(cp, cs, sp, tri, tol, cut))
        if n_valid:
            rows = ops.planereg_select(score, T, centre, n_cand, rot, trans)
            rows = rows[rows >= 0]
            res.update(candidates=int(rows.shape[0]), select_ms=med(lambda: ops.planereg_select(score, T, centre, n_cand, rot, trans)))
            sd.reserve(n)
            Tc = T[rows].contiguous()
            i1 = torch.empty((n, 1), dtype=torch.int32, device=dev)
            d1 = torch.empty((n, 1), dtype=torch.float64, device=dev)

            def fitness():
                for c in range(Tc.shape[0]):
                    ops.knn_grid_query(sd.grid, fp, Tc[c], 1, r=eps, idx=i1, dist=d1)
            fitness()
            res['fitness_ms'] = med(fitness)
        # the whole call, and the refinement alone
        reg = register_planes(q, sv)
        res['whole_ms'], res['whole_coarse_only_ms'] = med2(lambda: register_planes(q, sv), lambda: register_planes(q, sv, refine=False))
        res.update(status=reg.status, hypothesis=reg.hypothesis, score=reg.score, fitness=reg.fitness, runner_up=reg.runner_up,
                   n_valid=reg.n_valid, n_planes=list(reg.n_planes), coarse_point_error=point_error(reg.T_coarse))
        if reg.refined is not None:
            res['refine_ms'] = med(lambda: register_cloud(q, sv, init=reg.T_coarse, max_dist=2 * voxel))
            res.update(refined_status=reg.refined.status, refined_iterations=reg.refined.iterations, refined_point_error=point_error(reg.T))
        out['survey_%d' % size] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
