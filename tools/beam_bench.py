"""Finite-beam rendering on the GPU (csrc/dc_raycast.hip dc_raycast_beams): --poses poses x --size beams against a >= 1 M-triangle
grid_terrain_mesh and a pillared room_mesh, for S = 8, 16 and 64 sub-rays per beam, (a) next to the thin dc_raycast on the same
pattern and (b) next to the un-fused composition on identical inputs: dc_beam_subrays + dc_raycast_rays over n S rays + the
reduction in torch (stable sort by depth, cumsum, threshold, nearest return), whose results are compared with the fused launch's.
(c) The bias over the true incidence angle that the default BeamModel leaves in the scans of the room, measured with eval_bias.
Median, min and max of --reps synchronised runs in a warm process, the variants interleaved.  Prints one JSON line.

    python tools/beam_bench.py [--n 710] [--poses 10] [--size 64 2048] [--reps 10] [--samples 8 16 64] [--eval-poses 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/beam_bench.py --reps 2 --eval-poses 0      # kernel times
"""
import argparse
import contextlib
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bias_bench import _poses, _stats_ms          # noqa: E402


def _torch_reduce(sub_face, sub_t, sub_w, tau):
    """The QUANTILE reduction of dc_raycast_beams in torch on sub_* [n,S] -> (face, depth, n_hits)."""
    n, S = sub_face.shape
    hit = sub_face >= 0
    n_hits = hit.sum(dim=1).int()
    t_sorted, order = torch.sort(sub_t, dim=1, stable=True)            # misses carry t = inf and w = 0: they sort last, ties keep j
    c = torch.cumsum(torch.gather(sub_w, 1, order), dim=1)
    total = c[:, -1:]
    first = (c >= tau * total).int().argmax(dim=1, keepdim=True)
    depth = torch.gather(t_sorted, 1, first)
    near = torch.where(hit, (sub_t - depth).abs(), torch.full_like(sub_t, float('inf'))).argmin(dim=1, keepdim=True)
    ok = (n_hits > 0) & (total[:, 0] > 0)
    face = torch.where(ok, torch.gather(sub_face, 1, near)[:, 0], torch.full_like(n_hits, -1))
    depth = torch.where(ok, depth[:, 0], torch.full_like(depth[:, 0], float('inf')))
    return face, depth, n_hits


def _bias_table(args, dev):
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_bias
    from depth_correction_amd.mesh import room_mesh
    from depth_correction_amd.render import BeamModel, RenderedMeshDataset
    path = os.path.join(tempfile.mkdtemp(), 'bench_room.ply')
    room_mesh().save_ply(path)
    cfg = Config(device=dev, float_type='float64', min_depth=0.5, max_depth=25.0, grid_res=0.05, nn_k=0, nn_r=0.25)
    ds = RenderedMeshDataset(path, poses=_poses(args.eval_poses, 0.1, 3.0), size=(64, 1024), fov=(45.0, 360.0), num_segments=16, device=dev,
                             beam=BeamModel())
    with contextlib.redirect_stdout(sys.stderr):
        res = eval_bias(cfg, test_datasets=[ds], model=None)[0]
    b = res['before']
    return dict(scans=args.eval_poses, rays=int(b['totals']['rays']), used=int(b['totals']['used']),
                count=[int(x) for x in b['count'].cpu().tolist()], rel_mean=[float(x) for x in b['rel_mean'].cpu().tolist()],
                mean_m=[float(x) for x in b['mean'].cpu().tolist()], rel_rms=b['overall']['rel_rms'],
                fit_class=res['fit']['model_class'], fit_exponent=res['fit']['exponent'],
                w_true_angles=[float(x) for x in res['fit']['w_true_angles']], w_est_angles=[float(x) for x in res['fit']['w_est_angles']])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=710, help='terrain cells per side (2 n^2 triangles)')
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--samples', type=int, nargs='+', default=(8, 16, 64))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--eval-poses', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('beam_bench needs a GPU')
    from depth_correction_amd.mesh import grid_terrain_mesh, room_mesh
    from depth_correction_amd.ops import beam_subrays, raycast, raycast_beams, raycast_rays
    from depth_correction_amd.render import BeamModel, lidar_directions
    dev = torch.device('cuda:0')
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs1 = torch.as_tensor(np.array(d), device=dev)
    R, tmin0 = dirs1.shape[0], float(np.max(t_min))                       # one near clip everywhere: dc_raycast_rays takes a scalar
    tmin = torch.full((R,), tmin0, dtype=torch.float64, device=dev)
    out = dict(tool='beam_bench', poses=args.poses, size=list(args.size), reps=args.reps)
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    merge = lambda rs: dict(median=float(np.median([r['median'] for r in rs])), min=min(r['min'] for r in rs), max=max(r['max'] for r in rs),
                            medians=[r['median'] for r in rs])
    for name, mesh, height, spread in (('terrain', grid_terrain_mesh(args.n), 8.0, 60.0), ('room', room, 0.0, 3.0)):
        bvh = mesh.on_device(dev)[3]
        poses = torch.as_tensor(_poses(args.poses, height, spread), device=dev)
        P = poses.shape[0]
        dirs = dirs1.repeat(P, 1).contiguous()
        vps = torch.zeros_like(dirs)
        off = torch.arange(P + 1, dtype=torch.int64, device=dev) * R
        res = dict(faces=len(mesh), beams=int(dirs.shape[0]))
        for S in args.samples:
            beam = BeamModel(samples=S)
            kw = dict(t_min=tmin0, weight='uniform', detection='quantile', tau=beam.tau)
            fused = lambda: raycast_beams(bvh, vps, dirs, off, poses, beam.pattern, beam.r0, beam.spread, **kw)
            off_s = off * S

            def unfused():
                o, D = beam_subrays(vps, dirs, beam.pattern, beam.r0, beam.spread)
                f, t, _ = raycast_rays(bvh, o.reshape(-1, 3), D.reshape(-1, 3), off_s, poses, t_min=tmin0)
                f, t = f.reshape(-1, S), t.reshape(-1, S)
                return _torch_reduce(f, t, (f >= 0).double(), beam.tau)
            a, b = fused(), unfused()
            equal = all(torch.equal(x, y) for x, y in zip(a, b))
            ta, tb, tc = [], [], []
            for _ in range(3):                                            # interleaved: a drift of the machine's load meets all alike
                ta.append(_stats_ms(lambda: raycast(bvh, dirs1, poses, tmin), args.reps))
                tb.append(_stats_ms(fused, args.reps))
                tc.append(_stats_ms(unfused, max(2, args.reps // 2)))
            r = dict(sub_rays=int(dirs.shape[0]) * S, hit_beams=int((a[0] >= 0).sum()), equal_to_unfused=bool(equal), thin_ms=merge(ta),
                     fused_ms=merge(tb), unfused_ms=merge(tc))
            r['sub_rays_per_s'] = r['sub_rays'] / (r['fused_ms']['median'] * 1e-3)
            r['fused_over_thin'] = r['fused_ms']['median'] / r['thin_ms']['median']
            r['fused_over_unfused'] = r['fused_ms']['median'] / r['unfused_ms']['median']
            # the parts of the composition, once each
            r['subrays_ms'] = _stats_ms(lambda: beam_subrays(vps, dirs, beam.pattern, beam.r0, beam.spread), 3)
            o, D = beam_subrays(vps, dirs, beam.pattern, beam.r0, beam.spread)
            o, D = o.reshape(-1, 3), D.reshape(-1, 3)
            r['raycast_rays_ms'] = _stats_ms(lambda: raycast_rays(bvh, o, D, off_s, poses, t_min=tmin0), 3)
            del o, D
            res['S%d' % S] = r
            print('%s S %d: %s' % (name, S, json.dumps(r)), file=sys.stderr, flush=True)
        out[name] = res
    if args.eval_poses > 0:
        out['room_bias'] = _bias_table(args, 'cuda:0')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
