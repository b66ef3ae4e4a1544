"""Loss landscape over the model weights: the one-pass path (eval.landscape_clouds -> dc_sequence_landscape) against the loop of
eval_loss_clouds it replaces, for W in {1, 8, 21, 100} candidate weights, on two workloads:
  c2     10 scans x 200k points of the room, k = 10, float32, ScaledPolynomial with exponents [2, 4] (P = 2), masks given;
  planes the room with plane neighbourhoods (tools/planes_bench.py set-up), P = 1 (dc_plane_landscape).
Two loop baselines: ``loop_ms`` evaluates a copy of the model per row (the landscape's contract; every copy brings its own exponent
tensor, so the plan rebuilds its basis rows per row), ``loop_inplace_ms`` updates the weights of one model in place (basis rows
built once).  Medians of --reps synchronised runs in a warm process.  Prints one JSON line.

    python tools/landscape_bench.py [--n-pts 200000] [--n-poses 10] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/landscape_bench.py --reps 2      # kernel times
"""
import argparse
import copy
import json
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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-pts', type=int, default=200_000)
    ap.add_argument('--n-poses', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ws', type=str, default='1,8,21,100')
    ap.add_argument('--skip-planes', action='store_true')
    ap.add_argument('--skip-c2', action='store_true')
    args = ap.parse_args()
    from depth_correction_amd.config import Config, NeighborhoodType
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.eval import (_model_with_weights, eval_loss_clouds, landscape_clouds, landscape_paths)
    from depth_correction_amd.loss import create_loss
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.preproc import establish_neighborhoods, filtered_cloud, global_cloud
    dev = 'cuda:0'
    ws_list = [int(x) for x in args.ws.split(',')]
    result = {'n_pts': args.n_pts, 'n_poses': args.n_poses, 'reps': args.reps}

    def run(tag, clouds, poses, masks, ns, model, cfg, rows_of):
        loss_fun = create_loss(cfg)
        out = {}
        for W in ws_list:
            w = rows_of(W)
            k0 = dict(landscape_paths)

            def one():
                landscape_clouds(clouds, poses, [None], masks, ns, model, w, cfg)

            def loop():
                with torch.no_grad():
                    for row in w.reshape(W, -1):
                        eval_loss_clouds(clouds, poses, [None], masks, ns, _model_with_weights(model, row), loss_fun, cfg)
            def loop_inplace():
                m = copy.deepcopy(model)
                with torch.no_grad():
                    for row in w.reshape(W, -1):
                        m.w.copy_(row.reshape(m.w.shape))
                        eval_loss_clouds(clouds, poses, [None], masks, ns, m, loss_fun, cfg)
            t1 = _median_ms(one, args.reps)
            path = 'kernel' if landscape_paths['kernel'] > k0.get('kernel', 0) else 'loop'
            t2 = _median_ms(loop, args.reps)
            t3 = _median_ms(loop_inplace, args.reps)
            out[str(W)] = {'landscape_ms': round(t1, 3), 'loop_ms': round(t2, 3), 'loop_inplace_ms': round(t3, 3),
                           'speedup': round(t2 / t1, 2), 'speedup_inplace': round(t3 / t1, 2), 'path': path}
        result[tag] = out

    # ---- c2: 10 x 200k room, k = 10, float32 --------------------------------------------------------------------------------
    if not args.skip_c2:
        run_c2(args, dev, run)

    # ---- room with plane neighbourhoods ------------------------------------------------------------------------------------
    if not args.skip_planes:
        pcfg = Config(nn_type=NeighborhoodType.plane, grid_res=0.2, min_depth=0.0, max_depth=float('inf'), min_valid_neighbors=250,
                      max_neighborhoods=None, device=dev)
        pds = RoomBoxDataset(n_pts=args.n_pts, n_poses=args.n_poses)
        pclouds = [filtered_cloud(DepthCloud.from_structured_array(a, dtype=np.float64, device=dev), pcfg) for a, _ in pds]
        pposes = torch.as_tensor(np.stack([p for _, p in pds]), device=dev)
        planes = establish_neighborhoods(cloud=global_cloud(clouds=pclouds, poses=pposes), cfg=pcfg)
        pmodel = ScaledPolynomial(w=[0.0], exponent=[4.0], device=dev)
        run('planes', [pclouds], [pposes], [None], [planes], pmodel, pcfg,
            lambda W: torch.linspace(-0.01, 0.01, W, dtype=torch.float64))
    print(json.dumps(result))


def run_c2(args, dev, run):
    from depth_correction_amd.config import Config
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.pipeline import build_sequence
    ds = RoomBoxDataset(n_pts=args.n_pts, n_poses=args.n_poses, dtype=np.float32)
    scans_xyz = [np.stack([c[f] for f in 'xyz'], axis=1) for c, _ in ds]
    poses_np = np.stack([p for _, p in ds])
    _, info = build_sequence(scans_xyz, poses_np, k=10, dtype=torch.float32, device=dev)
    cfg = Config(nn_k=10, nn_r=0.0, float_type='float32', device=dev)

    class _Cloud:
        def __init__(self, c):
            self.vps, self.dirs, self.depth, self.inc_angles, self.mask = c['vps'], c['dirs'], c['depth'], c['inc_angles'], c['mask']
    clouds = [[_Cloud(c) for c in info['clouds']]]
    poses = [info['poses']]
    ns = [(info['neighbors'], None)]
    masks = [info['mask']]
    model = ScaledPolynomial(w=[0.0, 0.0], exponent=[2.0, 4.0], device=dev)

    def rows2(W):
        g = torch.linspace(-0.004, 0.004, W, dtype=torch.float64)
        return torch.stack([g, g.flip(0)], 1)
    run('c2', clouds, poses, masks, ns, model, cfg, rows2)


if __name__ == '__main__':
    main()
