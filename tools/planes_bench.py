"""Plane neighbourhoods on the room (RoomBoxDataset, 10 scans x 200k points by default): segmentation time and the per-iteration
plane forward + backward (dc_plane_moments_fwd / _bwd + eigh + loss) time.  Prints one JSON line.

    python tools/planes_bench.py [--n-pts 200000] [--n-poses 10] [--iters 50]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/planes_bench.py      # kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-pts', type=int, default=200_000)
    ap.add_argument('--n-poses', type=int, default=10)
    ap.add_argument('--grid-res', type=float, default=0.2)
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    from depth_correction_amd.config import Config, NeighborhoodType
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.loss import min_eigval_loss
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.preproc import compute_neighborhood_features, establish_neighborhoods, filtered_cloud, global_cloud
    dev = 'cuda:0'
    cfg = Config(nn_type=NeighborhoodType.plane, grid_res=args.grid_res, min_depth=0.0, max_depth=float('inf'),
                 min_valid_neighbors=250, max_neighborhoods=None, device=dev)
    ds = RoomBoxDataset(n_pts=args.n_pts, n_poses=args.n_poses)
    clouds = [filtered_cloud(DepthCloud.from_structured_array(a, dtype=np.float64, device=dev), cfg) for a, _ in ds]
    poses = torch.as_tensor(np.stack([p for _, p in ds]), device=dev)
    g = global_cloud(clouds=clouds, poses=poses)
    establish_neighborhoods(cloud=g, cfg=cfg)                            # warm-up (library load, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    planes = establish_neighborhoods(cloud=g, cfg=cfg)
    torch.cuda.synchronize()
    t_seg = time.perf_counter() - t0
    model = ScaledPolynomial(w=[1e-3], exponent=[4.0], device=dev)

    def step():
        model.w.grad = None
        feat = compute_neighborhood_features(cloud=g, model=model, neighborhoods=planes, cfg=cfg)
        loss, _ = min_eigval_loss([feat])
        loss.backward()
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        step()
    torch.cuda.synchronize()
    t_it = (time.perf_counter() - t0) / args.iters
    print(json.dumps(dict(points=len(g), planes=len(planes), plane_points=int(sum(len(i) for i in planes.indices)),
                          segmentation_ms=round(1e3 * t_seg, 3), fwd_bwd_ms=round(1e3 * t_it, 4))))


if __name__ == '__main__':
    main()
