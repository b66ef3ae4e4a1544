"""Range-image neighbourhoods against ball neighbourhoods on the same scans (csrc/dc_rangeimage.hip, range_image.py): one synthetic
H x W scan of a room (one ray per pixel, jittered) and --scans of them, as raw device rows.  Times, per scan,
  * local_feature_cloud with local_nn_type = 'image' (organise + image shadow mask + window features + planarity mask) and with the
    default 'ball' (dc_scan_prefilter + k-NN + dc_features_fwd + planarity mask), with and without the scan-shadow filter,
  * the stages of the image path on their own (organise, shadow mask, features),
  * online.correct_cloud in both modes (the online node: its bar is 0.45 ms per scan),
and counts the kernel launches per scan in both modes (torch.profiler; null when the profiler cannot see the library's launches --
use the rocprofv3 line then).  The two modes do not compute the same neighbourhoods (DESIGN "Range-image neighbourhoods"); the ball
path is the one this package has always had, so it runs in the same process.  Medians of --reps synchronised runs in a warm process.
Prints one JSON line.

    python tools/rangeimage_bench.py [--size 128 1024] [--scans 10] [--window 2 2] [--k 10] [--reps 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/rangeimage_bench.py --reps 3      # kernel times and launch counts
"""
import argparse
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
    return float(np.median(ts)), float(np.min(ts))


def room_scan(rows, cols, fov, seed, half=(6.0, 4.0, 1.5), jitter=0.6):
    """Sensor-frame points float32 [H W, 3] in pixel order: one ray per pixel of the spherical grid, jittered inside its bin, against
    the inside of a 12 x 8 x 3 m box seen from a pose that depends on ``seed``, with 1 cm of range noise."""
    rng = np.random.default_rng(seed)
    up, down = np.radians(fov[0]), np.radians(fov[1])
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    u = (c + 0.5 + jitter * (rng.random((rows, cols)) - 0.5)) / cols
    v = (r + 0.5 + jitter * (rng.random((rows, cols)) - 0.5)) / rows
    yaw, pitch = (2.0 * u - 1.0) * np.pi, (1.0 - v) * (abs(up) + abs(down)) - abs(down)
    d = np.stack([np.cos(pitch) * np.cos(yaw), -np.cos(pitch) * np.sin(yaw), np.sin(pitch)], axis=-1).reshape(-1, 3)
    o = np.array([1.5 * np.cos(seed), 1.0 * np.sin(1.7 * seed), 0.2 * np.sin(0.3 * seed)])
    h = np.asarray(half)
    with np.errstate(divide='ignore'):
        t = np.where(d > 0, (h - o) / d, np.where(d < 0, (-h - o) / d, np.inf)).min(axis=1)
    t = t + 0.01 * rng.normal(size=t.shape)
    return (d * t[:, None]).astype(np.float32)


def _launches(fn):
    """Device kernels one call of ``fn`` launches, or None when the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception:                                   # (a profiler that cannot start must not take the timings with it)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, nargs=2, default=(128, 1024))
    ap.add_argument('--fov', type=float, nargs=2, default=(45.0, -45.0))
    ap.add_argument('--scans', type=int, default=10)
    ap.add_argument('--window', type=int, nargs=2, default=(2, 2))
    ap.add_argument('--k', type=int, default=10, help='k of the ball path\'s k-NN')
    ap.add_argument('--r', type=float, default=0.25, help='gate of the window')
    ap.add_argument('--float-type', default='float64')
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rangeimage_bench needs a GPU')
    from depth_correction_amd import ops, range_image as ri
    from depth_correction_amd.config import Config
    from depth_correction_amd.model import ScaledPolynomial
    from depth_correction_amd.online import correct_cloud
    from depth_correction_amd.preproc import local_feature_cloud
    dev = torch.device('cuda:0')
    H, W = args.size
    scans = [torch.as_tensor(room_scan(H, W, args.fov, s), device=dev) for s in range(args.scans)]
    shadow = dict(shadow_neighborhood_angle=0.017453, shadow_angle_bounds=[float(np.radians(5.0)), float('inf')])
    common = dict(float_type=args.float_type, device='cuda:0', log_filters=False)
    image = dict(local_nn_type='image', image_size=[H, W], image_fov=list(args.fov), image_window=list(args.window), nn_r=args.r)
    ball = dict(nn_k=args.k, nn_r=None)
    cfgs = {'image': Config(**common, **image, **shadow), 'ball': Config(**common, **ball, **shadow),
            'image_noshadow': Config(**common, **image), 'ball_noshadow': Config(**common, **ball)}
    model = ScaledPolynomial(w=[1e-3, 2e-3], exponent=[2.0, 4.0], device='cuda:0')
    out = dict(tool='rangeimage_bench', size=[H, W], points_per_scan=H * W, scans=args.scans, window=list(args.window), k=args.k, r=args.r,
               float_type=args.float_type, reps=args.reps)
    for name, cfg in cfgs.items():
        one, one_min = _median_ms(lambda: local_feature_cloud(scans[0], cfg), args.reps)
        many, _ = _median_ms(lambda: [local_feature_cloud(s, cfg) for s in scans], max(3, args.reps // 4))
        c = local_feature_cloud(scans[0], cfg)
        out['local_feature_cloud_' + name] = dict(one_scan_ms=one, one_scan_min_ms=one_min, scans_ms=many, per_scan_ms=many / args.scans,
                                                  points_kept=len(c), planar=int(c.mask.sum()) if c.mask is not None else None,
                                                  launches_per_scan=_launches(lambda: local_feature_cloud(scans[0], cfg)))
    for name in ('image', 'ball'):
        ms, mn = _median_ms(lambda: correct_cloud(scans[0], model, cfgs[name]), args.reps)
        many, _ = _median_ms(lambda: [correct_cloud(s, model, cfgs[name]) for s in scans], max(3, args.reps // 4))
        out['correct_cloud_' + name] = dict(one_scan_ms=ms, one_scan_min_ms=mn, per_scan_ms=many / args.scans,
                                            launches_per_scan=_launches(lambda: correct_cloud(scans[0], model, cfgs[name])))
    # the stages of the image path on their own
    grid = ri.SphericalGrid(H, W, args.fov[0], args.fov[1])
    dtype = getattr(torch, args.float_type)
    cloud = ri.organize(scans[0], grid, dtype=dtype)
    stages = {}
    stages['organize_ms'] = _median_ms(lambda: ri.organize_buffers(scans[0], grid, dtype=dtype), args.reps)[0]
    stages['organize_grid_ms'] = _median_ms(lambda: ri.organize_buffers(scans[0].reshape(H, W, 3), grid, dtype=dtype), args.reps)[0]
    stages['image_shadow_mask_ms'] = _median_ms(lambda: ri.image_shadow_mask(cloud, shadow['shadow_neighborhood_angle'], shadow['shadow_angle_bounds']),
                                                args.reps)[0]
    stages['shadow_window'] = list(ri.shadow_window(grid, shadow['shadow_neighborhood_angle']))
    for window in (tuple(args.window), (1, 1), (3, 3)):
        stages['image_features_%dx%d_ms' % window] = _median_ms(
            lambda: ops.image_features_fwd(cloud.points, cloud.dirs, cloud.pixel, cloud.index_image, grid, window, r=args.r), args.reps)[0]
    # the ball path's stages on the same cloud: k-NN + dc_features_fwd
    _, nbr = ops.knn(cloud.points, args.k, want_dist=False)[:2]
    stages['knn_ms'] = _median_ms(lambda: ops.knn(cloud.points, args.k, want_dist=False), args.reps)[0]
    stages['features_fwd_ms'] = _median_ms(lambda: ops.features_fwd(cloud.points, nbr, dirs=cloud.dirs), args.reps)[0]
    stages['shadow_filter_ms'] = _median_ms(lambda: ops.shadow_filter(cloud.points, cloud.vps, cloud.dirs, 0.017453, float(np.radians(5.0)), np.pi),
                                            args.reps)[0]
    out['stages'] = stages
    print(json.dumps(out))


if __name__ == '__main__':
    main()
