"""Surface reconstruction on the GPU (csrc/dc_tsdf.hip): --poses rendered H x W scans of a pillared room fused into a --voxel grid
(dc_tsdf_integrate, timed per scan) and the surface-nets extraction of the result (count, scan, fill and its one host read), with device
events, medians of --reps runs in a warm process.  The yardstick is a torch restatement of the same rule -- a loop over the steps along
the ray, elementwise fp64 operations and index_add_ on the int64 sums -- whose volume must EQUAL the kernel's (asserted).  Also the
accuracy and completeness of the mesh against the room.  Prints one JSON line.

--sparse adds the block-allocated volume (csrc/dc_tsdf_sparse.hip) on the same scene and the same lattice: dc_tsdf_sparse_allocate and
dc_tsdf_sparse_integrate timed per scan, each on its own, into a pool of the size the scene needs; blocks and pool bytes beside the
dense volume's; the extraction; the pool must EQUAL the dense volume on the dense box (asserted).  Then one scene the dense volume
refuses (asserted): scans of the 1 M-triangle terrain at --reach-voxel, fused with a growing pool.

    python tools/recon_bench.py [--poses 10] [--size 64 2048] [--voxel 0.05] [--reps 10] [--sparse]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/recon_bench.py --reps 3      # kernel times
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_ms(fn, reps, before=None):
    """Median and minimum device time of fn() over reps runs after one warm-up; before() runs outside the timed window."""
    times = []
    for r in range(reps + 1):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def _poses(n, spread):
    out = []
    for i in range(n):
        yaw = 0.37 * i
        p = np.eye(4)
        p[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]
        p[:3, 3] = (spread * math.cos(1.3 * i), spread * math.sin(0.7 * i), 0.1 * math.sin(i))
        out.append(p)
    return np.stack(out)


def torch_integrate(sum_, count, origin, voxel, trunc, dirs, depth, pose):
    """The rule of csrc/dc_tsdf_math.h in torch for rays from the sensor origin (no mask, no range limits, no carving): sum i64 /
    count i32 [nx,ny,nz] in place; returns the visits."""
    from depth_correction_amd.ops import tsdf_k_steps
    dims = sum_.shape
    flat_s, flat_c = sum_.view(-1), count.view(-1)
    R, t0 = pose[:3, :3], pose[:3, 3]
    o = t0.expand(dirs.shape[0], 3)
    u = torch.stack([(R[r, 0] * dirs[:, 0] + R[r, 1] * dirs[:, 1]) + R[r, 2] * dirs[:, 2] for r in range(3)], dim=1)
    ok = torch.isfinite(depth) & (depth > 0.0) & torch.isfinite(u).all(dim=1)
    o, u, d = o[ok], u[ok], depth[ok]
    h, K = voxel / 2.0, tsdf_k_steps(trunc, voxel)
    og = torch.as_tensor(origin, dtype=torch.float64, device=dirs.device)
    # divisors as device tensors: torch divides by a host scalar through its reciprocal, which is not the rule's division
    voxel_t, trunc_t = (torch.tensor(x, dtype=torch.float64, device=dirs.device) for x in (voxel, trunc))
    last = torch.full((d.shape[0],), -1, dtype=torch.int64, device=dirs.device)
    visits = 0
    for k in range(-K, K + 1):
        t = d + float(k) * h
        g = torch.floor(((o + t[:, None] * u) - og) / voxel_t)
        inside = (t > 0.0) & (g[:, 0] >= 0) & (g[:, 0] < dims[0]) & (g[:, 1] >= 0) & (g[:, 1] < dims[1]) & (g[:, 2] >= 0) & (g[:, 2] < dims[2])
        i = g.to(torch.int64)
        v = (i[:, 0] * dims[1] + i[:, 1]) * dims[2] + i[:, 2]
        new = inside & (v != last)
        last = torch.where(new, v, last)
        c = og + (g + 0.5) * voxel
        s = d - ((u[:, 0] * (c[:, 0] - o[:, 0]) + u[:, 1] * (c[:, 1] - o[:, 1])) + u[:, 2] * (c[:, 2] - o[:, 2]))
        add = new & (s >= -trunc)
        q = torch.round(torch.clamp(s, max=trunc) / trunc_t * float(2 ** 20)).to(torch.int64)
        flat_s.index_add_(0, v[add], q[add])
        flat_c.index_add_(0, v[add], torch.ones_like(v[add], dtype=torch.int32))
        visits += add.sum()
    return visits


def _cloud(vps, dirs, depth):
    from depth_correction_amd.depth_cloud import DepthCloud
    return DepthCloud(vps.expand(dirs.shape[0], 3).contiguous(), dirs, depth.reshape(-1, 1).contiguous())


def sparse_room(args, vol, vps, dirs, depth, poses):
    """The room's scans into a sparse volume on the dense volume's lattice: figures beside the dense ones."""
    from depth_correction_amd import ops
    from depth_correction_amd.reconstruction import SparseTsdfVolume
    dev = dirs.device
    grown = SparseTsdfVolume(vol.voxel_size, trunc=vol.trunc, origin=vol.origin, device=dev)
    for p in range(args.poses):
        grown.integrate(_cloud(vps, dirs, depth[p]), pose=poses[p])
    blocks = grown.n_blocks
    del grown
    sv = SparseTsdfVolume(vol.voxel_size, trunc=vol.trunc, origin=vol.origin, max_blocks=blocks, device=dev)
    k = ops.tsdf_k_steps(vol.trunc, vol.voxel_size)
    ws = torch.empty((int(ops.lib().dc_tsdf_sparse_workspace_bytes(dirs.shape[0], k, blocks)),), dtype=torch.uint8, device=dev)
    rule = (sv.origin, sv.voxel_size, sv.trunc, vps, dirs)
    alloc, integ = [[] for _ in range(args.poses)], [[] for _ in range(args.poses)]
    for r in range(args.reps + 1):
        sv.reset()
        marks = []
        for p in range(args.poses):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            ops.tsdf_sparse_allocate(sv._keys, sv._slots, sv._n_blocks, sv._info, *rule, depth[p], pose=poses[p], ws=ws)
            ev[1].record()
            ops.tsdf_sparse_integrate(sv._keys, sv._slots, sv._n_blocks, sv._sum, sv._count, sv._stats, *rule, depth[p], pose=poses[p])
            ev[2].record()
            marks.append(ev)
        torch.cuda.synchronize()
        if r:
            for p, ev in enumerate(marks):
                alloc[p].append(ev[0].elapsed_time(ev[1]))
                integ[p].append(ev[1].elapsed_time(ev[2]))
    sv._n_host = None
    stats = sv.stats()
    assert stats['blocks'] == blocks and stats['visits_dropped'] == 0
    s, c = sv.window((0, 0, 0), vol.dims)
    assert torch.equal(s, vol.sums()) and torch.equal(c, vol.counts()), 'the sparse pool and the dense volume differ on the dense box'
    ews = torch.empty((int(ops.lib().dc_tsdf_sparse_extract_workspace_bytes(blocks)),), dtype=torch.uint8, device=dev)
    extract = lambda: ops.tsdf_sparse_extract(sv._keys, sv._slots, blocks, sv._sum, sv._count, sv.origin, sv.voxel_size, ws=ews)
    e_ms, e_min = _event_ms(extract, args.reps)
    vertices, faces = extract()
    return dict(blocks=blocks, pool_bytes=sv.nbytes, dense_bytes=12 * int(np.prod(vol.dims)), allocate_ws_bytes=int(ws.shape[0]),
                extract_ws_bytes=int(ews.shape[0]), allocate_scan_ms=float(np.median([np.median(a) for a in alloc])),
                allocate_scan_min_ms=float(np.min([np.min(a) for a in alloc])), integrate_scan_ms=float(np.median([np.median(a) for a in integ])),
                integrate_scan_min_ms=float(np.min([np.min(a) for a in integ])), extract_ms=e_ms, extract_min_ms=e_min,
                vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), visits=stats['visits'], samples_outside=stats['samples_outside'],
                equal_on_dense_box=True)


def sparse_reach(args, vps, dirs, tmin):
    """Scans of the 1 M-triangle terrain (200 x 200 m) at a voxel size whose box the dense volume refuses, into a growing pool."""
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import grid_terrain_mesh
    from depth_correction_amd.reconstruction import SparseTsdfVolume, TsdfVolume
    dev = dirs.device
    terrain = grid_terrain_mesh(710)
    lo, hi = terrain.bounds
    refused = False
    try:
        TsdfVolume.from_bounds(lo, hi, args.reach_voxel, device=dev)
    except ValueError:
        refused = True
    assert refused, 'the dense volume takes the terrain at %g m: choose a smaller --reach-voxel' % args.reach_voxel
    poses = _poses(args.poses, 60.0)
    poses[:, 2, 3] += 8.0
    poses = torch.as_tensor(poses, device=dev)
    face, depth, _ = ops.raycast(terrain.on_device(dev)[3], dirs, poses, tmin)
    depth = torch.where(face >= 0, depth, torch.full_like(depth, float('inf'))).contiguous()
    sv = SparseTsdfVolume(args.reach_voxel, device=dev)
    times = []
    for p in range(args.poses):
        cloud = _cloud(vps, dirs, depth[p])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sv.integrate(cloud, pose=poses[p], max_range=args.reach_range)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    stats = sv.stats()
    e_ms, e_min = _event_ms(sv.extract, max(2, args.reps // 3))
    vertices, faces = sv.extract()
    box = np.ceil((hi - lo + 6.0 * args.reach_voxel) / args.reach_voxel)
    return dict(scene='terrain', faces_in=len(terrain), voxel=args.reach_voxel, max_range=args.reach_range, dense_refused=True,
                dense_voxels=float(np.prod(box)), dense_bytes=12.0 * float(np.prod(box)), blocks=stats['blocks'], capacity=sv.capacity,
                used_bytes=stats['blocks'] * (12 + 512 * 12), pool_bytes=sv.nbytes, scan_ms_with_growth=times,
                scan_ms_median=float(np.median(times)), extract_ms=e_ms, extract_min_ms=e_min, vertices=int(vertices.shape[0]),
                faces=int(faces.shape[0]), stats=stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--poses', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=2, default=(64, 2048))
    ap.add_argument('--segments', type=int, default=16)
    ap.add_argument('--voxel', type=float, default=0.05)
    ap.add_argument('--samples', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sparse', action='store_true', help='also the block-allocated volume on the same scene, and the terrain the dense one refuses')
    ap.add_argument('--reach-voxel', type=float, default=0.04)
    ap.add_argument('--reach-range', type=float, default=30.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('recon_bench needs a GPU')
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import TriangleMesh, room_mesh
    from depth_correction_amd.metrics import reconstruction_accuracy
    from depth_correction_amd.reconstruction import TsdfVolume
    from depth_correction_amd.render import lidar_directions
    dev = torch.device('cuda:0')
    room = room_mesh((10.0, 7.0, 2.0), 0.5, pillars=[((3.0, 2.0, 0.0), (0.5, 0.5, 2.0)), ((-4.0, -2.5, 0.0), (0.4, 0.6, 2.0)),
                                                      ((0.0, 3.5, 0.0), (0.3, 0.3, 2.0))])
    d, t_min = lidar_directions(size=args.size, fov=(45.0, 360.0), num_segments=args.segments)
    dirs, tmin = torch.as_tensor(np.array(d), device=dev).contiguous(), torch.as_tensor(np.array(t_min), device=dev)
    poses = torch.as_tensor(_poses(args.poses, 3.0), device=dev)
    face, depth, _ = ops.raycast(room.on_device(dev)[3], dirs, poses, tmin)
    depth = torch.where(face >= 0, depth, torch.full_like(depth, float('inf'))).contiguous()          # [poses, rays]; a miss is skipped
    vps = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    lo, hi = room.bounds
    vol = TsdfVolume.from_bounds(lo, hi, args.voxel, device=dev)
    out = dict(tool='recon_bench', poses=args.poses, size=list(args.size), rays_per_scan=int(dirs.shape[0]), voxel=args.voxel,
               dims=list(vol.dims), voxels=int(np.prod(vol.dims)), reps=args.reps)

    def fuse(p):
        ops.tsdf_integrate(vol.sums(), vol.counts(), vol._stats, vol.origin, vol.voxel_size, vol.trunc, vps, dirs, depth[p], pose=poses[p])

    per_scan = [_event_ms(lambda: fuse(p), args.reps) for p in range(args.poses)]           # (the sums grow; the work per call does not)
    vol.reset()
    ms, _ = _event_ms(lambda: [fuse(p) for p in range(args.poses)], args.reps, before=vol.reset)
    stats = vol.stats()
    out.update(integrate_scan_ms=float(np.median([m for m, _ in per_scan])), integrate_scan_min_ms=float(np.min([m for _, m in per_scan])),
               integrate_all_ms=ms, visits=stats['visits'], mvisits_per_s=stats['visits'] / ms / 1e3, stats=stats)
    # the yardstick: the same rule in torch, equal volume
    ref_s, ref_c = torch.zeros_like(vol.sums()), torch.zeros_like(vol.counts())

    def torch_fuse():
        return [torch_integrate(ref_s, ref_c, vol.origin, vol.voxel_size, vol.trunc, dirs, depth[p], poses[p]) for p in range(args.poses)]

    def torch_reset():
        ref_s.zero_()
        ref_c.zero_()

    t_ms, _ = _event_ms(torch_fuse, max(2, args.reps // 3), before=torch_reset)
    assert torch.equal(ref_s, vol.sums()) and torch.equal(ref_c, vol.counts()), 'the torch restatement and the kernel differ'
    out.update(torch_all_ms=t_ms, torch_over_kernel=t_ms / ms, equal=True)
    del ref_s, ref_c
    if args.sparse:
        out['sparse'] = sparse_room(args, vol, vps, dirs, depth, poses)
    # extraction (with its one host read)
    ws = torch.empty((int(ops.lib().dc_tsdf_extract_workspace_bytes(*vol.dims)),), dtype=torch.uint8, device=dev)
    e_ms, e_min = _event_ms(lambda: ops.tsdf_extract(vol.sums(), vol.counts(), vol.origin, vol.voxel_size, ws=ws), args.reps)
    vertices, faces = ops.tsdf_extract(vol.sums(), vol.counts(), vol.origin, vol.voxel_size, ws=ws)
    out.update(extract_ms=e_ms, extract_min_ms=e_min, vertices=int(vertices.shape[0]), faces=int(faces.shape[0]))
    mesh = TriangleMesh(vertices.cpu().numpy(), faces.cpu().numpy())
    acc = reconstruction_accuracy(mesh, room, n_samples=args.samples, max_dist=2.0 * args.voxel)
    out.update(accuracy_mean=acc['accuracy']['mean'], accuracy_rms=acc['accuracy']['rms'], accuracy_max=acc['accuracy']['max'],
               completeness_mean=acc['completeness']['mean'], completeness_rms=acc['completeness']['rms'], coverage=acc['coverage'])
    if args.sparse:
        del vol, ws
        out['reach'] = sparse_reach(args, vps, dirs, tmin)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
