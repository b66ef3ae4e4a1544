"""The designed cases of the surface reconstruction, shared by the host tests (host build against oracle, hand-written figures) and the GPU
tests (device against oracle).

An integration case is (name, volume, batches): volume = dict(origin, dims, voxel, trunc) and every batch a dict(vps, dirs, depth,
pose, mask, min_depth, max_range, carve_from) for one call.  The designed rays live on a 4 x 4 x 8 grid of unit voxels at the origin with
tau = 2 (h = 0.5, K = 4) and run along +z through the voxel centres (1.5, 1.5, z + 0.5), so that every figure can be written by hand.

An extraction case is (name, volume, sum [nx,ny,nz], count [nx,ny,nz], min_count).
"""
import numpy as np

GRID = dict(origin=(0.0, 0.0, 0.0), dims=(4, 4, 8), voxel=1.0, trunc=2.0)
Q = 2 ** 20


def batch(vps, dirs, depth, dtype=np.float64, **kw):
    out = dict(vps=np.asarray(vps, dtype).reshape(-1, 3), dirs=np.asarray(dirs, dtype).reshape(-1, 3), depth=np.asarray(depth, dtype).reshape(-1),
               pose=None, mask=None, min_depth=0.0, max_range=None, carve_from=None)
    out.update(kw)
    return out


def z_ray(depth, x=1.5, y=1.5, z0=0.0, **kw):
    return batch([[x, y, z0]], [[0.0, 0.0, 1.0]], [depth], **kw)


def integration_cases():
    tie = [4.5 + 1.0 / Q, 4.5 + 3.0 / Q]                # s / tau 2^20 = 0.5 and 1.5 in the voxel of the surface
    skipped = batch([[1.5, 1.5, 0.0]] * 7,
                    [[0, 0, 1], [0, np.nan, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [np.inf, 0, 1]],
                    [4.5, 4.5, np.inf, 4.5, 1.0, np.nextafter(6.0, 7.0), 4.5],
                    mask=np.array([1, 1, 1, 0, 1, 1, 1], np.uint8), min_depth=1.0, max_range=6.0)
    f32 = [[1.25, 1.5, 0.25], [0.5, 3.25, 0.75]], [[0.0, 0.6, 0.8], [0.6, -0.8, 0.0]], [3.5, 1.25]
    yaw = np.array([[0.0, -1.0, 0.0, 3.5], [1.0, 0.0, 0.0, 0.5], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]])
    return [
        ('s_equals_tau_both_ends', GRID, [z_ray(4.5)]),                 # s = 2, 1, 0, -1, -2: +2^20 .. -2^20, the last one kept
        ('clamp', GRID, [z_ray(4.75)]),                                 # s = 2.25 in voxel 2: clamped to +2^20
        ('below_minus_tau_dropped', GRID, [z_ray(5.0)]),                # the sample at z = 7 meets s = -2.5: nothing added
        ('face_goes_up', GRID, [z_ray(4.5, x=2.0, y=3.0)]),             # x = 2.0 and y = 3.0 exactly: voxel (2, 3, .)
        ('leaves_grid', GRID, [z_ray(7.0)]),                            # the samples at z = 8, 8.5, 9 are outside
        ('tie_to_even', GRID, [z_ray(tie[0])]),
        ('tie_to_even_odd', GRID, [z_ray(tie[1])]),
        ('skipped_rays', GRID, [skipped]),
        ('carve', GRID, [z_ray(4.5, carve_from=0.5)]),
        ('behind_the_sensor', GRID, [z_ray(1.0, z0=0.25)]),             # t = d + k h <= 0 for k <= -2: not sampled
        ('f32', GRID, [batch(*f32, dtype=np.float32)]),
        ('f64_of_f32', GRID, [batch(*f32, dtype=np.float64)]),
        ('posed', GRID, [batch(*f32, pose=yaw), z_ray(4.5, pose=yaw)]),
        ('two_calls_one_voxel', GRID, [z_ray(4.5), z_ray(4.25), z_ray(4.5, x=1.75)]),
    ]


def _vol(dims, origin=(0.0, 0.0, 0.0), voxel=1.0):
    return dict(origin=origin, dims=dims, voxel=voxel, trunc=3.0 * voxel)


def extraction_cases():
    cases = []
    s = np.full((2, 2, 2), Q, np.int64)
    s[0, 0, 0] = -Q
    cases.append(('one_cell', _vol((2, 2, 2)), s, np.ones((2, 2, 2), np.int32), 1))
    s = np.full((3, 3, 3), Q // 2, np.int64)
    s[1, 1, 1] = -Q // 4
    cases.append(('centre_inside', _vol((3, 3, 3), origin=(-1.0, 0.5, 2.0), voxel=0.25), s, np.ones((3, 3, 3), np.int32), 1))
    c = np.ones((3, 3, 3), np.int32)
    c[0, 0, 0] = 0
    cases.append(('one_corner_unobserved', _vol((3, 3, 3)), s, c, 1))
    s0 = s.copy()
    s0[1, 1, 1] = 0
    s0[1, 1, 2] = -3
    cases.append(('zero_is_outside', _vol((3, 3, 3)), s0, np.ones((3, 3, 3), np.int32), 1))
    # a linear field f = (2 x + 3 y - 5 z + 1.25) / 16 on 4 x 4 x 4 with counts 2 and 3, and 1 along the line x = y = 0
    x, y, z = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing='ij')
    cnt = np.where((x == 0) & (y == 0), 1, 2 + (x + y + z) % 2).astype(np.int32)
    lin = ((2 * x + 3 * y - 5 * z) * 4 + 5) * (Q // 64) * cnt
    cases.append(('linear', _vol((4, 4, 4), origin=(0.5, -0.25, 1.0), voxel=0.5), lin.astype(np.int64), cnt, 1))
    cases.append(('linear_min_count_2', _vol((4, 4, 4), origin=(0.5, -0.25, 1.0), voxel=0.5), lin.astype(np.int64), cnt, 2))
    rng = np.random.default_rng(7)
    dims = (6, 5, 7)
    cases.append(('random', _vol(dims, voxel=0.1), rng.integers(-Q, Q, dims).astype(np.int64), rng.integers(0, 4, dims).astype(np.int32), 1))
    cases.append(('random_min_count_2', _vol(dims, voxel=0.1), rng.integers(-Q, Q, dims).astype(np.int64), rng.integers(0, 4, dims).astype(np.int32),
                  2))
    return cases
