"""Designed cases of the scan-to-TSDF registration (csrc/dc_tsdf_track_math.h), shared by tests/test_tsdf_track_host.py (the host build)
and tests/test_gpu_tsdf_track.py (the kernels): volumes at a = 1, og = 0, tau = 2 filled by hand, query points whose arithmetic is exact
with their hand-written expected values, and the inputs of the row's edges.

The linear field v(i) = (ix + 2 iy - 4 iz) / 128 has power-of-two coefficients: every difference, product and sum of the trilinear
interpolant is exact for dyadic f, so phi = tau v(q) and grad = (tau / a) (1, 2, -4) / 128 everywhere, to the bit.
"""
import numpy as np

import tsdf_sparse_reference as S

VOLUME = dict(voxel=1.0, trunc=2.0, origin=(0.0, 0.0, 0.0))
Q = 2 ** 20
TAU = 2.0
GRAD = np.array([1.0, 2.0, -4.0]) / 128.0 * TAU           # (tau / a) x the field's slope
EDGE = 2 ** 23
S_RANGE, S_UNOBSERVED = 1, 2                               # the flags


def linear(i):
    """The field at the voxel indices i [..., 3]."""
    i = np.asarray(i, np.float64)
    return (i[..., 0] + 2.0 * i[..., 1] - 4.0 * i[..., 2]) / 128.0


def linear_block(b, count=1):
    """(b, sum [8,8,8], count [8,8,8]) of the block b holding the linear field, every voxel seen ``count`` times."""
    idx = np.stack(np.meshgrid(*[np.arange(8 * c, 8 * c + 8) for c in b], indexing='ij'), axis=-1)
    s = np.rint(linear(idx) * Q).astype(np.int64) * count
    return (tuple(b), s, np.full((8, 8, 8), count, np.int32))


def constant_block(b, value=1.0, count=1):
    return (tuple(b), np.full((8, 8, 8), int(round(value * Q)) * count, np.int64), np.full((8, 8, 8), count, np.int32))


def make_volume(blocks, capacity=None, volume=VOLUME):
    """The oracle volume holding ``blocks`` [(coord, sum, count)] in the order of their slots, the table sorted by key."""
    cap = (len(blocks) + 2) if capacity is None else capacity
    vol = S.SparseVolume(capacity=cap, **volume)
    keys = np.array([int(S.block_key(np.array(b))) for b, _, _ in blocks], np.uint64)
    order = np.argsort(keys, kind='stable')
    vol.keys, vol.slots = keys[order], order.astype(np.int32)
    for slot, (_, s, c) in enumerate(blocks):
        vol.sum[slot], vol.count[slot] = s.ravel(), c.ravel()
    return vol


def around(exclude=()):
    """The 27 blocks {-1, 0, 1}^3 of the linear field, in an order that is not the key order, without ``exclude``."""
    coords = [(x, y, z) for z in (1, -1, 0) for x in (0, 1, -1) for y in (-1, 1, 0)]
    return [linear_block(b) for b in coords if b not in exclude]


def at_q(q):
    """Points x whose q = x - 0.5 is exactly ``q`` [n, 3] (asserted)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    x = q + 0.5
    assert np.array_equal(x - 0.5, q)
    return x


def expect_linear(q):
    q = np.asarray(q, np.float64).reshape(-1, 3)
    return dict(flag=np.zeros(len(q), np.uint8), value=TAU * linear(q), grad=np.tile(GRAD, (len(q), 1)))


def expect_flag(n, flag):
    return dict(flag=np.full(n, flag, np.uint8), value=np.full(n, np.nan), grad=np.zeros((n, 3)))


# an exact pose: a quarter turn about z and an integer translation; INV_POSE moves x back
POSE = np.array([[0.0, -1.0, 0.0, 3.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])
GENERIC_POSE = np.array([[0.936293, -0.275096, 0.218351, 0.31], [0.289629, 0.956425, -0.036957, -0.17],
                         [-0.198669, 0.097843, 0.975170, 0.23], [0.0, 0.0, 0.0, 1.0]])


def unposed(x, pose=POSE):
    """p with pose p = x, exact for POSE and dyadic x."""
    R, t = pose[:3, :3], pose[:3, 3]
    return (x - t) @ R


def sample_cases():
    """[(name, blocks, min_count, points [n,3], pose or None, expected dict(flag, value, grad) or None)]; expected None: the oracle alone."""
    cases = []
    inside = np.array([[2.25, 3.0, 1.125], [0.5, 0.25, 6.75], [5.0, 5.0, 5.0], [6.875, 0.0, 0.0625]])
    cases.append(('linear_inside_one_block', [linear_block((0, 0, 0))], 1, at_q(inside), None, expect_linear(inside)))
    centre = np.array([[2.0, 3.0, 1.0], [0.0, 0.0, 0.0], [6.0, 6.0, 6.0]])                     # f = 0: the cell above the voxel
    cases.append(('on_a_voxel_centre', [linear_block((0, 0, 0))], 1, at_q(centre), None, expect_linear(centre)))
    straddle = np.array([[7.0, 3.0, 1.0], [7.0, 7.0, 1.0], [7.0, 7.0, 7.0], [7.5, 7.25, 7.125]])   # 2, 4, 8 and 8 blocks
    cases.append(('local_seven_straddles_blocks', around(), 1, at_q(straddle), None, expect_linear(straddle)))
    neg = np.array([[-0.25, 2.0, 2.0], [2.0, -0.5, 2.0], [2.0, 2.0, -0.75], [-0.25, -0.25, -0.25], [-1.0, -1.0, -1.0], [-7.5, -8.0, -3.25]])
    cases.append(('across_block_zero_and_minus_one', around(), 1, at_q(neg), None, expect_linear(neg)))
    # the corner (8, 8, 8) of the last straddling points lies in the missing block; the first two do not touch it
    want = expect_linear(straddle)
    for row in (2, 3):
        want['flag'][row], want['value'][row], want['grad'][row] = S_UNOBSERVED, np.nan, 0.0
    cases.append(('missing_block_at_one_corner', around(exclude=[(1, 1, 1)]), 1, at_q(straddle), None, want))
    # voxel (3, 4, 2), corner 7 of the first point's cell, seen twice where the others were seen three times
    b, s, c = linear_block((0, 0, 0), count=3)
    s[3, 4, 2], c[3, 4, 2] = s[3, 4, 2] // 3 * 2, 2
    want = expect_linear(inside)
    want['flag'][0], want['value'][0], want['grad'][0] = S_UNOBSERVED, np.nan, 0.0
    cases.append(('count_one_below_min_count', [(b, s, c)], 3, at_q(inside), None, want))
    cases.append(('count_equals_min_count', [(b, s, c)], 2, at_q(inside), None, expect_linear(inside)))
    zero = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 1.0], [4.0, 2.0, 2.0]])                        # sum == 0 is an observed zero
    want = expect_linear(zero)
    assert not want['value'].any()
    cases.append(('sum_zero', [linear_block((0, 0, 0))], 1, at_q(zero), None, want))
    clamped = np.array([[1.25, 2.5, 3.75], [0.0, 0.0, 0.0]])
    cases.append(('all_corners_clamped', [constant_block((0, 0, 0))], 1, at_q(clamped), None,
                  dict(flag=np.zeros(2, np.uint8), value=np.full(2, TAU), grad=np.zeros((2, 3)))))
    bad = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [1e300, 1.0, 1.0]])
    cases.append(('not_finite', [linear_block((0, 0, 0))], 1, bad, None, expect_flag(4, S_RANGE)))
    # q one ulp inside and outside both ends of [-2^23, 2^23 - 1); the blocks at the ends hold the constant 0.5
    lo_in, lo_out = -float(EDGE), np.nextafter(-float(EDGE), -np.inf)
    hi_in, hi_out = np.nextafter(float(EDGE - 1), -np.inf), float(EDGE - 1)
    ends = np.array([[lo_in, 2.25, 1.5], [lo_out, 2.25, 1.5], [hi_in, 2.25, 1.5], [hi_out, 2.25, 1.5], [2.25, lo_in, 1.5], [2.25, 1.5, hi_out]])
    want = dict(flag=np.array([0, S_RANGE, 0, S_RANGE, S_UNOBSERVED, S_RANGE], np.uint8),
                value=np.array([1.0, np.nan, 1.0, np.nan, np.nan, np.nan]), grad=np.zeros((6, 3)))
    cases.append(('range_ends', [constant_block((-2 ** 20, 0, 0), 0.5), constant_block((2 ** 20 - 1, 0, 0), 0.5)], 1, at_q(ends), None, want))
    cases.append(('exact_pose', around(), 1, unposed(at_q(np.concatenate([inside, straddle, neg]))), POSE,
                  expect_linear(np.concatenate([inside, straddle, neg]))))
    rng = np.random.default_rng(5)
    cases.append(('generic_pose_oracle_only', around(), 1, rng.uniform(-9.0, 17.0, (400, 3)), GENERIC_POSE, None))
    cases.append(('generic_points_oracle_only', around(exclude=[(0, 0, 0)]), 1, rng.uniform(-9.0, 17.0, (400, 3)), None, None))
    return cases



# ---- the row ---------------------------------------------------------------------------------------------------------------------------
def row_edge_sample():
    """A hand-made sample of six points and (thr, max_residual): the kept flags are [1, 1, 0, 0, 0, 0] --
    dist < thr; dist == thr (kept); dist > thr; dist == max_residual under a larger thr is tested apart; flag 1; flag 2."""
    x = np.array([[1.0, 2.0, 3.0], [0.5, -1.0, 2.0], [2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [np.nan, 0.0, 0.0], [3.0, 3.0, 3.0]])
    value = np.array([0.25, -0.5, 0.75, 2.0, np.nan, np.nan])
    grad = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    dist = np.where(np.isnan(value), np.inf, np.abs(value))
    flag = np.array([0, 0, 0, 0, 1, 2], np.uint8)
    return dict(x=x, value=value, grad=grad, dist=dist, flag=flag)


def row_by_hand():
    """The 30 sums of the two kept points of row_edge_sample at thr = 0.5: J = [x cross g, g]."""
    J0, r0 = np.array([2.0, -1.0, 0.0, 0.0, 0.0, 1.0]), 0.25          # (1,2,3) x (0,0,1) = (2, -1, 0)
    J1, r1 = np.array([0.0, 2.0, 1.0, 1.0, 0.0, 0.0]), -0.5           # (0.5,-1,2) x (1,0,0) = (0, 2, 1)
    row = []
    for a in range(6):
        for b in range(a, 6):
            row.append(J0[a] * J0[b] + J1[a] * J1[b])
    row += list(J0 * r0 + J1 * r1) + [2.0, r0 * r0 + r1 * r1, 2.0]
    return np.array(row)


def random_sample(m, seed=3, share_invalid=0.15):
    """A sample of m points as the sampling kernel could have written it (values within tau = 0.3, unit-ish gradients, some invalid)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5.0, 5.0, (m, 3))
    value = rng.uniform(-0.3, 0.3, m)
    grad = rng.normal(size=(m, 3))
    flag = np.where(rng.random(m) < share_invalid, rng.integers(1, 3, m), 0).astype(np.uint8)
    value[flag != 0], grad[flag != 0] = np.nan, 0.0
    dist = np.where(flag != 0, np.inf, np.abs(value))
    return dict(x=x, value=value, grad=grad, dist=dist, flag=flag)


ROW_SIZES = [1, 63, 64, 255, 256, 257, 131072, 131073]          # the last two: kBlock kIcpBlocksMax = 256 x 512 and one past it


def totals_bound(n_pairs, abs_totals):
    """test_gpu_slam_parity's derived bound: n + 16 roundings of at most 2^-53 of the sum of |term| each."""
    return (n_pairs + 16) * 2.0 ** -53 * abs_totals


# ---- a plane seen from two viewpoints (the analytic check) -----------------------------------------------------------------------------
def plane_scan(vp, n_side=40, half=2.0, z=0.0):
    """Rays from ``vp`` (sensor frame = world frame) to a grid of points on the plane z = ``z``: dict(points, vps, dirs, depth)."""
    g = np.linspace(-half, half, n_side)
    pts = np.stack([np.repeat(g, n_side), np.tile(g, n_side), np.full(n_side * n_side, z)], axis=1)
    vps = np.tile(np.asarray(vp, np.float64), (len(pts), 1))
    ray = pts - vps
    depth = np.linalg.norm(ray, axis=1)
    return dict(points=pts, vps=vps, dirs=ray / depth[:, None], depth=depth)


# ---- the step-by-step scene (tests/test_gpu_tsdf_track.py) and its host-built copy -----------------------------------------------------
STEP = dict(slam_tsdf_voxel_size=0.4, slam_tsdf_trunc=1.2)        # 20 000 rays a scan over 832 m^2 of wall: voxels that ray density can fill
STEP_FUSED, STEP_SCAN = (0, 1, 3), 2                              # the scans fused at the ground truth, and the one registered
# the largest change of the reference mapper's per-iteration poses over 200 random orders of its sums on the host-built copy of the
# scene (measured on the CPU; test_tsdf_track_host recomputes it over a few orders); the device's pose bar is 2 000 x this
POSE_SENSITIVITY = 1.734723475976807e-18


def roombox_host_scene():
    """(scans [dict(points, vps, dirs, depth)], ground-truth poses) of RoomBoxDataset(20 000 points, 6 poses), rays formed in numpy."""
    from depth_correction_amd.dataset import RoomBoxDataset
    scans, gt = [], []
    for cloud, pose in RoomBoxDataset(n_pts=20000, n_poses=6, dtype=np.float64):
        pts = np.stack([cloud[f] for f in 'xyz'], axis=1).astype(np.float64)
        depth = np.linalg.norm(pts, axis=1)
        scans.append(dict(points=pts, vps=np.zeros_like(pts), dirs=pts / depth[:, None], depth=depth))
        gt.append(np.asarray(pose, np.float64))
    return scans, np.stack(gt)
