"""The motion model of a moving sweep on the host (numpy): what render.SweepModel, preproc.deskew_cloud, dataset.DeskewedDataset and
slam.run_slam share.  The per-point arithmetic of the kernels is csrc/dc_sweepmath.h; the definition is in include/dc_hip.h and DESIGN
"Moving-sweep rendering and de-skew".

A scan has a start pose (world from sensor at sweep time 0) and a twist (v, w) -- translation, then axis-angle, the layout of
matrix_to_xyz_axis_angle -- expressed in the start frame and covering the whole sweep.  At sweep time tau the sensor stands at
start . D(tau), D(tau) = [Exp(tau w) | tau v]: rotation and translation interpolated separately, not the SE(3) exponential.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ['rotation_matrix', 'sweep_matrix', 'twists_from_poses', 'motion_twist', 'shifted_twist', 'sweep_times', 'check_fraction_ref']


def rotation_matrix(a):
    """Exp(a) 3 x 3 of the axis-angle vector a (Rodrigues, with the kernels' B = (sin(th/2) / (th/2))^2 / 2)."""
    a = np.asarray(a, dtype=np.float64).reshape(3)
    th = float(np.linalg.norm(a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    if th < 2.0 ** -26:
        A, B = 1.0, 0.5
    else:
        A, B = math.sin(th) / th, 0.5 * (math.sin(0.5 * th) / (0.5 * th)) ** 2
    return np.eye(3) + A * K + B * (K @ K)


def sweep_matrix(twist, tau):
    """D(tau) = [Exp(tau w) | tau v] as a 4 x 4 matrix."""
    twist = np.asarray(twist, dtype=np.float64).reshape(6)
    D = np.eye(4)
    D[:3, :3] = rotation_matrix(tau * twist[3:])
    D[:3, 3] = tau * twist[:3]
    return D


def motion_twist(T):
    """The twist (v, w) [6] of the rigid motion T (4 x 4): matrix_to_xyz_axis_angle."""
    import torch
    from .transform import matrix_to_xyz_axis_angle
    return matrix_to_xyz_axis_angle(torch.as_tensor(np.asarray(T, dtype=np.float64).reshape(1, 4, 4))).numpy()[0]


def twists_from_poses(poses, fraction=1.0):
    """Twists [N,6] of the scans taken at ``poses`` [N,4,4] under constant velocity between scans: the twist of T_i^-1 T_{i+1} times
    ``fraction`` (the part of the inter-scan period a sweep takes); the last scan repeats the previous twist, a single scan gets zero."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    n = poses.shape[0]
    if n < 2:
        return np.zeros((n, 6))
    tw = np.stack([motion_twist(np.linalg.solve(poses[i], poses[i + 1])) for i in range(n - 1)])
    return float(fraction) * np.concatenate([tw, tw[-1:]])


def shifted_twist(twist, ref):
    """The twist (Exp(-ref w) v, w) with D(ref)^-1 D(tau) = D(tau - ref; that twist): the sweep seen from the frame at sweep time ref."""
    twist = np.asarray(twist, dtype=np.float64).reshape(6)
    return np.concatenate([rotation_matrix(-float(ref) * twist[3:]) @ twist[:3], twist[3:]])


def check_fraction_ref(fraction, ref):
    fraction, ref = float(fraction), float(ref)
    if not 0.0 < fraction <= 1.0:
        raise ValueError('fraction must lie in (0, 1], got %r' % (fraction,))
    if not 0.0 <= ref <= 1.0:
        raise ValueError('ref must lie in [0, 1], got %r' % (ref,))
    return fraction, ref


def sweep_times(dirs, fov, direction='ccw'):
    """Sweep time tau float64 [R] in [0, 1) of every ray of lidar_directions' pattern from its azimuth: tau = ((atan2(d_y, d_x) - a0)
    mod 2 pi) / F_h with a0 = -F_h / 2 + 1e-3, the yaw of the pattern's first segment, clamped below 1; 'cw' sweeps the other way,
    1 - tau of that, clamped the same way.  ``fov`` = (vertical, horizontal) degrees.  Deterministic."""
    if direction not in ('ccw', 'cw'):
        raise ValueError("direction must be 'ccw' or 'cw', got %r" % (direction,))
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    fh = math.radians(float(fov[1]))
    if not 0.0 < fh <= 2.0 * math.pi * (1.0 + 1e-12):
        raise ValueError('the horizontal field of view must lie in (0, 360] degrees, got %r' % (fov[1],))
    a0 = -fh / 2.0 + 1e-3
    below_one = np.nextafter(1.0, 0.0)
    tau = np.minimum(np.mod(np.arctan2(d[:, 1], d[:, 0]) - a0, 2.0 * math.pi) / fh, below_one)
    if direction == 'cw':
        tau = np.minimum(1.0 - tau, below_one)
    return tau
