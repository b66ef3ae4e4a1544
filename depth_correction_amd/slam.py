"""SLAM evaluation without ROS: the perturbed odometry and the metric of scripts/robot_data:123-204 and a scan-to-map point-to-plane
ICP mapper configured like the reference's norlab_icp_mapper (config/slam/icp.yaml, input_filters.yaml, launch/slam.launch).

The mapper is a restatement of that configuration, not libpointmatcher; DESIGN "SLAM evaluation" states the algorithm and its
deviations.  Its device state is the map (points and the normals of the scans they came from), the map's k-NN grid and one
registration's state; an ICP iteration runs on the device without the host (csrc/dc_slam.hip), which reads one status word every
``status_every`` iterations.  With cfg.slam_compute_prob_dynamic every map point also carries the probability that it belongs to
something that moved (csrc/dc_dynamic.hip, DESIGN "Dynamic points in the map").

With cfg.slam_map = 'tsdf' the map is a sparse TSDF volume instead (TsdfMapper, csrc/dc_tsdf_track.hip, DESIGN "Scan-to-TSDF
registration"): a scan is registered against the fused volume by the same loop and the same finish kernel, without a nearest-neighbour
search, and every registered scan is fused into it.  make_mapper(cfg) picks the class.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nv
from . import ops
from .config import Config, SLAM
from .utils import delta_transform, rotation_angle, translation_norm

__all__ = ['IcpMapper', 'MapperScan', 'TsdfMapper', 'TsdfScan', 'make_mapper', 'LAUNCHES_PER_ITERATION', 'LAUNCHES_PER_ITERATION_CT',
           'LAUNCHES_PER_ITERATION_TSDF', 'dynamic_params', 'mapper_input', 'odometry_cov', 'odometry_poses',
           'path_lengths', 'run_slam', 'slam_errors']

# launches of one ICP iteration: dc_knn_grid_query 3 (moved queries, the 16-lanes-per-query search, the tail search), dc_quantile 18
# (a state memset, 8 x histogram + pick, next value, threshold), dc_icp_accumulate 1, dc_icp_finish 1
LAUNCHES_PER_ITERATION = 23
# the sweep-aware iteration: dc_deskew 1 more, dc_icp_ct_accumulate and dc_icp_ct_finish in the places of the two last
LAUNCHES_PER_ITERATION_CT = 24
# the scan-to-TSDF iteration: dc_tsdf_sparse_sample 1, dc_quantile 18, dc_tsdf_icp_accumulate 1, dc_icp_finish 1 -- no search
LAUNCHES_PER_ITERATION_TSDF = 21
FAILED = ('empty', 'too_few_pairs', 'singular', 'not_finite', 'bound')


def odometry_cov(odom_cov):
    """The 6 x 6 covariance of the odometry noise from the forms robot_data:56-68 accepts: a scalar (every variance), [rot, trans],
    six variances (the diagonal) or a 6 x 6 matrix; None = no noise."""
    if odom_cov is None:
        return None
    if isinstance(odom_cov, str):
        import yaml
        odom_cov = yaml.safe_load(odom_cov)
    if isinstance(odom_cov, (int, float)):
        odom_cov = 6 * [float(odom_cov)]
    cov = np.asarray(odom_cov, dtype=np.float64)
    if cov.shape == (2,):
        cov = np.array(3 * [cov[0]] + 3 * [cov[1]])
    if cov.shape == (6,):
        cov = np.diag(cov)
    if cov.shape != (6, 6):
        raise ValueError('odom_cov must be a scalar, 2 or 6 variances or a 6 x 6 matrix, got shape %s' % (cov.shape,))
    return cov


def odometry_poses(gt_poses, odom_cov, seed=135):
    """Odometry of robot_data.precompute_poses / random_transform: odom[0] = gt[0], odom[i] = odom[i-1] delta(gt[i-1], gt[i]) T(noise_i)
    with noise_i ~ N(0, odom_cov) drawn from default_rng(seed) and T = euler_matrix(*noise[:3]) with noise[3:] as translation."""
    from .dataset import euler_matrix
    gt = np.asarray(gt_poses, dtype=np.float64)
    cov = odometry_cov(odom_cov)
    rng = np.random.default_rng(seed)
    odom = gt.copy()
    for i in range(1, len(gt)):
        delta = delta_transform(gt[i - 1], gt[i])
        if cov is not None:
            noise = rng.multivariate_normal(np.zeros((6,)), cov)
            T = euler_matrix(*noise[:3])
            T[:3, 3] = noise[3:]
            delta = np.matmul(delta, T)
        odom[i] = np.matmul(odom[i - 1], delta)
    return odom


def path_lengths(gt_poses):
    """Travelled distance at every pose (robot_data:127-141): 0, then the sum of the ground-truth steps' translation norms."""
    gt = np.asarray(gt_poses, dtype=np.float64)
    out = [0.0]
    for i in range(1, len(gt)):
        out.append(out[i - 1] + translation_norm(delta_transform(gt[i - 1], gt[i])))
    return np.asarray(out)


def slam_errors(slam_poses, gt_poses, lengths):
    """(r_angle, t_norm, rel_angle, rel_offset): the means over every pose, index 0 included, of robot_data.evaluate_pose's errors of
    delta(slam, gt); the relative ones divide by the path length and are 0 where it is 0 (robot_data:153-187)."""
    r, t, ra, ro = [], [], [], []
    for slam, gt, length in zip(slam_poses, gt_poses, lengths):
        delta = delta_transform(slam, gt)
        r_angle, t_norm = rotation_angle(delta), translation_norm(delta)
        r.append(r_angle)
        t.append(t_norm)
        ra.append(r_angle / length if length > 0. else 0.)
        ro.append(t_norm / length if length > 0. else 0.)
    return tuple(float(np.mean(v)) for v in (r, t, ra, ro))


def mapper_input(cloud, model, cfg: Config):
    """One scan as the mapper receives it (launch/slam_eval.launch): the depth and grid filters of cfg, then, with a model, the
    correction node (online.correct_cloud).  A DepthCloud in the sensor frame."""
    from .depth_cloud import DepthCloud
    from .online import correct_cloud
    from .preproc import filtered_cloud
    cloud = filtered_cloud(cloud, cfg)
    if cfg.slam_ct and 't' in (getattr(getattr(cloud, 'dtype', None), 'names', None) or ()):
        return _timed_input(cloud, model, cfg)           # (only the sweep-aware registration reads the times)
    if model is not None:
        return correct_cloud(cloud, model, cfg)
    if isinstance(cloud, DepthCloud):
        return cloud
    return DepthCloud.from_structured_array(cloud, dtype=np.float64, device=cfg.device)


def _timed_input(cloud, model, cfg: Config):
    """mapper_input for a structured cloud with sweep times (the field ``t``; the host filters above select rows of the structured
    array, times included): the same DepthCloud with the times as its ``sweep_t`` f64 [N].  The correction is online.correct_cloud
    itself, given the cloud it would have made from the array; its filters and the model's copy take the times along
    (DepthCloud.sweep_t)."""
    from .depth_cloud import DepthCloud
    from .online import correct_cloud
    t = torch.as_tensor(np.ascontiguousarray(cloud['t'], dtype=np.float64), device=cfg.device)
    if model is None:
        dc = DepthCloud.from_structured_array(cloud, dtype=np.float64, device=cfg.device)
        dc.sweep_t = t
        return dc
    dc = DepthCloud.from_structured_array(cloud, dtype=cfg.numpy_float_type(), device=cfg.device)     # local_feature_cloud's own call
    dc.sweep_t = t
    dc = correct_cloud(dc, model, cfg)
    if dc.sweep_t is None or dc.sweep_t.shape[0] != len(dc):
        raise RuntimeError('the sweep times did not follow their points through the correction (%s times, %d points)'
                           % ('no' if dc.sweep_t is None else dc.sweep_t.shape[0], len(dc)))
    return dc


def dynamic_params(cfg: Config):
    """The parameters of the dynamic-point rule from cfg, checked (ValueError): dict(prior, threshold, beam_half_angle, chord_max,
    epsilon_a, epsilon_d, alpha, beta, max_range) with chord_max = 2 sin(beam_half_angle), the chord of twice the half angle."""
    import math
    p = dict(prior=float(cfg.slam_prior_dynamic), threshold=float(cfg.slam_threshold_dynamic), beam_half_angle=float(cfg.slam_beam_half_angle),
             epsilon_a=float(cfg.slam_epsilon_a), epsilon_d=float(cfg.slam_epsilon_d), alpha=float(cfg.slam_alpha), beta=float(cfg.slam_beta),
             max_range=float(cfg.slam_sensor_max_range))
    if not 0.0 < p['beam_half_angle'] < math.pi / 2:
        raise ValueError('slam_beam_half_angle must lie in (0, pi/2), got %r' % p['beam_half_angle'])
    for name in ('epsilon_a', 'epsilon_d'):
        if not (p[name] >= 0.0 and math.isfinite(p[name])):
            raise ValueError('slam_%s must be finite and >= 0, got %r' % (name, p[name]))
    for name in ('alpha', 'beta'):
        if not 0.0 < p[name] < 1.0:
            raise ValueError('slam_%s must lie in (0, 1), got %r' % (name, p[name]))
    if not 0.0 < p['threshold'] <= 1.0:
        raise ValueError('slam_threshold_dynamic must lie in (0, 1], got %r' % p['threshold'])
    if not 0.0 <= p['prior'] <= 1.0:
        raise ValueError('slam_prior_dynamic must lie in [0, 1], got %r' % p['prior'])
    if math.isnan(p['max_range']):
        raise ValueError('slam_sensor_max_range must not be NaN')
    p['chord_max'] = 2.0 * math.sin(p['beam_half_angle'])
    return p


class MapperScan(object):
    """A reading as the ICP uses it: points fp64 [M,3] in the sensor frame, their normals [M,3] (k nearest neighbours inside the scan,
    oriented toward the sensor: input_filters.yaml) and depths [M]; ``t`` (optional) fp64 [M], the sweep time of every point."""

    def __init__(self, points, normals, depth, t=None):
        self.points, self.normals, self.depth, self.t = points, normals, depth, t

    def __len__(self):
        return self.points.shape[0]


def _registration_loop(mapper, prior, launches, iterate):
    """The loop every mapper's registration runs (IcpMapper's two, TsdfMapper's): icp_init from ``prior`` into the mapper's state and
    status, ``iterate(pose_d)`` (one iteration of ``launches`` launches, queued; pose_d the device-side estimate) ``status_every`` at a
    time with one status read per group, and the read-back.  -> (pose, info), the prior's copy when the registration failed."""
    cfg = mapper.cfg
    pose_d = mapper.state[nv.DC_ICP_STATE_POSE:nv.DC_ICP_STATE_POSE + 16].view(4, 4)
    ops.icp_init(torch.as_tensor(prior, device=mapper.device), mapper.state, mapper.status)
    done = 0
    code = 0
    while done < cfg.icp_max_iters:
        for _ in range(min(mapper.status_every, cfg.icp_max_iters - done)):
            iterate(pose_d)
            done += 1
        st = mapper.status.cpu()
        mapper.host_reads += 1
        code = int(st[0])
        if code != 0:
            break
    st = mapper.state.cpu().numpy()
    iters = int(mapper.status[1].item())
    info = mapper._info(nv.ICP_STATUS[code], iters, float(st[nv.DC_ICP_STATE_OVERLAP]), int(st[nv.DC_ICP_STATE_PAIRS]),
                        float(st[nv.DC_ICP_STATE_SSE]), launches=launches)
    if not info['ok']:
        return prior.copy(), info
    return st[nv.DC_ICP_STATE_POSE:nv.DC_ICP_STATE_POSE + 16].reshape(4, 4).copy(), info


class IcpMapper(object):
    """Scan-to-map point-to-plane ICP and map of the reference's mapper configuration (see DESIGN "SLAM evaluation").

    ``register(scan, prior)`` -> (pose, info): the registered pose (the prior when the registration fails: info['ok'] is False) and
    info (status, iterations, overlap, pairs, sse); ``update(scan, pose, overlap=None)`` adds the reading points that are new to the
    map; ``map_points()`` -> (points, normals) of the map.  ``update_dynamic(scan, pose)`` updates the map points' probabilities of
    being dynamic (``map_dynamic()``) from a registered scan; ``update`` runs it first when cfg.slam_compute_prob_dynamic is set, and
    with cfg.slam_cut_dynamic the registration matches against the points below cfg.slam_threshold_dynamic only."""

    def __init__(self, cfg: Config, device=None, status_every=4):
        if not (1 <= int(cfg.icp_smooth_length) <= nv.DC_ICP_MAX_SMOOTH):
            raise ValueError('icp_smooth_length must be in 1..%d' % nv.DC_ICP_MAX_SMOOTH)
        self.cfg = cfg
        self.device = torch.device(device or cfg.device)
        if self.device.type != 'cuda':
            raise RuntimeError('IcpMapper runs on the GPU (depth_correction_amd has no CPU path)')
        self.status_every = max(1, int(status_every))
        self.knn = int(cfg.icp_knn)
        self.n_map = 0
        self._pts = torch.empty((0, 3), dtype=torch.float64, device=self.device)
        self._nrm = torch.empty((0, 3), dtype=torch.float64, device=self.device)
        self._prob = torch.empty((0,), dtype=torch.float64, device=self.device)
        self.dyn = dynamic_params(cfg) if (cfg.slam_compute_prob_dynamic or cfg.slam_cut_dynamic) else None
        self.n_dynamic = 0             # map points with P >= threshold (a host count, refreshed by update_dynamic and update)
        self.last_dyn = None           # what the last update() got from update_dynamic, None when it did not run
        self._dyn_ws = None            # workspace of the reading directions' grid
        self._eye = None
        self._version = 0              # counts the changes of the map and of its probabilities
        self._ref = None               # the reference cloud of slam_cut_dynamic: dict(version, grid, points, normals, rows)
        self.grid = None
        self.grid_builds = 0
        self.state = torch.zeros((nv.DC_ICP_STATE_COUNT,), dtype=torch.float64, device=self.device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=self.device)
        self.host_reads = 0            # status reads of the last registration
        self.quantile_ws = torch.empty((max(int(nv.lib().dc_quantile_workspace_bytes()), 1),), dtype=torch.uint8, device=self.device)

    # ---- input --------------------------------------------------------------------------------------------------------------
    def prepare(self, cloud):
        """MapperScan of a DepthCloud / points (sensor frame): fp64 points, k = cfg.slam_normals_k normals oriented toward the sensor
        (computed here even when a correction computed normals of its own), depths."""
        from .depth_cloud import DepthCloud
        if isinstance(cloud, MapperScan):
            return cloud
        if isinstance(cloud, DepthCloud):
            pts = cloud.get_points().detach().to(device=self.device, dtype=torch.float64).contiguous()
            vps = cloud.vps.detach().to(device=self.device, dtype=torch.float64).expand_as(pts).contiguous()
        else:
            if getattr(getattr(cloud, 'dtype', None), 'names', None):
                cloud = DepthCloud.from_structured_array(cloud, dtype=np.float64, device=self.device)
                return self.prepare(cloud)
            pts = torch.as_tensor(cloud, dtype=torch.float64, device=self.device).reshape(-1, 3).contiguous()
            vps = torch.zeros_like(pts)
        m = pts.shape[0]
        if m == 0:
            z = torch.empty((0, 3), dtype=torch.float64, device=self.device)
            return MapperScan(z, z.clone(), torch.empty((0,), dtype=torch.float64, device=self.device))
        dc = DepthCloud.from_points(pts, vps=vps, dtype=torch.float64, device=self.device)
        dc.update_all(k=min(int(self.cfg.slam_normals_k), m))
        normals = torch.nan_to_num(dc.normals.detach(), nan=0.0).to(torch.float64).contiguous()
        depth = dc.depth.detach().reshape(-1).to(torch.float64).contiguous()
        t = getattr(cloud, 'sweep_t', None)
        if t is not None:
            t = t.detach().to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
            if t.shape[0] != m:
                raise ValueError('%d sweep times for %d points' % (t.shape[0], m))
        return MapperScan(pts, normals, depth, t)

    # ---- registration ---------------------------------------------------------------------------------------------------------
    def _info(self, status, iterations=0, overlap=0.0, pairs=0, sse=0.0, launches=LAUNCHES_PER_ITERATION):
        return dict(status=status, ok=status not in FAILED, iterations=iterations, overlap=overlap, pairs=pairs, sse=sse,
                    host_reads=self.host_reads, launches_per_iteration=launches)

    def register(self, scan, prior, twist=None):
        """Pose of ``scan`` in the map from ``prior`` (4 x 4): ICP iterations queued ``status_every`` at a time, one status read
        after each group.  An empty scan or failed registration returns the prior; an empty map returns the prior with status
        'init' (the first scan initialises the map).  With cfg.slam_ct and a scan that has sweep times the twist of the sweep is
        estimated with the pose (register_ct), from ``twist`` [6] = (v0, w0) as start and prior (zero when None)."""
        cfg = self.cfg
        scan = self.prepare(scan)
        if cfg.slam_ct and scan.t is not None:
            return self.register_ct(scan, prior, twist)
        prior = np.asarray(prior, dtype=np.float64).reshape(4, 4)
        self.host_reads = 0
        m = len(scan)
        if m == 0:
            return prior.copy(), self._info('empty')
        if self.n_map == 0:
            return prior.copy(), self._info('init')
        grid, map_pts, map_nrm, _ = self.reference(m)
        if grid is None:
            return prior.copy(), self._info('too_few_pairs')
        partials = torch.empty((ops.icp_blocks(m), nv.DC_ICP_PARTIALS), dtype=torch.float64, device=self.device)
        return self._run_registration(m, prior, LAUNCHES_PER_ITERATION, lambda pose_d, idx, dist, thr, cos_min: self.iteration(
            scan, pose_d, idx, dist, thr, partials, map_pts, map_nrm, cos_min, grid=grid))

    def _run_registration(self, m, prior, launches, iterate):
        """What register and register_ct share once there is something to match against: the match / distance / threshold buffers
        of an m-point scan, icp_init from ``prior``, ``iterate(pose_d, idx, dist, thr, cos_min)`` (one iteration of ``launches``
        launches, queued) ``status_every`` at a time with one status read per group, and the read-back.  -> (pose, info), the
        prior's copy when the registration failed."""
        cfg = self.cfg
        dev, k = self.device, self.knn
        idx = torch.empty((m, k), dtype=torch.int32, device=dev)
        dist = torch.empty((m, k), dtype=torch.float64, device=dev)
        thr = torch.empty((1,), dtype=torch.float64, device=dev)
        cos_min = float(np.cos(cfg.icp_max_normal_angle))
        return _registration_loop(self, prior, launches, lambda pose_d: iterate(pose_d, idx, dist, thr, cos_min))

    def _match(self, points, pose_d, idx, dist, thr, grid):
        """The two launches every iteration starts with: the k-NN of ``points`` moved by the device-side pose, the trimmed threshold."""
        cfg = self.cfg
        ops.knn_grid_query(self.grid if grid is None else grid, points, pose_d, self.knn, r=cfg.icp_max_dist, stop=self.status, idx=idx,
                           dist=dist)
        ops.quantile(dist, cfg.icp_trim_ratio, stop=self.status, out=thr, ws=self.quantile_ws)

    def iteration(self, scan, pose_d, idx, dist, thr, partials, map_pts, map_nrm, cos_min, kept=None, grid=None):
        """One ICP iteration, queued on the stream: match, trimmed threshold, pairs and partials, solve and update.  ``grid`` is the
        grid of ``map_pts`` (the whole map's unless given: reference())."""
        cfg = self.cfg
        self._match(scan.points, pose_d, idx, dist, thr, grid)
        ops.icp_accumulate(scan.points, scan.normals, map_pts, map_nrm, idx, dist, thr, cos_min, self.state, self.status, partials,
                           kept=kept)
        ops.icp_finish(partials, len(scan), self.state, self.status, cfg.icp_min_diff_rot, cfg.icp_min_diff_trans, cfg.icp_smooth_length,
                       cfg.icp_max_iters, cfg.icp_max_rotation, cfg.icp_max_translation)

    # ---- sweep-aware registration (DESIGN "Sweep-aware registration") ---------------------------------------------------------------
    def ct_params(self):
        """(beta_v, beta_w, max_twist_trans, max_twist_rot) of cfg, checked (ValueError)."""
        cfg = self.cfg
        beta = [float(b) for b in cfg.slam_ct_prior]
        mt = cfg.slam_ct_max_twist
        mt = [float(cfg.icp_max_translation), float(cfg.icp_max_rotation)] if mt is None else [float(b) for b in mt]
        if len(beta) != 2 or not all(b >= 0.0 and np.isfinite(b) for b in beta):
            raise ValueError('slam_ct_prior must be [beta_v, beta_w], finite and >= 0, got %r' % (cfg.slam_ct_prior,))
        if len(mt) != 2:
            raise ValueError('slam_ct_max_twist must be [trans, rot], got %r' % (cfg.slam_ct_max_twist,))
        return beta[0], beta[1], mt[0], mt[1]

    def ct_buffers(self, m):
        """The device buffers of a sweep-aware registration of an m-point scan: the twist state, the de-skewed points and normals
        (scratch, rewritten by every iteration), the scan offsets of dc_deskew and the block partials."""
        dev = self.device
        return dict(ct=torch.zeros((nv.DC_ICP_CT_STATE_COUNT,), dtype=torch.float64, device=dev),
                    q=torch.empty((m, 3), dtype=torch.float64, device=dev), nq=torch.empty((m, 3), dtype=torch.float64, device=dev),
                    off=torch.tensor([0, m], dtype=torch.int64, device=dev),
                    partials=torch.empty((ops.icp_blocks(m), nv.DC_ICP_CT_PARTIALS), dtype=torch.float64, device=dev))

    def register_ct(self, scan, prior, twist=None):
        """register() with the twist (v, w) of the sweep as six more unknowns: -> (pose at sweep time 0, info).  info['twist'] is the
        estimated twist (the prior twist when the registration fails) and info['deskewed'] the scan de-skewed by it (points and
        normals of a last dc_deskew, the depths as they were), which is what update / update_dynamic are to be given."""
        prior = np.asarray(prior, dtype=np.float64).reshape(4, 4)
        twist0 = np.zeros(6) if twist is None else np.asarray(twist, dtype=np.float64).reshape(6)
        if not np.isfinite(twist0).all() or float(np.linalg.norm(twist0[3:])) > np.pi:
            raise ValueError('the prior twist must be finite with a rotation of at most pi, got %r' % (twist0,))
        prm = self.ct_params()
        self.host_reads = 0
        m = len(scan)
        launches = LAUNCHES_PER_ITERATION_CT

        def ended(status, **kw):
            info = self._info(status, launches=launches, **kw)
            info['twist'], info['deskewed'] = twist0.copy(), scan
            return prior.copy(), info
        if m == 0:
            return ended('empty')
        if self.n_map == 0:
            # the first scan: nothing to register against, the map takes it de-skewed by the prior twist
            x, _, nx = ops.deskew(scan.points, scan.t, [0, m], twist0[None], normals=scan.normals)
            pose, info = ended('init')
            info['deskewed'] = MapperScan(x, nx, scan.depth, scan.t)
            return pose, info
        grid, map_pts, map_nrm, _ = self.reference(m)
        if grid is None:
            return ended('too_few_pairs')
        buf = self.ct_buffers(m)
        ops.icp_ct_init(torch.as_tensor(twist0, device=self.device), buf['ct'])
        pose, info = self._run_registration(m, prior, launches, lambda pose_d, idx, dist, thr, cos_min: self.iteration_ct(
            scan, pose_d, idx, dist, thr, buf, map_pts, map_nrm, cos_min, prm, grid=grid))
        if not info['ok']:
            info['twist'], info['deskewed'] = twist0.copy(), scan
            return pose, info
        tw = buf['ct'][nv.DC_ICP_CT_STATE_TWIST:nv.DC_ICP_CT_STATE_TWIST + 6]
        ops.deskew_device_twist(scan.points, scan.normals, scan.t, tw, buf['off'], buf['q'], buf['nq'])      # by the final twist
        info['twist'] = tw.cpu().numpy().copy()
        info['deskewed'] = MapperScan(buf['q'], buf['nq'], scan.depth, scan.t)
        return pose, info

    def iteration_ct(self, scan, pose_d, idx, dist, thr, buf, map_pts, map_nrm, cos_min, prm, kept=None, grid=None):
        """One sweep-aware iteration, queued on the stream: de-skew by the device's twist, match, trimmed threshold, pairs and
        partials, the 12 x 12 solve and the update of pose and twist.  ``buf`` from ct_buffers, ``prm`` from ct_params."""
        cfg = self.cfg
        tw = buf['ct'][nv.DC_ICP_CT_STATE_TWIST:nv.DC_ICP_CT_STATE_TWIST + 6]
        ops.deskew_device_twist(scan.points, scan.normals, scan.t, tw, buf['off'], buf['q'], buf['nq'])
        self._match(buf['q'], pose_d, idx, dist, thr, grid)
        ops.icp_ct_accumulate(scan.points, buf['q'], buf['nq'], scan.t, map_pts, map_nrm, idx, dist, thr, cos_min, self.state, buf['ct'],
                              self.status, buf['partials'], kept=kept)
        ops.icp_ct_finish(buf['partials'], len(scan), self.state, buf['ct'], self.status, cfg.icp_min_diff_rot, cfg.icp_min_diff_trans,
                          cfg.icp_smooth_length, cfg.icp_max_iters, cfg.icp_max_rotation, cfg.icp_max_translation, *prm)

    # ---- map ------------------------------------------------------------------------------------------------------------------
    def _ensure_grid(self, m):
        if self.grid is not None and self.grid.n == self.n_map and self.grid.n_query_max >= m:
            return
        n_query_max = max(m, self.grid.n_query_max if self.grid is not None else 0)
        self.grid = ops.knn_grid_build(self._pts[:self.n_map], n_query_max, self.knn,
                                       ws=self.grid.ws if self.grid is not None else None)
        self.grid_builds += 1

    def reference(self, m):
        """(grid, points, normals, rows) the registration of an m-point scan matches against: the whole map (rows None), or with
        cfg.slam_cut_dynamic the map rows ``rows`` (int32, ascending) whose P < threshold, compacted, with a grid of their own (the
        effect of a CutAtDescriptorThreshold filter on the reference cloud), rebuilt when the map or a probability changed.  grid is
        None when no static point is left."""
        n = self.n_map
        if not self.cfg.slam_cut_dynamic or self.n_dynamic == 0:
            self._ensure_grid(m)
            return self.grid, self._pts[:n], self._nrm[:n], None
        ref = self._ref
        if ref is None or ref['version'] != self._version or (ref['grid'] is not None and ref['grid'].n_query_max < m):
            (pts, nrm), rows = ops.compact_rows(self._prob[:n] < self.dyn['threshold'], [self._pts[:n], self._nrm[:n]], want_index=True)
            old = ref['grid'] if ref is not None else None
            grid = None
            if pts.shape[0] > 0:
                grid = ops.knn_grid_build(pts, max(m, old.n_query_max if old is not None else 0), self.knn,
                                          ws=old.ws if old is not None else None)
                self.grid_builds += 1
            ref = self._ref = dict(version=self._version, grid=grid, points=pts, normals=nrm, rows=rows)
        return ref['grid'], ref['points'], ref['normals'], ref['rows']

    # ---- dynamic points -------------------------------------------------------------------------------------------------------
    def update_dynamic(self, scan, pose, timer=None):
        """Update the map points' probabilities of being dynamic from ``scan`` registered at ``pose`` (DESIGN "Dynamic points in the
        map"): directions of the map points in range as the sensor sees them, each one's nearest reading direction within the
        beam (the grid k-NN over the reading's unit vectors), then the visibility test and the Bayesian update of the matched rows.
        Returns dict(in_range, matched, occluded, updated, dynamic): map points in range, matched to a beam, of those behind the
        beam's return / updated, and the map points with P >= threshold afterwards.  ``timer`` (optional) is called with a stage
        name after every stage (tools/dynamic_bench.py)."""
        prm = self.dyn if self.dyn is not None else dynamic_params(self.cfg)
        self.dyn = prm
        tick = timer if timer is not None else (lambda stage: None)
        scan = self.prepare(scan)
        n, m = self.n_map, len(scan)
        out = dict(in_range=0, matched=0, occluded=0, updated=0, dynamic=self.n_dynamic)
        if n == 0 or m == 0:
            return out
        dev = self.device
        pose_d = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(4, 4), device=dev)
        map_pts, map_nrm, prob = self._pts[:n], self._nrm[:n], self._prob[:n]
        u, _, u_ok = ops.dyn_directions(map_pts, pose_d, prm['max_range'])
        v, _, v_ok = ops.dyn_directions(scan.points, None, 0.0)
        tick('directions')
        (u,), rows = ops.compact_rows(u_ok, [u], want_index=True)
        (v,), vrows = ops.compact_rows(v_ok, [v], want_index=True)
        tick('compaction')
        out['in_range'] = int(u.shape[0])
        if u.shape[0] == 0 or v.shape[0] == 0:
            return out
        grid = ops.knn_grid_build(v, u.shape[0], 1, ws=self._dyn_ws)
        self._dyn_ws = grid.ws
        tick('grid_build')
        if self._eye is None:
            self._eye = torch.eye(4, dtype=torch.float64, device=dev)
        chord, idx = ops.knn_grid_query(grid, u, self._eye, 1, r=prm['chord_max'])
        chord, idx = chord.reshape(-1), idx.reshape(-1)
        match = torch.where(idx >= 0, vrows[idx.clamp(min=0).long()], idx)          # compacted reading rows -> rows of the scan
        tick('query')
        seen = torch.zeros((n,), dtype=torch.uint8, device=dev)
        ops.dyn_update(map_pts, map_nrm, pose_d, scan.points, rows, match, chord, prm['chord_max'], prm['epsilon_a'], prm['epsilon_d'],
                       prm['alpha'], prm['beta'], prm['threshold'], prm['max_range'], prob, seen)
        counts = torch.stack([(idx >= 0).sum(), (seen == 1).sum(), (seen == 2).sum(), (prob >= prm['threshold']).sum()]).cpu()
        tick('update')
        out['matched'], out['occluded'], out['updated'], out['dynamic'] = (int(c) for c in counts)
        self.n_dynamic = out['dynamic']
        if out['updated'] > 0:
            self._version += 1
        return out

    def map_dynamic(self):
        """P fp64 [N]: every map point's probability of being dynamic (the prior where nothing was computed)."""
        return self._prob[:self.n_map]

    def update(self, scan, pose, overlap=None):
        """Add the reading points of ``scan`` at ``pose`` whose nearest map point is farther than cfg.slam_min_dist_new_point and whose
        depth is <= cfg.slam_sensor_max_range -- unless ``overlap`` (of its registration) is >= cfg.slam_min_overlap.  The first scan
        initialises the map.  Returns the number of points added; the map's grid is rebuilt when it changes."""
        cfg = self.cfg
        scan = self.prepare(scan)
        m = len(scan)
        self.last_dyn = None
        if m == 0 or (self.n_map > 0 and overlap is not None and overlap >= cfg.slam_min_overlap):
            return 0
        pose_d = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(4, 4), device=self.device)
        if cfg.slam_compute_prob_dynamic and self.n_map > 0:
            # norlab's order: the probabilities of the points the map has, then the new points appended with the prior
            self.last_dyn = self.update_dynamic(scan, pose)
        dist1 = None
        if self.n_map > 0:
            self._ensure_grid(m)
            dist1, _ = ops.knn_grid_query(self.grid, scan.points, pose_d, 1)
            dist1 = dist1.reshape(-1)
        mask, pts, nrm = ops.map_select(scan.points, scan.normals, scan.depth, pose_d, dist1, cfg.slam_min_dist_new_point,
                                        cfg.slam_sensor_max_range)
        new_pts, new_nrm = ops.compact_rows(mask, [pts, nrm])
        added = new_pts.shape[0]
        if added == 0:
            return 0
        need = self.n_map + added
        if need > self._pts.shape[0]:
            cap = max(need, 2 * self._pts.shape[0])
            for name in ('_pts', '_nrm', '_prob'):
                old = getattr(self, name)
                grown = torch.empty((cap,) + tuple(old.shape[1:]), dtype=torch.float64, device=self.device)
                grown[:self.n_map] = old[:self.n_map]
                setattr(self, name, grown)
        self._pts[self.n_map:need] = new_pts
        self._nrm[self.n_map:need] = new_nrm
        prior = float(cfg.slam_prior_dynamic)
        self._prob[self.n_map:need] = prior
        if self.dyn is not None and prior >= self.dyn['threshold']:
            self.n_dynamic += added
        self.n_map = need
        self._version += 1
        self._ensure_grid(m)
        return added

    def clear(self):
        """Empty the map (points, normals, probabilities, grids); the buffers and the counters of grid builds stay."""
        self.n_map, self.n_dynamic = 0, 0
        self.last_dyn, self._ref, self.grid = None, None, None
        self._version += 1

    def map_points(self, static_only=False):
        """(points, normals) fp64 [N,3] of the map (world frame); ``static_only``: the rows with P < cfg.slam_threshold_dynamic."""
        pts, nrm = self._pts[:self.n_map], self._nrm[:self.n_map]
        if not static_only:
            return pts, nrm
        pts, nrm = ops.compact_rows(self._prob[:self.n_map] < float(self.cfg.slam_threshold_dynamic), [pts, nrm])
        return pts, nrm


class TsdfScan(object):
    """A reading as the TSDF mapper uses it: points fp64 [M,3] in the sensor frame for the registration, and the rays they came from
    (vps, dirs fp64 [M,3], depth fp64 [M,1]) for the fusion; no normals.  ``t`` is None (the sweep-aware registration has a point map)."""
    t = None

    def __init__(self, points, vps, dirs, depth):
        self.points, self.vps, self.dirs, self.depth = points, vps, dirs, depth

    def __len__(self):
        return self.points.shape[0]

    def cloud(self):
        from .depth_cloud import DepthCloud
        return DepthCloud(vps=self.vps, dirs=self.dirs, depth=self.depth)


def _tsdf_map_refusals(cfg: Config):
    """The switches that are rules of the point map and mean nothing for a TSDF map: ValueError."""
    for name in ('slam_ct', 'slam_compute_prob_dynamic', 'slam_cut_dynamic'):
        if getattr(cfg, name):
            raise ValueError("%s is a rule of the point map: not with slam_map='tsdf'" % name)


class TsdfMapper(object):
    """Frame-to-model tracking: every scan is registered against a sparse TSDF volume (reconstruction.SparseTsdfVolume) that fuses the
    registered scans (DESIGN "Scan-to-TSDF registration").  The surface of IcpMapper: ``register(scan, prior)`` -> (pose, info),
    ``update(scan, pose, overlap=None)`` fuses the scan's rays at the pose (every registered scan, whatever its overlap) and returns the
    rays used, ``map_points()``, ``clear()``, ``n_map`` (the volume's blocks); and ``volume`` / ``extract_mesh()``: the map the SLAM
    ends with is the reconstruction.  An iteration samples the volume at the moved points, takes the trimmed threshold of |distance|,
    builds the point-to-surface row and runs IcpMapper's finish; it has no nearest-neighbour search, and the map side has no normals
    and no minimum distance between points.  The prior must lie within about the truncation of the truth (the capture range)."""

    def __init__(self, cfg: Config, device=None, status_every=4):
        from .reconstruction import SparseTsdfVolume
        if not (1 <= int(cfg.icp_smooth_length) <= nv.DC_ICP_MAX_SMOOTH):
            raise ValueError('icp_smooth_length must be in 1..%d' % nv.DC_ICP_MAX_SMOOTH)
        _tsdf_map_refusals(cfg)
        self.cfg = cfg
        self.device = torch.device(device or cfg.device)
        if self.device.type != 'cuda':
            raise RuntimeError('TsdfMapper runs on the GPU (depth_correction_amd has no CPU path)')
        self.status_every = max(1, int(status_every))
        self.min_count = int(cfg.slam_tsdf_min_count)
        if self.min_count < 1:
            raise ValueError('slam_tsdf_min_count must be >= 1, got %r' % (cfg.slam_tsdf_min_count,))
        self.volume = SparseTsdfVolume(cfg.slam_tsdf_voxel_size, trunc=cfg.slam_tsdf_trunc, max_blocks=cfg.slam_tsdf_max_blocks,
                                       device=self.device)
        self.max_residual = self.volume.trunc if cfg.slam_tsdf_max_residual is None else float(cfg.slam_tsdf_max_residual)
        if not self.max_residual > 0.0:
            raise ValueError('slam_tsdf_max_residual must be > 0, got %r' % (cfg.slam_tsdf_max_residual,))
        self.n_dynamic, self.last_dyn = 0, None          # (run_slam reports them; a TSDF map has no dynamic-point rule)
        self.state = torch.zeros((nv.DC_ICP_STATE_COUNT,), dtype=torch.float64, device=self.device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=self.device)
        self.host_reads = 0
        self.quantile_ws = torch.empty((max(int(nv.lib().dc_quantile_workspace_bytes()), 1),), dtype=torch.uint8, device=self.device)

    @property
    def n_map(self):
        return self.volume.n_blocks

    def prepare(self, cloud):
        """TsdfScan of a DepthCloud / structured array / points (sensor frame; points alone are rays from the origin): the fp64 points
        and the rays next to them.  No normals are computed."""
        from .depth_cloud import DepthCloud
        if isinstance(cloud, TsdfScan):
            return cloud
        if not isinstance(cloud, DepthCloud):
            if getattr(getattr(cloud, 'dtype', None), 'names', None):
                cloud = DepthCloud.from_structured_array(cloud, dtype=np.float64, device=self.device)
            else:
                pts = torch.as_tensor(cloud, dtype=torch.float64, device=self.device).reshape(-1, 3).contiguous()
                if pts.shape[0] == 0:
                    return TsdfScan(pts, pts.clone(), pts.clone(), torch.empty((0, 1), dtype=torch.float64, device=self.device))
                cloud = DepthCloud.from_points(pts, vps=torch.zeros_like(pts), dtype=torch.float64, device=self.device)
        kw = dict(device=self.device, dtype=torch.float64)
        dirs = cloud.dirs.detach().to(**kw).contiguous()
        vps = cloud.vps.detach().to(**kw).expand_as(dirs).contiguous()
        depth = cloud.depth.detach().to(**kw).reshape(-1, 1).contiguous()
        pts = cloud.get_points().detach().to(**kw).contiguous()
        return TsdfScan(pts, vps, dirs, depth)

    def _info(self, status, iterations=0, overlap=0.0, pairs=0, sse=0.0, launches=LAUNCHES_PER_ITERATION_TSDF):
        return dict(status=status, ok=status not in FAILED, iterations=iterations, overlap=overlap, pairs=pairs, sse=sse,
                    host_reads=self.host_reads, launches_per_iteration=launches)

    def buffers(self, m):
        """The device buffers of a registration of an m-point scan: the sample (x, value, grad, dist, flag), the threshold, the block
        partials."""
        dev = self.device
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        return dict(x=f64(m, 3), value=f64(m), grad=f64(m, 3), dist=f64(m), flag=torch.empty((m,), dtype=torch.uint8, device=dev),
                    thr=f64(1), partials=f64(ops.icp_blocks(m), nv.DC_ICP_PARTIALS))

    def register(self, scan, prior):
        """Pose of ``scan`` in the volume from ``prior`` (4 x 4), by IcpMapper's loop.  An empty scan ('empty') or a failed registration
        returns the prior; an empty volume returns the prior with status 'init' (the first scan initialises the map)."""
        scan = self.prepare(scan)
        prior = np.asarray(prior, dtype=np.float64).reshape(4, 4)
        self.host_reads = 0
        m = len(scan)
        if m == 0:
            return prior.copy(), self._info('empty')
        if self.n_map == 0:
            return prior.copy(), self._info('init')
        buf = self.buffers(m)
        return _registration_loop(self, prior, LAUNCHES_PER_ITERATION_TSDF, lambda pose_d: self.iteration(scan, pose_d, buf))

    def iteration(self, scan, pose_d, buf, kept=None):
        """One iteration, queued on the stream: sample at the moved points, trimmed threshold, pairs and partials, solve and update."""
        cfg, vol = self.cfg, self.volume
        ops.tsdf_sparse_sample(vol._keys, vol._slots, vol._n_blocks, vol._sum, vol._count, vol.origin, vol.voxel_size, vol.trunc, scan.points,
                               pose=pose_d, min_count=self.min_count, stop=self.status, out=buf)
        ops.quantile(buf['dist'], cfg.icp_trim_ratio, stop=self.status, out=buf['thr'], ws=self.quantile_ws)
        ops.tsdf_icp_accumulate(buf, buf['thr'], self.max_residual, self.state, self.status, buf['partials'], kept=kept)
        ops.icp_finish(buf['partials'], len(scan), self.state, self.status, cfg.icp_min_diff_rot, cfg.icp_min_diff_trans, cfg.icp_smooth_length,
                       cfg.icp_max_iters, cfg.icp_max_rotation, cfg.icp_max_translation)

    def update(self, scan, pose, overlap=None):
        """Fuse the rays of ``scan`` at ``pose`` into the volume (depths up to cfg.slam_sensor_max_range); ``overlap`` is accepted and
        not used: a fused volume gains from every scan.  Returns the rays used."""
        scan = self.prepare(scan)
        if len(scan) == 0:
            return 0
        stats = self.volume.integrate(scan.cloud(), pose=np.asarray(pose, dtype=np.float64).reshape(4, 4),
                                      max_range=self.cfg.slam_sensor_max_range)
        return int(stats['rays_used'])

    def clear(self):
        self.volume.reset()

    def extract_mesh(self, min_count=None):
        return self.volume.extract_mesh(self.min_count if min_count is None else min_count)

    def map_points(self):
        """(points, normals) fp64 [N,3]: the surface-net vertices of the volume and the unit sampled gradient there (zero where the
        sample is invalid)."""
        pts, _ = self.volume.extract(self.min_count)
        if pts.shape[0] == 0:
            return pts, pts.clone()
        g = self.volume.sample(pts, min_count=self.min_count)['grad']
        norm = torch.linalg.norm(g, dim=1, keepdim=True)
        return pts, torch.where(norm > 0.0, g / norm.clamp(min=1e-300), g)


def make_mapper(cfg: Config, device=None, status_every=4):
    """The mapper of cfg.slam_map: 'points' -> IcpMapper, 'tsdf' -> TsdfMapper (which refuses the point map's switches)."""
    if cfg.slam_map == 'points':
        return IcpMapper(cfg, device=device, status_every=status_every)
    if cfg.slam_map == 'tsdf':
        return TsdfMapper(cfg, device=device, status_every=status_every)
    raise ValueError("unknown slam_map %r; available: 'points', 'tsdf'" % (cfg.slam_map,))


def _redo_first_scan(mapper, first, pose0, scan, prior, twist, pose, info, info0, cfg, passes=2):
    """The first scan of a sweep-aware run has no map to be registered against, so its twist cannot be estimated: it entered the map
    de-skewed by the odometry's first step, and a map bent by that step's error bends every later estimate with it.  Once the second
    scan is registered, the constant-velocity twist of the first is known from the registered step pose0^-1 pose instead (times
    cfg.slam_sweep_fraction): the map, which holds nothing but the first scan, is rebuilt from the scan de-skewed by that twist and
    the second scan registered again, ``passes`` times.  Returns the second scan's (pose, info); info0 (the first scan's) gets the
    twist used, ``added`` and ``map_size``.  A registration that fails on the way ends it with that result."""
    from .sweep import motion_twist
    m = len(first)
    for _ in range(passes):
        tw0 = float(cfg.slam_sweep_fraction) * motion_twist(delta_transform(pose0, pose))
        if not np.isfinite(tw0).all() or float(np.linalg.norm(tw0[3:])) > np.pi:
            break
        x, _, nx = ops.deskew(first.points, first.t, [0, m], tw0[None], normals=first.normals)
        mapper.clear()
        info0['added'] = mapper.update(MapperScan(x, nx, first.depth, first.t), pose0)
        info0['map_size'], info0['twist'] = mapper.n_map, tw0
        pose, info = mapper.register(scan, prior, twist=twist)
        if not info['ok']:
            break
    return pose, info


def run_slam(dataset, model, cfg: Config, mapper=None, verbose=False):
    """The mapper over one sequence with the perturbed odometry of cfg.odom_cov (robot_data): prior[i] = slam[i-1] odom[i-1]^-1 odom[i],
    slam[0] = odom[0] = gt[0]; a failed registration keeps its prior and leaves the map and its probabilities as they are.  Every info
    has ``dynamic`` (map points with P >= cfg.slam_threshold_dynamic) and ``dyn`` (update_dynamic's counts, None when it did not run).
    With cfg.slam_deskew a cloud that carries sweep times (the field ``t``) is de-skewed before anything else sees it, with the twist
    of slam[i-1]^-1 prior[i] times cfg.slam_sweep_fraction (preproc.deskew_cloud; the poses hold at the sweep's start).
    With cfg.slam_ct the cloud is left as it is, that twist is the prior twist of the sweep-aware registration (IcpMapper.register_ct)
    and the map takes the scan de-skewed by the estimated twist (info['twist']); both together are refused (ValueError).  The first
    scan of an empty map is de-skewed by the odometry's first step and, once the second scan is registered, again by the twist of
    the registered step (_redo_first_scan).
    The map is cfg.slam_map's (make_mapper): 'tsdf' registers against a fused sparse TSDF volume (TsdfMapper; ``added`` is then the rays
    fused and ``map_size`` the volume's blocks) and refuses slam_ct and the dynamic-point switches (ValueError); slam_deskew works.
    Returns dict(slam, odom, gt [N,4,4], path_lengths [N], info [N dicts], ids)."""
    if cfg.slam not in SLAM:
        raise ValueError('unknown SLAM pipeline %r; available: %s' % (cfg.slam, ', '.join(SLAM)))
    if cfg.slam_ct and cfg.slam_deskew:
        raise ValueError('slam_ct estimates the twist of a sweep inside the ICP and slam_deskew removes it beforehand: set one of them')
    if cfg.slam_map == 'tsdf':
        _tsdf_map_refusals(cfg)
    items = [(cloud, np.asarray(pose, dtype=np.float64)) for cloud, pose in dataset]
    gt = np.stack([pose for _, pose in items]) if items else np.zeros((0, 4, 4))
    odom = odometry_poses(gt, cfg.odom_cov)
    lengths = path_lengths(gt)
    mapper = mapper or make_mapper(cfg)
    slam = odom.copy()
    infos = []
    first = None
    for i, (cloud, _) in enumerate(items):
        prior = odom[0] if i == 0 else np.matmul(slam[i - 1], delta_transform(odom[i - 1], odom[i]))
        twist = None
        if (cfg.slam_deskew or cfg.slam_ct) and 't' in (getattr(getattr(cloud, 'dtype', None), 'names', None) or ()):
            # constant velocity: the sweep's twist is that of the motion from the last estimate to this prior (scan 0: the odometry's
            # first step; a single scan: none), times the part of the period the sweep takes
            from .preproc import deskew_cloud
            from .sweep import motion_twist
            step = delta_transform(slam[i - 1], prior) if i > 0 else (delta_transform(odom[0], odom[1]) if len(items) > 1 else np.eye(4))
            twist = float(cfg.slam_sweep_fraction) * motion_twist(step)
            if cfg.slam_deskew:
                cloud = deskew_cloud(cloud, twist, device=mapper.device)
        scan = mapper.prepare(mapper_input(cloud, model, cfg))
        if cfg.slam_ct:
            # the twist above is only the prior twist: the registration estimates the sweep's own and returns the scan de-skewed by it
            pose, info = mapper.register(scan, prior, twist=twist)
            if info['status'] == 'init' and scan.t is not None and len(scan) > 0:
                first = scan                          # entered the map de-skewed by the odometry's first step: redone below
            elif i == 1 and first is not None and info['ok']:
                pose, info = _redo_first_scan(mapper, first, slam[0], scan, prior, twist, pose, info, infos[0], cfg)
            scan = info.pop('deskewed', scan)
        else:
            pose, info = mapper.register(scan, prior)
        mapper.last_dyn = None
        if info['ok']:
            info['added'] = mapper.update(scan, pose, overlap=info['overlap'] if info['status'] != 'init' else None)
            if cfg.slam_compute_prob_dynamic and cfg.slam_dynamic_every_scan and mapper.last_dyn is None and info['status'] != 'init':
                mapper.last_dyn = mapper.update_dynamic(scan, pose)         # the overlap skipped the map update
        else:
            print('SLAM: registration of scan %d failed (%s); keeping the odometry prior.' % (i, info['status']))
            info['added'] = 0
        info['map_size'] = mapper.n_map
        info['dynamic'], info['dyn'] = mapper.n_dynamic, mapper.last_dyn
        slam[i] = pose
        infos.append(info)
        if verbose:
            print('scan %d: %s' % (i, info))
    ids = list(getattr(dataset, 'ids', range(len(items))))
    return dict(slam=slam, odom=odom, gt=gt, path_lengths=lengths, info=infos, ids=ids)
