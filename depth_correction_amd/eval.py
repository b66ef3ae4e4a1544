"""Loss evaluation over sequences with the reference's signatures (eval.py:31-112).

``eval_loss_clouds`` is the body of one training iteration.  When the configuration is the one the fused kernels
cover (ball neighbourhoods on the GPU, min-eigenvalue or trace loss -- with or without quantile inliers -- without
offsets / distance weights, any of the reference's models or none) every sequence is evaluated by its cached
``SequencePlan`` -- one to three kernel launches -- and the returned loss carries the hand-derived backward to
``model.w`` / ``model.exponent`` / the pose corrections.  Any other configuration goes through the un-fused DepthCloud operators with identical results.

``eval_loss`` / ``eval_loss_all`` are the reference's test-set evaluation (eval.py:115-211); ``eval_slam`` / ``eval_slam_all`` its
localization-accuracy evaluation (eval.py:214-290) with this package's ICP mapper instead of ROS (slam.py); ``eval_map`` /
``eval_map_all`` the accuracy of the map against the ground-truth mesh (scripts/mapping_accuracy:82-118); ``eval_bias`` /
``eval_bias_all`` the depth error of every ray against the mesh over the true incidence angle and the supervised fit
(scripts/bias_estimation, depth_bias.py); ``eval_recon`` / ``eval_recon_all`` the surface fused from the corrected scans against
the ground-truth mesh (what scripts/reconstruction_eval is named after).  ``landscape_clouds`` evaluates
the loss for many candidate weights of the model at once: every model with a basis form is affine in its weights, so a
neighbourhood's covariance is a quadratic form in w and one pass over the neighbours (dc_sequence_landscape) serves every
row; configurations outside that path loop over ``eval_loss_clouds`` ("Loss landscape").
"""
from __future__ import annotations

import copy
from collections import Counter

import numpy as np
import torch

from .config import SLAM, Config, NeighborhoodType, PoseCorrection, bias_eval_csv, loss_eval_csv, map_eval_csv, nonempty, recon_eval_csv, slam_eval_csv
from .depth_cloud import DepthCloud
from .plan import PlanRegistry, SequencePlan, consistency_loss
from .preproc import (compute_neighborhood_features, global_cloud, global_cloud_mask, local_feature_cloud,
                      offset_cloud)
from .transform import corrected_poses, xyz_axis_angle_to_matrix

__all__ = ['create_corrected_poses', 'eval_loss', 'eval_loss_all', 'eval_loss_clouds', 'eval_bias', 'eval_bias_all', 'eval_loss_landscape', 'eval_map', 'eval_map_all', 'eval_recon', 'eval_recon_all', 'eval_slam', 'eval_slam_all',
           'initialize_pose_corrections', 'fused_supported', 'landscape_clouds', 'landscape_paths', 'PlanCloud', 'LazyFeatureCloud']


def initialize_pose_corrections(datasets, cfg: Config):
    """Zero 6-vector corrections per cfg.pose_correction (eval.py:31-65); lengths of ``datasets`` are used."""
    kwargs = dict(dtype=cfg.torch_float_type(), device=cfg.device, requires_grad=True)
    deltas = []
    for ds in datasets:
        if cfg.pose_correction == PoseCorrection.common:
            delta = deltas[0] if deltas else torch.zeros((1, 6), **kwargs)
        elif cfg.pose_correction == PoseCorrection.sequence:
            delta = torch.zeros((1, 6), **kwargs)
        elif cfg.pose_correction == PoseCorrection.pose:
            delta = torch.zeros((len(ds), 6), **kwargs)
        else:
            delta = None
        deltas.append(delta)
    return deltas


def create_corrected_poses(poses, pose_deltas, cfg: Config):
    """T_s = T0_s * [Exp(axis-angle) | xyz] (eval.py:68-82)."""
    if cfg.pose_correction == PoseCorrection.none:
        return poses
    assert len(poses) == len(pose_deltas)
    if cfg.pose_correction == PoseCorrection.common:
        assert all(d is pose_deltas[0] for d in pose_deltas[1:])
    return [corrected_poses(p, d) for p, d in zip(poses, pose_deltas)]


def fused_supported(clouds, model, cfg: Config):
    kw = cfg.loss_kwargs
    return (getattr(cfg, 'fused', True) and cfg.nn_type == NeighborhoodType.ball
            and cfg.loss in ('min_eigval_loss', 'trace_loss') and not cfg.loss_offset and not cfg.nn_scale
            # NaN-dropping reductions run inside the fused kernels (round 4); together with quantile gating: un-fused operators
            and not ((kw.get('only_finite') or kw.get('skip_nans'))
                     and (kw.get('inlier_ratio', 1.0) < 1.0 or kw.get('inlier_max_loss') is not None))
            and (model is None or getattr(model, 'kernel_kind', None) is not None)
            and clouds[0][0].dirs.is_cuda and all(c.inc_angles is not None for seq in clouds for c in seq))


class PlanCloud(object):
    """Lazy view of a fused evaluation: the DepthCloud fields callers may inspect (points, eigvals, loss, mask) are
    produced on first access by one more forward with the per-point outputs switched on."""

    def __init__(self, plan, w, exponent, poses, count=None, inliers=None):
        self._plan, self._args, self._out = plan, (w, exponent, poses), None
        self.count = plan.count if count is None else count      # pointwise terms behind the sequence's share of the mean loss
        self._inliers = inliers                  # gated evaluation (loss.py:256-277): the centre rows that were kept

    def _materialize(self):
        if self._out is None:
            p = self._plan
            w, e, poses = self._args
            out = p.forward(w, e, poses, want_pointwise=True, want_eigvals=True)
            loss = p.unpermute(out['pointwise'])
            mask = None if p.mask_full is None else p.unpermute(p.mask_full)
            if self._inliers is not None:        # gated evaluation: the loss cloud is the inliers (loss.py:269-277)
                inl = self._inliers
                if p.centre_idx is not None:     # compact centre rows -> all points
                    inl = torch.zeros((p.n,), dtype=torch.bool, device=inl.device).index_put_((p.centre_idx.long(),), inl)
                mask = p.unpermute(inl)
            self._out = dict(points=p.points(), eigvals=p.unpermute(out['eigvals']), loss=loss, mask=mask)
        return self._out

    def __getattr__(self, name):
        if name in ('points', 'eigvals', 'loss', 'mask'):
            return self._materialize()[name]
        raise AttributeError(name)

    def __len__(self):
        return self._plan.n


_plans = PlanRegistry()


class LazyFeatureCloud(object):
    """The global feature cloud of a sequence (global_cloud -> compute_neighborhood_features, eval.py:90-98), computed on
    first access.  The reference builds it every iteration even when the ICP loss never looks at it (eval.py:100-104);
    callers that do (callbacks logging the map) get the same cloud, everyone else pays nothing."""

    def __init__(self, seq_clouds, model, poses, nn, cfg):
        self._args, self._cloud = (seq_clouds, model, poses, nn, cfg), None

    def _materialize(self):
        if self._cloud is None:
            seq_clouds, model, poses, nn, cfg = self._args
            with torch.no_grad():
                g = global_cloud(clouds=seq_clouds, model=model, poses=poses.detach())
                self._cloud = compute_neighborhood_features(cloud=g, neighborhoods=nn, cfg=cfg)
        return self._cloud

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self._materialize(), name)

    def __len__(self):
        return sum(len(c) for c in self._args[0])


def _plan_for(seq_clouds, poses, nn, mask, model, cfg):
    """SequencePlan of (local clouds, neighbourhoods, mask), all constant over the optimisation: kept in a registry keyed
    by the identity and version of every tensor it was built from (plan.PlanRegistry)."""
    neighbors = nn[0]
    kw = cfg.loss_kwargs
    nan_policy = 'only_finite' if kw.get('only_finite') else ('skip_nans' if kw.get('skip_nans') else None)     # loss.py:125-137
    # ball neighbourhoods (a ragged table) and no pose corrections: rows of similar length share wavefronts (SequencePlan.degree_group)
    by_degree = bool(getattr(cfg, 'nn_r', None)) and not getattr(cfg, 'nn_k', None) and str(getattr(cfg, 'pose_correction', 'none')).endswith('none')
    ball = bool(getattr(cfg, 'nn_r', None)) and not getattr(cfg, 'nn_k', None)       # rows of different lengths: SequencePlan.heavy_first
    flags = (cfg.loss, bool(kw.get('normalization', False)), bool(kw.get('sqrt', False)),
             getattr(model, 'kernel_kind', None) if model is not None else None, nan_policy, by_degree, ball)
    tensors = [t for c in seq_clouds for t in (c.vps, c.dirs, c.depth, c.inc_angles, c.mask)] + [neighbors, mask]

    def build():
        return SequencePlan(seq_clouds, poses.detach(), neighbors, None if mask is None else mask.to(neighbors.device),
                            model_kind=flags[3] or 'ScaledPolynomial', loss=cfg.loss,
                            normalization=flags[1] and cfg.loss == 'min_eigval_loss', sqrt=flags[2], nan_policy=nan_policy,
                            degree_group=by_degree, heavy_first=ball)
    return _plans.get(tensors, flags, build)


def eval_loss_clouds(clouds, poses, pose_deltas, masks, ns, model, loss_fun, cfg: Config):
    """Loss of all sequences for the current model / pose corrections (eval.py:85-112).

    Returns (loss, loss_clouds, updated poses, feature clouds) like the reference."""
    poses_upd = create_corrected_poses(poses, pose_deltas, cfg)

    if cfg.loss == 'icp_loss':
        if clouds[0][0].normals is None:
            clouds = [[local_feature_cloud(c, cfg) for c in seq] for seq in clouds]
        loss, loss_cloud = loss_fun(clouds, poses_upd, model, masks=masks)
        feat = [LazyFeatureCloud(c, model, p, nn, cfg) for c, p, nn in zip(clouds, poses_upd, ns)] if ns else None
        return loss, loss_cloud, poses_upd, feat

    if cfg.loss in ('mesh_loss', 'cloud_loss', 'tsdf_loss'):
        # masks[i] = (the sequence's ground-truth mesh / survey / TSDF target, point mask or None) -- see mesh_masks, survey_masks,
        # tsdf_masks
        loss, loss_cloud = loss_fun(clouds, poses_upd, model, masks=masks)
        feat = [LazyFeatureCloud(c, model, p, nn, cfg) for c, p, nn in zip(clouds, poses_upd, ns)] if ns else None
        return loss, loss_cloud, poses_upd, feat

    if fused_supported(clouds, model, cfg):
        # masks are established once (train.py:212-215); when absent they come from one un-fused evaluation
        if not masks or masks[0] is None:
            masks = []
            for c, p, nn in zip(clouds, poses_upd, ns):
                g = compute_neighborhood_features(cloud=global_cloud(clouds=c, model=model, poses=p.detach()),
                                                  neighborhoods=nn, cfg=cfg)
                masks.append(global_cloud_mask(g, g.mask, cfg))
        use_model = model is not None and getattr(model, 'kernel_kind', None) is not None
        total, count, views = 0.0, 0.0, []
        kw = cfg.loss_kwargs
        gating = dict(inlier_ratio=kw.get('inlier_ratio', 1.0), inlier_max_loss=kw.get('inlier_max_loss'),
                      inlier_loss_mult=kw.get('inlier_loss_mult', 1.0))
        for c, p, nn, m in zip(clouds, poses_upd, ns, masks):
            plan = _plan_for(c, p, nn, m, model, cfg)
            w, e = model.kernel_params() if use_model else (None, None)
            s, cnt = consistency_loss(plan, w, e, p, **gating)          # cnt: masked points, or inliers (device scalar)
            total, count = total + s, count + cnt
            views.append(PlanCloud(plan, w, e, p, count=cnt,
                                   inliers=getattr(plan, 'inlier_rows', None) if (isinstance(cnt, torch.Tensor) and not plan.nan_policy) else None))
        if isinstance(count, torch.Tensor):
            loss = total / count                                          # 0 / 0 = nan, like the mean of no inliers
        else:
            loss = total / count if count > 0 else total * float('nan')   # mean over all masked points (loss.py:211)
        return loss, views, poses_upd, views

    offsets = [offset_cloud(c, model) for c in clouds] if cfg.loss_offset else None
    # plane neighbourhoods: the model is applied per plane with the plane normals (eval.py:90-96)
    plane = cfg.nn_type == NeighborhoodType.plane
    global_clouds = [global_cloud(clouds=c, model=None if plane else model, poses=p) for c, p in zip(clouds, poses_upd)]
    feat_clouds = [compute_neighborhood_features(cloud=cloud, model=model if plane else None, neighborhoods=nn, cfg=cfg)
                   for cloud, nn in zip(global_clouds, ns)]
    if (not masks or masks[0] is None) and isinstance(feat_clouds[0], DepthCloud):
        masks = [global_cloud_mask(cloud, cloud.mask if hasattr(cloud, 'mask') else None, cfg) for cloud in feat_clouds]
    loss, loss_cloud = loss_fun(feat_clouds, mask=masks, offset=offsets)
    return loss, loss_cloud, poses_upd, feat_clouds


def mesh_masks(datasets, names, all_clouds):
    """mesh_loss's per-sequence ``masks``: (the dataset's ground-truth mesh, the scans' masks concatenated -- the points the model
    corrects -- or None when no scan has one)."""
    out = []
    for ds, name, clouds in zip(datasets, names, all_clouds):
        mesh = _dataset_mesh(ds, name, who='mesh_loss')
        point_mask = None
        if any(c.mask is not None for c in clouds):
            point_mask = torch.cat([c.mask if c.mask is not None else torch.ones((len(c),), dtype=torch.bool, device=c.dirs.device)
                                    for c in clouds])
        out.append((mesh, point_mask))
    return out


def _dataset_survey(ds, name, cfg=None, who='cloud_loss', required=True):
    """The dataset's surveyed cloud: its own ``survey`` attribute when it carries one, else what get_survey(cfg.cloud_samples) samples
    from its mesh (MeshDataset, RenderedMeshDataset; reached through the Forwarding wrappers)."""
    get = getattr(ds, 'get_survey', None)
    if callable(get):
        return get(getattr(cfg, 'cloud_samples', None) if cfg is not None else None)
    own = getattr(ds, 'survey', None)
    if own is not None and hasattr(own, 'on_device') and hasattr(own, 'normals'):
        return own
    if required:
        raise ValueError('dataset %s gives no surveyed cloud (no survey attribute, no get_survey()): %s needs one' % (name, who))
    return None


def survey_masks(datasets, names, all_clouds, cfg=None):
    """cloud_loss's per-sequence ``masks``: (the dataset's survey.SurveyCloud, the scans' masks concatenated -- the points the model
    corrects -- or None when no scan has one)."""
    out = []
    for ds, name, clouds in zip(datasets, names, all_clouds):
        survey = _dataset_survey(ds, name, cfg)
        point_mask = None
        if any(c.mask is not None for c in clouds):
            point_mask = torch.cat([c.mask if c.mask is not None else torch.ones((len(c),), dtype=torch.bool, device=c.dirs.device)
                                    for c in clouds])
        out.append((survey, point_mask))
    return out


def tsdf_masks(datasets, names, all_clouds, cfg=None):
    """tsdf_loss's per-sequence ``masks``: (a loss.TsdfTarget of its own, built from cfg.loss_kwargs over config.TSDF_LOSS_DEFAULTS, the
    scans' masks concatenated -- the points the model corrects, which are the rays the target fuses -- or None when no scan has one)."""
    from .config import TSDF_LOSS_DEFAULTS
    from .loss import TsdfTarget
    kw = dict(TSDF_LOSS_DEFAULTS)
    kw.update({k: v for k, v in (getattr(cfg, 'loss_kwargs', None) or {}).items() if k in TSDF_LOSS_DEFAULTS})
    out = []
    for ds, name, clouds in zip(datasets, names, all_clouds):
        target = TsdfTarget(kw['tsdf_voxel_size'], trunc=kw['tsdf_trunc'], leave_one_out=kw['tsdf_leave_one_out'],
                            refresh_every=kw['tsdf_refresh_every'])
        point_mask = None
        if any(c.mask is not None for c in clouds):
            point_mask = torch.cat([c.mask if c.mask is not None else torch.ones((len(c),), dtype=torch.bool, device=c.dirs.device)
                                    for c in clouds])
        out.append((target, point_mask))
    return out


def _load_test_sequences(cfg: Config, test_datasets):
    """Local clouds and poses of every test sequence (eval.py:147-164): ball neighbourhoods get local feature clouds, plane
    neighbourhoods plain DepthClouds (as train._load_sequences)."""
    all_clouds, all_poses = [], []
    for ds in test_datasets:
        clouds, poses = [], []
        for cloud, pose in ds:
            if cfg.nn_type == NeighborhoodType.ball:
                cloud = local_feature_cloud(cloud, cfg)
            else:
                cloud = DepthCloud.from_structured_array(cloud, dtype=cfg.numpy_float_type(), device=cfg.device)
            clouds.append(cloud)
            poses.append(pose)
        all_clouds.append(clouds)
        all_poses.append(torch.as_tensor(np.stack(poses).astype(dtype=cfg.numpy_float_type()), device=cfg.device))
    return all_clouds, all_poses


def _test_setup(cfg: Config, test_datasets, model):
    from .dataset import create_dataset
    from .model import load_model
    if test_datasets:
        test_names = [str(ds) for ds in test_datasets]
        print('Using provided test datasets: %s.' % ', '.join(test_names))
    else:
        print('Creating test datasets from config: %s.' % ', '.join(cfg.test_names))
        test_names = cfg.test_names
        test_datasets = []
        for i, name in enumerate(cfg.test_names):
            # the synthetic datasets take no poses_path: passed only when the configuration names one
            kwargs = {'poses_path': cfg.test_poses_path[i]} if cfg.test_poses_path and cfg.test_poses_path[i] else {}
            test_datasets.append(create_dataset(name, cfg, **kwargs))
    if model is None:
        model = load_model(cfg=cfg, eval_mode=True)
    return test_names, test_datasets, model


def _test_pose_deltas(cfg: Config, test_datasets):
    if cfg.test_poses_path and nonempty(cfg.test_poses_path):          # eval.py:166-170
        assert cfg.pose_correction != PoseCorrection.none
        return torch.load(cfg.test_pose_deltas, map_location=cfg.device)
    return initialize_pose_corrections(test_datasets, cfg)


def eval_loss(cfg: Config, test_datasets=None, test_ns=None, model=None, loss_fun=None, return_neighborhood=False):
    """Loss on the test sequences (eval.py:115-191): datasets from ``cfg.test_names`` unless given, model from the
    configuration unless given, neighbourhoods established unless ``test_ns`` is given; the global masks are recomputed for
    the evaluated model.  Prints the loss, appends it to ``cfg.loss_eval_csv`` when set and returns it (with the
    neighbourhoods when ``return_neighborhood``)."""
    from .io import append
    from .loss import create_loss
    from .preproc import establish_neighborhoods
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    if loss_fun is None:
        loss_fun = create_loss(cfg)
    assert callable(loss_fun)
    test_clouds, test_poses = _load_test_sequences(cfg, test_datasets)
    test_masks = [None] * len(test_datasets)
    if cfg.loss == 'mesh_loss':
        test_masks = mesh_masks(test_datasets, test_names, test_clouds)
    elif cfg.loss == 'cloud_loss':
        test_masks = survey_masks(test_datasets, test_names, test_clouds, cfg)
    elif cfg.loss == 'tsdf_loss':
        test_masks = tsdf_masks(test_datasets, test_names, test_clouds, cfg)
    test_pose_deltas = _test_pose_deltas(cfg, test_datasets)
    if test_ns is None:
        test_ns = [establish_neighborhoods(clouds=clouds, poses=poses, cfg=cfg) for clouds, poses in zip(test_clouds, test_poses)]
    test_loss, _, _, _ = eval_loss_clouds(test_clouds, test_poses, test_pose_deltas, test_masks, test_ns, model, loss_fun, cfg)
    print('Test loss on %s: %.9f' % (', '.join(test_names), test_loss.item()))
    if cfg.loss_eval_csv:
        append(cfg.loss_eval_csv, '%s %.9f\n' % (','.join(test_names), test_loss))
        if len(test_names) > 1:
            print('Test loss on %s written to %s.' % (', '.join(test_names), cfg.loss_eval_csv))
    if return_neighborhood:
        return test_loss, test_ns
    return test_loss


def eval_loss_all(cfg: Config):
    """Every loss of ``cfg.eval_losses`` on the train, val and test subsets with ground-truth poses, one CSV file per loss and
    subset (eval.py:194-211)."""
    for names, suffix in zip([cfg.train_names, cfg.val_names, cfg.test_names], ['train', 'val', 'test']):
        if not names:
            continue
        for loss in cfg.eval_losses:
            eval_cfg = cfg.copy()
            eval_cfg.test_names = names
            eval_cfg.train_poses_path = []
            eval_cfg.val_poses_path = []
            eval_cfg.test_poses_path = []
            eval_cfg.loss = loss
            eval_cfg.loss_eval_csv = loss_eval_csv(cfg.log_dir, loss, suffix)
            eval_loss(cfg=eval_cfg)


def eval_slam(cfg: Config, test_datasets=None, model=None):
    """SLAM accuracy on the test sequences (eval.py:214-260 with scripts/robot_data:176-204): each sequence's scans go through the
    depth and grid filters, the correction by ``model`` (from the configuration unless given, as slam_eval.launch runs the
    correction node) and the mapper of ``cfg.slam``, fed with the odometry of ``cfg.odom_cov``.  Appends
    ``name r_angle t_norm rel_angle rel_offset`` to ``cfg.slam_eval_csv``; writes the SLAM poses to ``cfg.slam_poses_csv`` when
    set (one sequence only).  Returns the per-sequence results of slam.run_slam with their ``errors``."""
    import os
    from .io import append
    from .scan_io import write_poses_csv
    from .registration import align_paths
    from .slam import run_slam, slam_errors
    if cfg.slam not in SLAM:
        raise ValueError('SLAM pipeline %r is not available here; available: %s' % (cfg.slam, ', '.join(SLAM)))
    assert cfg.slam_eval_csv
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    assert not cfg.slam_poses_csv or len(test_names) == 1
    if cfg.slam_eval_bag:
        print('slam_eval_bag %s ignored: no bag is recorded.' % cfg.slam_eval_bag)
    results = []
    for name, ds in zip(test_names, test_datasets):
        print('SLAM evaluation on %s started.' % name)
        res = run_slam(ds, model, cfg)
        r_angle, t_norm, rel_angle, rel_offset = res['errors'] = slam_errors(res['slam'], res['gt'], res['path_lengths'])
        print('Average error: rot. %.6f deg. (%.3f deg/m), transl. %.6f m (%.3f %%).'
              % (np.degrees(r_angle), np.degrees(rel_angle), t_norm, 100. * rel_offset))
        if cfg.slam_compute_prob_dynamic and res['info']:
            print('Dynamic map points: %d of %d.' % (res['info'][-1]['dynamic'], res['info'][-1]['map_size']))
        append(cfg.slam_eval_csv, '%s %.9f %.9f %.9f %.9f\n' % (name, r_angle, t_norm, rel_angle, rel_offset))
        # the SLAM path rigidly aligned to the ground truth (scripts/paths_alignment): what is left is the path's shape error
        res['aligned'] = align_paths(res['slam'], res['gt'], fix_reflection=True)
        print('Aligned path error: rmse %.6f m (mean %.6f m).' % (res['aligned']['rmse'], res['aligned']['mean']))
        if cfg.slam_poses_csv:
            if os.path.exists(cfg.slam_poses_csv):
                print('File with SLAM poses already exists: %s. It will be overwritten.' % cfg.slam_poses_csv)
            os.makedirs(os.path.dirname(os.path.abspath(cfg.slam_poses_csv)), exist_ok=True)
            write_poses_csv(res['ids'], res['slam'], cfg.slam_poses_csv)
        print('SLAM evaluation on %s finished.' % name)
        results.append(res)
    return results


def eval_slam_all(cfg: Config):
    """Every SLAM pipeline of ``cfg.eval_slams`` on the train, val and test subsets with ground-truth poses, one CSV file per pipeline
    and subset, no bag and no poses file (eval.py:263-290)."""
    out = {}
    for names, suffix in zip([cfg.train_names, cfg.val_names, cfg.test_names], ['train', 'val', 'test']):
        if not names:
            continue
        for slam in cfg.eval_slams:
            eval_cfg = cfg.copy()
            eval_cfg.test_names = names
            eval_cfg.train_poses_path = []
            eval_cfg.val_poses_path = []
            eval_cfg.test_poses_path = []
            eval_cfg.slam = slam
            eval_cfg.slam_eval_bag = ''
            eval_cfg.slam_eval_csv = slam_eval_csv(cfg.log_dir, slam, suffix)
            eval_cfg.slam_poses_csv = ''
            out[(slam, suffix)] = eval_slam(cfg=eval_cfg)
    return out


# ---- map accuracy against the ground-truth mesh ----------------------------------------------------------------------------------
MAP_EVAL_FIELDS = ('n', 'mean', 'rms', 'median', 'trimmed_mean', 'signed_mean')


def _dataset_mesh(ds, name, who='eval_map'):
    get = getattr(ds, 'get_mesh', None)          # reached through the Forwarding wrappers
    if not callable(get):
        raise ValueError('dataset %s gives no ground-truth mesh (no get_mesh()): %s needs one' % (name, who))
    return get()


def eval_map(cfg: Config, test_datasets=None, model=None):
    """Accuracy of the map of every test sequence against its dataset's mesh (scripts/mapping_accuracy:82-118 against the mesh
    instead of a surveyed cloud): each scan goes through slam.mapper_input (depth and grid filters, the correction by ``model``,
    from the configuration unless given), is moved by its pose -- ``cfg.map_eval_poses`` 'dataset': the poses the dataset yields,
    'slam': the poses slam.run_slam estimates -- the clouds are concatenated and voxel-filtered with filter_grid(keep='first') at
    cfg.grid_res (mapping_accuracy:106; skipped when 0), and metrics.map_accuracy is taken.  With ``cfg.map_eval_register`` the
    filtered map is first registered to the dataset's survey (its own, or the one sampled from its mesh) by
    registration.register_cloud(**cfg.register_kwargs), the accuracy is that of the registered points and ``res['registration']``
    holds the Registration; with ``cfg.map_eval_register_init`` 'global' it starts from the prior of registration.register_global
    (**cfg.register_global_kwargs) and with 'planes' from that of registration.register_planes (**cfg.register_planes_kwargs), which
    ``res['registration_coarse']`` then holds.  Appends ``name n mean rms median trimmed_mean signed_mean`` to ``cfg.map_eval_csv`` when set and
    returns the per-sequence dicts."""
    from .filters import filter_grid
    from .io import append
    from .metrics import map_accuracy
    from .slam import mapper_input, run_slam
    if cfg.map_eval_poses not in ('dataset', 'slam'):
        raise ValueError("map_eval_poses must be 'dataset' or 'slam', got %r" % (cfg.map_eval_poses,))
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    results = []
    for name, ds in zip(test_names, test_datasets):
        if callable(getattr(ds, 'get_mesh', None)):
            mesh = _dataset_mesh(ds, name)
        else:                                      # a survey and no mesh: the accuracy against the surveyed cloud
            mesh = _dataset_survey(ds, name, cfg, who='eval_map', required=False)
            if mesh is None:
                mesh = _dataset_mesh(ds, name)     # (raises: neither)
        items = [(cloud, np.asarray(pose, dtype=np.float64)) for cloud, pose in ds]
        poses = run_slam(ds, model, cfg)['slam'] if cfg.map_eval_poses == 'slam' else [pose for _, pose in items]
        moved = []
        for (cloud, _), pose in zip(items, poses):
            scan = mapper_input(cloud, model, cfg)
            with torch.no_grad():
                pts = scan.get_points().detach().to(device=cfg.device, dtype=torch.float64)
                T = torch.as_tensor(np.asarray(pose, dtype=np.float64), device=pts.device)
                moved.append(pts @ T[:3, :3].t() + T[:3, 3])
        points = torch.cat(moved).contiguous() if moved else torch.empty((0, 3), dtype=torch.float64, device=cfg.device)
        if cfg.grid_res and cfg.grid_res > 0.0 and points.shape[0]:
            points = filter_grid(points, float(cfg.grid_res), keep='first').contiguous()
        reg = None
        if cfg.map_eval_register:
            from .registration import register_cloud
            kw = dict(cfg.register_kwargs)
            if cfg.map_eval_register_init is not None:
                if cfg.map_eval_register_init not in ('global', 'planes'):
                    raise ValueError("map_eval_register_init must be None, 'global' or 'planes', got %r" % (cfg.map_eval_register_init,))
                kw.update(init=cfg.map_eval_register_init, global_kwargs=dict(
                    cfg.register_global_kwargs if cfg.map_eval_register_init == 'global' else cfg.register_planes_kwargs))
            reg = register_cloud(points, _dataset_survey(ds, name, cfg, who='eval_map with map_eval_register'), **kw)
            if reg.coarse is not None and reg.coarse.method == 'planes':
                print('Plane registration of the map of %s: %s, %s planes, hypothesis %d of %d valid, score %d, fitness %d of %d points.'
                      % (name, reg.coarse.status, reg.coarse.n_planes, reg.coarse.hypothesis, reg.coarse.n_valid, reg.coarse.score,
                         reg.coarse.fitness, reg.coarse.n_points))
            elif reg.coarse is not None:
                print('Global registration of the map of %s: %s, hypothesis %d, score %d of %d matches, fitness %d of %d points.'
                      % (name, reg.coarse.status, reg.coarse.hypothesis, reg.coarse.score, reg.coarse.n_correspondences,
                         reg.coarse.fitness, reg.coarse.n_points))
            print('Registration of the map of %s to its survey: %s after %d iterations, %d pairs, rms %.6f m.'
                  % (name, reg.status, reg.iterations, reg.pairs, reg.rms))
            T = torch.as_tensor(reg.T, device=points.device)
            points = (points @ T[:3, :3].t() + T[:3, 3]).contiguous()
        res = map_accuracy(points, mesh, inlier_ratio=cfg.map_eval_inlier_ratio, n_samples=cfg.map_eval_samples or None,
                           seed=cfg.random_seed)
        res['name'] = name
        if reg is not None:
            res['registration'] = reg
            if reg.coarse is not None:
                res['registration_coarse'] = reg.coarse
        print('Map accuracy on %s: %d points, mean %.6f m, rms %.6f m, median %.6f m, trimmed mean %.6f m, signed mean %.6f m.'
              % ((name, int(res['n'])) + tuple(res[f] for f in MAP_EVAL_FIELDS[1:])))
        if cfg.map_eval_csv:
            append(cfg.map_eval_csv, '%s %d %s\n' % (name, int(res['n']), ' '.join('%.9f' % res[f] for f in MAP_EVAL_FIELDS[1:])))
        results.append(res)
    return results


def eval_map_all(cfg: Config):
    """eval_map on the train, val and test subsets with the poses the datasets yield, one CSV file per subset (the shape of
    eval_slam_all)."""
    out = {}
    for names, suffix in zip([cfg.train_names, cfg.val_names, cfg.test_names], ['train', 'val', 'test']):
        if not names:
            continue
        eval_cfg = cfg.copy()
        eval_cfg.test_names = names
        eval_cfg.train_poses_path = []
        eval_cfg.val_poses_path = []
        eval_cfg.test_poses_path = []
        eval_cfg.map_eval_csv = map_eval_csv(cfg.log_dir, suffix)
        out[suffix] = eval_map(cfg=eval_cfg)
    return out


# ---- surface reconstruction against the ground-truth mesh --------------------------------------------------------------------------
RECON_EVAL_FIELDS = ('mean', 'rms', 'median', 'trimmed_mean')


def eval_recon(cfg: Config, test_datasets=None, model=None):
    """The surface fused from every test sequence against its dataset's mesh: each scan goes through the depth filter and the
    correction by ``model`` (from the configuration unless given) -- slam.mapper_input without the grid filter, a fusion wants all rays
    -- and is moved by its pose (``cfg.recon_poses`` 'dataset' or 'slam', as eval_map's); reconstruction.reconstruct fuses them at
    cfg.recon_voxel_size and extracts the mesh; metrics.reconstruction_accuracy holds it against get_mesh().  Appends ``name vertices
    faces accuracy(mean rms median trimmed_mean) completeness(mean rms median trimmed_mean) coverage`` to ``cfg.recon_eval_csv`` and
    writes the mesh to ``cfg.recon_mesh_ply`` when set; returns the per-sequence dicts (with 'mesh' and 'volume')."""
    from .io import append
    from .metrics import reconstruction_accuracy
    from .reconstruction import reconstruct
    from .slam import mapper_input, run_slam
    if cfg.recon_poses not in ('dataset', 'slam'):
        raise ValueError("recon_poses must be 'dataset' or 'slam', got %r" % (cfg.recon_poses,))
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    all_rays = cfg.copy()
    all_rays.grid_res = 0.0
    results = []
    for name, ds in zip(test_names, test_datasets):
        gt = _dataset_mesh(ds, name, who='eval_recon')
        items = [(cloud, np.asarray(pose, dtype=np.float64)) for cloud, pose in ds]
        poses = run_slam(ds, model, cfg)['slam'] if cfg.recon_poses == 'slam' else [pose for _, pose in items]
        scans = [mapper_input(cloud, model, all_rays) for cloud, _ in items]
        mesh, volume = reconstruct(scans, poses, cfg.recon_voxel_size, trunc=cfg.recon_trunc, bounds=cfg.recon_bounds,
                                   min_count=cfg.recon_min_count, max_range=cfg.recon_max_range, carve_from=cfg.recon_carve_from,
                                   device=cfg.device, sparse=cfg.recon_sparse)
        res = reconstruction_accuracy(mesh, gt, n_samples=cfg.recon_eval_samples, seed=cfg.random_seed,
                                      inlier_ratio=cfg.map_eval_inlier_ratio, max_dist=cfg.recon_eval_max_dist)
        res.update(name=name, mesh=mesh, volume=volume, stats=volume.stats())
        acc, com = res['accuracy'], res['completeness']
        print('Reconstruction of %s: %d vertices, %d faces; accuracy mean %.6f m, rms %.6f m; completeness mean %.6f m, rms %.6f m; '
              'coverage %.4f.' % (name, mesh.vertices.shape[0], len(mesh), acc['mean'], acc['rms'], com['mean'], com['rms'], res['coverage']))
        if cfg.recon_mesh_ply:
            mesh.save_ply(cfg.recon_mesh_ply)
        if cfg.recon_eval_csv:
            append(cfg.recon_eval_csv, '%s %d %d %s %s %.9f\n' % (name, mesh.vertices.shape[0], len(mesh),
                                                                 ' '.join('%.9f' % acc[f] for f in RECON_EVAL_FIELDS),
                                                                 ' '.join('%.9f' % com[f] for f in RECON_EVAL_FIELDS), res['coverage']))
        results.append(res)
    return results


def eval_recon_all(cfg: Config):
    """eval_recon on the train, val and test subsets with the poses the datasets yield, one CSV file per subset (the shape of
    eval_map_all)."""
    out = {}
    for names, suffix in zip([cfg.train_names, cfg.val_names, cfg.test_names], ['train', 'val', 'test']):
        if not names:
            continue
        eval_cfg = cfg.copy()
        eval_cfg.test_names = names
        eval_cfg.train_poses_path = []
        eval_cfg.val_poses_path = []
        eval_cfg.test_poses_path = []
        eval_cfg.recon_eval_csv = recon_eval_csv(cfg.log_dir, suffix)
        eval_cfg.recon_mesh_ply = None
        out[suffix] = eval_recon(cfg=eval_cfg)
    return out


# ---- depth bias against the ground-truth mesh -------------------------------------------------------------------------------------
def _fmt_weights(w):
    return ','.join('%.9g' % x for x in np.asarray(w, dtype=np.float64).reshape(-1))


def bias_eval_line(name, res, fit):
    """One line of cfg.bias_eval_csv: ``name used mean_abs rms rel_rms (before) mean_abs rms rel_rms (after, nan without a model)
    angle_err_rms w_true_angles w_est_angles`` (the weight vectors comma-separated)."""
    b = res['before']['overall']
    a = res['after']['overall'] if res.get('after') else {k: float('nan') for k in b}
    vals = [b['mean_abs'], b['rms'], b['rel_rms'], a['mean_abs'], a['rms'], a['rel_rms'], b['angle_err_rms']]
    return '%s %d %s %s %s\n' % (name, int(res['before']['totals']['used']), ' '.join('%.9f' % v for v in vals),
                                 _fmt_weights(fit['w_true_angles']), _fmt_weights(fit['w_est_angles']))


def write_bias_curve_csv(path, name, res):
    """Append the per-bin table of a depth_bias result to ``path``: a header line, then per bin ``name bin angle_lo angle_hi`` and
    count, mean, rms, mean_abs, rel_mean, rel_rms, angle_err_mean, angle_err_rms before and after (nan without a model)."""
    from .io import append
    from .metrics import BIAS_BIN_FIELDS
    edges = res['bin_edges'].cpu().numpy()
    cols = {}
    for part in ('before', 'after'):
        for f in BIAS_BIN_FIELDS:
            cols[part, f] = res[part][f].detach().cpu().numpy() if res.get(part) else np.full(len(edges) - 1, np.nan)
    lines = ['# name bin angle_lo angle_hi ' + ' '.join('%s_%s' % (f, part) for part in ('before', 'after') for f in BIAS_BIN_FIELDS) + '\n']
    for b in range(len(edges) - 1):
        lines.append('%s %d %.9f %.9f %s\n' % (name, b, edges[b], edges[b + 1], ' '.join(
            '%.9g' % cols[part, f][b] for part in ('before', 'after') for f in BIAS_BIN_FIELDS)))
    append(path, ''.join(lines))


def _bias_truth(ds, name, cfg):
    """What eval_bias casts the rays of ``ds`` against (cfg.bias_eval_against): its mesh, or its surveyed cloud."""
    against = cfg.bias_eval_against
    if against == 'tsdf':                        # no ground truth: the sequence's own fused volume, made by depth_bias from the scans
        from .loss import TsdfTarget
        return TsdfTarget(cfg.bias_eval_tsdf_voxel_size, trunc=cfg.bias_eval_tsdf_trunc, leave_one_out=cfg.bias_eval_tsdf_leave_one_out,
                          refresh_every=0, min_count=cfg.bias_eval_tsdf_min_count)
    if against == 'mesh' or (against == 'auto' and callable(getattr(ds, 'get_mesh', None))):
        return _dataset_mesh(ds, name, 'eval_bias')
    survey = _dataset_survey(ds, name, cfg, who='eval_bias', required=against == 'survey')
    return survey if survey is not None else _dataset_mesh(ds, name, 'eval_bias')          # 'auto' with neither: raises


def eval_bias(cfg: Config, test_datasets=None, model=None):
    """Depth bias of every test sequence against its dataset's ground truth (cfg.bias_eval_against: the mesh, or the surveyed cloud
    through its surfels -- metrics.depth_bias, DESIGN "Depth bias against a surveyed cloud" -- for a dataset such as the FEE corridor
    that has a survey and no mesh; or, with 'tsdf', which 'auto' never chooses, no ground truth at all: the sequence's own scans
    fused into a loss.TsdfTarget by the cfg.bias_eval_tsdf_* keys, every scan cast against the volume of the others -- the residual
    is then the ray's bias minus the mean bias of the other views, DESIGN "Ray casting the fused volume").  Against the mesh (what scripts/bias_estimation and depth_bias.py measure with a
    board; DESIGN "Depth bias against the mesh"): each scan goes through preproc.filtered_cloud and local_feature_cloud -- the
    estimated incidence angles and the planarity mask train() sees -- and its rays are cast in the mesh frame with the poses the
    dataset yields.  Only ground-truth poses are meaningful here: with any other pose the difference to the mesh measures the pose
    error, not the sensor's bias, so there is no 'slam' option.  metrics.depth_bias gives the error over the true incidence angle
    before and after ``model`` (from the configuration unless given); metrics.fit_bias the weights a supervised fit of the model's
    class (ScaledPolynomial [2, 4] for a model that is no polynomial) finds at true and at estimated angles.  Prints one line per
    sequence, appends bias_eval_line to ``cfg.bias_eval_csv`` and the per-bin table to ``cfg.bias_eval_curve_csv`` when set, and
    returns the per-sequence dicts of depth_bias with ``name`` and ``fit``."""
    from .io import append
    from .metrics import depth_bias, fit_bias
    from .preproc import filtered_cloud
    if cfg.bias_eval_against not in ('auto', 'mesh', 'survey', 'tsdf'):
        raise ValueError("bias_eval_against must be 'auto', 'mesh', 'survey' or 'tsdf', got %r" % (cfg.bias_eval_against,))
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    meshes = [_bias_truth(ds, name, cfg) for name, ds in zip(test_names, test_datasets)]
    if torch.device(cfg.device).type != 'cuda':
        raise RuntimeError('eval_bias needs a GPU (cfg.device %s): depth_correction_amd has no CPU path' % (cfg.device,))
    results = []
    for name, ds, mesh in zip(test_names, test_datasets, meshes):
        clouds, poses = [], []
        for cloud, pose in ds:
            clouds.append(local_feature_cloud(filtered_cloud(cloud, cfg), cfg))
            poses.append(np.asarray(pose, dtype=np.float64))
        res = depth_bias(clouds, np.stack(poses), mesh, model=model, bins=cfg.bias_eval_bins, max_residual=cfg.bias_eval_max_residual,
                         cull=cfg.bias_eval_cull, surfel_radius=cfg.bias_eval_surfel_radius, surfel_k=cfg.bias_eval_surfel_k,
                         surfel_scale=cfg.bias_eval_surfel_scale, surfel_window=cfg.bias_eval_surfel_window,
                         surfel_max_normal_angle=cfg.bias_eval_surfel_max_normal_angle, tsdf_step=cfg.bias_eval_tsdf_step,
                         tsdf_max_range=cfg.bias_eval_tsdf_max_range)
        fit = res['fit'] = fit_bias(res, res['fit_class'], res['fit_exponent'])
        res['name'] = name
        b, a = res['before']['overall'], (res['after'] or {}).get('overall')
        print('Depth bias on %s: %d of %d rays used, mean |r| %.6f m, rms %.6f m, rel. rms %.6f%s, angle error rms %.6f rad; '
              'supervised %s fit: w [%s] at true angles, [%s] at estimated angles.'
              % (name, int(res['before']['totals']['used']), int(res['before']['totals']['rays']), b['mean_abs'], b['rms'], b['rel_rms'],
                 ' (after correction: %.6f m, %.6f m, %.6f)' % (a['mean_abs'], a['rms'], a['rel_rms']) if a else '',
                 b['angle_err_rms'], fit['model_class'], _fmt_weights(fit['w_true_angles']), _fmt_weights(fit['w_est_angles'])))
        if fit['message']:
            print('Supervised fit on %s: %s.' % (name, fit['message']))
        if cfg.bias_eval_csv:
            append(cfg.bias_eval_csv, bias_eval_line(name, res, fit))
        if cfg.bias_eval_curve_csv:
            write_bias_curve_csv(cfg.bias_eval_curve_csv, name, res)
        results.append(res)
    return results


def eval_bias_all(cfg: Config):
    """eval_bias on the train, val and test subsets with the poses the datasets yield, one CSV file per subset (the shape of
    eval_map_all)."""
    out = {}
    for names, suffix in zip([cfg.train_names, cfg.val_names, cfg.test_names], ['train', 'val', 'test']):
        if not names:
            continue
        eval_cfg = cfg.copy()
        eval_cfg.test_names = names
        eval_cfg.train_poses_path = []
        eval_cfg.val_poses_path = []
        eval_cfg.test_poses_path = []
        eval_cfg.bias_eval_csv = bias_eval_csv(cfg.log_dir, suffix)
        eval_cfg.bias_eval_curve_csv = ''
        out[suffix] = eval_bias(cfg=eval_cfg)
    return out


# ---- loss landscape over the model weights --------------------------------------------------------------------------------
landscape_paths = Counter()     # 'kernel' / 'loop': how many landscape_clouds calls took each path
_MAX_EIG_BOUNDS = 8


def _n_weights(model):
    if model is None:
        return 0
    if getattr(model, 'kernel_kind', None) is not None:
        return model.kernel_params()[0].numel()
    return sum(p.numel() for p in model.parameters())


def _weight_rows(weights, n_params, device):
    """[W, P] fp64 device rows; a [W] vector is accepted when P == 1."""
    w = torch.as_tensor(weights).detach().to(device=device, dtype=torch.float64)
    if w.dim() == 1:
        if n_params != 1:
            raise ValueError('weights of shape %s for a model with %d weights: expected [W, %d]' % (tuple(w.shape), n_params, n_params))
        w = w.reshape(-1, 1)
    if w.dim() != 2 or w.shape[1] != n_params or n_params == 0:
        raise ValueError('weights of shape %s for a model with %d weights: expected [W, %d]' % (tuple(w.shape), n_params, n_params))
    return w.contiguous()


def _model_with_weights(model, row):
    """A copy of ``model`` whose kernel weights (or, for models without a kernel form, its parameters in order) are ``row``."""
    m = copy.deepcopy(model)
    with torch.no_grad():
        if getattr(m, 'kernel_kind', None) == 'Linear':
            params = [m.w0, m.w1, m.b]
        elif getattr(m, 'kernel_kind', None) is not None:
            params = [m.w]
        else:
            params = list(m.parameters())
        off = 0
        for p in params:
            p.copy_(row[off:off + p.numel()].reshape(p.shape).to(device=p.device, dtype=p.dtype))
            off += p.numel()
    return m


def _eig_bounds(cfg: Config):
    """(eigenvalue, denominator or -1, lo, hi) of the eigenvalue and eigenvalue-ratio bounds of global_cloud_mask."""
    lo_hi = lambda lo, hi: (float('-inf') if lo is None else float(lo), float('inf') if hi is None else float(hi))
    out = [(int(b[0]), -1) + lo_hi(b[1], b[2]) for b in (cfg.eigenvalue_bounds or [])]
    out += [(int(b[0]), int(b[1])) + lo_hi(b[2], b[3]) for b in (cfg.eigenvalue_ratio_bounds or [])]
    return out


def _landscape_supported(clouds, model, n_params, cfg: Config):
    kw = cfg.loss_kwargs
    return (fused_supported(clouds, model, cfg) and model is not None and getattr(model, 'kernel_kind', None) is not None
            and n_params in (1, 2) and kw.get('inlier_ratio', 1.0) == 1.0 and kw.get('inlier_max_loss') is None
            and not kw.get('only_finite') and not kw.get('skip_nans') and not cfg.vp_dispersion_to_depth2_bounds
            and len(_eig_bounds(cfg)) <= _MAX_EIG_BOUNDS)


def _static_mask(seq_clouds, poses, nn, cfg: Config):
    """The part of global_cloud_mask that does not depend on the model: local masks, valid neighbours, direction and
    viewpoint dispersion (eval.py:105-107 without the eigenvalue bounds, which the kernel applies per weight row)."""
    cfg0 = cfg.copy()
    cfg0.eigenvalue_bounds, cfg0.eigenvalue_ratio_bounds = [], []
    g = compute_neighborhood_features(cloud=global_cloud(clouds=seq_clouds, model=None, poses=poses.detach()), neighborhoods=nn,
                                      cfg=cfg0)
    return global_cloud_mask(g, g.mask, cfg0)


def _landscape_kernel(clouds, poses_upd, masks, ns, model, w, cfg: Config):
    """(sums [W], counts [W]) of every sequence through SequencePlan.eval_landscape, or None when a plan has no basis form."""
    _, e = model.kernel_params()
    e = e.detach().reshape(-1).to(device=w.device, dtype=torch.float64).contiguous()
    total = torch.zeros((w.shape[0],), dtype=torch.float64, device=w.device)
    count = torch.zeros_like(total)
    recompute = not masks or masks[0] is None
    for i, (c, p, nn) in enumerate(zip(clouds, poses_upd, ns)):
        m = _static_mask(c, p, nn, cfg) if recompute else masks[i]
        plan = _plan_for(c, p, nn, m, model, cfg)
        if not plan.supports_landscape(w.shape[1]):
            return None
        out = torch.empty((w.shape[0], 2), dtype=torch.float64, device=w.device)
        plan.eval_landscape(w, e, plan.poses12(p), out, bounds=_eig_bounds(cfg) if recompute else ())
        total += out[:, 0]
        count += out[:, 1]
    return total, count


def _loop_count(views, cfg: Config):
    """Entries behind the loop's mean: the fused views' counts, else the loss clouds' entries (loss.reduce keeps the finite /
    non-NaN ones under only_finite / skip_nans); nan for the ICP loss, which is no mean over points."""
    if cfg.loss in ('icp_loss', 'mesh_loss', 'cloud_loss', 'tsdf_loss'):   # (mesh_loss, cloud_loss, tsdf_loss: the mean of the sequences' means)
        return float('nan')
    kw = cfg.loss_kwargs
    total = 0.0
    for v in views:
        if isinstance(v, PlanCloud):
            total += float(v.count)
            continue
        loss = getattr(v, 'loss', None)
        if not isinstance(loss, torch.Tensor):
            return float('nan')
        loss = loss.reshape(-1)
        total += float(torch.isfinite(loss).sum() if kw.get('only_finite') else
                       (~torch.isnan(loss)).sum() if kw.get('skip_nans') else loss.numel())
    return total


def _plane_landscape_supported(clouds, model, n_params, cfg: Config):
    from .segmentation import PLANE_LANDSCAPE_KINDS
    kw = cfg.loss_kwargs
    return (getattr(cfg, 'fused', True) and cfg.nn_type == NeighborhoodType.plane and cfg.loss in ('min_eigval_loss', 'trace_loss')
            and not cfg.loss_offset and model is not None and getattr(model, 'kernel_kind', None) in PLANE_LANDSCAPE_KINDS
            and n_params in (1, 2) and kw.get('inlier_ratio', 1.0) == 1.0 and kw.get('inlier_max_loss') is None
            and not kw.get('only_finite') and not kw.get('skip_nans') and clouds[0][0].dirs.is_cuda)


def _plane_landscape_kernel(clouds, poses_upd, masks, ns, model, w, cfg: Config):
    """(sums [W], counts [W]) of every sequence through Planes.eval_landscape (the global cloud before the model, as
    eval_loss_clouds builds it for plane neighbourhoods)."""
    _, e = model.kernel_params()
    kw = cfg.loss_kwargs
    normalization = bool(kw.get('normalization', False)) and cfg.loss == 'min_eigval_loss'
    total = torch.zeros((w.shape[0],), dtype=torch.float64, device=w.device)
    count = torch.zeros_like(total)
    for i, (c, p, planes) in enumerate(zip(clouds, poses_upd, ns)):
        g = global_cloud(clouds=c, model=None, poses=p)
        out = torch.empty((w.shape[0], 2), dtype=torch.float64, device=w.device)
        planes.eval_landscape(g, model.kernel_kind, w, e, out, loss=cfg.loss, normalization=normalization, sqrt=bool(kw.get('sqrt')),
                              mask=masks[i] if masks else None)
        total += out[:, 0]
        count += out[:, 1]
    return total, count


def landscape_clouds(clouds, poses, pose_deltas, masks, ns, model, weights, cfg: Config):
    """Loss for every row of ``weights`` ([W, P], or [W] when P == 1; P = the model's kernel weights, exponents from the model)
    -> (loss [W] fp64, count [W] fp64 of the points or planes behind each mean).  Entry j equals ``eval_loss_clouds`` under
    no_grad for a copy of the model with weights[j], for given masks and for masks of None (the global mask recomputed per
    row).  Ball neighbourhoods in a configuration of the fused path (min-eigenvalue or trace loss, no quantile gating, no
    NaN policy, no vp_dispersion_to_depth2 bounds) and P in {1, 2} take one pass over the neighbourhoods
    (dc_sequence_landscape); plane neighbourhoods with a Polynomial / ScaledPolynomial model of 1 or 2 weights and the same
    losses one pass over the plane points (dc_plane_landscape); everything else loops over eval_loss_clouds.
    ``landscape_paths`` counts the path taken."""
    from .loss import create_loss
    device = clouds[0][0].dirs.device
    n_params = _n_weights(model)
    w = _weight_rows(weights, n_params, device)
    with torch.no_grad():
        ball = _landscape_supported(clouds, model, n_params, cfg)
        if ball or _plane_landscape_supported(clouds, model, n_params, cfg):
            poses_upd = [p.detach() for p in create_corrected_poses(poses, pose_deltas, cfg)]
            res = (_landscape_kernel if ball else _plane_landscape_kernel)(clouds, poses_upd, masks, ns, model, w, cfg)
            if res is not None:
                landscape_paths['kernel'] += 1
                total, count = res
                return total / count, count          # 0 / 0 = nan, like the mean over an empty mask
        landscape_paths['loop'] += 1
        loss_fun = create_loss(cfg)
        losses, counts = [], []
        for row in w:
            m = _model_with_weights(model, row)
            loss, views, _, _ = eval_loss_clouds(clouds, poses, pose_deltas, list(masks) if masks else masks, ns, m, loss_fun, cfg)
            losses.append(torch.as_tensor(loss, dtype=torch.float64, device=device).reshape(()))
            counts.append(_loop_count(views, cfg))
        return torch.stack(losses), torch.tensor(counts, dtype=torch.float64, device=device)


def eval_loss_landscape(cfg: Config, weights, test_datasets=None, test_ns=None, model=None, return_neighborhood=False):
    """``eval_loss`` for every row of ``weights`` (see landscape_clouds): datasets, model and neighbourhoods as eval_loss, the
    global masks recomputed per row.  Returns (loss [W], count [W]) (and the neighbourhoods when ``return_neighborhood``)."""
    from .preproc import establish_neighborhoods
    test_names, test_datasets, model = _test_setup(cfg, test_datasets, model)
    test_clouds, test_poses = _load_test_sequences(cfg, test_datasets)
    test_pose_deltas = _test_pose_deltas(cfg, test_datasets)
    if test_ns is None:
        test_ns = [establish_neighborhoods(clouds=clouds, poses=poses, cfg=cfg) for clouds, poses in zip(test_clouds, test_poses)]
    loss, count = landscape_clouds(test_clouds, test_poses, test_pose_deltas, [None] * len(test_datasets), test_ns, model, weights,
                                   cfg)
    if return_neighborhood:
        return loss, count, test_ns
    return loss, count
