"""The slice of the reference's Config (config.py:143-292) that the hot path reads, as a plain attribute bag.

Same attribute names and defaults, ``from_dict`` / ``to_dict`` / ``copy`` / YAML round trip; the ROS-param,
argparse and roslaunch front ends and the experiment bookkeeping are out of scope.  Unlike the
reference's constructor this one does not shell out to ``git``.
"""
from __future__ import annotations

import copy as _copy
import os
import tempfile

import yaml

__all__ = ['bias_eval_csv', 'CLOUD_LOSS_DEFAULTS', 'TSDF_LOSS_DEFAULTS', 'Config', 'Loss', 'loss_eval_csv', 'map_eval_csv', 'Model', 'NeighborhoodType', 'PoseCorrection', 'PoseProvider', 'recon_eval_csv', 'SLAM', 'nonempty',
           'slam_eval_bag', 'slam_eval_csv', 'slam_poses_csv']


class _Names(type):
    def __iter__(cls):
        # the names a default sweep runs (Config.eval_losses = list(Loss)); ``_unlisted`` names are members that a sweep must ask for
        skip = vars(cls).get('_unlisted', ())
        return iter(v for k, v in vars(cls).items() if not k.startswith('_') and isinstance(v, str) and v not in skip)

    def __contains__(cls, item):
        return item in list(iter(cls)) or item in vars(cls).get('_unlisted', ())


class NeighborhoodType(metaclass=_Names):
    ball = 'ball'
    plane = 'plane'


class Loss(metaclass=_Names):
    min_eigval_loss = 'min_eigval_loss'
    trace_loss = 'trace_loss'
    icp_loss = 'icp_loss'
    mesh_loss = 'mesh_loss'          # supervised: distance to the dataset's ground-truth mesh (loss.mesh_loss)
    cloud_loss = 'cloud_loss'        # supervised: distance to the dataset's surveyed cloud (loss.cloud_loss)
    tsdf_loss = 'tsdf_loss'          # self-supervised: distance to the volume the sequence's own scans fuse into (loss.tsdf_loss)
    # need a dataset with a mesh / a survey, or a target that is re-fused as training goes: not part of the default eval_losses sweep
    _unlisted = ('mesh_loss', 'cloud_loss', 'tsdf_loss')


class Model(metaclass=_Names):
    Polynomial = 'Polynomial'
    ScaledPolynomial = 'ScaledPolynomial'


class PoseCorrection(metaclass=_Names):
    none = 'none'
    common = 'common'
    sequence = 'sequence'
    pose = 'pose'


class SLAM(metaclass=_Names):
    """SLAM pipelines eval_slam can run (config.py:82-84).  The reference's one is norlab_icp_mapper through ROS; this package has
    its own scan-to-map point-to-plane ICP configured like it (slam.py, DESIGN "SLAM evaluation")."""
    icp_mapper = 'icp_mapper'


class PoseProvider(metaclass=_Names):
    ground_truth = 'ground_truth'


for _slam in SLAM:                # SLAM pipelines are pose providers too (config.py:91-93)
    setattr(PoseProvider, _slam, _slam)


def nonempty(iterable):
    return [x for x in iterable if x]


def loss_eval_csv(log_dir: str, loss: str, subset: str = None):
    """CSV file eval_loss_all appends to for one loss and subset (config.py:96-103)."""
    if subset:
        path = 'loss_eval_{loss}_{subset}.csv'.format(loss=loss, subset=subset)
    else:
        path = 'loss_eval_{loss}.csv'.format(loss=loss)
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def slam_eval_csv(log_dir: str, slam: str, subset: str = None):
    """CSV file eval_slam_all appends to for one SLAM pipeline and subset (config.py:106-113)."""
    if subset:
        path = 'slam_eval_{slam}_{subset}.csv'.format(slam=slam, subset=subset)
    else:
        path = 'slam_eval_{slam}.csv'.format(slam=slam)
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def bias_eval_csv(log_dir: str, subset: str = None):
    """CSV file eval_bias_all appends to for one subset (named as map_eval_csv names its files; not in the reference)."""
    path = 'bias_eval_{subset}.csv'.format(subset=subset) if subset else 'bias_eval.csv'
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def map_eval_csv(log_dir: str, subset: str = None):
    """CSV file eval_map_all appends to for one subset (named as slam_eval_csv names its files; not in the reference)."""
    path = 'map_eval_{subset}.csv'.format(subset=subset) if subset else 'map_eval.csv'
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def recon_eval_csv(log_dir: str, subset: str = None):
    """CSV file eval_recon_all appends to for one subset (named as map_eval_csv names its files; not in the reference)."""
    path = 'recon_eval_{subset}.csv'.format(subset=subset) if subset else 'recon_eval.csv'
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def slam_eval_bag(log_dir: str, slam: str):
    """(config.py:126-130; no bag is recorded here)"""
    path = 'slam_eval_{slam}.bag'.format(slam=slam)
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


def slam_poses_csv(log_dir: str, name: str, slam: str):
    """Poses CSV of one sequence's SLAM run (config.py:133-140)."""
    if name:
        path = os.path.join(name, 'slam_poses_{slam}.csv'.format(slam=slam))
    else:
        path = os.path.join('slam_poses_{slam}.csv'.format(slam=slam))
    if log_dir:
        path = os.path.join(log_dir, path)
    return path


# the keys loss.cloud_loss reads from Config.loss_kwargs and their defaults (None: required)
CLOUD_LOSS_DEFAULTS = {'cloud_point_to_plane': True, 'cloud_squared': False, 'cloud_max_dist': None, 'cloud_inlier_ratio': 1.0}

# the keys loss.tsdf_loss and eval.tsdf_masks read from Config.loss_kwargs and their defaults (tsdf_trunc None: three voxels;
# tsdf_max_residual None: the truncation)
TSDF_LOSS_DEFAULTS = {'tsdf_voxel_size': 0.1, 'tsdf_trunc': None, 'tsdf_leave_one_out': True, 'tsdf_refresh_every': 10,
                      'tsdf_squared': True, 'tsdf_max_residual': None}


class Config(object):
    def __init__(self, **kwargs):
        self.random_seed = 135
        self.log_dir = os.path.join(tempfile.gettempdir(), 'depth_correction_amd')
        self.enable_ros = False
        # model (config.py:168-180)
        self.model_class = Model.ScaledPolynomial
        self.optimize_model = True
        self.model_args = []
        self.model_kwargs = {}
        self.model_state_dict = ''
        self.float_type = 'float64'
        self.device = 'cuda:0'          # the reference defaults to 'cpu'; this package has no CPU path
        # cloud preprocessing (:182-185)
        self.min_depth = 5.0
        self.max_depth = 25.0
        self.grid_res = 0.2
        # neighbourhoods (:186-194)
        self.nn_type = NeighborhoodType.ball
        self.nn_k = 0
        self.nn_r = 0.25
        self.nn_grid_res = 0.5
        self.min_valid_neighbors = 5
        self.max_neighborhoods = None
        # plane neighbourhoods (NeighborhoodType.plane): RANSAC inlier distance, hypotheses per round, sample size
        self.ransac_dist_thresh = 0.03
        self.num_ransac_iters = 500
        self.ransac_model_size = 3
        self.nn_scale = None
        # neighbourhoods of the per-scan stages (local_feature_cloud, hence correct_cloud and IcpMapper.prepare): 'ball' (nn_k / nn_r,
        # the reference's) or 'image' -- the scan organised on a spherical image_size = [H, W] grid over image_fov = [up, down] degrees
        # (scripts/depth_denoising:44-91), neighbours from the image_window = [ah, aw] half extents around a pixel, gated at nn_r
        # (range_image.py, DESIGN "Range-image neighbourhoods"; not in the reference's Config)
        self.local_nn_type = 'ball'
        self.image_size = [128, 1024]
        self.image_fov = [45., -45.]
        self.image_wrap = True
        self.image_window = [2, 2]
        # filters (:204-218)
        self.shadow_neighborhood_angle = 0.017453
        self.shadow_angle_bounds = []
        self.dir_dispersion_bounds = []
        self.vp_dispersion_bounds = [0.36, float('inf')]
        self.vp_dispersion_to_depth2_bounds = []
        self.vp_dist_to_depth_bounds = []
        self.eigenvalue_bounds = []
        self.eigenvalue_ratio_bounds = [[0, 1, 0, 0.25], [1, 2, 0.25, 1.]]
        # data (:220-235)
        self.dataset = 'room'
        self.dataset_args = []
        self.dataset_kwargs = {}
        self.train_names = []
        self.val_names = []
        self.test_names = []
        self.data_start = None
        self.data_stop = None
        self.data_step = 1
        self.train_poses_path = []
        self.val_poses_path = []
        self.test_poses_path = []
        # training (:246-266)
        self.loss = Loss.min_eigval_loss
        self.loss_offset = False
        self.loss_kwargs = {'sqrt': False, 'normalization': True, 'inlier_max_loss': None, 'inlier_loss_mult': 1.0,
                            'inlier_ratio': 1.0, 'icp_inlier_ratio': 0.3, 'icp_point_to_plane': True}
        # cloud_loss reads its own keys from loss_kwargs with these defaults (CLOUD_LOSS_DEFAULTS; the default dict above, hence
        # every written YAML, stays as it was): cloud_point_to_plane True, cloud_squared False, cloud_inlier_ratio 1.0 and
        # cloud_max_dist, which has no default and must be set.  cloud_samples: the points of the survey a mesh dataset samples
        # from its mesh (SurveyCloud.from_mesh) when it has no survey of its own
        self.cloud_samples = 200000
        self.n_opt_iters = 100
        self.optimizer = 'Adam'
        self.optimizer_args = []
        self.optimizer_kwargs = {}
        self.lr = 2e-4
        # not in the reference: None = shard the sequences over the ranks whenever torch.distributed is initialised with
        # more than one (train.py of this package), False = every process trains on all sequences
        self.distributed = None
        self.pose_correction = PoseCorrection.none
        self.pose_provider = PoseProvider.ground_truth      # (config.py:169-170)
        self.slam = SLAM.icp_mapper
        self.train_pose_deltas = None
        self.test_pose_deltas = None
        self.log_filters = False
        # evaluation (:275, :282): eval_loss appends its result to loss_eval_csv when set; eval_loss_all evaluates these losses
        self.loss_eval_csv = None
        self.eval_losses = list(Loss)
        # SLAM evaluation (config.py:276-283; slam.py): eval_slam appends to slam_eval_csv, writes slam_poses_csv when set
        self.slam_eval_csv = None
        self.slam_eval_bag = None
        self.slam_poses_csv = None
        self.odom_cov = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]     # odometry noise: a scalar, [rot, trans], 6 variances or a 6 x 6 matrix
        self.eval_slams = list(SLAM)
        # the mapper (config/slam/input_filters.yaml, icp.yaml, launch/slam.launch)
        self.slam_normals_k = 9                 # SurfaceNormalDataPointsFilter knn, normals oriented toward the sensor
        self.icp_knn = 3                        # KDTreeMatcher knn
        self.icp_max_dist = 10.0                # KDTreeMatcher maxDist
        self.icp_trim_ratio = 0.8               # TrimmedDistOutlierFilter ratio
        self.icp_max_normal_angle = 1.57        # SurfaceNormalOutlierFilter maxAngle
        self.icp_min_diff_rot = 0.001           # DifferentialTransformationChecker minDiffRotErr
        self.icp_min_diff_trans = 0.01          # minDiffTransErr
        self.icp_smooth_length = 2              # smoothLength
        self.icp_max_iters = 100                # CounterTransformationChecker maxIterationCount
        self.icp_max_rotation = 0.8             # BoundTransformationChecker maxRotationNorm
        self.icp_max_translation = 30.0         # maxTranslationNorm
        self.slam_min_overlap = 0.9             # map_update_overlap
        self.slam_min_dist_new_point = 0.1      # min_dist_new_point
        self.slam_sensor_max_range = 25.0       # sensor_max_range
        # moving sweeps (DESIGN "Moving-sweep rendering and de-skew"; not in the reference's Config): run_slam de-skews every scan that
        # has sweep times with the constant-velocity twist of its prior motion times slam_sweep_fraction before the mapper sees it
        self.slam_deskew = False
        self.slam_sweep_fraction = 1.0
        # sweep-aware registration (DESIGN "Sweep-aware registration"): the ICP estimates the twist of every scan that has sweep times
        # together with its pose; that twist of the prior motion is then the prior twist.  Not together with slam_deskew.
        self.slam_ct = False
        self.slam_ct_prior = [1e-4, 1e-4]       # [beta_v, beta_w]: weight per kept pair of the twist's departure from its prior
                                                # (measured, DESIGN: larger values pull the twist to a noisy odometry's)
        self.slam_ct_max_twist = None           # [trans, rot] bound of that departure; None: [icp_max_translation, icp_max_rotation]
        # dynamic points in the map (launch/slam.launch compute_prob_dynamic and its parameters; DESIGN "Dynamic points in the map").
        # slam.launch runs with compute_prob_dynamic on; the three switches are off here so that existing results and timings stand.
        self.slam_compute_prob_dynamic = False  # update the map points' probabilities of being dynamic before every map update
        self.slam_dynamic_every_scan = False    # ... and for registered scans whose overlap skips the map update (run_slam)
        self.slam_cut_dynamic = False           # keep points with P >= threshold out of the ICP's reference cloud
        self.slam_prior_dynamic = 0.6           # prior_dynamic
        self.slam_threshold_dynamic = 0.9       # threshold_dynamic
        self.slam_beam_half_angle = 0.01        # beam_half_angle
        self.slam_epsilon_a = 0.01              # epsilon_a
        self.slam_epsilon_d = 0.01              # epsilon_d
        self.slam_alpha = 0.8                   # alpha
        self.slam_beta = 0.99                   # beta
        # the map of the icp_mapper pipeline (DESIGN "Scan-to-TSDF registration"; not in the reference's Config): 'points' is the point
        # map above; 'tsdf' registers every scan against a sparse TSDF volume that fuses the registered scans (slam.TsdfMapper)
        self.slam_map = 'points'
        self.slam_tsdf_voxel_size = 0.1         # voxel size of that volume [m]
        self.slam_tsdf_trunc = None             # its truncation [m]; None: 3 voxels
        self.slam_tsdf_min_count = 1            # a voxel is observed from this many visits on
        self.slam_tsdf_max_blocks = None        # a fixed pool of blocks; None: the pool grows
        self.slam_tsdf_max_residual = None      # |distance| from which a sample is no pair [m]; None: the truncation
        # map accuracy against the ground-truth mesh (eval.eval_map, DESIGN "Map accuracy"; not in the reference's Config):
        # eval_map appends to map_eval_csv; map_eval_poses 'dataset' (the poses the dataset yields) or 'slam' (the poses run_slam
        # estimates); the quantile of trimmed_mean; samples of the mesh for completeness_mean (0 = not computed)
        self.map_eval_csv = None
        self.map_eval_poses = 'dataset'
        self.map_eval_inlier_ratio = 0.8
        self.map_eval_samples = 0
        # map_eval_register: eval_map first registers the map to the dataset's survey (registration.register_cloud with
        # register_kwargs; DESIGN "Survey registration") and takes the accuracy of the registered points -- for maps whose poses are
        # not in the survey's frame
        self.map_eval_register = False
        self.register_kwargs = {'inlier_ratio': 0.8, 'max_dist': 1.0, 'n_iters': 50, 'min_rot': 1e-6, 'min_trans': 1e-6}
        # map_eval_register_init: None (the registration starts from the identity) or 'global' (from the prior of
        # registration.register_global with register_global_kwargs; DESIGN "Global registration") -- for maps that are an arbitrary
        # rigid motion away from the survey -- or 'planes' (registration.register_planes with register_planes_kwargs; DESIGN "Plane
        # registration"), for maps of rooms and corridors
        self.map_eval_register_init = None
        self.register_global_kwargs = {}
        self.register_planes_kwargs = {}
        # surface reconstruction (eval.eval_recon, DESIGN "Surface reconstruction"; not in the reference's Config): the scans are fused
        # into a TSDF volume of recon_voxel_size metres truncated at recon_trunc (None: 3 voxels) inside recon_bounds ((lo, hi), None:
        # the box of the posed points); rays beyond recon_max_range are left out; recon_carve_from >= 0 also records the free space
        # from that range on; a voxel seen fewer than recon_min_count times is unobserved.  recon_poses 'dataset' or 'slam' as
        # map_eval_poses.  eval_recon appends to recon_eval_csv and writes the mesh to recon_mesh_ply when set; the accuracy is taken
        # on recon_eval_samples samples of either mesh, the coverage within recon_eval_max_dist (None: not computed)
        self.recon_voxel_size = 0.1
        self.recon_trunc = None
        self.recon_min_count = 1
        self.recon_max_range = None
        self.recon_carve_from = None
        self.recon_bounds = None
        self.recon_sparse = False                # a block-allocated SparseTsdfVolume instead of the dense box (no bounds, no carving)
        self.recon_poses = 'dataset'
        self.recon_eval_csv = None
        self.recon_mesh_ply = None
        self.recon_eval_samples = 100000
        self.recon_eval_max_dist = None
        # depth bias against the ground-truth mesh (eval.eval_bias, DESIGN "Depth bias against the mesh"; not in the reference's
        # Config): eval_bias appends a line per sequence to bias_eval_csv and writes the per-bin table to bias_eval_curve_csv; bins of
        # the true incidence angle over [0, pi/2]; rays with |d - t| above bias_eval_max_residual (metres) are left out; back-face
        # culling of the cast
        self.bias_eval_csv = None
        self.bias_eval_curve_csv = None
        self.bias_eval_bins = 18
        self.bias_eval_max_residual = None
        self.bias_eval_cull = True
        # bias_eval_against: 'auto' (the mesh when the dataset has get_mesh(), else its survey), 'mesh' or 'survey' (a mesh dataset's
        # survey is the one sampled from its mesh: the validation path).  Against a survey the rays are cast on its surfels
        # (metrics.depth_bias' surfel_* arguments; DESIGN "Depth bias against a surveyed cloud"): radius None = scale x the distance
        # to the k-th nearest other survey point; window in metres behind the first disk; the blend's normal gate in radians
        self.bias_eval_against = 'auto'
        self.bias_eval_surfel_radius = None
        self.bias_eval_surfel_k = 10
        self.bias_eval_surfel_scale = 1.0
        self.bias_eval_surfel_window = 0.1
        self.bias_eval_surfel_max_normal_angle = 0.7853981633974483      # pi / 4
        # bias_eval_against = 'tsdf' (never chosen by 'auto'): no ground truth at all -- every test sequence's filtered scans are fused
        # at the poses the dataset yields into a loss.TsdfTarget (voxel size in metres; trunc None: three voxels; min_count) and every
        # ray is cast against that volume (leave_one_out: against the volume of the OTHER scans), marched in steps of
        # bias_eval_tsdf_step (None: half a voxel) up to bias_eval_tsdf_max_range (None: the sequence's farthest depth plus the
        # truncation).  The residual is the ray's bias minus the mean bias of the other views of the surface, not the bias itself
        # (DESIGN "Ray casting the fused volume")
        self.bias_eval_tsdf_voxel_size = 0.1
        self.bias_eval_tsdf_trunc = None
        self.bias_eval_tsdf_min_count = 1
        self.bias_eval_tsdf_leave_one_out = True
        self.bias_eval_tsdf_step = None
        self.bias_eval_tsdf_max_range = None
        self.show_results = False
        # this build: use the fused per-sequence kernels whenever the configuration allows it
        self.depth_bias_model_class = Model.ScaledPolynomial   # dataset.noisy_dataset: a known bias through model.inverse
        self.depth_bias_model_args = []                         # (config.py:237-240); all-zero weights add nothing
        self.depth_bias_model_kwargs = {}
        self.depth_noise = 0.0           # dataset.noisy_dataset (config.py:242-244)
        self.pose_noise = 0.0
        self.pose_noise_mode = None
        self.fused = True
        # train(): iterations between two host synchronisations when nobody watches single iterations (no-op callbacks, one
        # process); 1 = the reference's per-iteration bookkeeping (train.py _batched_loop); loop_graph: replay the iteration as
        # one hipGraph
        self.loop_batch = 64
        self.loop_graph = True
        self.loop_graph_iters = 8      # iterations per captured graph of the loops with pose corrections (train._native_pose_loop)
        self.loop_native = True        # model-only runs: the library's chained step, one launch per iteration (train._native_loop)
        self.keep_plans = False        # train() releases the per-sequence plans it built when it returns; True keeps them cached
        self.from_dict(kwargs)

    # ---- Configurable subset (configurable.py:44-58,166-179) ----
    def from_dict(self, d):
        for k, v in d.items():
            setattr(self, k, v)
        return self

    def to_dict(self):
        return {k: v for k, v in vars(self).items() if not k.startswith('_')}

    def copy(self):
        return _copy.deepcopy(self)

    def diff(self, other):
        a, b = self.to_dict(), other.to_dict()
        return {k: v for k, v in a.items() if k not in b or b[k] != v}

    def non_default(self):
        return self.diff(type(self)())

    def to_yaml(self, path=None):
        text = yaml.safe_dump(self.to_dict())
        if path is None:
            return text
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text)

    def from_yaml(self, path):
        with open(path) as f:
            return self.from_dict(yaml.safe_load(f) or {})

    def data_slice(self):
        return slice(self.data_start, self.data_stop, self.data_step)

    def numpy_float_type(self):
        import numpy as np
        return getattr(np, self.float_type)

    def torch_float_type(self):
        import torch
        return getattr(torch, self.float_type)
