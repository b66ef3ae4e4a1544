"""Plane neighbourhoods without a GPU: the RANSAC sampler, the configuration fields, the clear error on CPU clouds."""
import numpy as np
import pytest
import torch


def _splitmix64_np(x):
    """An independent restatement of splitmix64 in numpy uint64 arithmetic (wraps modulo 2^64)."""
    with np.errstate(over='ignore'):
        z = np.uint64(x) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))


PINNED = [((135, 0, 0, 20000), (19410, 12446, 12360)),
          ((135, 0, 499, 20000), (16091, 18908, 18719)),
          ((135, 3, 17, 12345), (9833, 7858, 6421)),
          ((0, 0, 1, 3), (1, 2, 2)),
          ((2 ** 63 + 5, 7, 250, 1000003), (694489, 264203, 478978))]


@pytest.mark.parametrize('args,want', PINNED)
def test_ransac_sampler_pinned_table(args, want):
    from depth_correction_amd.segmentation import ransac_sample
    assert ransac_sample(*args) == want


def test_ransac_sampler_matches_uint64_restatement():
    from depth_correction_amd.segmentation import ransac_sample
    for seed, m, h, n in [(135, 0, 0, 20000), (1, 2, 3, 7), (2 ** 64 - 1, 11, 1023, 99991)]:
        s = seed & (2 ** 64 - 1)
        want = tuple(_splitmix64_np(s ^ ((m << 40) & (2 ** 64 - 1)) ^ (h << 2) ^ t) % n for t in range(3))
        assert ransac_sample(seed, m, h, n) == want


def test_config_has_ransac_fields():
    from depth_correction_amd.config import Config
    cfg = Config()
    assert cfg.ransac_dist_thresh == 0.03
    assert cfg.num_ransac_iters == 500
    assert cfg.ransac_model_size == 3


def test_plane_neighbourhoods_on_cpu_need_a_gpu():
    from depth_correction_amd.config import Config, NeighborhoodType
    from depth_correction_amd.depth_cloud import DepthCloud
    from depth_correction_amd.preproc import establish_neighborhoods
    cfg = Config(nn_type=NeighborhoodType.plane, device='cpu')
    cloud = DepthCloud.from_points(torch.rand((100, 3), dtype=torch.float64) + 1.0)
    with pytest.raises(RuntimeError, match='needs a GPU|need a GPU'):
        establish_neighborhoods(cloud=cloud, cfg=cfg)


def test_planes_container():
    from depth_correction_amd.segmentation import Planes
    p = Planes(torch.tensor([[0.0, 0.0, 1.0, -1.0], [1.0, 0.0, 0.0, 2.0]], dtype=torch.float64),
               cloud=[None, None], indices=[torch.arange(3), torch.arange(3, 5)])
    assert len(p) == 2 and len(p.copy()) == 2
    d = p.distance(torch.tensor([[0.0, 0.0, 3.0]], dtype=torch.float64))
    assert torch.equal(d, torch.tensor([2.0, 2.0], dtype=torch.float64))
    q = p.orient(torch.tensor([[-5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]], dtype=torch.float64))
    assert len(q) == 2
    sub = p[torch.tensor([False, True])]
    assert len(sub) == 1 and torch.equal(sub.indices[0], torch.arange(3, 5))
