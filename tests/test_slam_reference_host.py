"""The reference mapper (tests/slam_reference.py) on its own, no GPU: it recovers a perturbed prior on RoomBoxDataset scans, does not
depend on the order of its pair sums, and every discrete decision it takes on the inputs of the GPU comparison keeps a margin many
orders above fp64 rounding -- so a device that differs from it by rounding takes the same decisions.  A margin that becomes small
fails here; a case is never dropped for it."""
import math

import numpy as np
import pytest

import slam_reference as R
from helpers import slam_pose as _pose

MARGIN_FLOOR = 1e-9          # relative (absolute for the cosine and the metres of the map rule): 1e7 x fp64 rounding
ORDER_BAR = 1e-14            # pose change from permuting the pair sums

OFFSET = _pose(0.03, (0.1, -0.05, 0.02))


@pytest.fixture(scope='module')
def scans():
    from depth_correction_amd.dataset import RoomBoxDataset
    out = []
    for cloud, pose in RoomBoxDataset(n_pts=20000, n_poses=4, dtype=np.float64):
        p = np.stack([cloud[f] for f in 'xyz'], axis=1).astype(np.float64)
        n, _ = R.normals(p, 9)
        out.append((p, n, np.linalg.norm(p, axis=1), pose))
    return out


@pytest.fixture(scope='module')
def first_map(scans):
    p, n, d, pose = scans[0]
    pts, nrm, added, _ = R.update(np.zeros((0, 3)), np.zeros((0, 3)), p, n, d, pose, R.params())
    assert added == len(p)
    return pts, nrm


def _margins_ok(reg):
    for r in reg.records:
        assert r.margins['thr'] >= MARGIN_FLOOR, r.margins
        assert r.margins['normal'] >= MARGIN_FLOOR, r.margins
        for key in ('conv_rot', 'conv_trans'):
            assert r.margins.get(key, 1.0) >= MARGIN_FLOOR, r.margins


@pytest.mark.parametrize('max_dist', [10.0, 0.3])
def test_reference_recovers_perturbed_prior(scans, first_map, max_dist):
    prm = R.params(icp_max_dist=max_dist)
    for i in (1, 2, 3):
        p, n, d, gt = scans[i]
        reg = R.register(first_map[0], first_map[1], p, n, gt @ OFFSET, prm)
        D = np.linalg.solve(reg.pose, gt)
        rot, trans = R.rotation_angle(D), float(np.linalg.norm(D[:3, 3]))
        print(i, reg.status, reg.iterations, 'error rad / m', rot, trans, 'unmatched', reg.records[0].margins['unmatched'])
        assert reg.status == 'converged' and reg.iterations == 4
        # the range noise of the scans is 1e-3 relative (about 1 cm at 10 m): the pose is recovered well inside it
        assert rot <= 1e-3 and trans <= 5e-3, (rot, trans)
        assert len(reg.poses) == len(reg.increments) == 4
        _margins_ok(reg)
        if max_dist == 0.3:
            assert 0.05 < reg.records[0].margins['unmatched'] < 0.2
            table = reg.records[0].dist
            assert reg.records[0].thr == np.quantile(table[np.isfinite(table)], 0.8) < np.quantile(table, 0.8)


def test_reference_independent_of_summation_order(scans, first_map):
    prm = R.params()
    worst = 0.0
    for i in (1, 2, 3):
        p, n, d, gt = scans[i]
        a = R.register(first_map[0], first_map[1], p, n, gt @ OFFSET, prm)
        b = R.register(first_map[0], first_map[1], p, n, gt @ OFFSET, prm, order_seed=11 * i)
        assert a.status == b.status and a.iterations == b.iterations
        for ra, rb in zip(a.records, b.records):
            assert np.array_equal(ra.kept, rb.kept)
            worst = max(worst, np.abs(ra.pose - rb.pose).max())
    print('largest pose change from the order of the pair sums:', worst)
    assert worst <= ORDER_BAR


def test_reference_sequence_and_map_margins(scans):
    prm = R.params(slam_min_overlap=1.01)
    gt = np.stack([s[3] for s in scans])
    res = R.run([s[:3] for s in scans], gt, prm)
    sizes = [i['map_size'] for i in res['info']]
    print([(i['status'], i['iterations'], i['added'], i['map_size']) for i in res['info']])
    assert res['info'][0]['status'] == 'init' and all(i['status'] == 'converged' for i in res['info'][1:])
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and sizes[-1] == len(res['map_pts']) == len(res['map_nrm'])
    for i in res['info'][1:]:
        assert i['margins']['min_dist'] >= MARGIN_FLOOR and i['margins']['thr'] >= MARGIN_FLOOR, i
    # default overlap rule: a scan that overlaps the map by 0.9 or more adds nothing
    res2 = R.run([s[:3] for s in scans], gt, R.params())
    for a, b in zip(res['info'], res2['info']):
        if b['status'] != 'init':
            assert b['margins']['overlap'] >= MARGIN_FLOOR
            assert (b['added'] == 0) == (b['overlap'] >= 0.9)


def test_reference_failures_keep_prior():
    rng = np.random.default_rng(3)
    mp = rng.uniform(-1, 1, size=(2, 3))
    mn = np.tile([0.0, 0.0, 1.0], (2, 1))
    p = rng.uniform(-1, 1, size=(50, 3))
    pn = np.tile([0.0, 0.0, 1.0], (50, 1))
    prior = _pose(0.1, (0.2, 0.0, 0.0))
    reg = R.register(mp, mn, p, pn, prior, R.params())
    assert reg.status == 'singular' and np.array_equal(reg.pose, prior) and reg.iterations == 1
    reg = R.register(mp, mn, p[:1], pn[:1], prior, R.params())
    assert reg.status == 'too_few_pairs' and np.array_equal(reg.pose, prior)
    assert R.register(mp, mn, p[:0], pn[:0], prior, R.params()).status == 'empty'
    assert R.register(mp[:0], mn[:0], p, pn, prior, R.params()).status == 'init'
    # a table with missing neighbours: the threshold is the quantile of the matched distances, NaN only when nothing matched
    assert R.quantile_finite([1.0, 2.0, np.inf], 0.5) == 1.5
    assert math.isnan(R.quantile_finite([np.inf, np.nan], 0.5))


def test_reference_normals_on_planes():
    rng = np.random.default_rng(4)
    p = np.concatenate([np.c_[rng.uniform(-1, 1, (500, 2)), np.full(500, 2.0)], np.c_[np.full(500, -3.0), rng.uniform(-1, 1, (500, 2))]])
    n, grazing = R.normals(p, 9)
    assert np.abs(np.abs(n[:500, 2]) - 1).max() < 1e-12 and np.abs(np.abs(n[500:, 0]) - 1).max() < 1e-12
    assert (np.einsum('ij,ij->i', n, p) < 0).all() and grazing.min() > 0.5
