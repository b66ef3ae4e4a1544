"""The surfel ray caster's per-ray arithmetic (csrc/dc_surfelmath.h) on the host build: test_disk against exact rational arithmetic,
the disks' boxes, property 1 (no box rejects a disk the test accepts), the brute-force cast against the numpy oracle
(tests/surfel_reference.py), the statistical argument for blending on the oracle, the Python layer's refusals and the code object's
notes.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import surfel_reference as S


@pytest.fixture(scope='module')
def lib():
    return S.surfel_host_lib()


# ---- 1. test_disk -------------------------------------------------------------------------------------------------------------------
def _exact(row, o, d, t_min):
    """The rule in exact rational arithmetic: (hit, t) for finite inputs."""
    p, n, rho2 = [Fraction(v) for v in row[:3]], [Fraction(v) for v in row[3:6]], Fraction(row[6])
    o, d = [Fraction(v) for v in o], [Fraction(v) for v in d]
    q = [a - b for a, b in zip(p, o)]
    den = sum(a * b for a, b in zip(n, d))
    if den == 0:
        return False, None
    t = sum(a * b for a, b in zip(n, q)) / den
    h = [t * a - b for a, b in zip(d, q)]
    return t > Fraction(t_min) and sum(a * a for a in h) <= rho2, t


def test_disk_rule_on_dyadic_inputs(lib):
    up, down = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, -np.inf)
    wall = [0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 1.5625, 0.0]                  # p = (0, 0, 4), n = z, rho = 1.25
    cases = [                                                            # (row, o, d, t_min, expected verdict)
        (wall, [0.75, 1.0, 0.0], [0.0, 0.0, 1.0], 0.0, True),            # h = (0.75, 1, 0): exactly on the rim
        (wall, [up(0.75), 1.0, 0.0], [0.0, 0.0, 1.0], 0.0, False),       # one ulp outside
        (wall, [0.75, up(1.0), 0.0], [0.0, 0.0, 1.0], 0.0, False),
        (wall, [down(0.75), 1.0, 0.0], [0.0, 0.0, 1.0], 0.0, True),
        (wall, [0.0, 0.0, 4.0], [1.0, 0.0, 0.0], -1.0, False),           # in the disk's plane: den = 0
        (wall, [0.0, 0.0, 0.0], [1.0, 1.0, 0.0], 0.0, False),            # parallel to it
        (wall, [0.75, 1.0, 0.0], [0.0, 0.0, 1.0], 4.0, False),           # t = t_min
        (wall, [0.75, 1.0, 0.0], [0.0, 0.0, 1.0], down(4.0), True),
        (wall, [0.75, 1.0, 8.0], [0.0, 0.0, -1.0], 0.0, True),           # from the back side
        (wall, [0.75, 1.0, 8.0], [0.0, 0.0, 1.0], 0.0, False),           # behind the ray
        (wall, [0.5, 0.5, 0.0], [0.0, 0.0, 0.5], 0.0, True),             # t in units of |d|: t = 8
        ([0.0, 0.0, 4.0, 0.0, 0.0, -2.0, 1.5625, 0.0], [0.75, 1.0, 0.0], [0.0, 0.0, 1.0], 0.0, True),      # n flipped, |n| = 2
        ([0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 0.0, True),           # rho = 0, through the centre
        ([0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 0.0, 0.0], [2.0 ** -500, 0.0, 0.0], [0.0, 0.0, 1.0], 0.0, False),
        ([1.0, 2.0, 2.0, 1.0, 2.0, 2.0, 0.25, 0.0], [0.0, 0.0, 0.0], [0.5, 1.0, 1.0], 0.0, True),          # tilted: den = 4.5 ... exact t = 2
    ]
    rng = np.random.default_rng(3)
    n_random = 0
    while n_random < 400:                                                # random dyadic pairs whose quotient is exact (den a power of 2)
        n = rng.integers(-3, 4, 3).astype(float)
        d = rng.integers(-4, 5, 3).astype(float) / 2
        den = float(n @ d)
        if den == 0 or math.log2(abs(den)) % 1:
            continue
        p = rng.integers(-16, 17, 3) / 4.0
        o = p + rng.integers(-4, 5, 3) / 4.0 - float(rng.integers(-1, 4)) * d          # the ray passes within a metre or so of the centre
        rho2 = float(rng.integers(0, 40)) / 8
        cases.append(([*p, *n, rho2, 0.0], list(o), list(d), float(rng.integers(-2, 3)), None))
        n_random += 1
    rows = np.array([c[0] for c in cases])
    o, d, t_min = np.array([c[1] for c in cases]), np.array([c[2] for c in cases]), np.array([c[3] for c in cases])
    hit, t, _ = S.host_test_pairs(lib, rows, o, d, t_min)
    n_hit = 0
    for i, c in enumerate(cases):
        want, t_exact = _exact(rows[i], o[i], d[i], t_min[i])
        assert c[4] is None or c[4] == want, i
        assert hit[i] == want, (i, c)
        if t_exact is not None:
            assert Fraction(t[i]) == t_exact, i
        n_hit += want
    assert 100 < n_hit < len(cases) - 100


def test_disk_rule_not_finite(lib):
    nan, inf = np.nan, np.inf
    wall = [0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 1.5625, 0.0]
    o, d = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    cases = [([0.0, 0.0, 4.0, nan, 0.0, 1.0, 1.5625, 0.0], o, d), ([0.0, 0.0, 4.0, 0.0, 0.0, nan, 1.5625, 0.0], o, d),
             (wall, o, [nan, 0.0, 1.0]), (wall, o, [0.0, 0.0, nan]), (wall, [nan, 0.0, 0.0], d), (wall, o, [0.0, 0.0, inf]),
             (wall, [0.0, 0.0, -inf], d), ([0.0, 0.0, 4.0, 0.0, 0.0, 1.0, nan, 0.0], o, d), ([0.0, 0.0, inf, 0.0, 0.0, 1.0, 1.5625, 0.0], o, d),
             (wall, o, [0.0, 0.0, 0.0])]
    hit, _, _ = S.host_test_pairs(lib, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], -inf)
    assert not hit.any()
    assert S.host_test_pairs(lib, [wall], [o], [d], -inf)[0][0]
    idx, t1, t, inc, cnt = S.host_cast_brute(lib, [wall], [o, o], [[nan, 0.0, 1.0], d], 0.0, 0.1, 0.5)
    assert idx.tolist() == [-1, 0] and t1[0] == inf and t[0] == inf and np.isnan(inc[0]) and cnt.tolist() == [0, 1]
    assert t1[1] == 4.0 and t[1] == 4.0 and inc[1] == 0.0


# ---- 2. boxes ----------------------------------------------------------------------------------------------------------------------
def _random_disks(seed, n):
    """Disks of every kind the box must hold: random normals of random length, normals normalised in fp64 (|n| = 1 to an ulp),
    axis-aligned normals, rho = 1e-3 at |p| = 1e3, rho = 10, dyadic centres."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-30, 30, size=(n, 3))
    nrm = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10, size=(n, 1))
    rho = rng.uniform(0.01, 0.5, size=n)
    k = np.arange(n) % 8
    unit = k == 1
    nrm[unit] /= np.linalg.norm(nrm[unit], axis=1, keepdims=True)
    axis = k == 2
    nrm[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-1.0, 1.0, 0.5, -3.0], size=(axis.sum(), 1))
    far = k == 3
    p[far] = rng.normal(size=(far.sum(), 3))
    p[far] *= 1e3 / np.linalg.norm(p[far], axis=1, keepdims=True)
    rho[far] = 1e-3
    rho[k == 4] = 10.0
    dy = k == 5                                                          # dyadic centres and radii with axis-aligned normals: nothing rounds
    p[dy] = rng.integers(-64, 65, size=(dy.sum(), 3)) / 8.0
    rho[dy] = rng.integers(1, 9, size=dy.sum()) / 8.0
    nrm[dy] = np.eye(3)[rng.integers(0, 3, dy.sum())]
    return p, nrm, rho, axis | dy


def _margin(p, rho):
    return 2.0 ** -48 * (np.abs(p).sum(axis=1) + rho)


def test_boxes_hold_their_disks_and_stay_flat(lib):
    p, nrm, rho, aligned = _random_disks(5, 10000)
    box = S.host_boxes(lib, p, nrm, rho).astype(np.longdouble)
    L = np.longdouble
    pl, nl = p.astype(L), nrm.astype(L)
    nl = nl / np.sqrt((nl ** 2).sum(axis=1, keepdims=True))
    helper = np.eye(3)[np.argmin(np.abs(nrm), axis=1)].astype(L)          # the axis least along n
    u = np.cross(nl, helper)
    u = u / np.sqrt((u ** 2).sum(axis=1, keepdims=True))
    v = np.cross(nl, u)
    for phi in np.arange(64) * (2 * np.pi / 64):
        rim = pl + rho.astype(L)[:, None] * (L(math.cos(phi)) * u + L(math.sin(phi)) * v)
        assert (rim >= box[:, :3]).all() and (rim <= box[:, 3:]).all(), phi
    assert (pl >= box[:, :3]).all() and (pl <= box[:, 3:]).all()
    # a wall-aligned disk: no thickness but the margin and one fp32 ulp per side
    a = np.argmax(np.abs(nrm[aligned]), axis=1)
    rows = np.arange(aligned.sum())
    b = box[aligned].astype(np.float64)
    thick = b[rows, 3 + a] - b[rows, a]
    ulp = np.spacing(np.maximum(np.abs(b[rows, a]), np.abs(b[rows, 3 + a])).astype(np.float32)).astype(np.float64)
    assert (thick <= 2 * ulp + 2 * _margin(p[aligned], rho[aligned])).all()
    # and the in-plane extent is tight: within the margin and the roundings of rho on the other two axes
    other = (a + 1) % 3
    wide = b[rows, 3 + other] - b[rows, other]
    ulp_o = np.spacing(np.maximum(np.abs(b[rows, other]), np.abs(b[rows, 3 + other])).astype(np.float32)).astype(np.float64)
    assert (wide >= 2 * rho[aligned]).all() and (wide <= 2 * rho[aligned] * (1 + 1e-15) + 2 * ulp_o + 2 * _margin(p[aligned], rho[aligned])).all()


# ---- 3. property 1 -----------------------------------------------------------------------------------------------------------------
def _property_one_rays(seed):
    """(points, normals, radii, o, d): (ray, disk) pairs near acceptance -- random rays through the disk, rays aimed at rim points and
    one ulp to either side, axis-parallel rays from the world origin grazing a rim; ranges from 0.1 m to 1e3 m."""
    rng = np.random.default_rng(seed)
    P, N, Rho, O, D = [], [], [], [], []

    def frame(n):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        u = np.cross(n, np.eye(3)[np.argmin(np.abs(n), axis=1)])
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return u, np.cross(n, u)

    def add(p, n, rho, o, d):
        P.append(p), N.append(n), Rho.append(rho), O.append(o), D.append(d)

    m = 20000
    for kind in ('inside', 'rim', 'axis'):
        p, n, rho, _ = _random_disks(seed + len(P), m)
        u, v = frame(n)
        phi = rng.uniform(0, 2 * np.pi, m)
        rad = rho * (np.sqrt(rng.uniform(0, 1, m)) if kind == 'inside' else 1.0)
        x = p + rad[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
        rng_len = 10.0 ** rng.uniform(-1, 3, m)
        if kind == 'axis':                                               # the disk moved so that the rim point lies on a world axis
            ax = np.eye(3)[rng.integers(0, 3, m)] * rng.choice([-1.0, 1.0], size=(m, 1))
            p = p + (ax * rng_len[:, None] - x)
            add(p, n, rho, np.zeros((m, 3)), ax * 10.0 ** rng.uniform(-2, 2, size=(m, 1)))
            continue
        w = rng.normal(size=(m, 3))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        o = x - w * rng_len[:, None]
        d = (x - o) * 10.0 ** rng.uniform(-2, 2, size=(m, 1))
        add(p, n, rho, o, d)
        if kind == 'rim':
            for step in (-1.0, 1.0):
                comp = rng.integers(0, 3, m)
                o2, d2 = o.copy(), d.copy()
                o2[np.arange(m), comp] = np.nextafter(o2[np.arange(m), comp], step * np.inf)
                add(p, n, rho, o2, d)
                d2[np.arange(m), comp] = np.nextafter(d2[np.arange(m), comp], step * np.inf)
                add(p, n, rho, o, d2)
    return tuple(np.concatenate(a) for a in (P, N, Rho, O, D))


def test_no_box_rejects_an_accepted_disk(lib):
    from helpers import host_ray_box_entry, host_ray_prune_far
    p, n, rho, o, d = _property_one_rays(40)
    hit, t, _ = S.host_test_pairs(lib, S.disk_rows(p, n, rho), o, d, 0.0)
    kinds = np.arange(len(hit)) // 20000
    for k in range(kinds.max() + 1):                                     # every family has accepted pairs: the test is not vacuous
        assert hit[kinds == k].sum() > 2000, (k, hit[kinds == k].sum())
    box = S.host_boxes(lib, p, n, rho)[hit]
    o, d, t = o[hit], d[hit], t[hit]
    assert np.isfinite(host_ray_box_entry(lib, o, d, box, np.inf)).all()
    far = host_ray_prune_far(lib, t)
    entry = host_ray_box_entry(lib, o, d, box, far)
    assert np.isfinite(entry).all(), int((~np.isfinite(entry)).sum())
    # and with the bound of the second pass, prune_far(t + window) >= prune_far(t)
    assert (host_ray_prune_far(lib, t + 0.1) >= far).all()


# ---- 4. the brute-force cast against the oracle ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def room():
    pts, nrm, rho = S.room_survey()
    vps, dirs, off, poses = S.room_rays()
    o, d = S.world_rays(vps, dirs, off, poses)
    return pts, nrm, rho, o, d


def test_brute_force_first_pass_is_the_oracle_bit_for_bit(lib, room):
    pts, nrm, rho, o, d = room
    rows = S.disk_rows(pts, nrm, rho)
    for t_min in (0.0, 1.5):
        ref = S.oracle(pts, nrm, rho, o, d, t_min=t_min, window=0.0)
        idx, t1, t, inc, cnt = S.host_cast_brute(lib, rows, o, d, t_min, 0.0, 0.5)
        assert (idx >= 0).sum() > (0.99 if t_min == 0.0 else 0.4) * len(idx)
        assert np.array_equal(idx, ref.index) and np.array_equal(t1, ref.t_first) and np.array_equal(cnt, ref.count)
        assert np.array_equal(t, t1) and np.array_equal(t, ref.t.astype(np.float64))
        assert np.array_equal(inc, ref.inc, equal_nan=True) and set(np.unique(cnt)) <= {0, 1}


@pytest.mark.parametrize('min_cos', [math.cos(math.pi / 4), 0.0])
def test_brute_force_blend_within_the_error_count(lib, room, min_cos):
    pts, nrm, rho, o, d = room
    ref = S.oracle(pts, nrm, rho, o, d, window=0.1, min_cos=min_cos)
    idx, t1, t, inc, cnt = S.host_cast_brute(lib, S.disk_rows(pts, nrm, rho), o, d, 0.0, 0.1, min_cos)
    assert np.array_equal(idx, ref.index) and np.array_equal(t1, ref.t_first) and np.array_equal(cnt, ref.count)
    assert cnt.max() >= 8 and (t[idx >= 0] >= t1[idx >= 0]).all() and (t[idx >= 0] <= t1[idx >= 0] + 0.1).all()
    et, bt = S.t_err_units(t, ref)
    ec, bc = S.cos_err_units(inc, ref)
    print('min_cos %.3f: largest multiple of the error count: t %.3f (%.2f units), cos(inc) %.3f (%.2f units); k up to %d, kappa up to %.3f'
          % (min_cos, (et / bt).max(), et.max(), (ec / bc).max(), ec.max(), cnt.max(), ref.kappa.max()))
    assert (et <= bt).all() and (ec <= bc).all()
    # the restated counts are the header's
    for k, tt, t0, kap in ((1, 2.0, 2.0, 1.0), (9, 3.25, 3.2, 1.4), (40, 100.0, 99.9, 7.0)):
        assert lib.dc_host_surfel_t_err(k, tt, t0) == k * (tt - t0) + 0.5 * tt
        assert lib.dc_host_surfel_cos_err(k, kap) == (0.5 * k + 1.75) * kap + 7.5


def test_acos01_is_an_arc_cosine(lib):
    x = np.concatenate([np.random.default_rng(0).uniform(0, 1, 20000), [0.0, 1.0, 0.5, 2.0 ** -58, 1 - 2.0 ** -53, np.nextafter(0.5, 0)]])
    got = S.host_acos(lib, x)
    want = np.array([math.acos(v) for v in x])
    assert (np.abs(got - want) <= np.spacing(want)).all() and np.array_equal(got, S.acos01(x))
    assert np.isnan(S.host_acos(lib, [np.nan]))[0]


# ---- 5. why the blend: the statistics of the first hit ---------------------------------------------------------------------------------
def test_first_hit_is_biased_and_the_blend_is_not():
    """A survey with 5 mm of noise along the normal, about ten overlapping disks per ray: the first disk a ray meets is the one moved
    farthest towards the sensor, by about -1.5 sigma / cos(theta) -- a depth error that grows with the incidence angle, the curve
    eval_bias exists to measure.  The blend's mean stays within a quarter of it in every bin.  Measured here (seed 135): first hit
    -7.5 .. -27.1 mm, blended |mean| <= 1.1 mm, worst ratio 0.14."""
    pts, nrm, dirs, theta, depth = S.wall_scene()
    o = np.tile(S.WALL_SENSOR, (len(dirs), 1))
    ref = S.oracle(pts, nrm, np.full(len(pts), S.WALL_RHO), o, dirs, window=S.WALL_WINDOW)
    assert (ref.index >= 0).all()
    assert 8.0 < ref.count.mean() < 11.0
    S.check_wall(theta, ref.t_first - depth, ref.t.astype(np.float64) - depth)


# ---- 6. the Python layer's refusals -----------------------------------------------------------------------------------------------------
def test_python_refusals():
    import torch
    from depth_correction_amd import ops
    from depth_correction_amd.survey import SurfelBVH, SurveyCloud
    pts, nrm, _ = S.room_survey(m=50)
    survey = SurveyCloud(pts, nrm)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='radius'):
            survey.surfels('cuda:0', radius=bad)
    with pytest.raises(RuntimeError, match='GPU'):
        survey.surfels('cpu', radius=0.1)
    z3, z1 = torch.zeros((4, 3), dtype=torch.float64), torch.ones((4,), dtype=torch.float64)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.surfel_bvh_build(z3, z3, z1, [0, 0, 0, 1, 1, 1])
    bvh = SurfelBVH(torch.zeros(1, dtype=torch.int32), None, None, None, None)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.surfel_cast_rays(bvh, z3, z3, [0, 4], torch.eye(4, dtype=torch.float64)[None])
    assert ops.SURFEL_MIN_COS == math.cos(math.pi / 4)


def test_cast_argument_checks_come_before_the_launch(monkeypatch):
    """window < 0, min_cos = 1 and a NaN t_min are refused by ops.surfel_cast_rays itself (the operand checks stubbed out: no GPU
    here), with the messages a caller sees."""
    import torch
    from depth_correction_amd import ops
    from depth_correction_amd.survey import SurfelBVH
    monkeypatch.setattr(ops, 'need', lambda t, *a, **k: t)
    bvh = SurfelBVH(torch.zeros(1, dtype=torch.int32), None, None, None, None)
    z3 = torch.zeros((4, 3), dtype=torch.float64)
    poses = torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(ValueError, match='window'):
        ops.surfel_cast_rays(bvh, z3, z3, [0, 4], poses, window=-0.1)
    with pytest.raises(ValueError, match='window'):
        ops.surfel_cast_rays(bvh, z3, z3, [0, 4], poses, window=float('nan'))
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='min_cos'):
            ops.surfel_cast_rays(bvh, z3, z3, [0, 4], poses, min_cos=bad)
    with pytest.raises(ValueError, match='t_min'):
        ops.surfel_cast_rays(bvh, z3, z3, [0, 4], poses, t_min=float('nan'))
    with pytest.raises(ValueError, match='scan_offset'):
        ops.surfel_cast_rays(bvh, z3, z3, [0, 3], poses)


def test_eval_bias_chooses_its_ground_truth():
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import _bias_truth, eval_bias
    from depth_correction_amd.model import BaseModel
    from depth_correction_amd.survey import SurveyCloud
    pts, nrm, _ = S.room_survey(m=50)

    class Neither(object):
        def __iter__(self):
            return iter(())

        def __str__(self):
            return 'plain/seq'

    class SurveyOnly(Neither):
        survey = SurveyCloud(pts, nrm)

    class MeshOnly(Neither):
        def get_mesh(self):
            return 'the mesh'

        def get_survey(self, n=None):
            return 'its survey'

    cfg = Config(device='cpu')
    assert (cfg.bias_eval_against, cfg.bias_eval_surfel_radius, cfg.bias_eval_surfel_k, cfg.bias_eval_surfel_scale, cfg.bias_eval_surfel_window,
            cfg.bias_eval_surfel_max_normal_angle) == ('auto', None, 10, 1.0, 0.1, math.pi / 4)
    cfg.bias_eval_against, cfg.bias_eval_surfel_window = 'survey', 0.25
    other = cfg.copy()
    assert (other.bias_eval_against, other.bias_eval_surfel_window, other.bias_eval_surfel_k) == ('survey', 0.25, 10)
    cfg.bias_eval_against = 'auto'
    assert _bias_truth(SurveyOnly(), 's', cfg) is SurveyOnly.survey and _bias_truth(MeshOnly(), 'm', cfg) == 'the mesh'
    cfg.bias_eval_against = 'survey'
    assert _bias_truth(SurveyOnly(), 's', cfg) is SurveyOnly.survey and _bias_truth(MeshOnly(), 'm', cfg) == 'its survey'
    with pytest.raises(ValueError, match='no surveyed cloud'):
        eval_bias(cfg, test_datasets=[Neither()], model=BaseModel())
    cfg.bias_eval_against = 'mesh'
    assert _bias_truth(MeshOnly(), 'm', cfg) == 'the mesh'
    with pytest.raises(ValueError, match=r'no get_mesh\(\)'):
        eval_bias(cfg, test_datasets=[SurveyOnly()], model=BaseModel())
    cfg.bias_eval_against = 'cloud'
    with pytest.raises(ValueError, match='bias_eval_against'):
        eval_bias(cfg, test_datasets=[SurveyOnly()], model=BaseModel())
    cfg.bias_eval_against = 'auto'
    with pytest.raises(RuntimeError, match='needs a GPU'):               # a survey-only dataset gets as far as a mesh dataset does
        eval_bias(cfg, test_datasets=[SurveyOnly()], model=BaseModel())


# ---- 7. the code object ----------------------------------------------------------------------------------------------------------------
def test_cast_kernel_resources():
    """surfel_cast_kernel keeps nothing in scratch memory and its per-lane stack takes 32 KB of LDS per 128-lane block, in both
    dtypes.  Metadata notes of the built library only."""
    import re
    from test_step_kernel_resources import _code_objects, _kernels
    import __graft_entry__ as ge
    ge.build()
    from depth_correction_amd import _native
    blob = open(_native.lib_path(), 'rb').read()
    found = {}
    for elf in _code_objects(blob):
        for k in _kernels(elf):
            m = re.search(r'\d+(surfel_cast_kernel)I([fd])E|\d+(surfel_fit_kernel|surfel_morton_kernel)E', k['.name'])
            if m:
                found[(m.group(1) or m.group(3), m.group(2))] = k
    assert sorted(found, key=str) == sorted([('surfel_cast_kernel', 'd'), ('surfel_cast_kernel', 'f'), ('surfel_fit_kernel', None),
                                             ('surfel_morton_kernel', None)], key=str)
    for key, k in sorted(found.items(), key=str):
        print('%s<%s>: vgpr %d sgpr %d scratch %d lds %d' % (key + (k['.vgpr_count'], k['.sgpr_count'], k['.private_segment_fixed_size'],
                                                                     k['.group_segment_fixed_size'])))
        assert k['.private_segment_fixed_size'] == 0
    for t in 'fd':
        assert found[('surfel_cast_kernel', t)]['.group_segment_fixed_size'] == 32768
