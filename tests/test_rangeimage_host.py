"""The range-image arithmetic of the kernels (csrc/dc_rangeimage_math.h) compiled for the host (libdc_hostcheck.so) against the
numpy restatement tests/rangeimage_reference.py: the pixel rule on designed and random points, the window slots at the seam and
the rim, membership at the gate and the nearest-point-wins rule with exact ties.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import rangeimage_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')


@pytest.fixture(scope='module')
def host():
    if not os.path.exists(LIB) or not hasattr(ctypes.CDLL(LIB), 'dc_host_range_pixel'):
        import __graft_entry__ as ge
        ge.build()
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_pixels(host, pts, rows, cols, up, down, clamp=True, min_depth=0.0):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    pix, depth = np.zeros(len(pts), dtype=np.int32), np.zeros(len(pts))
    host.dc_host_range_pixel(_p(pts), ctypes.c_int64(len(pts)), rows, cols, ctypes.c_double(up), ctypes.c_double(down), int(clamp),
                             ctypes.c_double(min_depth), _p(pix), _p(depth))
    return pix, depth


def host_window(host, rows, cols, wrap, r, c, ah, aw):
    slots = np.full((2 * ah + 1) * (2 * aw + 1) if ah >= 0 and aw >= 0 else 1, -7, dtype=np.int32)
    rc = host.dc_host_image_window(rows, cols, int(wrap), r, c, ah, aw, _p(slots))
    return rc, slots


def test_pixel_rule_designed_points(host):
    """Points whose pixel exact arithmetic decides, on a 16 x 64 grid with fov +-45 degrees."""
    H, W = 16, 64
    pts = np.array([[1, 0, 0], [-1, 0.0, 0], [-1, -0.0, 0], [0, 1, 0], [0, -1, 0], [2, 2, 0], [3, 0, 3]], dtype=np.float64)
    want_col = [32, 0, 63, 16, 48, 24, 32]
    want_row = [8, 8, 8, 8, 8, 8, 0]
    for pix in (host_pixels(host, pts, H, W, 45.0, -45.0)[0], ref.pixel_rule(pts, H, W, 45.0, -45.0)[0]):
        assert list(pix % W) == want_col
        assert list(pix // W) == want_row
    px, py, _ = ref.pixel_coords(pts, H, W, 45.0, -45.0)
    assert px[2] == 64.0                                   # (-1, -0, 0): yaw = +pi lands on column W, clamped to W - 1
    assert 1e-8 < py[6] < 1e-7                             # (3, 0, 3): the 1e-8 of the denominator keeps it inside row 0 (2.4e-8)
    # rejected rows: NaN, infinities, zero depth; a depth bound; beyond the field of view without the clamp
    bad = np.array([[np.nan, 0, 1], [1, np.inf, 0], [-np.inf, 0, 0], [0, 0, 0]])
    for fn in (lambda *a, **k: host_pixels(host, *a, **k)[0], lambda *a, **k: ref.pixel_rule(*a, **k)[0]):
        assert list(fn(bad, H, W, 45.0, -45.0)) == [-1, -1, -1, -1]
        assert list(fn(np.array([[1.0, 0, 0], [2.0, 0, 0], [2.0000001, 0, 0]]), H, W, 45.0, -45.0, min_depth=2.0)) == [-1, -1, 8 * W + 32]
        steep = np.array([[1.0, 0, 3.0], [1.0, 0, -3.0], [1.0, 0, 0.5]])
        assert list(fn(steep, H, W, 45.0, -45.0, clamp=True)) == [32, 15 * W + 32, 3 * W + 32]
        assert list(fn(steep, H, W, 45.0, -45.0, clamp=False)) == [-1, -1, 3 * W + 32]


def test_pixel_rule_random_points(host):
    """200 k random points at 128 x 1024: equal pixels outside a band of 1e-9 pixel around integer pixel coordinates; the band may
    leave out at most 0.1 % of the points (with this seed: none)."""
    rng = np.random.default_rng(20240607)
    n = 200000
    pts = rng.normal(size=(n, 3)) * np.array([8.0, 8.0, 2.5]) * rng.uniform(0.05, 3.0, size=(n, 1))
    H, W, up, down = 128, 1024, 45.0, -45.0
    want, want_depth = ref.pixel_rule(pts, H, W, up, down)
    got, depth = host_pixels(host, pts, H, W, up, down)
    near = ref.near_pixel_edge(pts, H, W, up, down)
    print('points in the 1e-9 band: %d of %d' % (near.sum(), n))
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], want[~near])
    assert np.array_equal(depth, want_depth)                       # |p| bit for bit: the winner rule compares these
    assert (want >= 0).all() and len(np.unique(want)) > 0.25 * H * W
    got0 = host_pixels(host, pts, H, W, up, down, clamp=False)[0]
    want0 = ref.pixel_rule(pts, H, W, up, down, clamp=False)[0]
    assert np.array_equal(got0[~near], want0[~near]) and (want0 < 0).sum() > 1000


@pytest.mark.parametrize('wrap', [True, False])
def test_window_slots(host, wrap):
    H, W = 6, 9
    cases = [(r, c, ah, aw) for r in (0, 2, H - 1) for c in (0, 1, W - 1) for ah, aw in ((1, 1), (2, 2), (0, 3), (1, 4), (2, 0))]
    for r, c, ah, aw in cases:
        rc, slots = host_window(host, H, W, wrap, r, c, ah, aw)
        want = ref.window_slots(H, W, wrap, r, c, ah, aw)
        assert rc == len(want) and np.array_equal(slots, want), (r, c, ah, aw)
        inside = want[want >= 0]
        assert len(np.unique(inside)) == len(inside)               # no pixel twice
        assert want[ah * (2 * aw + 1) + aw] == r * W + c           # the centre slot
    # 2 aw + 1 == W exactly: with wrap every column of the row appears once, whatever the centre
    for c in (0, 4, W - 1):
        rc, slots = host_window(host, H, W, wrap, 3, c, 0, 4)
        assert rc == W
        if wrap:
            assert sorted(slots) == list(range(3 * W, 4 * W))
        else:
            assert sorted(slots[slots >= 0]) == list(range(3 * W + max(c - 4, 0), 3 * W + min(c + 4, W - 1) + 1))
    # windows the grid does not admit
    for ah, aw in ((0, 5), (3, 0), (5, 5), (-1, 0), (0, -1)):
        assert not ref.window_ok(H, W, ah, aw)
        assert host_window(host, H, W, wrap, 1, 1, ah, aw)[0] == -1
    assert not ref.window_ok(64, 64, 5, 6) and host_window(host, 64, 64, wrap, 9, 9, 5, 6)[0] == -1      # 11 x 13 = 143 slots
    assert ref.window_ok(64, 64, 5, 5) and host_window(host, 64, 64, wrap, 9, 9, 5, 5)[0] == 121


def test_membership_at_the_gate(host):
    xi = np.array([2.0, 0.0, 0.0])
    on = np.array([2.5, 0.0, 0.0])                                 # exactly r = 0.5 away: <= includes it
    off = np.array([np.nextafter(2.5, 3.0), 0.0, 0.0])             # one ulp farther
    def m(occ, cen, xj, r):
        got = host.dc_host_image_member(int(occ), int(cen), _p(xi), _p(xj), ctypes.c_double(r))
        assert bool(got) == ref.member(occ, cen, xi, xj, r)
        return bool(got)
    assert m(True, False, on, 0.5) and not m(True, False, off, 0.5)
    assert m(True, True, off, 0.5)                                 # the centre always
    assert not m(False, False, on, 0.5) and not m(False, True, on, 0.5)
    for r in (0.0, -1.0, float('inf')):                            # no gate
        assert m(True, False, off, r)


def test_winner_rule(host):
    """Several points per pixel, exact fp64 depth ties (the lower index wins), rejected rows in between."""
    H, W, up, down = 4, 8, 45.0, -45.0
    rng = np.random.default_rng(3)
    base = rng.normal(size=(400, 3)) * np.array([4.0, 4.0, 1.0])
    scale = rng.choice([1.0, 2.0, 4.0], size=(400, 1))             # powers of two: the direction's pixel is unchanged, depths tie exactly
    pts = np.concatenate([base * scale, base, base * scale, [[np.nan, 1, 1], [0, 0, 0]], base, base * 2.0])
    pts = pts[rng.permutation(len(pts))]
    pix, depth = ref.pixel_rule(pts, H, W, up, down)
    want_idx, want_rng = ref.winners(pix, depth, H * W)
    got_pix = np.zeros(len(pts), dtype=np.int32)
    got_idx, got_rng = np.zeros(H * W, dtype=np.int32), np.zeros(H * W)
    rc = host.dc_host_range_project(_p(np.ascontiguousarray(pts)), ctypes.c_int64(len(pts)), H, W, ctypes.c_double(up), ctypes.c_double(down),
                                    1, ctypes.c_double(0.0), _p(got_pix), _p(got_idx), _p(got_rng))
    assert rc == 0
    near = ref.near_pixel_edge(pts, H, W, up, down)
    assert not near[pix >= 0].any()
    assert np.array_equal(got_pix, pix) and np.array_equal(got_idx, want_idx) and np.array_equal(got_rng, want_rng)
    # the ties are there: pixels whose minimum depth is held by more than one point
    ties = sum(1 for p in range(H * W) if want_idx[p] >= 0 and (depth[pix == p] == want_rng[p]).sum() > 1)
    assert ties >= H * W // 2
    # an empty cloud and an empty pixel
    rc = host.dc_host_range_project(_p(np.zeros((1, 3))), ctypes.c_int64(0), H, W, ctypes.c_double(up), ctypes.c_double(down), 1,
                                    ctypes.c_double(0.0), _p(got_pix), _p(got_idx), _p(got_rng))
    assert rc == 0 and (got_idx == -1).all() and (got_rng == -1.0).all()
