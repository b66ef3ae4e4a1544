"""Plane registration on the host (no GPU): the rules of csrc/dc_planereg_math.h through their host build (libdc_hostcheck.so, the
header the kernels inline) against tests/planereg_reference.py -- the valid set, h, every score and the suppression order equal, T
within planereg_reference.T_BAR -- on designed inputs; then the oracle itself end to end on the six scenes.

Figures of the end-to-end runs (the prototype's parameters, planes on the unfiltered clouds; coarse winner's largest point error):
turn140 11.5 mm, half_turn_z 54.5 mm, turn75 2.3 mm, part_low 1.7 mm, part_mid 22.0 mm, last60 2.1 mm (the 19th distinct pose walked).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_reference as A  # noqa: E402
import globalreg_reference as G  # noqa: E402
import planereg_reference as P  # noqa: E402


def host_lib():
    """libdc_hostcheck.so with the plane registration exports (rebuilt when the library at hand predates them)."""
    from helpers import hostcheck_lib
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_planereg_enumerate'):
        import __graft_entry__ as ge
        ge.build()
        lib = hostcheck_lib()
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.dc_host_planereg_enumerate.restype = i64
    lib.dc_host_planereg_enumerate.argtypes = [vp, vp, ci, vp, ci, vp, i64, i64, i64, f64, f64, f64, f64, i64, vp, vp, vp]
    lib.dc_host_planereg_score.restype = i64
    lib.dc_host_planereg_score.argtypes = [vp, vp, vp, ci, vp, ci, f64, f64]
    lib.dc_host_planereg_pair.argtypes = [vp, vp, vp, vp, vp, vp, ci, f64, f64, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_enumerate(lib, cp, cs, sp, tri, h_begin=0, h_end=None, prm=None):
    """dict(n, h, T, score) of the host build over [h_begin, h_end); n = -1: refused arguments."""
    prm = dict(P.PARAMS, **(prm or {}))
    cp, sp = np.ascontiguousarray(cp, dtype=np.float64), np.ascontiguousarray(sp, dtype=np.float64)
    cs, tri = np.ascontiguousarray(cs, dtype=np.int64), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    h_end = len(tri) * len(sp) ** 3 * 8 if h_end is None else h_end
    args = (_p(cp), _p(cs), len(cp), _p(sp), len(sp), _p(tri), len(tri), h_begin, h_end, prm['min_det'], prm['tol_dot'], prm['cos_tol'],
            prm['tol_d'])
    n = lib.dc_host_planereg_enumerate(*args, 0, None, None, None)
    if n < 0:
        return dict(n=n)
    h, T, sc = np.zeros(n, np.int64), np.zeros((n, 4, 4)), np.zeros(n, np.int64)
    assert lib.dc_host_planereg_enumerate(*args, n, _p(h), _p(T), _p(sc)) == n
    return dict(n=n, h=h, T=T, score=sc)


def assert_equal_lists(got, want, what=''):
    """The valid list, h and every score equal; T within the bar.  Returns the largest |T - T_oracle| entry."""
    assert got['h'].tolist() == want['h'].tolist(), what
    assert (np.diff(got['h']) > 0).all()
    assert got['score'].tolist() == want['score'].tolist(), what
    worst = float(np.abs(got['T'] - want['T']).max()) if len(want['h']) else 0.0
    assert worst <= P.T_BAR, (what, worst)
    return worst


CASES = {(3, 3): 1, (4, 3): 1, (3, 4): 0, (6, 6): 0, (12, 14): 1}      # (Pc, Ps) -> seed of planereg_reference.random_planes


_RANDOM = {}


def random_case(pc, ps):
    """(cp, cs, sp, T_true, oracle result) of a random case, computed once."""
    if (pc, ps) not in _RANDOM:
        cp, cs, sp, T = P.random_planes(pc, ps, CASES[(pc, ps)])
        _RANDOM[(pc, ps)] = (cp, cs, sp, T, P.hypotheses(cp, cs, sp))
    return _RANDOM[(pc, ps)]


# ---- designed inputs ----------------------------------------------------------------------------------------------------------------
def three_planes():
    """Pc = Ps = 3 with pairwise dot products 0.29, 0.39 and 0.57 (distinct by more than tol_dot) and |det| = 0.75."""
    m = np.array([[1.0, 0.0, 0.0], [0.3, 1.0, 0.0], [0.5, 0.6, 1.0]])
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    sp = np.concatenate([m, [[-1.0], [2.0], [0.5]]], axis=1)
    R, t = A.axis_angle((0.2, -0.5, 0.8), 1.9), np.array([2.0, -1.0, 0.5])
    sg = np.array([1.0, -1.0, -1.0])
    cp = np.concatenate([sg[:, None] * (m @ R), (sg * (sp[:, 3] + m @ t))[:, None]], axis=1)
    return np.ascontiguousarray(cp), np.array([100, 200, 300], dtype=np.int64), sp, A.rigid(R, t)


def test_three_planes_have_one_valid_hypothesis(lib):
    cp, cs, sp, T = three_planes()
    want = P.hypotheses(cp, cs, sp)
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    assert want['tri'].tolist() == [[0, 1, 2]] and want['n_enumerated'] == 27 * 8
    assert got['n'] == 1 and len(want['h']) == 1
    assert_equal_lists(got, want)
    u, i, j, k, s = P.decode(got['h'], 3)
    assert (u[0], i[0], j[0], k[0], s[0]) == (0, 0, 1, 2, 0b110)      # sigma_b = sigma_c = -1
    assert np.abs(got['T'][0] - T).max() < 1e-12 and got['score'][0] == 600
    # the score of one transform: moved 0.2 m along the first survey normal, only that plane stops agreeing (its offset is 0.2 off)
    T2 = T.copy()
    T2[:3, 3] += 0.2 * sp[0, :3]
    T2 = np.ascontiguousarray(T2)
    sc = lib.dc_host_planereg_score(_p(T2), _p(cp), _p(cs), 3, _p(sp), 3, P.COS_TOL, P.OFFSET_TOL)
    assert sc == P.score(T2[None], cp, cs, sp)[0][0]
    assert sc < 600


def test_box_rule4_halves_the_sign_patterns(lib):
    """Pc = Ps = 6, the faces of a box on both sides: every dot product is 0 or +-1, so rule 3 passes all eight sign patterns of every
    pairing that passes rules 1 and 2, and rule 4 keeps exactly the four proper ones."""
    cp, cs, sp = P.box_planes()
    want = P.hypotheses(cp, cs, sp)
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    assert len(want['tri']) == 8                    # one face of every axis
    assert_equal_lists(got, want)
    u, i, j, k, s = P.decode(got['h'], 6)
    groups, counts = np.unique(np.stack([u, i, j, k], axis=1), axis=0, return_counts=True)
    assert len(groups) == 8 * 48 and (counts == 4).all() and got['n'] == 8 * 48 * 4
    assert want['margins']['rule4'] == 1.0
    # the identity is among them with every plane agreeing
    ident = np.flatnonzero(np.abs(got['T'] - np.eye(4)).max(axis=(1, 2)) < 1e-12)
    assert len(ident) == 8 and (got['score'][ident] == cs.sum()).all()


def test_equal_survey_normals_are_rejected_by_rule2(lib):
    cp, cs, sp, _ = P.random_planes(4, 4, 1)
    sp[1, :3] = sp[0, :3]
    want = P.hypotheses(cp, cs, sp)
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    assert_equal_lists(got, want)
    _, i, j, k, _ = P.decode(got['h'], 4)
    used = np.stack([i, j, k], axis=1)
    assert not (((used == 0).any(axis=1)) & ((used == 1).any(axis=1))).any()
    sp3 = np.ascontiguousarray(sp[[0, 1, 2]])       # with three survey planes, two of them parallel: nothing is valid
    want3 = P.hypotheses(cp, cs, sp3)
    assert host_enumerate(lib, cp, cs, sp3, want3['tri'])['n'] == 0 and len(want3['h']) == 0


def test_nan_planes(lib):
    cp, cs, sp, _ = P.random_planes(8, 8, 3)
    cp[1], sp[2, 3] = np.nan, np.nan           # a NaN cloud plane; a survey plane whose normal passes rules 1 to 4 and whose fit is not finite
    want = P.hypotheses(cp, cs, sp)
    assert not (want['tri'] == 1).any() and len(want['tri']) > 0
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    assert_equal_lists(got, want)
    _, i, j, k, _ = P.decode(got['h'], 8)
    assert got['n'] > 0 and not ((i == 2) | (j == 2) | (k == 2)).any() and np.isfinite(got['T']).all()
    # a table that names the NaN plane all the same: the rules reject it
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    assert host_enumerate(lib, cp, cs, sp, tri)['n'] == 0


@pytest.mark.parametrize('pc,ps', sorted(CASES))
def test_host_equals_oracle_on_random_planes(lib, pc, ps):
    cp, cs, sp, T, want = random_case(pc, ps)
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    worst = assert_equal_lists(got, want)
    print('(%d, %d): %d triples, %d of %d valid, routes differ by %.3g, host against oracle %.3g, margins %s'
          % (pc, ps, len(want['tri']), got['n'], want['n_enumerated'], want['routes'], worst, want['margins']))
    assert got['n'] >= 1
    best = int(np.argmax(got['score']))
    assert np.abs(got['T'][best] - T).max() < 0.05  # the true pose (normals carry 1e-3 of noise) has the top score
    # sub-ranges add up: any split of the enumeration gives the same list
    cut = want['n_enumerated'] // 3 + 5
    a, b = host_enumerate(lib, cp, cs, sp, want['tri'], 0, cut), host_enumerate(lib, cp, cs, sp, want['tri'], cut, None)
    assert np.concatenate([a['h'], b['h']]).tolist() == got['h'].tolist()


def big_case(pc, ps, seed=0):
    """A case whose hypothesis numbers pass 2^32: min_det = 0.05 keeps most of the C(pc, 3) triples; the range is the whole of the
    triple u whose numbers straddle (or first pass) 2^32.  Returns (cp, cs, sp, tri, h_begin, h_end, prm)."""
    cp, cs, sp, _ = P.random_planes(pc, ps, seed)
    prm = dict(min_det=0.05)
    tri, _ = P.triples(cp, 0.05)
    per_u = ps ** 3 * 8
    u = (1 << 32) // per_u
    assert u + 1 < len(tri)
    return cp, cs, sp, tri, u * per_u, (u + 1) * per_u, prm


def test_hypothesis_numbers_past_32_bits(lib):
    cp, cs, sp, tri, h0, h1, prm = big_case(40, 64)
    assert h1 > 1 << 32
    want = P.hypotheses(cp, cs, sp, min_det=0.05, h_begin=h0, h_end=h1, tri=tri)
    got = host_enumerate(lib, cp, cs, sp, tri, h0, h1, prm)
    assert_equal_lists(got, want)
    print('%d valid of %d in [%d, %d), routes differ by %.3g' % (got['n'], h1 - h0, h0, h1, want['routes']))
    assert got['n'] >= 1 and got['h'].min() >= h0 and got['h'].max() >= 1 << 32


def test_refused_arguments(lib):
    cp, cs, sp, _ = three_planes()
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    assert host_enumerate(lib, cp, cs, sp, tri)['n'] == 1
    assert host_enumerate(lib, cp[:2], cs[:2], sp, tri)['n'] == -1
    assert host_enumerate(lib, cp, cs, sp[:2], tri)['n'] == -1
    assert host_enumerate(lib, cp, cs, sp, tri, 0, 27 * 8 + 1)['n'] == -1
    assert host_enumerate(lib, cp, cs, sp, tri, 5, 4)['n'] == -1
    many = np.zeros((41665, 3), dtype=np.int32)     # one triple more than C(64, 3)
    assert host_enumerate(lib, cp, cs, sp, many, 0, 8)['n'] == -1 and host_enumerate(lib, cp, cs, sp, many[:41664], 0, 8)['n'] == 0
    for key in ('min_det', 'tol_dot', 'cos_tol', 'tol_d'):
        assert host_enumerate(lib, cp, cs, sp, tri, prm={key: float('nan')})['n'] == -1
        assert host_enumerate(lib, cp, cs, sp, tri, prm={key: float('inf')})['n'] == -1


# ---- suppression --------------------------------------------------------------------------------------------------------------------
def test_suppression_order_on_host_lists(lib):
    """The oracle's walk over the host build's list equals its walk over its own (the lists are equal and the margins hold), and on a
    designed list with exact duplicates and score ties the kept rows are the stated ones."""
    cp, cs, sp, T, want = random_case(12, 14)
    got = host_enumerate(lib, cp, cs, sp, want['tri'])
    centre = np.array([0.3, -0.2, 0.1])
    a, ties_a, _ = P.select(want['h'], want['score'], want['T'], centre, 64)
    b, ties_b, _ = P.select(got['h'], got['score'], got['T'], centre, 64)
    assert a.tolist() == b.tolist() and ties_a == ties_b
    h, sc, Ts = designed_list()
    rows, ties, _ = P.select(h, sc, Ts, np.zeros(3), 8)
    assert rows.tolist() == [1, 4, 0, 6] and ties == 1


def designed_list():
    """(h, score, T) of seven hypotheses: rows 1 and 2 are the same pose with the same score (the lower h is kept, the other dropped),
    row 3 is that pose again with a lower score (dropped), row 4 ties with row 1 in score at another pose, row 0 has a lower score at a
    third pose, row 5 is row 0's rotation 0.1 m away (dropped), row 6 is row 0's rotation 1 m away (kept: only one of the two holds)."""
    Ra, Rb, Rc = A.axis_angle((0, 0, 1), 0.3), A.axis_angle((0, 1, 0), 1.2), A.axis_angle((1, 0, 0), 2.0)
    poses = [A.rigid(Rc, (0, 0, 0)), A.rigid(Ra, (1, 0, 0)), A.rigid(Ra, (1, 0, 0)), A.rigid(Ra, (1, 0, 0)), A.rigid(Rb, (0, 2, 0)),
             A.rigid(Rc, (0.1, 0, 0)), A.rigid(Rc, (1.0, 0, 0))]
    return np.array([3, 10, 11, 40, 50, 60, 70], dtype=np.int64), np.array([5, 9, 9, 7, 9, 4, 3], dtype=np.int64), np.array(poses)


# ---- the oracle end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', P.SCENES)
def test_oracle_end_to_end(name):
    """The coarse stage of the oracle on its own planes with the prototype's parameters: every margin holds (asserted inside), the
    plane fits make no decision within 1e-9 of the threshold, the winner lies within MAX_DIST / 2 = 0.25 m of the truth and has the
    top fitness alone."""
    c = P.coarse(name)
    cp, _ = P.cloud_planes(name)
    print('%s: %d / %d planes, %d triples, %d of %d valid; winner h %d score %d fitness %d of %d (runner-up %d), error %.4f m; routes '
          'differ by %.3g; score ties %d; margins %s' % (name, len(cp), len(P.survey_planes()[0]), c['n_triples'], c['n_valid'],
                                                         c['n_enumerated'], c['hypothesis'], c['score'], c['fitness'], c['n_points'],
                                                         c['runner_up'], c['error'], c['hyp']['routes'], c['ties'], c['margins']))
    assert c['status'] == 'ok' and c['error'] <= A.MAX_DIST / 2
    assert c['fitness_ties'] == 0 and c['runner_up'] < c['fitness']
    assert c['hyp']['routes'] <= P.T_BAR / 16
    if name != 'last60':                            # on the full and the half clouds the true pose has the top plane score as well
        assert c['score'] == c['hyp']['score'].max()


def test_sixteen_candidates_miss_the_partial_cloud():
    """The reason for n_candidates = 64: on 'last60' many distinct wrong poses score as high as the true one or higher (the infinite
    planes of a box room agree under many wrong poses) and the true one is the 19th walked, so 16 candidates select a wrong pose."""
    full, few = P.coarse('last60'), P.coarse('last60', 16)
    at = int(np.flatnonzero(full['candidates'][:, 0] == full['hypothesis'])[0])
    top = int((full['candidates'][:, 1] >= full['score']).sum())
    print('the winner is candidate %d; %d distinct poses score at least as high; with 16: fitness %d of %d, error %.3f m'
          % (at, top, few['fitness'], few['n_points'], few['error']))
    assert at >= 16 and top > 16
    assert few['error'] > 1.0 and few['fitness'] < full['fitness']
    assert full['error'] <= A.MAX_DIST / 2
