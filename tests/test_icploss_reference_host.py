"""The reference of the ICP-loss tests (icploss_reference.py) pinned on the host before it pins a kernel: against float64 torch
autograd of the oracle's point-to-plane / point-to-point formulas (with the float32 cast of the world points), against autograd
through xyz_axis_angle_to_matrix, and against torch.optim.Adam over four steps.  The distance of those float64 yardsticks from the
mpmath reference is printed in units of the bounds the GPU tests use (c 2^-52 magnitude, icploss_reference's c's): it is what a plain
float64 evaluation of the same formulas needs of them.  Then: the conventions at the singular points, the planted mistakes the designed
cases must notice, and the redraw cap of every case.  No GPU."""
import numpy as np
import pytest
import torch

import dc_oracle as O
import icploss_cases as C
import icploss_reference as R

U = R.U
F64 = torch.float64


_ratio = C.ratio
check_finish = C.check_finish


# ---- float64 torch restatement of one pair ----------------------------------------------------------------------------------------
def _torch_world(scan, model_parts, pose):
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=F64)
    n = len(scan['depth'])
    lm = torch.ones(n, dtype=torch.bool) if scan['lmask'] is None else torch.tensor(scan['lmask'])
    vps = tt(scan['vps']) if scan['vps'] is not None else torch.zeros(n, 3, dtype=F64)
    xl = vps + model_parts(tt(scan['depth']), tt(scan['inc']), lm)[:, None] * tt(scan['dirs'])
    T = pose.reshape(3, 4)
    x = xl @ T[:, :3].T + T[:, 3]
    x = x + (x.float().double() - x).detach()            # loss.py:436-437; the cast passes the gradient through
    return x, tt(scan['normals']) @ T[:, :3].T


def torch_pair(case, plane, idx_a, idx_b):
    """The pair layout {sum12, sum21, dw, de, dTa, dTb} by float64 autograd of the oracle's formulas"""
    A, B = case['scans']
    model = case['model']
    held = {}
    if model is not None:
        held = {f: torch.tensor(v, dtype=F64, requires_grad=True) for f, v in (('w', model[1]), ('e', model[2]))}

    def parts(d, inc, lm):
        if model is None:
            return d
        kind, w, e = model[0], held['w'], held['e']
        if kind == 'Linear':
            dc = w[0] * d + w[1] * inc + w[2]
        elif kind == 'InvCos':
            dc = d - w[0] / torch.cos(inc)
        elif kind == 'ScaledInvCos':
            dc = d * (1 - w[0] / torch.cos(inc).abs())
        else:
            b = (w[None, :] * inc[:, None] ** e[None, :]).sum(1)
            dc = d * (1 - b) if kind == 'ScaledPolynomial' else d - b
        return torch.where(lm, dc, d)
    pa = torch.tensor(case['poses'][0], dtype=F64, requires_grad=True)
    pb = torch.tensor(case['poses'][1], dtype=F64, requires_grad=True)
    xa, na = _torch_world(A, parts, pa)
    xb, nb = _torch_world(B, parts, pb)
    ia, ib = torch.tensor(idx_a, dtype=torch.int64), torch.tensor(idx_b, dtype=torch.int64)
    p1, p2, n1, n2 = xa[ia], xb[ib], na[ia], nb[ib]
    if plane:                                              # dc_oracle.point_to_plane, sums instead of means
        k = (n1 * (p2 - p1)).sum(-1, keepdim=True)
        s12 = torch.linalg.norm(k * n1, dim=-1).sum()
        k = (n2 * (p1 - p2)).sum(-1, keepdim=True)
        s21 = torch.linalg.norm(k * n2, dim=-1).sum()
    else:                                                  # dc_oracle.point_to_point
        s12, s21 = torch.linalg.norm(p2 - p1, dim=1).sum(), torch.zeros((), dtype=F64)
    (s12 + s21).backward()
    g = lambda v: np.zeros(0) if v is None else (np.zeros(v.shape) if v.grad is None else v.grad.numpy()).reshape(-1)
    out = np.concatenate([[s12.item(), s21.item()], g(held.get('w')), g(held.get('e')), g(pa), g(pb)])
    return out, (xa.detach(), xb.detach(), na.detach(), nb.detach())


def _generic_only(case):
    a, b, ia, ib, _ = case['pairs'][0]
    keep = (ia >= C.DESIGNED) & (ib >= C.DESIGNED)
    return ia[keep], ib[keep]


# (not the 65537-correspondence case: autograd's gather backward adds the ~2000 repeats of a point one after the other, which is
# torch's summation order and no yardstick for a tree of block sums)
KIND_CASES = sorted(k for k in C.PAIR_SPECS if k.startswith('kind-')) + ['m513', 'same_index']


@pytest.mark.parametrize('plane', [True, False], ids=['plane', 'point'])
def test_terms_and_gradients_match_float64_autograd(plane):
    """Every output of the pair layout, away from the designed singular correspondences (torch's pow gives NaN for d 0^e / de),
    against float64 autograd; the yardstick's distance from the reference in units of the GPU bound is printed per case."""
    worst = {}
    for name in KIND_CASES:
        case = C.settle(C.pair_case(name))
        ia, ib = _generic_only(case)
        val, mag, ties = R.pair(case['scans'][0], case['scans'][1], case['poses'][0], case['poses'][1], case['model'], ia, ib, plane)
        assert not ties
        got, (xa, xb, na, nb) = torch_pair(case, plane, ia, ib)
        c = R.c_sums(-(-len(ia) // R.BLOCK))
        worst[name] = _ratio(got - val, c * U * mag)
        assert worst[name] <= 1.0, (name, worst[name])
        if plane and case['dtype'] == np.float64 and len(ia) < 1000:           # the oracle itself, to the accuracy of its float32 differences
            ref = O.point_to_plane([xa, xb], [na, nb], [(torch.tensor(ia, dtype=torch.int64), torch.tensor(ib, dtype=torch.int64))])
            assert abs(float(ref) - 0.5 * (val[0] + val[1]) / len(ia)) <= 1e-5 * float(ref)
        if not plane:
            assert val[1] == 0.0
    print('float64 autograd against the reference, in units of the bound (%s): max %.3g' % ('plane' if plane else 'point', max(worst.values())), worst)


def test_conventions_at_the_singular_points():
    zeros = lambda v: np.all(v == 0.0)
    ref = lambda name, plane: C.reference(C.settle(C.pair_case(name)), plane)
    v, m = ref('single0', True)                  # identical world points: no term, no gradient (sign(0) = 0), nothing to round
    assert zeros(v) and zeros(m[:2])
    v, m = ref('single0', False)                 # |x2 - x1| = 0: the norm's subgradient at zero is zero
    assert zeros(v)
    v, m = ref('single1', True)                  # on A's plane: the 1 -> 2 term and its gradients vanish, the 2 -> 1 term does not
    assert v[0] == 0.0 and v[1] > 0.0
    v, m = ref('single2', True)                  # |n1| = 0
    assert v[0] == 0.0 and v[1] > 0.0 and np.all(np.isfinite(v))
    v, m = ref('single3', True)                  # both normals zero
    assert zeros(v)
    assert ref('single3', False)[0][0] > 0.0
    # inc = 0: pow_term(0, 0) = 1, pow_term(0, 8) = 0 = pow(0, 2.5), and no exponent gradient from that point
    case = C.pair_case('single4')
    mdl = R.as_model(case['model'])
    p = R.scan_point(case['scans'][0], 4, mdl, case['poses'][0])
    assert [float(R.pow_term(p.inc, e).v) for e in mdl[2]] == [1.0, 0.0, 0.0]
    one = [R.V(R.mpf(1))] * 3
    gw, ge, gT = R.scan_point_bwd(mdl, case['poses'][0], p, one, one)
    assert all(x.v == 0 for x in ge) and gw[0].v != 0 and gw[1].v == 0
    # outside the mask: the depth is kept, no model gradient, the pose gradient stays
    case = C.pair_case('single5')
    mdl = R.as_model(case['model'])
    p = R.scan_point(case['scans'][0], 5, mdl, case['poses'][0])
    s = case['scans'][0]
    assert all(float(p.xl[a].v) == float(R.mpf(float(s['vps'][5][a])) + R.mpf(float(s['depth'][5])) * R.mpf(float(s['dirs'][5][a]))) for a in range(3))
    gw, ge, gT = R.scan_point_bwd(mdl, case['poses'][0], p, one, one)
    assert all(x.v == 0 for x in gw + ge) and all(x.v != 0 for x in gT)
    # the cast: exactly a float32 number, and the nearest one
    x, _ = R.scan_world(case['scans'][0], case['model'], case['poses'][0])
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))


# ---- the pose chain ---------------------------------------------------------------------------------------------------------------
CHAIN_HOST = ['per-pose-2', 'per-pose-255', 'shared-generic-257', 'shared-at0-257'] + sorted(k for k in C.CHAIN_SPECS if k.endswith('-2') and k != 'per-pose-2')


def torch_chain(case):
    from depth_correction_amd.transform import xyz_axis_angle_to_matrix
    n = len(case['T0'])
    d = torch.tensor(case['deltas'], dtype=F64, requires_grad=True)
    T = torch.matmul(torch.tensor(case['T0'], dtype=F64).reshape(n, 4, 4), xyz_axis_angle_to_matrix(d))
    (T * torch.tensor(case['grad'], dtype=F64).reshape(n, 4, 4)).sum().backward()
    return T.detach().numpy().reshape(n, 16), d.grad.numpy()


def test_pose_chain_matches_autograd():
    worst = {}
    for name in CHAIN_HOST:
        case, ref = C.chain_case(name), C.chain_reference(name)
        T, g = torch_chain(case)
        n = len(case['T0'])
        c_bwd = R.C_CHAIN_BWD + (8 + -(-n // 256) if len(case['deltas']) == 1 else 0)
        worst[name] = (_ratio(T - ref['fwd'][0], R.C_CHAIN_FWD * U * ref['fwd'][1]), _ratio(g - ref['bwd'][0], c_bwd * U * ref['bwd'][1]))
        assert max(worst[name]) <= 1.0, (name, worst[name])
        cond = float(np.max(ref['bwd'][1] / np.maximum(np.abs(ref['bwd'][0]), 1e-300)))
        print('%-22s forward %.3g backward %.3g of the bound; largest magnitude / |value| of the backward %.3g' % ((name,) + worst[name] + (cond,)))


def test_small_angle_switch_is_below_float64_at_the_threshold():
    """Which branch the switch takes at theta = 1e-6 exactly cannot be seen in float64: the two expressions of sin(theta / 2) / theta
    differ by theta^4 / 3840 = 2.6e-28 there and their derivatives by 1e-19 relative, far inside one rounding.  The planted mistake
    (the series taken AT the threshold) therefore moves no output by a thousandth of its bound; the cases at, below and above the
    threshold pin the values on both sides instead."""
    for name in ('shared-at0-2', 'shared-at0-257', 'per-pose-255'):
        case, ref = C.chain_case(name), C.chain_reference(name)
        fwd = R.corrected_poses(case['T0'], case['deltas'], flaws=('small_at_switch',))
        bwd = R.corrected_poses_bwd(case['T0'], case['deltas'], case['grad'], flaws=('small_at_switch',))
        moved = max(_ratio(fwd[0] - ref['fwd'][0], R.C_CHAIN_FWD * U * ref['fwd'][1]), _ratio(bwd[0] - ref['bwd'][0], R.C_CHAIN_BWD * U * ref['bwd'][1]))
        print('%s: the series taken at the threshold moves the outputs by %.3g of their bound' % (name, moved))
        assert moved < 1e-3


# ---- the finishing step -----------------------------------------------------------------------------------------------------------
FINISH_HOST = ['S1-ring1x4', 'S2-ring3x4', 'S2-shared-x4']


def torch_finish_steps(case):
    """The case's steps with torch autograd and torch.optim.Adam; yields per step (state before, state after, T_next)"""
    from depth_correction_amd.transform import xyz_axis_angle_to_matrix
    sp = case['spec']
    S, P = sp['S'], sp['P']
    head = 2 if sp['layout'] == 0 else 1
    T0 = torch.tensor(case['T0'], dtype=F64).reshape(S, 4, 4)
    delta = torch.tensor(case['delta'], dtype=F64, requires_grad=True)
    groups = [dict(params=[delta], lr=C.ADAM['lr_d'])]
    w = None
    if case['w'] is not None:
        w = torch.tensor(case['w'], dtype=F64, requires_grad=True)
        groups.append(dict(params=[w], lr=sp['lr_w']))
    opt = torch.optim.Adam(groups, betas=(C.ADAM['b1'], C.ADAM['b2']), eps=C.ADAM['eps'], foreach=False)
    for p, m, v in ((delta, 'd_m', 'd_v'), (w, 'w_m', 'w_v')):
        if p is not None:
            opt.state[p] = dict(step=torch.tensor(float(case['step0'])), exp_avg=torch.tensor(case[m], dtype=F64).clone(),
                                exp_avg_sq=torch.tensor(case[v], dtype=F64).clone())
    for k in range(sp['steps']):
        get = lambda p, f: None if p is None else opt.state[p][f].detach().numpy().copy()
        before = dict(w=None if w is None else w.detach().numpy().copy(), w_m=get(w, 'exp_avg'), w_v=get(w, 'exp_avg_sq'),
                      delta=delta.detach().numpy().copy(), d_m=get(delta, 'exp_avg'), d_v=get(delta, 'exp_avg_sq'), step=case['step0'] + k)
        sums = torch.tensor(case['sums'][k], dtype=F64)
        if case['totals'] is not None:
            div, gw = float(case['totals'][k][1]), torch.tensor(case['totals'][k][2:], dtype=F64)
        else:
            div, gw = (float(sums[1]) if sp['layout'] == 0 else 1.0), sums[head:head + P]
        opt.zero_grad()
        T = torch.matmul(T0, xyz_axis_angle_to_matrix(delta if not sp['shared'] else delta.expand(S, 6)))
        loss = (T[:, :3, :] * sums[head + 2 * P:].reshape(S, 3, 4)).sum() / div
        if w is not None:
            loss = loss + (w * gw).sum() / div
        loss.backward()
        if sp['zero_first']:                     # train.py:316-317: the first pose stays where it is
            if sp['shared']:
                # a shared correction has no "first" row of its own: the kernel zeroes pose 0's contribution to the sum
                Tz = torch.matmul(T0[:1], xyz_axis_angle_to_matrix(delta))
                g0, = torch.autograd.grad((Tz[:, :3, :] * sums[head + 2 * P:].reshape(S, 3, 4)[:1]).sum() / div, delta)
                delta.grad -= g0
            else:
                delta.grad[0] = 0
        if w is not None and sp['lr_w'] == 0.0:
            w.grad = None
        opt.step()
        with torch.no_grad():
            Tn = torch.matmul(T0, xyz_axis_angle_to_matrix(delta if not sp['shared'] else delta.expand(S, 6)))
        after = dict(w=None if w is None else w.detach().numpy().copy(), w_m=get(w, 'exp_avg'), w_v=get(w, 'exp_avg_sq'),
                     delta=delta.detach().numpy().copy(), d_m=get(delta, 'exp_avg'), d_v=get(delta, 'exp_avg_sq'),
                     step=int(opt.state[delta]['step'].item()))
        yield k, before, after, Tn.numpy().reshape(S, 16)


@pytest.mark.parametrize('name', FINISH_HOST)
def test_finishing_step_matches_torch_adam(name):
    case = C.finish_case(name)
    worst = {}
    for k, before, after, Tn in torch_finish_steps(case):
        ref = check_finish(case, k, before, after, Tn, worst)
        n_sums = len(case['sums'][k])
        assert np.array_equal(ref['record'][:n_sums], case['sums'][k])
        assert np.array_equal(ref['record'][n_sums + case['spec']['P']:][:before['delta'].size], before['delta'].reshape(-1))
    print('torch.optim.Adam against the reference over %d steps, in units of the bound: %s' % (case['spec']['steps'], worst))


# ---- the designed cases are not harmless ------------------------------------------------------------------------------------------
def _moved_sums(case, plane, flaw, c):
    val, mag = C.reference(C.settle(case), plane)
    bad, _ = C.reference(case, plane, flaws=(flaw,))
    return _ratio(bad - val, c * U * mag)


def _moved_finish(name, flaw):
    case = C.finish_case(name)
    st = C.finish_state0(case)
    good, bad = C.finish_reference(case, 0, st), C.finish_reference(case, 0, st, flaws=(flaw,))
    r = 0.0 if np.array_equal(good['record'], bad['record']) else np.inf
    for f in ('w', 'delta', 'd_m', 'd_v', 'T_next'):
        r = max(r, _ratio(bad[f][0] - good[f][0], R.C_FINISH * U * good[f][1]))
    return r


PLANTED = {
    'no_cast': lambda: _moved_sums(C.pair_case('kind-ScaledPolynomial-float64'), True, 'no_cast', R.c_sums(2)),
    'sign0_is_1': lambda: _moved_sums(C.pair_case('single0'), True, 'sign0_is_1', R.c_sums(1)),
    'drop_norm': lambda: _moved_sums(C.pair_case('m257'), True, 'drop_norm', R.c_sums(2)),
    'ignore_lmask': lambda: _moved_sums(C.pair_case('single5'), False, 'ignore_lmask', R.c_sums(1)),
    'egrad_at_inc0': lambda: _moved_sums(C.pair_case('single4'), True, 'egrad_at_inc0', R.c_sums(1)),
    'omit_row': lambda: _moved_sums(C.pair_case('m65537'), True, 'omit_row', R.c_sums(257)),
    'wrong_slot': lambda: _moved_sums(C.seq_case('S1025-p17'), True, 'wrong_slot', R.c_sums(1, 17)),
    'bias_t': lambda: _moved_finish('S2-ring3x4', 'bias_t'),
    'ignore_zero_first': lambda: _moved_finish('S2-ring3x4', 'ignore_zero_first'),
    'record_after': lambda: _moved_finish('S2-ring3x4', 'record_after'),
}


@pytest.mark.parametrize('flaw', sorted(PLANTED))
def test_designed_cases_are_not_harmless(flaw):
    """A planted mistake in a copy of the reference moves an output of a designed case by more than that output's GPU bound (the
    eleventh of the list, the small-angle switch, is test_small_angle_switch_is_below_float64_at_the_threshold)."""
    moved = PLANTED[flaw]()
    print('%s moves an output by %.3g bounds' % (flaw, moved))
    assert moved > 1.0


# ---- the redraw cap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(C.PAIR_SPECS))
def test_redraw_cap_pair_cases(name):
    case = C.settle(C.pair_case(name))
    assert case['redrawn'] <= C.REDRAW_CAP * C.n_points(case), (name, case['redrawn'])


@pytest.mark.parametrize('name', sorted(C.SEQ_SPECS))
def test_redraw_cap_sequence_cases(name):
    case = C.settle(C.seq_case(name))
    assert case['redrawn'] <= C.REDRAW_CAP * C.n_points(case), (name, case['redrawn'])
