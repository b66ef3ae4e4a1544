"""The route the host chooser names is the kernel that runs: for small plans and the A-B options that move the route, dc_choose_route
(csrc/dc_cons_route.h through libdc_hostcheck.so) is given the plan's real descriptor and the option values, the kernel's name is put
together from the route it returns, and one dc_sequence_eval must report exactly that name (KernelTimer.kernels()) with status 0.

Plans: five of the small sequences of test_gpu_step_header.py (at most 3 * 256 + 37 points; the base cloud for the pose gradients), a
float64 plan and a ball-neighbourhood plan of the same size.  The whole file takes a few seconds."""
import ctypes

import numpy as np
import pytest
import torch

from test_route_host import FIELDS, OPTIONS, STEP_RAGGED, STEP_Q32, STEP_BASIS, STEP_SLOTS, TWO_PASS, POSE, GENERAL
from test_route_host import route_lib

pytestmark = pytest.mark.gpu

PLANS = ('k4', 'pos10', 'wide10', 'nomask', 'n100', 'f64', 'ball', 'pose')
N_TERMS = dict(k4=2, pos10=2, wide10=3, nomask=2, n100=1, f64=2, ball=2, pose=2)
# dc_set_option (option, value) -> the RouteOptions field it sets
SETTINGS = {None: {}, (6, 7): dict(step_var=7), (6, 0): dict(step_var=0), (9, 1): dict(step_six=1), (4, 1): dict(two_pass=1),
            (7, 1): dict(pose_three_pass=1)}
CASES = [(name, setting) for name in PLANS for setting in (None, (6, 7), (6, 0), (9, 1), (4, 1))] + [('pose', (7, 1))]
_extra = {}


@pytest.fixture(scope='module')
def hostlib():
    return route_lib()


def _plan(dev, name):
    from test_gpu_step_header import _sequences
    seqs = _sequences(dev)
    if name in seqs:
        return seqs[name][:2]
    if name == 'pose':
        return seqs['base10'][:2]
    if not _extra:
        from depth_correction_amd.dataset import RoomBoxDataset
        from depth_correction_amd.pipeline import build_sequence
        ds = RoomBoxDataset(n_pts=600, n_poses=5, seed_base=1000, dtype=np.float32)
        scans = [np.stack([c[f] for f in 'xyz'], axis=1)[:161] for c, _ in ds]
        poses = np.stack([p for _, p in ds])
        plan, info = build_sequence([s.astype(np.float64) for s in scans], poses, k=10, dtype=torch.float64, device=dev)
        _extra['f64'] = (plan, info['poses'])
        plan, info = build_sequence(scans, poses, k=None, r=0.5, dtype=torch.float32, device=dev)
        _extra['ball'] = (plan, info['poses'])
    return _extra[name]


def _kernel_name(r):
    """The source-level name of the forward (or one-pass) kernel of a route, as the launch code spells it."""
    pt = 'double' if r['f64'] else 'q32'
    kind, k, p = r['kind'], r['k'], r['P']
    if kind == STEP_RAGGED:
        return 'consistency_step_ragged_q32_kernel<%d, %d>' % (p, r['cap'])
    if kind == STEP_Q32:
        return 'consistency_step_q32_kernel<%d, %d, %d%s>' % (k, p, r['cap'], ', 6' if r['six'] else '')
    if kind == STEP_BASIS:
        return 'consistency_step_basis_kernel<%s, %d, %d, %s>' % (pt, k, p, '0' if r['round2'] else 'kStepVar')
    if kind == STEP_SLOTS:
        return 'consistency_step_basis_slots_kernel<%s, %d>' % (pt, p)
    if kind == TWO_PASS:
        return ('consistency_fwd_basis_kernel<%s, false, %d, %d>' % (pt, k, p)) if k else ('consistency_fwd_basis_slots_kernel<%s, false, %d>' % (pt, p))
    if kind == POSE:
        return 'consistency_step_pose_kernel<%d, %d>' % (k, p)
    return None


@pytest.mark.parametrize('name, setting', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_route_names_the_kernel_that_runs(dev, hostlib, name, setting):
    from depth_correction_amd import _native as nv
    from depth_correction_amd.plan import KernelTimer
    plan, poses = _plan(dev, name)
    nt = N_TERMS[name]
    want_pose = name == 'pose'
    w = torch.tensor([1e-3, 2e-3, 5e-4][:nt], dtype=torch.float64, device=dev)
    e = torch.tensor([2.0, 4.0, 6.0][:nt], dtype=torch.float64, device=dev)
    out = torch.zeros(2 + 2 * nt + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    setv = lambda o, v: nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')
    try:
        if setting:
            setv(*setting)
        plan.clear_status()
        with KernelTimer(every=1) as timer:
            plan.eval_native(w, e, plan.poses12(poses), out, want_pose=want_pose)          # raises unless dc_sequence_eval returns 0
            torch.cuda.synchronize()
            ran = timer.kernels()['consistency_fwd']
    finally:
        for o, v in ((6, 1), (9, 0), (4, 0), (7, 0)):
            setv(o, v)
    # the descriptor of that call (the plan fills the basis rows, the pose tables and the transposed lists into it on demand)
    d = plan.desc(nt)
    o = dict(no_tab=0, fwd_generic=0, no_basis=0, two_pass=0, step_var=1, pose_three_pass=0, step_six=0)
    o.update(SETTINGS[setting])
    options = (ctypes.c_int * 7)(*[o[f] for f in OPTIONS])
    vals = (ctypes.c_int64 * len(FIELDS))()
    rc = hostlib.dc_host_choose_route(ctypes.addressof(d), 1, 1, 1, 1, 0, int(want_pose), 0, ctypes.addressof(options), ctypes.addressof(vals))
    r = dict(zip(FIELDS, vals))
    print(name, setting, 'route', r, 'ran', ran)
    assert rc == 0, rc
    assert plan.status_bits() == 0 and np.isfinite(out.cpu().numpy()).all()
    expected = _kernel_name(r)
    if expected is None:
        # the three-kernel path: its forward kernel is consistency_fwd_impl's choice, not the route's
        assert r['kind'] == GENERAL and ran.startswith(('consistency_fwd_kernel<', 'consistency_fwd_fixed_kernel<', 'consistency_fwd_staged_kernel<')), (r, ran)
    else:
        assert ran == expected, (ran, expected, r)
    # what each plan was chosen to reach under the default options
    if setting is None:
        kinds = dict(k4=STEP_Q32, pos10=STEP_Q32, wide10=STEP_Q32, nomask=STEP_Q32, n100=STEP_Q32, f64=STEP_BASIS, ball=STEP_RAGGED, pose=POSE)
        assert r['kind'] == kinds[name], (name, r)
        assert r['cap'] == dict(wide10=768, ball=1024).get(name, 512 if r['kind'] == STEP_Q32 else 0), r
    if setting == (7, 1):
        assert r['kind'] == GENERAL, r
    if setting == (4, 1) and not want_pose:
        assert r['kind'] == TWO_PASS, r
