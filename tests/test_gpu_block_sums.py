"""A chained launch's row of partials {sum loss, count, dL/dw}: one per block, summed once by step_block_row (csrc/dc_cons_step.h),
the same function in every one-pass step kernel.

Sequences: the `crafted` one of tests/test_gpu_step_residency.py (1 300 points, K = 10: five full blocks and a partial sixth, a
block none of whose centres is inside the mask, blocks with wavefronts inside and entirely outside it, wavefronts with empty slots
and without) and a ball-neighbourhood plan of 805 points (three full blocks and a partial fourth), which runs the ragged kernel.

Bounds.
  * Across kernels: the q32 kernel, its six-block build, the basis kernel and the run-time-slot kernel on the same plan: bytes.
    Every kernel against its own second run: bytes.
    (The run-time-slot kernel has no compile-time slot count; a wavefront all of whose lanes have every slot takes 1 / nslots and
    1 / (nslots - 1) as correctly rounded divisions, the bits of the fixed-K kernels' constants -- step_point2's `ns`.  While it took
    them from recip1_, a few 1e-15 off, it differed from the q32 kernel on this plan by 2.3e-16 of the loss and 8.3e-9 / 5.9e-9 /
    2.0e-9 of the largest dL/dw for one / two / three weights: that is what the slots cases watch.)
  * Against the ordinary evaluation (one row per wavefront, reduce_eval_kernel -- not touched): the count is a sum of small
    integers, equal.  The loss is a sum of non-negative terms, so either order is off the exact sum by at most (its longest chain
    of sequential roundings) * 2^-53 relative.  Chained, a lane value passes 2 additions of the hand-over, 6 levels of the
    wavefront reduction, and in the leading block of the next launch (or the flush) at most 5 + 1 + 6 + 4 more: 24.  Ordinary: 6
    levels of the wavefront reduction, then in reduce_eval_kernel one strided trip, 6 levels and 16 wavefront totals: < 30.
    Together fewer than 54 roundings of 1.1e-16: 6e-15, inside the 1e-13 asserted.  dL/dw has terms of both signs: the
    tolerances of tests/test_gpu_scale.py's full-size comparison of chained with ordinary steps, rtol 1e-9 + 1e-12 max |dL/dw|.
  * Zero rows: +0.0 in every column, bit for bit, read from the chain's two row buffers in the plan's workspace.
  * A wait that ran out (dc_set_option(5, 0): bounded by design, every wait gives up at once): NaN in loss and count, the time-out
    bit in the status word.
The whole file takes a few seconds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 10
N_STEPS = 3
W0, E0 = [1e-3, 2e-3, 5e-4], [2.0, 4.0, 6.0]
# name -> dc_set_option (option, value) that selects the kernel, and how its name starts
FORMS = {'q32': (None, 'consistency_step_q32_kernel<%d, %%d, 512>' % K),
         'six': ((9, 1), 'consistency_step_q32_kernel<%d, %%d, 512'  % K),
         'basis': ((6, 7), 'consistency_step_basis_kernel<q32, %d, %%d, ' % K),
         'slots': ((1, 1), 'consistency_step_basis_slots_kernel<q32, %d>')}
RESET = ((9, 0), (6, 1), (1, 0))
_cache = {}


def _plans(dev):
    """{'crafted': (plan, poses), 'ball': (plan, poses)}, built once."""
    if _cache:
        return _cache
    from test_gpu_step_residency import _sequences
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.pipeline import build_sequence
    plan, info = _sequences(dev)['crafted']
    _cache['crafted'] = (plan, info['poses'])
    ds = RoomBoxDataset(n_pts=600, n_poses=5, seed_base=1000, dtype=np.float32)
    scans = [np.stack([c[f] for f in 'xyz'], axis=1)[:161] for c, _ in ds]
    poses = np.stack([p for _, p in ds])
    ball, binfo = build_sequence(scans, poses, k=None, r=0.5, dtype=torch.float32, device=dev)
    _cache['ball'] = (ball, binfo['poses'])
    return _cache


def _setv(o, v):
    from depth_correction_amd import _native as nv
    nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')


def _run(plan, poses, n_terms, dev, n_steps=N_STEPS):
    """{'eval': [sum loss, count, dL/dw] of the ordinary evaluation at the initial weights, 'steps': what n_steps chained steps and
    the flush returned (steps[1] is the chain's first evaluation, at the initial weights too), 'w': the weights after them,
    'kernel': the one-pass kernel's name} under the options the caller has set."""
    from depth_correction_amd.plan import KernelTimer, SequenceTrainer
    w0, e0 = W0[:n_terms], E0[:n_terms]
    w = torch.tensor(w0, dtype=torch.float64, device=dev)
    e = torch.tensor(e0, dtype=torch.float64, device=dev)
    out = torch.zeros(2 + 2 * n_terms + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    plan.clear_status()
    with KernelTimer(every=1) as timer:
        plan.eval_native(w, e, plan.poses12(poses), out)
        torch.cuda.synchronize()
        kernel = timer.kernels()['consistency_fwd']
    tr = SequenceTrainer([plan], w0, e0, [poses], lr=1e-3, chained=True)
    steps = []
    for _ in range(n_steps):
        steps.append(tr.step().clone())
    assert tr.chained, 'the plan refused to chain'
    steps.append(tr.flush().clone())
    torch.cuda.synchronize()
    return dict(eval=out[:2 + n_terms].cpu().numpy().copy(), steps=torch.stack(steps).cpu().numpy(), w=tr.w.cpu().numpy().copy(),
                kernel=kernel, status=plan.status_bits())


def _runs(dev, name, n_terms):
    """Two runs of form `name` (FORMS on the crafted plan, or 'ball': the ragged kernel on its own plan), made once and left alone."""
    key = ('runs', name, n_terms)
    if key not in _cache:
        plan, poses = _plans(dev)['ball' if name == 'ball' else 'crafted']
        setting, _ = FORMS.get(name, (None, None))
        try:
            if setting:
                _setv(*setting)
            _cache[key] = (_run(plan, poses, n_terms, dev), _run(plan, poses, n_terms, dev))
        finally:
            for o, v in RESET:
                _setv(o, v)
    return _cache[key]


@pytest.mark.parametrize('n_terms', [1, 2, 3])
@pytest.mark.parametrize('name', ['q32', 'six', 'basis', 'slots', 'ball'])
def test_kernel_repeats_itself_and_agrees_with_the_ordinary_evaluation(dev, name, n_terms):
    first, second = _runs(dev, name, n_terms)
    if name == 'ball':
        assert _plans(dev)['ball'][0].n == 3 * 256 + 37
        assert first['kernel'].startswith('consistency_step_ragged_q32_kernel<%d, ' % n_terms), first['kernel']
    else:
        assert first['kernel'].startswith(FORMS[name][1] % n_terms), (name, first['kernel'])
    if name == 'six' and n_terms <= 2:                     # (three weights are built for six anyway: the switch changes nothing)
        assert first['kernel'].endswith(', 6>'), first['kernel']
    assert first['status'] == 0 and second['status'] == 0
    assert np.isfinite(first['steps']).all() and np.isfinite(first['w']).all()
    assert not np.array_equal(first['steps'][1], first['steps'][-1])               # the chain moved the weights
    # the same inputs, the same bits, every run
    assert first['steps'].tobytes() == second['steps'].tobytes()
    assert first['w'].tobytes() == second['w'].tobytes()
    # the chain's first evaluation (per-block rows, step_block_row) against the ordinary one (per-wavefront rows), same weights
    a, b = first['steps'][1], first['eval']
    gmax = np.abs(b[2:]).max()
    print('%s P=%d: count %d / %d, |d loss| / loss = %.2e (bound 1e-13), max |d dL/dw| / max |dL/dw| = %.2e (bound 1e-9 |.| + 1e-12 max)' % (
        name, n_terms, a[1], b[1], abs(a[0] - b[0]) / abs(b[0]), np.abs(a[2:] - b[2:]).max() / gmax))
    assert a[1] == b[1] > 0
    assert b[0] > 0 and abs(a[0] - b[0]) <= 1e-13 * abs(b[0])
    np.testing.assert_allclose(a[2:], b[2:], rtol=1e-9, atol=1e-12 * gmax)


@pytest.mark.parametrize('n_terms', [1, 2, 3])
@pytest.mark.parametrize('name', ['six', 'basis', 'slots'])
def test_kernels_on_the_same_plan_give_the_same_bytes(dev, name, n_terms):
    ref, r = _runs(dev, 'q32', n_terms)[0], _runs(dev, name, n_terms)[0]
    d = np.abs(r['steps'][1:] - ref['steps'][1:]).max(0) / np.abs(ref['steps'][1:]).max(0)
    print('%s against q32, P=%d: largest difference per column / largest entry %s, of the weights %s' % (name, n_terms, d, np.abs(r['w'] - ref['w'])))
    assert r['steps'].tobytes() == ref['steps'].tobytes()
    assert r['w'].tobytes() == ref['w'].tobytes()


@pytest.mark.parametrize('form', ['q32', 'basis', 'slots'])
def test_rows_of_blocks_with_nothing_to_add_are_positive_zero(dev, form):
    """The rows of a chain live behind the columns of ordinary evaluations in the plan's workspace: two buffers of [2 + P][blocks of
    the launch], written in turn (route_partials_count, chain_buffer).  Both are filled with NaN first: every row must be written,
    the padding blocks' too; the rows of the skipped blocks and of the padding count nothing and hold +0.0 in every column."""
    from depth_correction_amd import ops
    plan, poses = _plans(dev)['crafted']
    n_terms = 2
    per_row = 2 + 2 * ops.nv.MAX_MODEL_TERMS + 12 * plan.n_scans + 2 * (2 + ops.nv.MAX_MODEL_TERMS)
    rows = plan.partials.numel() // per_row                       # one per wavefront of the launch's grid
    assert rows * per_row == plan.partials.numel() and rows % 4 == 0
    blocks = rows // 4
    first = (2 + 2 * n_terms + 12 * plan.n_scans) * rows
    plan.partials[first:first + 2 * (2 + n_terms) * rows].fill_(float('nan'))
    setting, _ = FORMS[form]
    try:
        if setting:
            _setv(*setting)
        r = _run(plan, poses, n_terms, dev, n_steps=2)
    finally:
        for o, v in RESET:
            _setv(o, v)
    assert r['status'] == 0 and np.isfinite(r['steps']).all()
    skip = plan.blk_skip.cpu().numpy() != 0
    assert skip.any() and not skip.all()
    for parity in (0, 1):
        at = first + parity * (2 + n_terms) * rows
        buf = plan.partials[at:at + (2 + n_terms) * rows].cpu().numpy()
        cols = np.stack([buf[q * blocks:(q + 1) * blocks] for q in range(2 + n_terms)], axis=1)        # [blocks, 2 + P]
        assert np.isfinite(cols).all(), 'a row of the launch was not written'
        nothing = cols[:, 1] == 0
        assert nothing.sum() == blocks - (~skip).sum(), (nothing.sum(), blocks, skip.sum())
        assert cols[nothing].tobytes() == bytes(cols[nothing].nbytes), cols[nothing]
        assert cols[:, 1].sum() == plan.count


def test_a_plan_whose_every_block_is_skipped_sums_to_positive_zero(dev):
    from depth_correction_amd.plan import SequencePlan
    from test_gpu_step_residency import _sequences
    _, info = _sequences(dev)['crafted']
    mask = torch.zeros_like(info['mask'])
    plan = SequencePlan(info['clouds'], info['poses'], info['neighbors'], mask, normalization=False)
    assert plan.count == 0
    r = _run(plan, info['poses'], 2, dev, n_steps=2)
    sums = r['steps'][1:]                                          # what the second launch and the flush finished
    assert r['status'] == 0 and sums[:, :2].tobytes() == bytes(sums[:, :2].nbytes), sums


def test_a_wait_that_ran_out_poisons_loss_and_count(dev):
    from depth_correction_amd.plan import SequencePlan
    plan, poses = _plans(dev)['crafted']
    _setv(5, 0)
    try:
        r = _run(plan, poses, 2, dev, n_steps=2)
    finally:
        _setv(5, -1)
        plan.clear_status()
    assert np.isnan(r['steps'][1:, 0]).all() and np.isnan(r['steps'][1:, 1]).all(), r['steps']
    assert r['status'] & SequencePlan.STATUS_CHAIN_TIMEOUT
