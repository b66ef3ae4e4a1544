"""The per-block row copy (dcSequenceDesc.step_rows, dc_step_rows_build) and the C2 step kernel that stages from it.

The copy holds, for every entry of the staged table's blk_ids, the basis row that entry names, per block in the order the block
stages its list (layout: csrc/dc_cons_basis.h, step_rows_piece_words; restated in _copy_reference below).  With it
consistency_step_q32_kernel fetches its rows right after its header and never reads blk_ids; without it (the field NULL, or
dc_set_option(10, 1)) it gathers the same words by id.  No staged word, no arithmetic and no order of a sum differs, so every
comparison here is byte for byte.

Sequences: those of tests/test_gpu_step_header.py (its builders, built once for both files), each with one, two and three weights.

  builder     the plan's copy against basis[blk_ids] put into the documented layout by numpy, word for word
  bits        evaluation, three chained steps, the flush and the final weights of three runs -- with the copy, under
              dc_set_option(10, 1), and with the descriptor field cleared (SequencePlan.use_step_rows = False) -- and the kernel's name
  live        base10 (every block has own rows: nothing but the weights and the staged rows enters the sums): the basis rows overwritten
              with a pattern after the copy exists -> the same bytes, so the kernel does read the copy
  staleness   exponents, then poses, changed in place: the first evaluation after a change (no copy yet) and the second (copy rebuilt)
              equal a fresh plan's that never saw the old values.  The fresh plan is constructed with the same arguments -- the layout
              and the q32 grid come from the construction poses, and a different layout is a different order of the sums -- and is
              evaluated with the new values
  laziness    a plan evaluated once per key never allocates a copy
The whole file takes a few seconds."""
import numpy as np
import pytest
import torch

from test_gpu_step_header import E0, N_STEPS, NAMES, W0, _sequences

pytestmark = pytest.mark.gpu

_fresh_args = {}


def _table(plan):
    return plan.fwd_table_loss or plan.fwd_table


def _copy_reference(plan, basis):
    """int32 [blk_ptr[blocks] * W]: basis[blk_ids] per block, piece-major (pieces of four words, the last one short)."""
    ft = _table(plan)
    blk_ptr, ids = ft.blk_ptr.cpu().numpy().astype(np.int64), ft.blk_ids.cpu().numpy().astype(np.int64)
    W = basis.shape[1]
    out = np.empty(blk_ptr[-1] * W, dtype=np.int32)
    for b in range(len(blk_ptr) - 1):
        base, end = blk_ptr[b], blk_ptr[b + 1]
        rows = basis[ids[base:end]]                                   # [nd, W]
        pieces = [rows[:, c:min(c + 4, W)].reshape(-1) for c in range(0, W, 4)]
        out[base * W:end * W] = np.concatenate(pieces) if end > base else []
    return out


def _eval(plan, w, e, P12, dev):
    out = torch.zeros(2 + 2 * w.numel() + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    plan.eval_native(w, e, P12, out)
    return out[:2 + w.numel()].cpu().numpy().copy()


def _run(plan, poses, n_terms, dev, expect_copy):
    """Two evaluations under one key (the second with the copy where the plan passes one), then three chained steps and the flush
    under a key that was evaluated twice before (the copy is there from the first step on)."""
    from depth_correction_amd.plan import KernelTimer, SequenceTrainer
    w = torch.tensor(W0[:n_terms], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:n_terms], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses)
    d = plan.desc(n_terms)
    with KernelTimer(every=1) as timer:
        first = _eval(plan, w, e, P12, dev)
        assert not d.step_rows, 'no copy on the first evaluation of a key'
        second = _eval(plan, w, e, P12, dev)
        torch.cuda.synchronize()
        kernel = timer.kernels()['consistency_fwd']
    assert bool(d.step_rows) == expect_copy
    tr = SequenceTrainer([plan], W0[:n_terms], E0[:n_terms], [poses], lr=1e-3, chained=True)
    for _ in range(2):
        _eval(plan, tr.w.clone(), tr.exponent, tr.poses12[0], dev)
    assert bool(d.step_rows) == expect_copy
    rows_at = d.step_rows
    steps = []
    for _ in range(N_STEPS):
        steps.append(tr.step().clone())
        assert d.step_rows == rows_at, 'the chain keeps its key'
    assert tr.chained, 'the plan refused to chain'
    steps.append(tr.flush().clone())
    torch.cuda.synchronize()
    return dict(first=first, eval=second, steps=torch.stack(steps).cpu().numpy(), w=tr.w.cpu().numpy().copy(), kernel=kernel,
                status=plan.status_bits())


@pytest.mark.parametrize('n_terms', [1, 2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_copy_is_the_gathered_basis_rows(dev, name, n_terms):
    plan, poses, _ = _sequences(dev)[name]
    w = torch.tensor(W0[:n_terms], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:n_terms], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses)
    _eval(plan, w, e, P12, dev)
    assert plan._basis[4] is None
    _eval(plan, w, e, P12, dev)
    copy = plan._basis[4]
    assert copy is not None and copy.dtype == torch.int32 and copy.data_ptr() % 16 == 0
    assert plan.desc(n_terms).step_rows == copy.data_ptr()
    basis = plan._basis[1].cpu().numpy()
    assert basis.shape == (plan.n, 6 + n_terms) and basis.dtype == np.int32
    ref = _copy_reference(plan, basis)
    got = copy.cpu().numpy()
    assert got.shape == (max(len(ref), 1),) or got.shape == ref.shape
    assert np.array_equal(got[:len(ref)], ref), (name, n_terms, np.flatnonzero(got[:len(ref)] != ref)[:8])
    assert len(ref) == int(_table(plan).blk_ptr[-1].item()) * (6 + n_terms)


@pytest.mark.parametrize('n_terms', [1, 2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_copy_option_and_cleared_field_give_the_same_bytes(dev, name, n_terms):
    from depth_correction_amd import _native as nv
    plan, poses, k = _sequences(dev)[name]
    setv = lambda o, v: nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')
    assert plan.use_step_rows and plan.step_hdr is not None
    try:
        plan.clear_status()
        new = _run(plan, poses, n_terms, dev, True)
        setv(10, 1)
        option = _run(plan, poses, n_terms, dev, True)                 # (the plan still passes the copy: the launch ignores it)
        setv(10, 0)
        plan.use_step_rows = False
        cleared = _run(plan, poses, n_terms, dev, False)
    finally:
        setv(10, 0)
        plan.use_step_rows = True
    tile = 768 if name == 'wide10' else 512
    for r in (new, option, cleared):
        assert r['kernel'] == 'consistency_step_q32_kernel<%d, %d, %d>' % (k, n_terms, tile), r['kernel']
        assert r['status'] == 0
        assert np.isfinite(r['eval']).all() and np.isfinite(r['steps']).all() and np.isfinite(r['w']).all()
    assert new['eval'][1] == plan.count > 0
    assert not np.array_equal(new['steps'][1], new['steps'][-1])                      # the chain moved the weights
    assert new['first'].tobytes() == new['eval'].tobytes(), 'the same key without and with the copy'
    for what, other in (('option 10', option), ('cleared', cleared)):
        for key in ('first', 'eval', 'steps', 'w'):
            print('%s P=%d %s %s: max |difference| = %.3g' % (name, n_terms, what, key, np.abs(new[key] - other[key]).max()))
            assert new[key].tobytes() == other[key].tobytes(), (name, n_terms, what, key, new[key], other[key])


@pytest.mark.parametrize('n_terms', [1, 2, 3])
def test_kernel_reads_the_copy(dev, n_terms):
    plan, poses, _ = _sequences(dev)['base10']
    assert (plan.step_hdr.cpu().numpy()[:, 4] >= 0).all(), 'every block takes its centres from the staged rows'
    w = torch.tensor(W0[:n_terms], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:n_terms], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses)
    _eval(plan, w, e, P12, dev)
    before = _eval(plan, w, e, P12, dev)
    rows = plan._basis[1]
    assert plan._basis[4] is not None
    saved = rows.clone()
    try:
        rows.fill_(0x5A5A5A5A)
        after = _eval(plan, w, e, P12, dev)
        assert plan._basis[1] is rows and plan.desc(n_terms).step_rows == plan._basis[4].data_ptr()
    finally:
        rows.copy_(saved)
    assert np.isfinite(before).all() and before[1] == plan.count
    assert after.tobytes() == before.tobytes(), (before, after)


def _fresh(dev):
    """A new plan of the base sequence: the same construction arguments every time."""
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.plan import SequencePlan
    if not _fresh_args:
        ds = RoomBoxDataset(n_pts=600, n_poses=5, seed_base=1000, dtype=np.float32)
        scans = [np.stack([c[f] for f in 'xyz'], axis=1) for c, _ in ds]
        _, info = build_sequence(scans, np.stack([p for _, p in ds]), k=10, dtype=torch.float32, device=dev)
        _fresh_args.update(clouds=info['clouds'], poses=info['poses'], nbr=info['neighbors'], mask=info['mask'])
    a = _fresh_args
    return SequencePlan(a['clouds'], a['poses'], a['nbr'], a['mask']), a['poses']


@pytest.mark.parametrize('n_terms', [1, 2, 3])
def test_copy_follows_the_exponents_and_the_poses(dev, n_terms):
    plan, poses = _fresh(dev)
    w = torch.tensor(W0[:n_terms], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:n_terms], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses).clone()
    old = [_eval(plan, w, e, P12, dev) for _ in range(2)]
    assert plan._basis[4] is not None and old[0].tobytes() == old[1].tobytes()
    last = old[1]
    for change in ('exponents', 'poses'):
        if change == 'exponents':
            e.mul_(1.25)
        else:
            P12[:, 3] += 0.004 * torch.arange(plan.n_scans, dtype=torch.float64, device=dev)        # every scan's x translation
        first = _eval(plan, w, e, P12, dev)
        assert plan._basis[4] is None and not plan.desc(n_terms).step_rows, 'the copy goes with the rows it copied'
        second = _eval(plan, w, e, P12, dev)
        assert plan._basis[4] is not None and plan.desc(n_terms).step_rows == plan._basis[4].data_ptr(), 'rebuilt by the second evaluation'
        assert np.array_equal(plan._basis[4].cpu().numpy(), _copy_reference(plan, plan._basis[1].cpu().numpy()))
        other, _ = _fresh(dev)
        want = _eval(other, w.clone(), e.clone(), P12.clone(), dev)
        assert np.isfinite(want).all() and want.tobytes() != last.tobytes(), 'the change changes the result'
        assert first.tobytes() == want.tobytes(), (change, first, want)
        assert second.tobytes() == want.tobytes(), (change, second, want)
        assert plan.status_bits() == 0 and other.status_bits() == 0
        last = want


def test_one_evaluation_per_key_allocates_no_copy(dev):
    plan, poses = _fresh(dev)
    w = torch.tensor(W0[:2], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:2], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses).clone()
    for i in range(4):
        if i % 2:
            e.add_(0.01)
        else:
            P12[:, 7] += 1e-3
        _eval(plan, w, e, P12, dev)
        assert plan._basis[4] is None and plan._basis[5] == 1 and not plan.desc(2).step_rows
    for i in range(3):                                                          # a new exponent tensor every time
        _eval(plan, w, e.clone(), P12, dev)
        assert plan._basis[4] is None and not plan.desc(2).step_rows
    assert getattr(plan, '_step_rows_total', None) is None
