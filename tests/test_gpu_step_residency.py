"""The C2 step kernel built for seven resident blocks per CU (the default) against the same body built for six (dc_set_option(9, 1))
and against the generic one-pass kernel on the same table (dc_set_option(6, 7)), on sequences of ~1 300 points chosen so that
every path of the kernel runs: a partly filled last block, a block none of whose centres is inside the loss mask, wavefronts
entirely outside the mask beside ones inside, rows with missing neighbours beside full wavefronts, one and two weights.

Bounds.  Seven against six: the two are one source under two launch bounds and every summation has a fixed order -- byte-equal
sums and weights.  Against the generic kernel: tests/test_gpu_eig_spectra.py::test_step_kernels holds both forms to the same
reference, the loss sum within EPS_Q32 = 1e-11 of sum_i lam_max_i and dL/dw within rtol 1e-5 / atol 2e-5 max |dL/dw|; here the
plans are built with normalization=False like there, so a centre's loss is its smallest eigenvalue and sum_i loss_i <= sum_i
lam_max_i: EPS_Q32 |sum loss| is the same bound or a tighter one.  The count is exactly equal.

Measured on an MI355X (the test prints the figures): every difference against the generic kernel is exactly 0 -- loss and dL/dw of
the ordinary evaluation, of the chain's first evaluation and of its last, both sequences, one and two weights: the two kernels
share the per-centre arithmetic and the order of the sums.  The whole file takes 1.5 s."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_Q32 = 1e-11                 # tests/test_gpu_eig_spectra.py
K = 10
N_STEPS = 5
_cache = {}


def _sequences(dev):
    """{'built': (plan, info), 'crafted': (plan, info)}: 4 scans x 325 points through build_sequence, and the same clouds and
    neighbours under a mask and a table designed on the Morton order of the initial cloud."""
    if _cache:
        return _cache
    from depth_correction_amd import ops
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.plan import SequencePlan
    ds = RoomBoxDataset(n_pts=325, n_poses=4, seed_base=1000, dtype=np.float32)
    scans = [np.stack([c[f] for f in 'xyz'], axis=1) for c, _ in ds]
    poses = np.stack([p for _, p in ds])
    plan, info = build_sequence(scans, poses, k=K, dtype=torch.float32, device=dev, normalization=False)
    _cache['built'] = (plan, info)
    n = plan.n
    order = ops.spatial_order(info['points0'].contiguous()).long()
    # 560 Morton-consecutive points outside the mask: nine whole wavefronts of the packed layout, so at least one block of four
    # of them whatever the alignment (any seven consecutive runs hold an aligned four), and all-out wavefronts in mixed blocks
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    mask[order[300:860]] = False
    # every third of the first 150 points of the curve loses its last 1..5 neighbours: wavefronts with empty slots at the
    # start of the curve, full ones elsewhere
    nbr = info['neighbors'].clone()
    rows = order[0:150:3]
    for j, r in enumerate(rows.tolist()):
        nbr[r, K - 1 - (j % 5):] = -1
    crafted = SequencePlan(info['clouds'], info['poses'], nbr, mask, normalization=False)
    _cache['crafted'] = (crafted, dict(info, neighbors=nbr, mask=mask))
    return _cache


def _run(plan, info, n_terms, dev):
    """{'eval': [sum loss, count, dL/dw], 'steps': the sums every chained step and the flush returned, 'w': the weights after
    them, 'kernel': the step kernel's name} under the options set by the caller."""
    from depth_correction_amd.plan import KernelTimer, SequenceTrainer
    w0, e0 = [1e-3, 2e-3][:n_terms], [2.0, 4.0][:n_terms]
    w = torch.tensor(w0, dtype=torch.float64, device=dev)
    e = torch.tensor(e0, dtype=torch.float64, device=dev)
    out = torch.zeros(2 + 2 * n_terms + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    with KernelTimer(every=1) as timer:
        plan.eval_native(w, e, plan.poses12(info['poses']), out)
        torch.cuda.synchronize()
        kernel = timer.kernels()['consistency_fwd']
    tr = SequenceTrainer([plan], w0, e0, [info['poses']], lr=1e-3, chained=True)
    steps = []
    for _ in range(N_STEPS):
        steps.append(tr.step().clone())
    assert tr.chained, 'the plan refused to chain'
    steps.append(tr.flush().clone())
    torch.cuda.synchronize()
    return dict(eval=out[:2 + n_terms].cpu().numpy().copy(), steps=torch.stack(steps).cpu().numpy(), w=tr.w.cpu().numpy().copy(),
                kernel=kernel, status=plan.status_bits(), timed_out=plan.chain_timed_out())


def test_sequences_reach_every_path(dev):
    """What the sequences were designed to contain is there (read from the plans, in their own order)."""
    plan, _ = _sequences(dev)['crafted']
    assert plan.n >= 4 * 256 and plan.n % 256 != 0
    assert getattr(plan, '_wave_packed', False) and plan.blk_skip is not None
    skip = plan.blk_skip.cpu().numpy() != 0
    m = plan.mask.cpu().numpy()
    pad = np.zeros((plan.n + 255) // 256 * 256, dtype=bool)
    pad[:plan.n] = m
    waves_in = pad.reshape(-1, 4, 64).any(2)                                   # [blocks, 4]: a centre of the wavefront is inside the mask
    assert skip.any() and not skip.all()
    assert np.array_equal(skip, ~waves_in.any(1))
    assert (waves_in.any(1) & ~waves_in.all(1)).any(), 'no block with wavefronts inside AND entirely outside the mask'
    miss = (plan.nbr.cpu().numpy() < 0).any(1)
    padm = np.zeros(len(pad), dtype=bool)
    padm[:plan.n] = miss & m
    wave_miss = padm.reshape(-1, 64).any(1)
    wave_full = pad.reshape(-1, 64).all(1) & ~np.pad(miss, (0, len(pad) - plan.n)).reshape(-1, 64).any(1)
    assert wave_miss.any() and wave_full.any(), 'both instantiations of the sweeps (empty slots / none) must run'
    built, _ = _sequences(dev)['built']
    assert built.n == plan.n and built.count > 0


@pytest.mark.parametrize('n_terms', [1, 2])
@pytest.mark.parametrize('seq', ['built', 'crafted'])
def test_seven_blocks_against_six_and_generic(dev, seq, n_terms):
    from depth_correction_amd import _native as nv
    plan, info = _sequences(dev)[seq]
    setv = lambda o, v: nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')
    try:
        plan.clear_status()
        seven = _run(plan, info, n_terms, dev)
        setv(9, 1)
        six = _run(plan, info, n_terms, dev)
        setv(9, 0)
        setv(6, 7)
        generic = _run(plan, info, n_terms, dev)
    finally:
        setv(9, 0)
        setv(6, 1)
    assert seven['kernel'] == 'consistency_step_q32_kernel<%d, %d, 512>' % (K, n_terms), seven['kernel']
    assert six['kernel'] == 'consistency_step_q32_kernel<%d, %d, 512, 6>' % (K, n_terms), six['kernel']
    assert generic['kernel'].startswith('consistency_step_basis_kernel<q32, %d, %d, ' % (K, n_terms)), generic['kernel']
    for r in (seven, six, generic):
        assert r['status'] == 0 and not r['timed_out']
        assert np.isfinite(r['eval']).all() and np.isfinite(r['steps']).all() and np.isfinite(r['w']).all()
    # ---- against the six-block build: bytes
    assert seven['eval'].tobytes() == six['eval'].tobytes(), (seven['eval'], six['eval'])
    assert seven['steps'].tobytes() == six['steps'].tobytes()
    assert seven['w'].tobytes() == six['w'].tobytes()
    assert seven['eval'][1] == plan.count > 0
    assert not np.array_equal(seven['steps'][1], seven['steps'][-1])              # the chain moved the weights
    # ---- against the generic kernel on the same table: the ordinary evaluation and the chain's first evaluation (steps[1]: what
    # the second launch finished), both at the initial weights; later evaluations of the two chains are at weights that Adam has
    # moved by each form's own gradient, so their sums are printed, and only the count is compared
    for form, r in (('seven', seven), ('six', six)):
        for what, a, b in (('eval', r['eval'], generic['eval']), ('chain[1]', r['steps'][1], generic['steps'][1]),
                           ('chain[last]', r['steps'][-1], generic['steps'][-1])):
            dl, gmax = abs(a[0] - b[0]), np.abs(b[2:]).max()
            print('%s %s P=%d %s: |d loss| / |loss| = %.2e (bound %.0e), max |d dL/dw| / max |dL/dw| = %.2e' % (
                seq, form, n_terms, what, dl / abs(b[0]), EPS_Q32, np.abs(a[2:] - b[2:]).max() / gmax))
            assert a[1] == b[1]
            if what != 'chain[last]':
                assert dl <= EPS_Q32 * abs(b[0])
                np.testing.assert_allclose(a[2:], b[2:], rtol=1e-5, atol=2e-5 * gmax)
