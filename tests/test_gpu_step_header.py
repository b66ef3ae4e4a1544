"""The per-block step headers (dcSequenceDesc.step_hdr, StepHdr of csrc/dc_cons_chain.h) and the C2 step kernel that reads them.

Header contents: the plan's header equals, word for word, one put together in numpy from the plan's own blk_ptr, slot_ptr,
own_base, mask and n (the table is fwd_table_loss where the plan has one, else fwd_table: what the one-pass evaluation stages from).

Kernel results: consistency_step_q32_kernel (header) against consistency_step_basis_kernel<q32, ..., kStepVar> (dc_set_option(6, 7):
reads slot_ptr, blk_ptr, own_base, blk_skip and the mask bytes themselves) and against the same plan with the descriptor's step_hdr
cleared (the fallback a caller without a header gets: the same generic kernel).  The two kernels share the per-centre arithmetic and
the order of every sum; at the parent commit they were byte-equal on exactly these sequences (all of _sequences(), one, two and three
weights: evaluation, every chained step, the flush and the weights -- checked on an MI355X with the parent commit's package and
library: every difference exactly 0), so the comparison here is byte for byte.

Sequences (a few hundred to ~3 000 points; one base cloud, every table a brute-force k-NN or a designed one):
  base10   the whole base cloud, k = 10, the pipeline's mask: wave-packed layout, loss-only table, several blocks and a tail block
  hole10   the same with 560 Morton-consecutive points outside the mask (a whole block without a centre: flag bit 0) and rows with
           missing neighbours (-1)
  k4 / k8 / k16   n = 3 * 256 + 37 (a tail block with 37 live lanes), the other slot counts
  n100     a single partial block
  nomask   n = 3 * 256 + 37 without a mask
  pos10    n = 3 * 256 + 37 in the caller's order (spatial_sort=False), a table of nearby positions and a mask set lane by lane: block
           1 keeps exactly one centre (lane 77), block 2 loses the 64 lanes of its second wavefront, the others stay whole
  wide10   the longest list between 513 and 768 rows (the 768-row tile): in the plan's own order every position references its own
           lane in the two following blocks besides seven neighbours inside its block -- 256 + 2 * (centres inside the mask) distinct
           rows per block
The whole file takes a few seconds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 3
W0, E0 = [1e-3, 2e-3, 5e-4], [2.0, 4.0, 6.0]
NAMES = ('base10', 'hole10', 'k4', 'k8', 'k16', 'n100', 'nomask', 'pos10', 'wide10')
_cache = {}


def _knn(x, k):
    """Brute-force [n, k] neighbour table (every point first among its own neighbours)."""
    d = torch.cdist(x.double(), x.double())
    d.fill_diagonal_(-1.0)
    return torch.topk(d, k, dim=1, largest=False).indices.to(torch.int32).contiguous()


def _sequences(dev):
    """{name: (plan, poses, k)}, built once."""
    if _cache:
        return _cache
    from depth_correction_amd import ops
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.plan import SequencePlan
    ds = RoomBoxDataset(n_pts=600, n_poses=5, seed_base=1000, dtype=np.float32)
    scans = [np.stack([c[f] for f in 'xyz'], axis=1) for c, _ in ds]
    poses_np = np.stack([p for _, p in ds])
    base, info = build_sequence(scans, poses_np, k=10, dtype=torch.float32, device=dev)
    clouds, poses, x0, mask0 = info['clouds'], info['poses'], info['points0'], info['mask']
    sizes = [len(c['dirs']) for c in clouds]
    starts = np.concatenate([[0], np.cumsum(sizes)])

    def sub(m):
        """The first m points of every scan: (clouds, global indices)."""
        cl = [{f: c[f][:m].contiguous() for f in ('vps', 'dirs', 'depth', 'inc_angles', 'mask')} for c in clouds]
        idx = torch.cat([torch.arange(m, device=dev) + int(s) for s in starts[:-1]])
        return cl, idx

    _cache['base10'] = (base, poses, 10)
    # ---- a hole in the mask along the Morton curve, rows with missing neighbours (tests/test_gpu_step_residency.py)
    order = ops.spatial_order(x0.contiguous()).long()
    mask = torch.ones(base.n, dtype=torch.bool, device=dev)
    mask[order[300:860]] = False
    nbr = info['neighbors'].clone()
    for j, r in enumerate(order[0:150:3].tolist()):
        nbr[r, 10 - 1 - (j % 5):] = -1
    _cache['hole10'] = (SequencePlan(clouds, poses, nbr, mask), poses, 10)
    # ---- n = 3 * 256 + 37 and n = 100
    cl, idx = sub(161)
    assert len(idx) == 3 * 256 + 37
    for k in (4, 8, 16):
        _cache['k%d' % k] = (SequencePlan(cl, poses, _knn(x0[idx], k), mask0[idx].contiguous()), poses, k)
    _cache['nomask'] = (SequencePlan(cl, poses, _knn(x0[idx], 10), None), poses, 10)
    cl20, idx20 = sub(20)
    _cache['n100'] = (SequencePlan(cl20, poses, _knn(x0[idx20], 10), mask0[idx20].contiguous()), poses, 10)
    # ---- the caller's order, a mask set lane by lane
    n = len(idx)
    p = torch.arange(n, device=dev)
    off = torch.tensor([0, 1, -1, 2, -2, 3, 17, -17, 40, -40], device=dev)
    nbr = (p[:, None] + off[None, :]).clamp(0, n - 1).to(torch.int32).contiguous()
    nbr[5::7, 8:] = -1
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    mask[256:512] = False
    mask[256 + 77] = True
    mask[512 + 64:512 + 128] = False
    _cache['pos10'] = (SequencePlan(cl, poses, nbr, mask, spatial_sort=False), poses, 10)
    # ---- the 768-row tile: designed in the base plan's order (which depends on the points and the mask, not on the table)
    n, o = base.n, base.order
    p = torch.arange(n, device=dev)
    b0 = p // 256 * 256
    blen = torch.clamp(n - b0, max=256)
    cols = [p, (p + 256) % n, (p + 512) % n] + [b0 + (p - b0 + j) % blen for j in range(1, 8)]
    nbr_pos = torch.stack(cols, dim=1)
    nbr = torch.empty((n, 10), dtype=torch.int32, device=dev)
    nbr[o] = o[nbr_pos].to(torch.int32)
    wide = SequencePlan(clouds, poses, nbr.contiguous(), mask0)
    assert torch.equal(wide.order, o)
    _cache['wide10'] = (wide, poses, 10)
    return _cache


def _run(plan, poses, n_terms, dev):
    """{'eval': [sum loss, count, dL/dw], 'steps': what three chained steps and the flush returned, 'w': the weights after them,
    'kernel': the step kernel's name} under the options and the descriptor the caller has set."""
    from depth_correction_amd.plan import KernelTimer, SequenceTrainer
    w0, e0 = W0[:n_terms], E0[:n_terms]
    w = torch.tensor(w0, dtype=torch.float64, device=dev)
    e = torch.tensor(e0, dtype=torch.float64, device=dev)
    out = torch.zeros(2 + 2 * n_terms + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    with KernelTimer(every=1) as timer:
        plan.eval_native(w, e, plan.poses12(poses), out)
        torch.cuda.synchronize()
        kernel = timer.kernels()['consistency_fwd']
    tr = SequenceTrainer([plan], w0, e0, [poses], lr=1e-3, chained=True)
    steps = []
    for _ in range(N_STEPS):
        steps.append(tr.step().clone())
    assert tr.chained, 'the plan refused to chain'
    steps.append(tr.flush().clone())
    torch.cuda.synchronize()
    return dict(eval=out[:2 + n_terms].cpu().numpy().copy(), steps=torch.stack(steps).cpu().numpy(), w=tr.w.cpu().numpy().copy(),
                kernel=kernel, status=plan.status_bits())


def _header_reference(plan):
    """[blocks, 16] int32: the header in numpy from the plan's table, mask and n."""
    ft = plan.fwd_table_loss or plan.fwd_table
    blk_ptr, slot_ptr = ft.blk_ptr.cpu().numpy().astype(np.int64), ft.slot_ptr.cpu().numpy().astype(np.int64)
    n = plan.nbr.shape[0]
    nb = (n + 255) // 256
    live = np.arange(nb * 256) < n
    inside = live.copy()
    if plan.mask is not None:
        inside[:n] &= plan.mask.cpu().numpy() != 0
    ref = np.zeros((nb, 16), dtype=np.int32)
    ref[:, 0], ref[:, 1] = slot_ptr[:-1], np.diff(slot_ptr)
    ref[:, 2], ref[:, 3] = blk_ptr[:-1], np.diff(blk_ptr)
    ref[:, 4] = ft.own_base.cpu().numpy()[:nb] if (ft.own_base is not None and plan.centre_idx is None) else -1
    skips = plan.mask is not None and plan.centre_idx is None and plan.blk_skip is not None
    ref[:, 5] = (~inside.reshape(nb, 256).any(1)).astype(np.int32) if skips else 0
    ref[:, 6] = np.minimum(256, n - 256 * np.arange(nb))
    bits = inside.reshape(nb, 4, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, None, :]
    ref[:, 8:] = np.bitwise_or.reduce(bits, axis=2).view(np.int32).reshape(nb, 8)       # little-endian: low half first
    return ref


@pytest.mark.parametrize('name', NAMES)
def test_header_contents(dev, name):
    plan, _, k = _sequences(dev)[name]
    assert plan.step_hdr is not None and plan.step_hdr.data_ptr() % 64 == 0
    got = plan.step_hdr.cpu().numpy()
    ref = _header_reference(plan)
    assert got.dtype == np.int32 and got.shape == ref.shape
    for col, what in enumerate(('s0', 'nslots', 'base', 'nd', 'own', 'flags', 'n_live', 'reserved') + tuple('in_mask[%d].%s' % (w, h) for w in range(4) for h in ('lo', 'hi'))):
        assert np.array_equal(got[:, col], ref[:, col]), (name, what, got[:, col], ref[:, col])
    # ---- what each sequence was designed to contain
    n, nb = plan.nbr.shape[0], ref.shape[0]
    words = got[:, 8:].copy().view(np.uint64)                                             # [blocks, 4]
    assert (got[:, 1] == k).all() and (got[:, 7] == 0).all()
    if plan.blk_skip is not None and plan.mask is not None:
        assert np.array_equal(got[:, 5] & 1, plan.blk_skip.cpu().numpy()[:nb].astype(np.int32))
    if name in ('k4', 'k8', 'k16', 'nomask', 'pos10'):
        assert n == 3 * 256 + 37 and got[-1, 6] == 37
        assert (words[-1, 0] >> np.uint64(37)) == 0 and (words[-1, 1:] == 0).all(), 'bits of dead lanes are clear'
    if name == 'nomask':
        assert (words[:-1] == np.uint64(2 ** 64 - 1)).all() and words[-1, 0] == np.uint64(2 ** 37 - 1) and (got[:, 5] == 0).all()
    if name == 'n100':
        assert n == 100 and nb == 1 and got[0, 6] == 100 and words[0, 2] == 0 and words[0, 3] == 0 and (words[0, 1] >> np.uint64(36)) == 0
    if name == 'hole10':
        assert (got[:, 5] & 1).any() and not (got[:, 5] & 1).all(), 'a whole block without a centre, beside others'
        assert (words[(got[:, 5] & 1) != 0] == 0).all()
        assert (plan.nbr.cpu().numpy() < 0).any()
    if name == 'pos10':
        assert [int(w) for w in words[1]] == [0, 1 << 13, 0, 0], 'exactly one centre (lane 77) in block 1'
        assert words[2, 1] == 0 and (words[2, [0, 2, 3]] == np.uint64(2 ** 64 - 1)).all(), 'an empty wavefront inside an active block'
        assert (got[:, 5] == 0).all()                                # (no blk_skip in the caller's order: the block with one centre runs)
    if name == 'wide10':
        longest = int(got[(got[:, 5] & 1) == 0, 3].max())
        assert 513 <= longest <= 768, longest

@pytest.mark.parametrize('n_terms', [1, 2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_header_kernel_against_generic_and_fallback(dev, name, n_terms):
    from depth_correction_amd import _native as nv
    plan, poses, k = _sequences(dev)[name]
    setv = lambda o, v: nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')
    d = plan.desc(n_terms)
    hdr = d.step_hdr
    assert hdr, 'the plan passes a header'
    try:
        plan.clear_status()
        new = _run(plan, poses, n_terms, dev)
        setv(6, 7)
        generic = _run(plan, poses, n_terms, dev)
        setv(6, 1)
        assert plan.desc(n_terms) is d
        d.step_hdr = None
        fallback = _run(plan, poses, n_terms, dev)
    finally:
        setv(6, 1)
        d.step_hdr = hdr
    tile = 768 if name == 'wide10' else 512
    assert new['kernel'] == 'consistency_step_q32_kernel<%d, %d, %d>' % (k, n_terms, tile), new['kernel']
    assert generic['kernel'].startswith('consistency_step_basis_kernel<q32, %d, %d, ' % (k, n_terms)), generic['kernel']
    assert fallback['kernel'] == generic['kernel'], (fallback['kernel'], generic['kernel'])
    for r in (new, generic, fallback):
        assert r['status'] == 0
        assert np.isfinite(r['eval']).all() and np.isfinite(r['steps']).all() and np.isfinite(r['w']).all()
    assert new['eval'][1] == plan.count > 0
    assert not np.array_equal(new['steps'][1], new['steps'][-1])                      # the chain moved the weights
    for what, other in (('generic', generic), ('fallback', fallback)):
        for key in ('eval', 'steps', 'w'):
            d_ = np.abs(new[key] - other[key]).max()
            print('%s P=%d %s %s: max |difference| = %.3g' % (name, n_terms, what, key, d_))
            assert new[key].tobytes() == other[key].tobytes(), (name, n_terms, what, key, new[key], other[key])
