"""The packed tile positions (dcSequenceDesc.step_loc, dc_step_loc_build) and the C2 step kernel that reads them.

step_loc holds, for every block of the table the one-pass evaluation stages from, the 16-bit positions of `loc` two to a 32-bit word
as a lane of consistency_step_q32_kernel holds them (layout: csrc/dc_cons_basis.h, step_loc_piece_words; restated in _pack_reference
below).  With it a working wavefront fetches its words as they are and the others fetch none; without it (the field NULL, or
dc_set_option(11, 1)) the kernel reads the table's `loc` and joins the halves itself.  The positions are the same either way, and so
are the first sweep's rows whether they are read as 12 or as 16 bytes: every comparison here is byte for byte, and the third party
is consistency_step_basis_kernel<q32, ..> (dc_set_option(6, 7)), which shares the first sweep's read and never sees step_loc.

Sequences: two scans of 3 000 points (a cloud that is no multiple of 256: the last block is partly live), brute-force k-NN.
  k10    k = 10 with a distance bound (rows with empty slots, 0xFFFF: the any_miss sweeps run) and a mask with a hole of 492
         Morton-consecutive points from position 356 on: 156 points of block 1 (whole wavefronts of it once the plan has grouped them),
         all of block 2, 80 points of block 3.  One, two and three weights.
  k4, k16   the other piece layouts (two words: one 8-byte load; eight words: two 16-byte loads), the pipeline's mask, two weights.

  builder    dc_step_loc_build into a buffer with guard words on both sides against the numpy packing of `loc`, block by block
  bits       evaluation, three chained steps, the flush and the weights: with step_loc, under dc_set_option(11, 1), with the generic kernel
  lifetime   not built by the first evaluation of a key, built once, kept across new weights, exponents and poses, dropped and rebuilt
             when the plan stages from another table object; a trainer over two plans passes both
The whole file takes a few seconds."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 3
W0, E0 = [1e-3, 2e-3, 5e-4], [2.0, 4.0, 6.0]
CASES = [('k10', 1), ('k10', 2), ('k10', 3), ('k4', 2), ('k16', 2)]
_cache, _args = {}, {}


def _knn(x, k):
    """Brute-force [n, k] neighbour table (every point first among its own neighbours) and the distances."""
    d = torch.cdist(x.double(), x.double())
    d.fill_diagonal_(-1.0)
    dist, idx = torch.topk(d, k, dim=1, largest=False)
    return idx.to(torch.int32).contiguous(), dist


def _sequences(dev):
    """{name: (plan, poses, k)}, built once."""
    if _cache:
        return _cache
    from depth_correction_amd import ops
    from depth_correction_amd.dataset import RoomBoxDataset
    from depth_correction_amd.pipeline import build_sequence
    from depth_correction_amd.plan import SequencePlan
    ds = RoomBoxDataset(n_pts=3000, n_poses=2, seed_base=1000, dtype=np.float32)
    scans = [np.stack([c[f] for f in 'xyz'], axis=1) for c, _ in ds]
    base, info = build_sequence(scans, np.stack([p for _, p in ds]), k=10, dtype=torch.float32, device=dev)
    clouds, poses, x0, mask0 = info['clouds'], info['poses'], info['points0'], info['mask']
    n = base.n
    assert n % 256 != 0 and n > 5 * 256, n
    # ---- k = 10: a distance bound (the farthest fifth of the tenth neighbours goes, and what lies beyond that distance from the fifth on) and a hole in the mask
    nbr, dist = _knn(x0, 10)
    bound = torch.quantile(dist[:, -1], 0.8)
    far = dist > bound
    far[:, :4] = False                                                        # (every row keeps four neighbours, itself among them)
    nbr = torch.where(far, torch.full_like(nbr, -1), nbr).contiguous()
    assert (nbr[:, 0] == torch.arange(n, device=dev)).all() and (nbr[:, -1] < 0).any() and (nbr[:, 3] >= 0).all()
    order = ops.spatial_order(x0.contiguous()).long()
    mask = mask0.clone()
    mask[order[356:356 + 492]] = False
    _args['k10'] = (clouds, poses, nbr, mask)
    for k in (4, 16):
        _args['k%d' % k] = (clouds, poses, _knn(x0, k)[0], mask0)
    for name, a in _args.items():
        _cache[name] = (SequencePlan(*a), poses, a[2].shape[1])
    return _cache


def _table(plan):
    return plan.fwd_table_loss or plan.fwd_table


def _pack_reference(plan):
    """uint32 [slot_ptr[blocks] * 128]: `loc` packed per block, piece-major (pieces of four words per lane, the last one short)."""
    ft = _table(plan)
    slot_ptr = ft.slot_ptr.cpu().numpy().astype(np.int64)
    loc = ft.loc.cpu().numpy().view(np.uint16).reshape(-1, 256).astype(np.uint32)
    out = np.zeros(slot_ptr[-1] * 128, dtype=np.uint32)
    for b in range(len(slot_ptr) - 1):
        s0, ns = slot_ptr[b], slot_ptr[b + 1] - slot_ptr[b]
        assert ns % 2 == 0
        nw = ns // 2
        words = loc[s0:s0 + ns:2] | (loc[s0 + 1:s0 + ns:2] << 16)                # [nw, 256]: word j of lane t
        pieces = [words[c:min(c + 4, nw)].T.reshape(-1) for c in range(0, nw, 4)]   # lane-major inside a piece
        out[s0 * 128:(s0 + ns) * 128] = np.concatenate(pieces)
    return out


def _holds(words, ref):
    """The plan's tensor (as long as `loc`, which may end in slack rows) starts with the reference."""
    got = words.cpu().numpy().view(np.uint32)
    return len(got) >= len(ref) and np.array_equal(got[:len(ref)], ref)


def _eval(plan, w, e, P12, dev):
    out = torch.zeros(2 + 2 * w.numel() + 12 * plan.n_scans, dtype=torch.float64, device=dev)
    plan.eval_native(w, e, P12, out)
    return out[:2 + w.numel()].cpu().numpy().copy()


def _run(plan, poses, n_terms, dev):
    """Two evaluations under one key, then three chained steps and the flush under a key evaluated twice before."""
    from depth_correction_amd.plan import KernelTimer, SequenceTrainer
    w = torch.tensor(W0[:n_terms], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:n_terms], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses)
    with KernelTimer(every=1) as timer:
        first = _eval(plan, w, e, P12, dev)
        second = _eval(plan, w, e, P12, dev)
        torch.cuda.synchronize()
        kernel = timer.kernels()['consistency_fwd']
    tr = SequenceTrainer([plan], W0[:n_terms], E0[:n_terms], [poses], lr=1e-3, chained=True)
    for _ in range(2):
        _eval(plan, tr.w.clone(), tr.exponent, tr.poses12[0], dev)
    steps = []
    for _ in range(N_STEPS):
        steps.append(tr.step().clone())
    assert tr.chained, 'the plan refused to chain'
    steps.append(tr.flush().clone())
    torch.cuda.synchronize()
    return dict(first=first, eval=second, steps=torch.stack(steps).cpu().numpy(), w=tr.w.cpu().numpy().copy(), kernel=kernel,
                status=plan.status_bits(), step_loc=plan.desc(n_terms).step_loc)


def test_sequences_hold_what_they_were_designed_for(dev):
    plan, _, _ = _sequences(dev)['k10']
    hdr = plan.step_hdr.cpu().numpy()
    words = hdr[:, 8:].copy().view(np.uint64)                                   # [blocks, 4]: the wavefronts' mask words
    skip = (hdr[:, 5] & 1) != 0
    assert hdr[-1, 6] < 256, 'the last block is partly live'
    assert skip.any() and not skip.all(), 'a whole block without a centre, beside others'
    lanes = np.minimum(np.maximum(hdr[:, 6:7] - 64 * np.arange(4)[None, :], 0), 64)    # live lanes per wavefront
    idle = (~skip)[:, None] & (words == 0) & (lanes == 64)
    assert idle.any(), 'a wavefront of 64 live lanes without a centre inside a block that runs'
    loc = _table(plan).loc.cpu().numpy().view(np.uint16)
    assert (loc == 0xFFFF).any(), 'empty slots'
    assert (hdr[:, 1] == 10).all()


@pytest.mark.parametrize('name', ['k10', 'k4', 'k16'])
def test_builder_packs_loc_inside_each_blocks_range(dev, name):
    from depth_correction_amd import _native as nv
    from depth_correction_amd._native import ptr, stream_ptr
    plan, _, k = _sequences(dev)[name]
    ft = _table(plan)
    ref = _pack_reference(plan)
    total = int(ft.slot_ptr[-1].item())
    assert len(ref) == total * 128 and ft.loc.numel() >= total * 256
    guard, fill = 1024, -559038737
    buf = torch.full((guard + len(ref) + guard,), fill, dtype=torch.int32, device=dev)
    body = buf[guard:guard + len(ref)]
    assert body.data_ptr() % 16 == 0
    nv.check(nv.lib().dc_step_loc_build(ft.ref(), plan.nbr.shape[0], ptr(body), stream_ptr()), 'dc_step_loc_build')
    got = buf.cpu().numpy()
    assert (got[:guard] == fill).all() and (got[guard + len(ref):] == fill).all(), 'nothing outside the table`s own range'
    got = got[guard:guard + len(ref)].view(np.uint32)
    # every block's words fill exactly the bytes its rows of `loc` occupy: the reference places them there block by block
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], ref[bad[:8]])
    if name == 'k10':
        assert ((ref & 0xFFFF) == 0xFFFF).any() and ((ref >> 16) == 0xFFFF).any(), 'empty slots in both halves, kept as they are'


@pytest.mark.parametrize('name,n_terms', CASES)
def test_step_loc_option_and_generic_kernel_give_the_same_bytes(dev, name, n_terms):
    from depth_correction_amd import _native as nv
    plan, poses, k = _sequences(dev)[name]
    setv = lambda o, v: nv.check(nv.lib().dc_set_option(o, v), 'dc_set_option')
    assert plan.use_step_loc and plan.step_hdr is not None
    try:
        plan.clear_status()
        new = _run(plan, poses, n_terms, dev)
        setv(11, 1)
        option = _run(plan, poses, n_terms, dev)                       # (the plan still passes the words: the launch ignores them)
        setv(11, 0)
        plan.use_step_loc = False
        cleared = _run(plan, poses, n_terms, dev)
        plan.use_step_loc = True
        setv(6, 7)
        generic = _run(plan, poses, n_terms, dev)
    finally:
        setv(11, 0)
        setv(6, 1)
        plan.use_step_loc = True
    assert new['step_loc'] and new['step_loc'] == plan._step_loc[1].data_ptr() and option['step_loc'] == new['step_loc']
    assert not cleared['step_loc']
    assert _holds(plan._step_loc[1], _pack_reference(plan))
    hdr = plan.step_hdr.cpu().numpy()
    tile = 512 if int(hdr[(hdr[:, 5] & 1) == 0, 3].max()) <= 512 else 768
    for r in (new, option, cleared):
        assert r['kernel'] == 'consistency_step_q32_kernel<%d, %d, %d>' % (k, n_terms, tile), r['kernel']
    assert generic['kernel'].startswith('consistency_step_basis_kernel<q32, %d, %d, ' % (k, n_terms)), generic['kernel']
    for r in (new, option, cleared, generic):
        assert r['status'] == 0
        assert np.isfinite(r['eval']).all() and np.isfinite(r['steps']).all() and np.isfinite(r['w']).all()
    assert new['eval'][1] == plan.count > 0
    assert not np.array_equal(new['steps'][1], new['steps'][-1])                      # the chain moved the weights
    assert new['first'].tobytes() == new['eval'].tobytes(), 'the same key without and with the packed positions'
    for what, other in (('option 11', option), ('cleared', cleared), ('generic', generic)):
        for key in ('first', 'eval', 'steps', 'w'):
            print('%s P=%d %s %s: max |difference| = %.3g' % (name, n_terms, what, key, np.abs(new[key] - other[key]).max()))
            assert new[key].tobytes() == other[key].tobytes(), (name, n_terms, what, key, new[key], other[key])


def test_lifetime_of_the_packed_positions(dev):
    from depth_correction_amd.plan import SequencePlan, SequenceTrainer
    _sequences(dev)
    plan, poses = SequencePlan(*_args['k4']), _args['k4'][1]              # a plan of its own: nothing evaluated yet
    w = torch.tensor(W0[:2], dtype=torch.float64, device=dev)
    e = torch.tensor(E0[:2], dtype=torch.float64, device=dev)
    P12 = plan.poses12(poses).clone()
    d = plan.desc(2)
    # ---- one evaluation per key: nothing is built
    for i in range(3):
        e.add_(0.01)
        _eval(plan, w, e, P12, dev)
        assert plan._step_loc is None and not d.step_loc
    # ---- the second evaluation of a key builds it, once
    first = _eval(plan, w, e, P12, dev)
    assert plan._step_loc is not None and d.step_loc == plan._step_loc[1].data_ptr()
    words = plan._step_loc[1]
    at = words.data_ptr()
    ref = _pack_reference(plan)
    assert _holds(words, ref)
    # ---- new weights, new exponents, new poses: the same tensor, not written again
    w.mul_(1.5)
    moved = _eval(plan, w, e, P12, dev)
    assert moved.tobytes() != first.tobytes()
    e.mul_(1.1)
    _eval(plan, w, e, P12, dev)
    assert plan._basis[4] is None, 'the row copy went with the basis rows'
    P12[:, 3] += 0.003
    _eval(plan, w, e, P12, dev)
    _eval(plan, w, e, P12, dev)
    assert plan._step_loc[1] is words and words.data_ptr() == at and d.step_loc == at
    before = _eval(plan, w, e, P12, dev)
    # ---- another table object: dropped, and rebuilt by the next evaluation that has a row copy
    attr = 'fwd_table_loss' if plan.fwd_table_loss is not None else 'fwd_table'
    old = getattr(plan, attr)
    try:
        setattr(plan, attr, copy.copy(old))
        after = _eval(plan, w, e, P12, dev)
        assert plan._step_loc is not None and plan._step_loc[0] is getattr(plan, attr) and plan._step_loc[1] is not words
        assert d.step_loc == plan._step_loc[1].data_ptr()
        assert _holds(plan._step_loc[1], ref)
        assert after.tobytes() == before.tobytes()
    finally:
        setattr(plan, attr, old)
    assert plan.status_bits() == 0
    # ---- a trainer over two plans passes both plans' words
    other, poses2, _ = _sequences(dev)['k16']
    tr = SequenceTrainer([plan, other], W0[:2], E0[:2], [poses, poses2], lr=1e-3, chained=True)
    for _ in range(3):
        tr.step()
    tr.flush()
    torch.cuda.synchronize()
    for p in (plan, other):
        assert p._step_loc is not None and p.desc(2).step_loc == p._step_loc[1].data_ptr(), 'both plans step with their packed positions'
        assert _holds(p._step_loc[1], _pack_reference(p))
    assert np.isfinite(tr.w.cpu().numpy()).all() and plan.status_bits() == 0 and other.status_bits() == 0
