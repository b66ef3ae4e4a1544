"""Which kernels a sequence evaluation runs, on the host (no GPU): dc_choose_route of csrc/dc_cons_route.h -- what sequence_eval_impl
(dc_sequence_eval, dc_sequence_step*, the chained and linked steps) runs before it launches anything -- through libdc_hostcheck.so.

The descriptors are ctypes structures of depth_correction_amd._native with dummy non-null pointers: the decision reads scalars and
whether pointers are null, never what they point to.  Every expected value below was written down from sequence_eval_impl as it stood
before the decision moved into the header (the conditions are quoted where they bind), not taken from the function under test.

The base case: a float32 cloud (q32 points), k = 10, two weights, a [rows, K] slots table with own_base whose longest list is 300 rows,
basis rows, block headers, a mask, want_grad only, no transposed lists -> consistency_step_q32_kernel<10, 2, 512>."""
import ctypes

import pytest

from helpers import hostcheck_lib

EMPTY, STEP_RAGGED, STEP_Q32, STEP_BASIS, STEP_SLOTS, TWO_PASS, POSE, GENERAL = range(8)
OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_BACKWARD_TABLES = 0, -1, -3, -4, -5
F32, F64, Q32 = 0, 1, 2
SLOTS, RUNS = 0, 1
FIELDS = ('kind', 'f64', 'k', 'P', 'cap', 'six', 'round2', 'table_loss', 'use_hdr', 'max_rows', 'lds_fwd', 'rows_fwd', 'lds_bwd', 'rows_bwd',
          'grouped', 'n_terms', 'n_acc', 'n_red', 'n_rows', 'g_blocks', 'rows', 'grid')
OPTIONS = ('no_tab', 'fwd_generic', 'no_basis', 'two_pass', 'step_var', 'pose_three_pass', 'step_six')
PTR = 0x1000                 # any non-null value: nothing is dereferenced
N = 3 * 256 + 37             # four blocks -> 8 after the rounding to the XCDs, 32 partial rows


def route_lib():
    """libdc_hostcheck.so with the chooser's exports (rebuilt when the library at hand predates them)."""
    import __graft_entry__ as ge
    lib = hostcheck_lib()
    if not hasattr(lib, 'dc_host_choose_route'):      # a library from before the export
        ge.build()
        lib = hostcheck_lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    lib.dc_host_choose_route.restype = i
    lib.dc_host_choose_route.argtypes = [vp] + 7 * [i] + [vp, vp]
    lib.dc_host_use_table.restype = i
    lib.dc_host_use_table.argtypes = [vp] + 5 * [i] + [ctypes.c_int64, vp]
    return lib


@pytest.fixture(scope='module')
def lib():
    return route_lib()


def slots_table(max_rows=300, **kw):
    """A [rows, K] forward table with own_base; kw overrides fields (ragged=True: a packed table from CSR lists with row_ptr)."""
    from depth_correction_amd._native import BlockTableDesc
    ragged = kw.pop('ragged', False)
    f = dict(blk_ptr=PTR, blk_ids=PTR, slot_ptr=PTR, loc=PTR, max_rows=max_rows, layout=SLOTS, run_ptr=None, own_base=PTR,
             packed=1 if ragged else 0, row_ptr=PTR if ragged else None)
    f.update(kw)
    return BlockTableDesc(**f)


def runs_table(max_rows=300):
    from depth_correction_amd._native import BlockTableDesc
    return BlockTableDesc(blk_ptr=PTR, blk_ids=PTR, slot_ptr=None, loc=PTR, max_rows=max_rows, layout=RUNS, run_ptr=PTR)


def partials_count(n, n_terms, n_scans):
    rows = ((n + 255) // 256 + 7) // 8 * 8 * 4
    return rows * (2 + 2 * n_terms + 12 * n_scans) + 2 * (2 + n_terms) * rows


def route(lib, want=(1, 0, 0), has=(1, 1, 1), chained=0, opts=None, short=0, csr=False, **kw):
    """(status, {field: value}) for the base descriptor with fields overridden by kw.  Tables are given as structures (fwd_table, bwd_table,
    fwd_table_loss, pose_table=True); csr: the transposed lists are there; short: doubles missing from partials_count."""
    from depth_correction_amd._native import PoseTableDesc, SequenceDesc
    f = dict(n=N, k=10, n_scans=5, dtype=F32, point_fmt=Q32, dirs=PTR, depth=PTR, inc=PTR, scan_id=PTR, nbr=PTR, mask=PTR, x=PTR, rec=PTR,
             partials=PTR, model_kind=1, n_terms=2, fwd_table=slots_table(), basis=PTR, step_hdr=PTR)
    if csr:
        f.update(csr_ptr=PTR, csr_src=PTR)
    f.update(kw)
    keep = []
    for name in ('fwd_table', 'bwd_table', 'fwd_table_loss'):
        if f.get(name) is not None:
            keep.append(f[name])
            f[name] = ctypes.addressof(f[name])
    if f.get('pose_table'):
        keep.append(PoseTableDesc(blk_ptr=PTR, ids=PTR, loc=PTR, own_pos=PTR, row_seg=PTR, row_scan=PTR))
        f['pose_table'] = ctypes.addressof(keep[-1])
    qparams = f.pop('qparams', (0.0, 0.0, 0.0, 1e-4))
    d = SequenceDesc(**f)
    d.qparams[:] = qparams
    if 'partials_count' not in kw:
        d.partials_count = partials_count(d.n, 0 if d.model_kind == 0 else d.n_terms, d.n_scans) - short
    o = dict(no_tab=0, fwd_generic=0, no_basis=0, two_pass=0, step_var=1, pose_three_pass=0, step_six=0)
    o.update(opts or {})
    options = (ctypes.c_int * 7)(*[o[name] for name in OPTIONS])
    out = (ctypes.c_int64 * len(FIELDS))()
    rc = lib.dc_host_choose_route(ctypes.addressof(d), has[0], has[1], has[2], want[0], want[1], want[2], chained, ctypes.addressof(options),
                                  ctypes.addressof(out))
    return rc, dict(zip(FIELDS, out))


def check(got, rc=OK, **expect):
    status, r = got
    assert status == rc, (status, r)
    for key, value in expect.items():
        assert r[key] == value, (key, r[key], value, r)


def test_base(lib):
    check(route(lib), kind=STEP_Q32, f64=0, k=10, P=2, cap=512, six=0, round2=0, table_loss=0, use_hdr=1, max_rows=300, lds_fwd=300 * 32,
          rows_fwd=300, n_terms=2, n_acc=2 * 2 + 12 * 5, n_red=4, n_rows=N, g_blocks=8, rows=32, grid=8)


@pytest.mark.parametrize('rows, kind, cap', [(512, STEP_Q32, 512), (513, STEP_Q32, 768), (768, STEP_Q32, 768), (769, STEP_BASIS, 0)])
def test_tile(lib, rows, kind, cap):
    """rows_s <= 512: the 512 build, <= 768: the 768 build, else consistency_step_basis_kernel (its tile is dynamic LDS)."""
    check(route(lib, fwd_table=slots_table(rows)), kind=kind, cap=cap, k=10, P=2, use_hdr=int(kind == STEP_Q32), lds_fwd=rows * 32, rows_fwd=rows,
          max_rows=rows)


@pytest.mark.parametrize('n_terms, row_bytes, last', [(3, 48, 1280), (2, 32, 1920), (1, 32, 1920)])
def test_tile_limit(lib, n_terms, row_bytes, last):
    """One pass while rows x StepRow bytes fit 60 KB; one row more and the basis form needs the backward table (two passes)."""
    check(route(lib, n_terms=n_terms, fwd_table=slots_table(last)), kind=STEP_BASIS, P=n_terms, lds_fwd=last * row_bytes, rows_fwd=last)
    assert last * row_bytes == 60 * 1024
    check(route(lib, n_terms=n_terms, fwd_table=slots_table(last + 1)), rc=ERR_BACKWARD_TABLES)
    check(route(lib, n_terms=n_terms, fwd_table=slots_table(last + 1), csr=True), kind=GENERAL)
    check(route(lib, n_terms=n_terms, fwd_table=slots_table(last + 1), csr=True, bwd_table=runs_table()), kind=TWO_PASS, P=n_terms, k=10,
          lds_fwd=(last + 1) * 16, rows_fwd=last + 1, lds_bwd=301 * 32, rows_bwd=301)


def test_table_size(lib):
    """Positions are 16 x row in 16 bits: a table whose longest list has 0xFFF rows is unusable whatever the LDS limit (here the backward's:
    runs, 32-byte records, one extra row, 128 KB)."""
    out = (ctypes.c_int64 * 2)()
    for rows, ok in ((4094, 1), (4095, 0)):
        t = runs_table(rows)
        assert (rows + 1) * 32 <= 128 * 1024
        assert lib.dc_host_use_table(ctypes.addressof(t), 0, RUNS, 4, 32, 1, 128 * 1024, ctypes.addressof(out)) == ok
        if ok:
            assert list(out) == [4095 * 32, 4095]
    t = runs_table(100)
    assert lib.dc_host_use_table(ctypes.addressof(t), 1, RUNS, 4, 32, 1, 128 * 1024, ctypes.addressof(out)) == 0       # dc_set_option(0, 1)
    assert lib.dc_host_use_table(ctypes.addressof(t), 0, SLOTS, 4, 32, 1, 128 * 1024, ctypes.addressof(out)) == 0      # the other layout
    assert lib.dc_host_use_table(ctypes.addressof(t), 0, RUNS, 3, 32, 1, 128 * 1024, ctypes.addressof(out)) == 0       # unpadded rows
    assert lib.dc_host_use_table(None, 0, RUNS, 4, 32, 1, 128 * 1024, ctypes.addressof(out)) == 0
    # in a sequence both sizes are beyond the forward's 60 KB of 16-byte rows: no basis form
    for rows in (4094, 4095):
        check(route(lib, fwd_table=slots_table(rows), csr=True), kind=GENERAL)


@pytest.mark.parametrize('k', [4, 8, 16])
def test_fixed_k(lib, k):
    check(route(lib, k=k), kind=STEP_Q32, k=k, P=2, cap=512)


def test_other_k(lib):
    check(route(lib, k=5), kind=STEP_SLOTS, k=0, P=2, f64=0, lds_fwd=300 * 32, rows_fwd=300)
    check(route(lib, opts=dict(fwd_generic=1)), kind=STEP_SLOTS, k=0, P=2)
    check(route(lib, k=5, dtype=F64, point_fmt=F64), kind=STEP_SLOTS, k=0, f64=1, lds_fwd=300 * 48)


def test_terms(lib):
    for p in (1, 2, 3):
        check(route(lib, n_terms=p), kind=STEP_Q32, P=p, cap=512, lds_fwd=300 * (48 if p == 3 else 32), n_acc=2 * p + 60, n_red=2 * p)
    check(route(lib, n_terms=0, csr=True), kind=GENERAL, n_terms=0, n_acc=60)
    check(route(lib, n_terms=0), rc=ERR_BACKWARD_TABLES)
    check(route(lib, model_kind=0, csr=True), kind=GENERAL, n_terms=0, n_acc=60, n_red=0)
    # more than three weights: the basis form in two passes, through the <.., 0> instantiations
    check(route(lib, n_terms=4, csr=True, bwd_table=runs_table()), kind=TWO_PASS, P=0, k=10, n_terms=4, n_red=8)
    check(route(lib, n_terms=4, k=5, csr=True, bwd_table=runs_table()), kind=TWO_PASS, P=0, k=0)


def test_format(lib):
    check(route(lib, dtype=F64, point_fmt=F64), kind=STEP_BASIS, f64=1, k=10, P=2, round2=0, use_hdr=0, lds_fwd=300 * 48, rows_fwd=300)
    check(route(lib, dtype=F32, point_fmt=F32, csr=True), kind=GENERAL)
    check(route(lib, dtype=F32, point_fmt=F32), rc=ERR_BACKWARD_TABLES)
    check(route(lib, qparams=(0.0, 0.0, 0.0, 0.0)), rc=ERR_ARG)                       # make_qparams: the grid step of q32 points


def test_header(lib):
    check(route(lib, step_hdr=None), kind=STEP_BASIS, k=10, P=2, use_hdr=0, f64=0)
    # a compact centre list: the kernel takes the centres by index, a header that names own rows does not describe that
    check(route(lib, centre_idx=PTR, n_centres=500), kind=STEP_BASIS, use_hdr=0, n_rows=500, g_blocks=8, grid=8, rows=32)
    check(route(lib, centre_idx=PTR, n_centres=500, fwd_table=slots_table(own_base=None)), kind=STEP_Q32, use_hdr=1, n_rows=500)


def test_loss_table(lib):
    """fwd_table_loss is tried first (mask, no centre list, want_grad only, basis, one to three weights); the header belongs to it."""
    loss = dict(fwd_table_loss=slots_table(200), fwd_rows_active_loss=150, fwd_rows_active=250)
    check(route(lib, **loss), kind=STEP_Q32, table_loss=1, use_hdr=1, max_rows=200, lds_fwd=200 * 32, rows_fwd=200, cap=512)
    check(route(lib, blk_skip=PTR, **loss), kind=STEP_Q32, table_loss=1, use_hdr=1, max_rows=150, rows_fwd=150)
    # not tried: no mask, a centre list, other gradients, no gradient -> fwd_table, and the header (built from the other table) is not used
    check(route(lib, mask=None, **loss), kind=STEP_BASIS, table_loss=0, use_hdr=0, max_rows=300, rows_fwd=300)
    check(route(lib, centre_idx=PTR, n_centres=N, **loss), kind=STEP_BASIS, table_loss=0, use_hdr=0)
    check(route(lib, want=(0, 0, 0), **loss), kind=TWO_PASS, table_loss=0, max_rows=300)
    # too long for the tile: DC_ERR_UNSUPPORTED from that attempt alone falls through to fwd_table ...
    for rows in (1921, 4000):
        check(route(lib, csr=True, fwd_table_loss=slots_table(rows)), kind=STEP_BASIS, table_loss=0, use_hdr=0, max_rows=300, lds_fwd=300 * 32)
        # ... but the attempt asks for the transposed lists before it gives up, as every pass does
        check(route(lib, fwd_table_loss=slots_table(rows)), rc=ERR_BACKWARD_TABLES)
    check(route(lib, opts=dict(two_pass=1), **loss), rc=ERR_BACKWARD_TABLES)
    check(route(lib, short=1, **loss), rc=ERR_WORKSPACE)
    check(route(lib, qparams=(0.0, 0.0, 0.0, -1.0), **loss), rc=ERR_ARG)
    check(route(lib, chained=1, **loss), kind=STEP_Q32, table_loss=1, grid=16)


def test_active_rows(lib):
    """blk_skip && mask && !centre_idx && 0 < fwd_rows_active < max_rows: the tile is sized by the blocks that are not skipped."""
    act = dict(fwd_table=slots_table(900), blk_skip=PTR, fwd_rows_active=200)
    check(route(lib, **act), kind=STEP_Q32, cap=512, max_rows=200, lds_fwd=200 * 32, rows_fwd=200)
    check(route(lib, mask=None, **act), kind=STEP_BASIS, max_rows=900, lds_fwd=900 * 32, rows_fwd=900)
    check(route(lib, centre_idx=PTR, n_centres=N, **act), kind=STEP_BASIS, max_rows=900, rows_fwd=900)
    check(route(lib, fwd_table=slots_table(900), fwd_rows_active=200), kind=STEP_BASIS, max_rows=900)                  # no blk_skip
    check(route(lib, fwd_table=slots_table(900), blk_skip=PTR, fwd_rows_active=0), kind=STEP_BASIS, max_rows=900)
    check(route(lib, fwd_table=slots_table(900), blk_skip=PTR, fwd_rows_active=900), kind=STEP_BASIS, max_rows=900)


RAGGED_CAPS = [(300, 1024), (1024, 1024), (1025, 1280), (1280, 1280), (1281, 1600), (1600, 1600), (1601, 2048), (2048, 2048), (2049, 2560),
               (2560, 2560), (2561, 4096), (4094, 4096)]


@pytest.mark.parametrize('rows, cap', RAGGED_CAPS)
@pytest.mark.parametrize('n_terms', [1, 2])
def test_ragged_caps(lib, rows, cap, n_terms):
    check(route(lib, n_terms=n_terms, fwd_table=slots_table(rows, ragged=True)), kind=STEP_RAGGED, P=n_terms, cap=cap, k=0, lds_fwd=cap * 32,
          rows_fwd=cap, max_rows=rows, use_hdr=0)


@pytest.mark.parametrize('rows, cap', [(300, 1024), (1024, 1024), (1025, 1600), (1600, 1600), (1601, 2560), (2560, 2560)])
def test_ragged_caps_three_weights(lib, rows, cap):
    check(route(lib, n_terms=3, fwd_table=slots_table(rows, ragged=True)), kind=STEP_RAGGED, P=3, cap=cap, lds_fwd=cap * 48, rows_fwd=cap)


def test_ragged_limits(lib):
    check(route(lib, n_terms=3, fwd_table=slots_table(2561, ragged=True), csr=True), kind=GENERAL)
    check(route(lib, n_terms=3, fwd_table=slots_table(2561, ragged=True)), rc=ERR_BACKWARD_TABLES)
    check(route(lib, fwd_table=slots_table(4097, ragged=True), csr=True), kind=GENERAL)
    # the active rows count for the ragged tile as well
    check(route(lib, fwd_table=slots_table(3000, ragged=True), blk_skip=PTR, fwd_rows_active=1100), kind=STEP_RAGGED, cap=1280, max_rows=1100)
    # not ragged: dc_set_option(6, 8), (0, 1), a centre list, no row_ptr, float64 clouds
    check(route(lib, fwd_table=slots_table(ragged=True), opts=dict(step_var=8)), kind=STEP_BASIS, k=10, P=2, round2=0)
    check(route(lib, fwd_table=slots_table(ragged=True), opts=dict(no_tab=1), csr=True), kind=GENERAL)
    check(route(lib, fwd_table=slots_table(ragged=True), centre_idx=PTR, n_centres=N), kind=STEP_BASIS)
    check(route(lib, fwd_table=slots_table(ragged=True, row_ptr=None)), kind=STEP_Q32)
    check(route(lib, fwd_table=slots_table(ragged=True), dtype=F64, point_fmt=F64), kind=STEP_BASIS, f64=1)
    check(route(lib, fwd_table=slots_table(ragged=True), k=5), kind=STEP_RAGGED, k=0)
    check(route(lib, fwd_table=slots_table(ragged=True), chained=1), kind=STEP_RAGGED, grid=16)


def test_step_var(lib):
    check(route(lib, opts=dict(step_var=0)), kind=STEP_BASIS, f64=0, k=10, P=2, round2=1)
    check(route(lib, opts=dict(step_var=0), dtype=F64, point_fmt=F64), kind=STEP_BASIS, f64=1, k=10, P=2, round2=1)
    check(route(lib, opts=dict(step_var=0), k=4), kind=STEP_BASIS, k=4, P=2, round2=0)
    check(route(lib, opts=dict(step_var=0), n_terms=3), kind=STEP_BASIS, k=10, P=3, round2=0)
    check(route(lib, opts=dict(step_var=0), n_terms=1), kind=STEP_BASIS, k=10, P=1, round2=0)
    check(route(lib, opts=dict(step_var=7)), kind=STEP_BASIS, f64=0, k=10, P=2, round2=0, use_hdr=0)


def test_step_six(lib):
    six = dict(opts=dict(step_six=1))
    check(route(lib, **six), kind=STEP_Q32, cap=512, six=1)
    check(route(lib, n_terms=1, k=16, **six), kind=STEP_Q32, cap=512, six=1, k=16, P=1)
    check(route(lib, n_terms=3, **six), kind=STEP_Q32, cap=512, six=0, P=3)
    check(route(lib, fwd_table=slots_table(600), **six), kind=STEP_Q32, cap=768, six=0)


def test_two_pass(lib):
    """dc_set_option(4, 1): forward and backward kernels, the backward's records within 44 KB: (rows + 1) x 32 bytes (64 for float64)."""
    two = dict(opts=dict(two_pass=1), csr=True)
    check(route(lib, bwd_table=runs_table(1407), **two), kind=TWO_PASS, k=10, P=2, f64=0, lds_fwd=300 * 16, rows_fwd=300, lds_bwd=1408 * 32,
          rows_bwd=1408, n_red=4)
    assert 1408 * 32 == 44 * 1024
    check(route(lib, bwd_table=runs_table(1408), **two), kind=GENERAL)
    check(route(lib, bwd_table=runs_table(703), dtype=F64, point_fmt=F64, **two), kind=TWO_PASS, f64=1, lds_fwd=300 * 32, lds_bwd=704 * 64)
    check(route(lib, bwd_table=runs_table(704), dtype=F64, point_fmt=F64, **two), kind=GENERAL)
    check(route(lib, **two), kind=GENERAL)                                              # no backward table
    check(route(lib, bwd_table=slots_table(), **two), kind=GENERAL)                     # not a run table
    check(route(lib, bwd_table=runs_table(), opts=dict(two_pass=1)), rc=ERR_BACKWARD_TABLES)


def test_general_switches(lib):
    check(route(lib, opts=dict(no_basis=1), csr=True), kind=GENERAL, n_rows=N, g_blocks=8, rows=32, n_red=4)
    check(route(lib, opts=dict(no_tab=1), csr=True), kind=GENERAL)
    check(route(lib, opts=dict(no_basis=1)), rc=ERR_BACKWARD_TABLES)
    check(route(lib, basis=None, csr=True), kind=GENERAL)
    check(route(lib, has=(0, 1, 1), csr=True), kind=GENERAL)                            # no weights
    check(route(lib, want=(1, 1, 0), csr=True), kind=GENERAL, n_red=4)                  # exponent gradients
    check(route(lib, fwd_table=None, csr=True), kind=GENERAL)


def test_forward_only(lib):
    check(route(lib, want=(0, 0, 0)), kind=TWO_PASS, k=10, P=2, n_red=0, lds_fwd=300 * 16, rows_fwd=300, lds_bwd=0)
    check(route(lib, want=(0, 0, 0), k=5, n_terms=3), kind=TWO_PASS, k=0, P=3)
    check(route(lib, want=(0, 0, 0), opts=dict(no_basis=1)), kind=GENERAL, n_red=0)


@pytest.mark.parametrize('k', [4, 8, 10, 16])
@pytest.mark.parametrize('n_terms', [1, 2])
def test_pose(lib, k, n_terms):
    check(route(lib, want=(1, 0, 1), k=k, n_terms=n_terms, pose_table=True, local_basis=PTR), kind=POSE, k=k, P=n_terms, f64=0,
          n_red=2 * n_terms + 60, n_acc=2 * n_terms + 60, rows=32)


NOT_POSE = [dict(n_terms=3), dict(vps=PTR), dict(centre_idx=PTR, n_centres=N), dict(n_scans=33), dict(want=(1, 1, 1)),
            dict(opts=dict(pose_three_pass=1)), dict(k=5), dict(pose_table=None), dict(local_basis=None), dict(has=(0, 1, 1)),
            dict(dtype=F64, point_fmt=F64)]


@pytest.mark.parametrize('case', range(len(NOT_POSE)))
def test_pose_not_eligible(lib, case):
    kw = dict(want=(1, 0, 1), pose_table=True, local_basis=PTR)
    kw.update(NOT_POSE[case])
    check(route(lib, csr=True, **kw), kind=GENERAL, grouped=0)
    check(route(lib, **kw), rc=ERR_BACKWARD_TABLES)
    # the plan's layout (points grouped by scan inside every block): the backward leaves the pose slots row-major
    check(route(lib, csr=True, scan_seg=PTR, **kw), kind=GENERAL, grouped=1)
    check(route(lib, csr=True, scan_seg=PTR, lane_perm=PTR, **kw), kind=GENERAL, grouped=0)


def test_pose_scans(lib):
    kw = dict(want=(1, 0, 1), pose_table=True, local_basis=PTR)
    check(route(lib, n_scans=32, **kw), kind=POSE)
    check(route(lib, n_scans=64, csr=True, scan_seg=PTR, **kw), kind=GENERAL, grouped=1)
    check(route(lib, n_scans=65, csr=True, scan_seg=PTR, **kw), kind=GENERAL, grouped=0)


def test_chained(lib):
    """A chain exists for the one-pass kernels only (eight leading blocks in front of the grid); every other route is
    DC_ERR_UNSUPPORTED -- after the check for the transposed lists, as in every call."""
    check(route(lib, chained=1), kind=STEP_Q32, grid=16, g_blocks=8)
    check(route(lib, chained=1, opts=dict(step_var=7)), kind=STEP_BASIS, grid=16)
    check(route(lib, chained=1, k=5), kind=STEP_SLOTS, grid=16)
    check(route(lib, chained=1, dtype=F64, point_fmt=F64), kind=STEP_BASIS, f64=1, grid=16)
    check(route(lib, chained=1, opts=dict(two_pass=1), csr=True, bwd_table=runs_table()), rc=ERR_UNSUPPORTED)
    check(route(lib, chained=1, opts=dict(no_basis=1), csr=True), rc=ERR_UNSUPPORTED)
    check(route(lib, chained=1, dtype=F32, point_fmt=F32, csr=True), rc=ERR_UNSUPPORTED)
    check(route(lib, chained=1, n_terms=4, csr=True, bwd_table=runs_table()), rc=ERR_UNSUPPORTED)
    check(route(lib, chained=1, opts=dict(no_basis=1)), rc=ERR_BACKWARD_TABLES)


def test_errors(lib):
    check(route(lib, n=0), kind=EMPTY, n_acc=64)
    check(route(lib, n=0, partials_count=0), kind=EMPTY)
    check(route(lib, short=1), rc=ERR_WORKSPACE)
    check(route(lib, short=0), kind=STEP_Q32)
    check(route(lib, centre_idx=PTR, n_centres=N + 1), rc=ERR_ARG)
    check(route(lib, centre_idx=PTR, n_centres=-1), rc=ERR_ARG)
    check(route(lib, centre_idx=PTR, n_centres=N), kind=STEP_BASIS)
    check(route(lib, has=(1, 0, 1)), rc=ERR_ARG)                                        # poses
    check(route(lib, has=(1, 1, 0)), rc=ERR_ARG)                                        # out
    check(route(lib, partials=None), rc=ERR_ARG)
    i = ctypes.c_int
    assert lib.dc_host_choose_route(None, 1, 1, 1, 1, 0, 0, 0, ctypes.addressof((i * 7)()), ctypes.addressof((ctypes.c_int64 * 22)())) == ERR_ARG
