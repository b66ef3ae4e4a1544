"""The DEVICE arm of the eigen-solvers (csrc/dc_eig3.h: raw v_rcp_f64 / v_rsq_f64 with zero or one Newton step, __cosf, raw
v_sqrt_f32 / v_rcp_f32) against the exact reference of eig_reference.py (mpmath, 60 digits) on designed spectra (eig_cases.py):
every kernel that calls a solver, on neighbourhoods that sit on every branch of it -- the direct path, the second Newton step
(half >= 0.9), the deflation paths (half >= 0.9 in eig3_smallest_r2, >= 0.999 in eig3_smallest_unit), either sign of det(B) in
eig3_sym / eig3_sym_v2, tiny and huge scales -- and with lanes of one wavefront on different branches ('mixed').

The bound is the solvers' contract, the one test_hostcheck.py holds the host arm to: |lam_dev - lam_ref| <= 1e-14 lam_max per
neighbourhood, plus one float32 ulp of the value where the kernel stores float32; test_eig_reference_host.py shows that the plain
LAPACK route meets it with a factor seven to spare.  Which test covers which solver:

    test_features_spectra      eig3_sym (features_fwd_kernel), eig3_sym_v2 (features_fwd_tile_kernel)
    test_consistency_spectra   eig3_sym (want_eigvals), eig3_smallest -> eig3_smallest_v2 -> eig3_smallest_unit<true>
    test_step_kernels          eig3_smallest_unit<true> (float64 points), eig3_smallest_unit<false> (q32 points), eig3_smallest_r2
    test_landscape             eig3_smallest (no bounds), eig3_sym_v2 (with an eigenvalue bound)

Every test prints the largest error it saw, in units of its bound's scale."""
import numpy as np
import pytest
import torch

import dc_oracle as O
import eig_cases as cases
import eig_reference as R
from helpers import t, npy
from eig_reference import ALL, offset_of, check_v0, loss_bound

pytestmark = pytest.mark.gpu

EPS = 1e-14                  # the solver contract (test_hostcheck.py), in units of lam_max
EPS_Q32 = 1e-11              # eig3_smallest_unit<false>: "~1e-12 of the spread" (dc_eig3.h), a factor ten for the "~"
ULP32 = 2.0 ** -23
SEQ_FAMILIES = cases.UNIT_FAMILIES + ('mixed', 'exact_rank')
SEPARATED = ('generic', 'planar', 'edge', 'threshold', 'threshold_unit', 'double_hi')

# the branches a family must populate (counted from the reference spectrum, see branches()): sign of det(B) for eig3_sym / _v2
# ('neg', 'zero', 'pos'), and the three paths of eig3_smallest_unit ('direct', 'newton2', 'deflate'; eig3_smallest_r2 deflates on
# 'newton2' and 'deflate')
CLAIMS = {'generic': ('neg', 'pos', 'direct', 'newton2'), 'planar': ('neg', 'direct'), 'needle': ('pos', 'deflate'),
          'double_lo': ('pos', 'deflate'), 'double_hi': ('neg', 'direct'), 'isotropic': (), 'near_isotropic': (),
          'edge': ('pos', 'direct', 'newton2', 'deflate'), 'sign_switch': ('zero', 'direct'), 'threshold': ('pos', 'direct', 'newton2'),
          'threshold_unit': ('pos', 'newton2', 'deflate'), 'tiny': ('neg', 'pos', 'direct', 'newton2'),
          'huge': ('neg', 'pos', 'direct', 'newton2'), 'mixed': ('neg', 'zero', 'pos', 'direct', 'newton2', 'deflate'),
          'exact_rank': ('pos', 'deflate')}


def branches(ref, k):
    """Neighbourhoods per branch, from half = cos(3 ang) of the reference spectrum, 1e-3 away from the thresholds 0 and 0.9 (the
    device computes half in float32: ~1e-6); above 0.999 the interval is itself 1e-3 wide: its upper half counts."""
    h = cases.half_of(ref['lam'])
    with np.errstate(invalid='ignore'):
        return dict(neg=int((h <= -1e-3).sum()), zero=int((np.abs(h) < 1e-3).sum()), pos=int((h >= 1e-3).sum()),
                    direct=int((h < 0.9 - 1e-3).sum()), newton2=int(((h >= 0.9 + 1e-3) & (h < 0.999 - 1e-3)).sum()),
                    deflate=int((h >= 0.9995).sum()))


def assert_claims(case, ref, k, kinds):
    """The family puts at least one neighbourhood on each branch of `kinds` it claims; 'mixed': some wavefront (64 consecutive
    centres) holds lanes on all of them at once."""
    got = branches(ref, k)
    for b in CLAIMS[case]:
        if b in kinds:
            assert got[b] >= 1, (case, b, got)
    if case == 'mixed':
        lam = ref['lam']
        waves = [branches({'lam': lam[i:i + 64]}, k) for i in range(0, len(lam), 64)]
        assert any(all(w[b] >= 1 for b in kinds) for w in waves), (case, kinds, waves)


SIGN, UNIT = ('neg', 'zero', 'pos'), ('direct', 'newton2', 'deflate')


def _lam_tol(ref, f32_out):
    lam = ref['lam']
    return EPS * lam[:, 2:3] + (ULP32 * np.abs(lam) if f32_out else 0.0)


def _worst(err, scale):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# (a) ops.features_fwd: eig3_sym_v2 in the tiled kernel, eig3_sym in the general one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ALL)
def test_features_spectra(dev, case, dtype):
    """mean / cov / eigvals / eigvecs of dc_features_fwd for k = 8, 10, 16, through features_fwd_tile_kernel (eig3_sym_v2) and,
    with dc_features_set_tiled(0), features_fwd_kernel (eig3_sym): ascending order, every eigenvalue within 1e-14 lam_max (+ a
    float32 ulp for float32 outputs), orthonormal eigenvectors (1e-12; float32 outputs: + 2 ulp, the rounding of the stored
    components), residual |C V - V lam| <= 1e-12 lam_max (float32: + 4 ulp), and for float64 outputs the eigenvector checks of
    test_hostcheck.py on v0."""
    from depth_correction_amd import ops, _native as nv
    from depth_correction_amd.plan import KernelTimer
    f32 = dtype == np.float32
    for k in (8, 10, 16):
        x, nbr, ref = R.reference(case, dtype, k, offset_of(case))
        assert_claims(case, ref, k, SIGN)
        xd, nd = t(x, dev), t(nbr, dev)
        lmax = ref['lam'][:, 2]
        for tiled in (1, 0):
            prev = nv.lib().dc_features_set_tiled(tiled)
            try:
                with KernelTimer(every=1) as timer:
                    f = ops.features_fwd(xd, nd, want=('mean', 'cov', 'eigvals', 'eigvecs'))
                    name = timer.kernels()['features_fwd']
            finally:
                nv.lib().dc_features_set_tiled(prev)
            assert name.startswith('features_fwd_tile_kernel' if tiled else 'features_fwd_kernel'), name
            lam, V = npy(f['eigvals']).astype(np.float64), npy(f['eigvecs']).astype(np.float64)
            assert np.all(np.diff(lam, axis=1) >= 0)
            err = np.abs(lam - ref['lam'])
            print('features %-15s %s k=%2d %-7s max |dlam| / lam_max = %.2e' % (case, np.dtype(dtype).name, k, 'tiled' if tiled else 'general',
                                                                               _worst(err.max(1), lmax)))
            assert np.all(err <= _lam_tol(ref, f32)), (k, tiled, _worst(err.max(1), lmax))
            assert np.abs(np.einsum('nji,njk->nik', V, V) - np.eye(3)).max() < 1e-12 + (2 * ULP32 if f32 else 0.0)
            res = np.abs(np.einsum('nij,njk->nik', ref['cov'], V) - V * lam[:, None, :]).max((1, 2))
            assert np.all(res <= (1e-12 + (4 * ULP32 if f32 else 0.0)) * lmax), _worst(res, lmax)
            scale = np.abs(x.astype(np.float64)).max() + np.sqrt(lmax.max())
            assert np.abs(npy(f['mean']) - ref['mean']).max() <= (ULP32 if f32 else 2.0 ** -50) * scale
            cerr = np.abs(npy(f['cov']).astype(np.float64) - ref['cov']).max((1, 2))
            assert np.all(cerr <= (EPS + (ULP32 if f32 else 0.0)) * lmax), _worst(cerr, lmax)
            if not f32:
                check_v0(V[:, :, 0], lam[:, 0], ref, norm_tol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# (b) ops.consistency_fwd: eig3_sym (want_eigvals) and eig3_smallest
# ---------------------------------------------------------------------------------------------------------------------
def _consistency_inputs(dev, case, fmt):
    """(points tensor, qfmt, neighbours, reference, rec -> v0) for fmt in f64 / f32 / q32.  q32: the sequence form of the cloud
    through ops.points_fwd with the format of its extent; the reference is computed from the grid points, decoded."""
    from depth_correction_amd import ops
    if fmt != 'q32':
        dtype = np.float64 if fmt == 'f64' else np.float32
        x, nbr, ref = R.reference(case, dtype, cases.K, offset_of(case))
        return t(x, dev), None, t(nbr, dev), ref
    s = R.sequence(case, np.float32)
    qfmt = ops.QFormat.for_extent(s['points'].min(0), s['points'].max(0))
    ps = ops.PointSet(t(s['vps'], dev), t(s['dirs'], dev), t(s['depth'], dev))
    xq = ops.points_fwd(ps, qfmt=qfmt)
    dec = np.asarray(qfmt.origin) + npy(xq)[:, :3].astype(np.float64) * qfmt.scale
    assert np.abs(dec - s['points']).max() <= 0.5 * qfmt.scale * 1.01
    return xq, qfmt, t(s['nbr'], dev), R.sequence_reference(case, np.float32, dec)


def _rec_v0(rec, fmt):
    r = npy(rec)
    if fmt == 'f64':
        return r[:, 4:7]
    return np.ascontiguousarray(r[:, 4:7]).view(np.float32).astype(np.float64)


# (q32: the sequence form of the clouds, one fixed-point format for the whole cloud -- no 'tiny' / 'huge')
@pytest.mark.parametrize('case,fmt', [(c, f) for c in ALL for f in ('f64', 'f32', 'q32') if f != 'q32' or c in SEQ_FAMILIES])
def test_consistency_spectra(dev, case, fmt):
    """dc_consistency_fwd, mask = None, the six loss variants, with want_eigvals (eig3_sym) and without (eig3_smallest), k = 10;
    then, on rows padded to four words, with a block table (consistency_fwd_fixed_kernel) and with dc_set_option(1, 1)
    (consistency_fwd_staged_kernel, the run-time slot loop); which kernel ran is asserted by name.  Per centre:

      eigvals    within 1e-14 lam_max (+ a float32 ulp where stored as float32), ascending
      v0 (rec)   the eigenvector checks of test_hostcheck.py wherever (lam1 - lam0) / lam_max > 1e-3, and | |v0| - 1 | < 1e-14.  Records
                 of float32 and q32 points hold v0 in float32 -- every component within half an ulp, the vector within
                 sqrt(3) 2^-24 < 0.87 ulp of the one computed --: | |v0| - 1 | < 2 ulp, the residual bound grows by one ulp
                 (|(C - lam0) dv| <= lam_max |dv|) and the alignment, taken of the normalised vector and so of second order in
                 the rounding, by ulp^2 (|dv|^2 / 2 < 0.4 ulp^2)
      pointwise  within the bound that |dlam_i| <= 1e-14 lam_max implies for the variant (eig_reference.loss_bound):
                 raw min-eigenvalue 1e-14 lam_max; trace 3e-14 lam_max; normalised l = lam0 / tc with tc = max(tr, 1e-6):
                 (1 + 3 l) 1e-14 lam_max / tc; relu changes nothing; sqrt: min(tol / sqrt(l_ref), sqrt(tol)), i.e. relative wherever
                 the value is above the tolerance; + a float32 ulp where stored as float32."""
    from depth_correction_amd import ops, _native as nv
    from depth_correction_amd.plan import KernelTimer
    x, qfmt, nbr, ref = _consistency_inputs(dev, case, fmt)
    n = len(ref['tr'])
    assert_claims(case, ref, cases.K, SIGN + UNIT)
    f32_out = fmt != 'f64'
    lmax = ref['lam'][:, 2]

    def check(fw, tag, loss, norm, sqrt, full, what):
        assert float(fw['sums'][1]) == n
        pw = npy(fw['pointwise']).astype(np.float64)
        tol = loss_bound(ref, norm, sqrt, loss, EPS, ULP32 if f32_out else 0.0)
        perr = np.abs(pw - ref[tag])
        print('consistency %-15s %s %-16s %-8s %-6s worst pointwise error / bound = %.3f' % (case, fmt, tag, 'eig3_sym' if full else 'smallest', what,
                                                                                            _worst(perr, tol)))
        assert np.all(perr <= tol), (tag, full, what, _worst(perr, tol))
        v0 = _rec_v0(fw['rec'], fmt)
        if full:
            lam = npy(fw['eigvals']).astype(np.float64)
            assert np.all(np.diff(lam, axis=1) >= 0)
            assert np.all(np.abs(lam - ref['lam']) <= _lam_tol(ref, f32_out)), _worst(np.abs(lam - ref['lam']).max(1), lmax)
            lam0 = lam[:, 0]
        else:
            lam0 = ref['lam'][:, 0]
        # (without the eigenvalue output the residual is taken about the reference's lam0: within 1e-14 lam_max of the device's)
        if fmt == 'f64':
            check_v0(v0, lam0, ref, norm_tol=1e-14)
        else:
            check_v0(v0, lam0, ref, norm_tol=2 * ULP32, store_ulp=ULP32)

    for tag, loss, norm, sqrt in R.VARIANTS:
        for full in (True, False):
            with KernelTimer(every=1) as timer:
                fw = ops.consistency_fwd(x, nbr, mask=None, loss=loss, normalization=norm, sqrt=sqrt, want_pointwise=True,
                                         want_eigvals=full, qfmt=qfmt)
                names = timer.kernels()
            assert names['consistency_fwd'].startswith('consistency_fwd_kernel<'), names
            check(fw, tag, loss, norm, sqrt, full, 'gather')
    # the LDS-staged kernels take padded rows of four words (q32 rows are)
    x4 = x if x.shape[1] == 4 else torch.cat([x, torch.zeros_like(x[:, :1])], 1).contiguous()
    table = ops.block_table(nbr=nbr)
    tag, loss, norm, sqrt = R.VARIANTS[1]
    for slots in (0, 1):
        nv.check(nv.lib().dc_set_option(1, slots), 'dc_set_option')
        try:
            for full in (True, False):
                with KernelTimer(every=1) as timer:
                    fw = ops.consistency_fwd(x4, nbr, mask=None, loss=loss, normalization=norm, sqrt=sqrt, want_pointwise=True,
                                             want_eigvals=full, qfmt=qfmt, table=table)
                    names = timer.kernels()
                assert names['consistency_fwd'].startswith('consistency_fwd_staged_kernel<' if slots else 'consistency_fwd_fixed_kernel<'), names
                check(fw, tag, loss, norm, sqrt, full, 'slots' if slots else 'table')
        finally:
            nv.check(nv.lib().dc_set_option(1, 0), 'dc_set_option')


# ---------------------------------------------------------------------------------------------------------------------
# (c), (d) the one-pass step kernels and the landscape kernel through a SequencePlan
# ---------------------------------------------------------------------------------------------------------------------
_plans = {}


def _plan(dev, case, dtype):
    """SequencePlan of the sequence form of a family (k = 10, ScaledPolynomial, raw min-eigenvalue loss, all-true mask, identity pose)
    with the reference of the points it materialises at w = 0; built once per (family, dtype)."""
    from depth_correction_amd import ops
    from depth_correction_amd.plan import SequencePlan
    key = (case, np.dtype(dtype).name)
    if key not in _plans:
        s = R.sequence(case, dtype)
        cloud = dict(vps=t(s['vps'], dev), dirs=t(s['dirs'], dev), depth=t(s['depth'], dev), inc_angles=t(s['inc'], dev),
                     mask=torch.ones(len(s['points']), dtype=torch.bool, device=dev))
        poses = torch.eye(4, dtype=torch.float64, device=dev)[None]
        nbr = t(s['nbr'], dev)
        plan = SequencePlan([cloud], poses, nbr, torch.ones(len(s['points']), dtype=torch.bool, device=dev), model_kind='ScaledPolynomial',
                            loss='min_eigval_loss', normalization=False, sqrt=False, spatial_sort=False)
        # (no Morton order: the groups stay where eig_cases put them, so that the wavefronts are the ones assert_claims looks at)
        assert plan.order is None and (plan.qfmt is None) == (dtype == np.float64)
        e = torch.tensor([2.0, 4.0], dtype=torch.float64, device=dev)
        w0 = torch.zeros(2, dtype=torch.float64, device=dev)
        P = plan.poses12(poses)
        xm = ops.points_fwd(plan.ps, P, 'ScaledPolynomial', w0, e, stride=4, qfmt=plan.qfmt)
        if plan.qfmt is not None:
            xm = torch.as_tensor(plan.qfmt.origin, dtype=torch.float64, device=dev) + xm[:, :3].double() * plan.qfmt.scale
        pts = npy(plan.unpermute(xm[:, :3]))
        if dtype == np.float64:
            assert np.array_equal(pts, s['points'])              # vps + depth * dirs has no rounding
        else:
            assert np.abs(pts - s['points']).max() <= 0.5 * plan.qfmt.scale * 1.01
        _plans[key] = dict(plan=plan, seq=s, e=e, w0=w0, P=P, poses=poses, pts=pts, ref=R.sequence_reference(case, dtype, pts))
    return _plans[key]


_STEP_FORMS = {       # name: (dtype, dc_set_option(6, .), prefix of the kernel's name, bound in lam_max per centre)
    'f64': (np.float64, 1, 'consistency_step_basis_kernel<double, 10, 2, kStepVar>', EPS),
    'q32': (np.float32, 1, 'consistency_step_q32_kernel<10, 2, ', EPS_Q32),
    'f64_r2': (np.float64, 0, 'consistency_step_basis_kernel<double, 10, 2, 0>', EPS),
    'q32_r2': (np.float32, 0, 'consistency_step_basis_kernel<q32, 10, 2, 0>', EPS),
    'q32_var7': (np.float32, 7, 'consistency_step_basis_kernel<q32, 10, 2, kStepVar>', EPS_Q32)}


def _oracle_grad(p):
    """dL/dw at w = 0 from fp64 autograd of the oracle on the points the plan materialised (x, y as viewpoints, z as depth)."""
    if 'grad' not in p:
        s, pts = p['seq'], p['pts']
        vps = torch.tensor(np.stack([pts[:, 0], pts[:, 1], np.zeros(len(pts))], 1))
        scan = dict(vps=vps, dirs=torch.tensor(s['dirs'].astype(np.float64)), depth=torch.tensor(pts[:, 2:3].copy()),
                    inc=torch.tensor(s['inc'].astype(np.float64)), mask=torch.ones(len(pts), dtype=torch.bool))
        w = torch.zeros((1, 2), dtype=torch.float64, requires_grad=True)
        lo, _ = O.eval_sequence([scan], torch.eye(4, dtype=torch.float64)[None], w, torch.tensor([[2.0, 4.0]], dtype=torch.float64),
                                torch.tensor(s['nbr']).long(), torch.ones(len(pts), dtype=torch.bool), kind='min_eigval_loss',
                                model='ScaledPolynomial', normalization=False, sqrt=False, reduction='sum')
        lo.backward()
        p['grad'] = w.grad.numpy().ravel().copy()
    return p['grad']


@pytest.mark.parametrize('form', list(_STEP_FORMS))
@pytest.mark.parametrize('case', SEQ_FAMILIES)
def test_step_kernels(dev, case, form):
    """SequencePlan.eval_native at w = 0 on one family per plan (the sum is homogeneous): the kernel named ran, count = N exactly, the
    loss sum within sum_i eps lam_max_i of the reference's -- eps = 1e-14 for float64 points and for the round-2 baseline form
    (dc_set_option(6, 0): eig3_smallest_r2), 1e-11 for the q32 kernels, whose eig3_smallest_unit<false> leaves the eigenvalue at its
    Newton iterate -- and, for the families whose lam0 is separated, dL/dw against fp64 autograd of the oracle with the tolerances
    of test_one_pass_step_all_loss_variants_vs_oracle.

    Measured on an MI355X, |sum - ref| / sum_i lam_max_i (the test prints it).  float64 points and both round-2 forms: <= 3.2e-16
    for every family.  The q32 kernels (consistency_step_q32_kernel and consistency_step_basis_kernel<q32, .., kStepVar>: the same
    figures, they share step_point2):

        generic 4.0e-15   planar 3.7e-15   needle 1.4e-18   double_lo 1.4e-16   double_hi 6.9e-16   isotropic 1.6e-16
        near_isotropic 3.1e-16   edge 1.2e-15   sign_switch 3.1e-15   threshold 6.4e-15   threshold_unit 1.4e-16   mixed 3.1e-15
        exact_rank 3.1e-18

    No family exceeds 1e-12 lam_max; the largest, 'threshold', sits just below the switch to the second Newton step.  dL/dw: the
    float64 and round-2 forms are within 2.2e-7 of the largest component, the q32 kernels (float32 second sweep) within 2.3e-5 on
    'edge' and 6.8e-6 on 'planar' -- neighbourhoods flattened to 1e-8 of their extent, where v0 . (x_j - mean) cancels to the last
    digits of a float32 -- and within 3e-7 elsewhere."""
    from depth_correction_amd import _native as nv
    from depth_correction_amd.plan import KernelTimer
    dtype, var, kernel, eps = _STEP_FORMS[form]
    p = _plan(dev, case, dtype)
    plan, ref = p['plan'], p['ref']
    n = plan.n
    assert_claims(case, ref, cases.K, UNIT)
    out = torch.zeros(2 + 4 + 12, dtype=torch.float64, device=dev)
    nv.check(nv.lib().dc_set_option(6, var), 'dc_set_option')
    try:
        with KernelTimer(every=1) as timer:
            plan.eval_native(p['w0'], p['e'], p['P'], out)
            name = timer.kernels()['consistency_fwd']
    finally:
        nv.check(nv.lib().dc_set_option(6, 1), 'dc_set_option')
    assert name.startswith(kernel), name
    o = npy(out)
    assert o[1] == n
    want = float(np.sum(ref['mineig_raw']))
    scale = float(ref['lam'][:, 2].sum())
    print('step %-15s %-8s |sum - ref| / sum lam_max = %.2e  (bound %.0e)' % (case, form, abs(o[0] - want) / scale, eps))
    assert abs(o[0] - want) <= eps * scale, (abs(o[0] - want) / scale, eps)
    if case in SEPARATED:
        g = _oracle_grad(p)
        f64 = dtype == np.float64
        gerr = np.abs(o[2:4] - g)
        print('step %-15s %-8s dL/dw error / max |dL/dw| = %.2e' % (case, form, gerr.max() / np.abs(g).max()))
        np.testing.assert_allclose(o[2:4], g, rtol=1e-6 if f64 else 1e-5, atol=(1e-8 if f64 else 2e-5) * np.abs(g).max())


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'q32'])
@pytest.mark.parametrize('case', SEQ_FAMILIES)
def test_landscape(dev, case, dtype):
    """SequencePlan.eval_landscape on the plans of test_step_kernels, weight rows [0, 0] and two others, without bounds
    (eig3_smallest) and with the bound (1, -1, -inf, inf), which keeps every centre and sends the kernel through eig3_sym_v2.  The
    w = 0 row: count = N, loss within sum_i 1e-14 lam_max_i of the reference's -- for q32 rows too: the landscape kernel never takes
    the RAYLEIGH = false form of the solver.  Every row: the two calls agree within the same bound at that row's points -- a weight
    row moves every point along its ray by at most delta = 2 (|w0| + |w1|) (depth <= 2, incidence <= 1), which moves the standard
    deviation along any direction by at most sqrt(k / (k - 1)) delta <= 1.06 delta: lam_max(w) <= (sqrt(lam_max(0)) + 1.06 delta)^2."""
    p = _plan(dev, case, dtype)
    plan, ref = p['plan'], p['ref']
    if not plan.supports_landscape(2):
        pytest.skip('no landscape on this plan')
    assert_claims(case, ref, cases.K, SIGN + UNIT)
    eps = EPS
    n = plan.n
    rows = [[0.0, 0.0], [1e-3, 2e-3], [-2e-3, 5e-4]]
    W = torch.tensor(rows, dtype=torch.float64, device=dev)
    outs = []
    for bounds in ((), ((1, -1, -np.inf, np.inf),)):
        out = torch.zeros((3, 2), dtype=torch.float64, device=dev)
        plan.eval_landscape(W, p['e'], p['P'], out, bounds=bounds)
        outs.append(npy(out))
    want = float(np.sum(ref['mineig_raw']))
    scale0 = float(ref['lam'][:, 2].sum())
    for o, what in zip(outs, ('eig3_smallest', 'eig3_sym_v2')):
        assert np.all(o[:, 1] == n)
        print('landscape %-15s %s %-13s |sum - ref| / sum lam_max = %.2e' % (case, np.dtype(dtype).name, what, abs(o[0, 0] - want) / scale0))
        assert abs(o[0, 0] - want) <= eps * scale0, (what, abs(o[0, 0] - want) / scale0)
    for r, w in enumerate(rows):
        delta = 2.0 * (abs(w[0]) + abs(w[1]))
        scale = float(((np.sqrt(ref['lam'][:, 2]) + 1.06 * delta) ** 2).sum())
        assert abs(outs[0][r, 0] - outs[1][r, 0]) <= eps * scale, (r, abs(outs[0][r, 0] - outs[1][r, 0]) / scale)
    assert outs[0][1, 0] != outs[0][0, 0]                       # the weights moved the points
