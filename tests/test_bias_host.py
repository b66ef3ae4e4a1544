"""Depth bias against the mesh on the host (no GPU): the per-ray arithmetic of dc_bias_accumulate through its host build
(libdc_hostcheck.so, the header the kernel includes) against the numpy restatement (tests/bias_reference.py), the supervised fit,
the finishing arithmetic of depth_bias on CPU tensors, the CSV helpers, the new Config fields and the refusals."""
import ctypes
import math
import os

import numpy as np
import pytest

import bias_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'depth_correction_amd', 'lib', 'libdc_hostcheck.so')
KINDS = {R.POLYNOMIAL: 1, R.SCALED_POLYNOMIAL: 2}
SEED = 11


@pytest.fixture(scope='module')
def host():
    if not os.path.exists(LIB) or not hasattr(ctypes.CDLL(LIB), 'dc_host_bias_accumulate'):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    lib.dc_host_bias_accumulate.restype = ctypes.c_int
    lib.dc_host_bias_accumulate.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 +
                                            [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_void_p])
    lib.dc_host_bias_bin.restype = ctypes.c_int
    lib.dc_host_bias_bin.argtypes = [ctypes.c_double, ctypes.c_int]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _host_out(host, depth, inc_est, mask, face, t, g, kind, exponent, n_bins, max_residual):
    e = np.asarray(exponent, dtype=np.float64)
    out = np.full(R.out_count(n_bins, len(e)), np.nan)
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    rc = host.dc_host_bias_accumulate(_p(depth), _p(inc_est), 0 if depth.dtype == np.float32 else 1, _p(m8), _p(face), _p(t), _p(g),
                                      len(depth), KINDS[kind], _p(e), len(e), n_bins, 0.0 if max_residual is None else max_residual, _p(out))
    return rc, out


def _synthetic(n=100000, seed=SEED):
    """Rays with everything the used-ray rule tests: masked-out rays, misses, depths <= 0, residuals beyond a 0.5 m gate, estimated
    angles that are missing (NaN)."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, np.pi / 2, size=n)
    t = rng.uniform(1.0, 20.0, size=n)
    face = rng.integers(0, 5000, size=n).astype(np.int32)
    miss = rng.uniform(size=n) < 0.05
    face[miss], t[miss], g[miss] = -1, np.inf, np.nan
    depth = np.where(miss, rng.uniform(1.0, 20.0, size=n), t) * (1.0 + 0.03 * np.nan_to_num(g) ** 2) + rng.normal(scale=0.02, size=n)
    far = rng.uniform(size=n) < 0.02
    depth[far] += rng.choice([-1.0, 1.0], size=int(far.sum())) * rng.uniform(0.6, 3.0, size=int(far.sum()))
    depth[rng.uniform(size=n) < 0.01] = 0.0
    depth[rng.uniform(size=n) < 0.01] = -1.5
    mask = rng.uniform(size=n) < 0.8
    est = np.clip(np.nan_to_num(g) + rng.normal(scale=0.05, size=n), 0.0, np.pi / 2)
    est[rng.uniform(size=n) < 0.03] = np.nan
    return depth, est, mask, face, t, g


def test_seed_keeps_angles_off_the_bin_edges():
    g = _synthetic()[5]
    for b in (1, 18, 90):
        assert R.distance_to_bin_edge(g, b) > 1e-9, b


@pytest.mark.parametrize('n_bins', [1, 18, 90])
@pytest.mark.parametrize('kind,exponent', [(R.SCALED_POLYNOMIAL, [2.0]), (R.POLYNOMIAL, [2.0, 4.0]), (R.SCALED_POLYNOMIAL, [1.0, 2.5, 4.0]),
                                           (R.POLYNOMIAL, [3.0])])
def test_host_accumulate_matches_reference(host, n_bins, kind, exponent):
    depth, est, mask, face, t, g = _synthetic()
    assert R.distance_to_bin_edge(g, n_bins) > 1e-9
    for with_est, with_mask, gate in ((True, True, 0.5), (False, True, None), (True, False, 0.5)):
        e_arg, m_arg = (est if with_est else None), (mask if with_mask else None)
        want, ab, m = R.accumulate(depth, e_arg, m_arg, face, t, g, kind, exponent, n_bins, gate)
        rc, got = _host_out(host, depth, e_arg, m_arg, face, t, g, kind, exponent, n_bins, gate)
        assert rc == 0 and np.isfinite(got).all()
        cnt = R.is_count(n_bins, len(exponent))
        assert np.array_equal(got[cnt], want[cnt])
        err, bound = np.abs(got - want), R.sum_bound(ab, m)
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (worst, got[worst], want[worst], err[worst], bound[worst])
        tot = dict(zip(('rays', 'masked', 'hits', 'used', 'gated'), got[:5]))
        assert tot['rays'] == len(depth) and tot['used'] + (tot['gated'] if gate else 0) < tot['hits'] < tot['masked'] <= tot['rays']
        assert (tot['gated'] > 100) == (gate is not None)
        if not with_est:                              # no estimate: the delta sums and the second system are zero
            rows = got[R.TOTALS:R.TOTALS + R.BIN_COLS * n_bins].reshape(n_bins, R.BIN_COLS)
            assert (rows[:, 6:] == 0).all() and (got[R.TOTALS + R.BIN_COLS * n_bins + R.system_len(len(exponent)):] == 0).all()


def test_host_accumulate_fp32_and_bins(host):
    depth, est, mask, face, t, g = _synthetic(20000, seed=5)
    d32, e32 = depth.astype(np.float32), est.astype(np.float32)
    want, ab, m = R.accumulate(d32, e32, mask, face, t, g, R.SCALED_POLYNOMIAL, [2.0, 4.0], 18, 0.5)
    rc, got = _host_out(host, d32, e32, mask, face, t, g, R.SCALED_POLYNOMIAL, [2.0, 4.0], 18, 0.5)
    cnt = R.is_count(18, 2)
    assert rc == 0 and np.array_equal(got[cnt], want[cnt]) and (np.abs(got - want) <= R.sum_bound(ab, m)).all()
    # the bin rule on its own, the edges included: pi/2 falls into the last bin
    assert R.distance_to_bin_edge(g, 18) > 1e-9
    fin = np.isfinite(g)
    assert np.array_equal([host.dc_host_bias_bin(float(x), 18) for x in g[fin][:5000]], R.bins_of(g[fin][:5000], 18))
    assert host.dc_host_bias_bin(0.0, 18) == 0 and host.dc_host_bias_bin(np.pi / 2, 18) == 17 and host.dc_host_bias_bin(0.5, 1) == 0


def test_host_accumulate_refuses_bad_arguments(host):
    depth, est, mask, face, t, g = _synthetic(100, seed=2)
    ok = lambda **kw: _host_out(host, depth, est, mask, face, t, g, kw.get('kind', R.POLYNOMIAL), kw.get('e', [2.0]), kw.get('b', 18),
                                kw.get('gate'))[0]
    assert ok() == 0 and ok(b=256) == 0 and ok(e=[1.0, 2.0, 3.0, 4.0]) == 0
    assert ok(b=0) == 1 and ok(b=257) == 1 and ok(e=[1.0] * 5) == 1 and ok(e=[np.nan]) == 1 and ok(gate=float('nan')) == 1
    KINDS['Linear'] = 3
    try:
        assert ok(kind='Linear') == 1
    finally:
        del KINDS['Linear']


# ---- the supervised fit ------------------------------------------------------------------------------------------------------------
def _exact_out(host, kind, w, exponent, n=50000, seed=3):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 1.4, size=n)
    y = R.basis(g, exponent) @ np.asarray(w)
    t = rng.uniform(2.0, 15.0, size=n)
    depth = t / (1.0 - y) if kind == R.SCALED_POLYNOMIAL else t + y
    face = np.zeros(n, dtype=np.int32)
    rc, out = _host_out(host, depth, g.copy(), None, face, t, g, kind, exponent, 18, None)
    assert rc == 0
    return out, g, depth, t


@pytest.mark.parametrize('kind,w,exponent', [(R.SCALED_POLYNOMIAL, [0.05], [2.0]), (R.SCALED_POLYNOMIAL, [0.02, 0.01], [2.0, 4.0]),
                                             (R.POLYNOMIAL, [0.03, -0.01, 0.004], [1.0, 2.0, 3.0]), (R.POLYNOMIAL, [0.1], [4.0])])
def test_fit_bias_recovers_exact_weights(host, kind, w, exponent):
    from depth_correction_amd import model as M
    from depth_correction_amd.metrics import fit_bias, fitted_model
    out, g, depth, t = _exact_out(host, kind, w, exponent)
    import torch
    for src in (out, torch.as_tensor(out)):
        fit = fit_bias(src, kind, exponent)
        assert fit['message'] is None
        for key in ('w_true_angles', 'w_est_angles'):           # the estimate equals the truth here: both systems are the same
            assert np.abs(fit[key] - w).max() <= 1e-9 * np.abs(w).max(), (key, fit[key], w)
        assert fit['n_true_angles'] == len(g) and np.isfinite(fit['cond_true_angles']) and fit['cond_true_angles'] >= 1.0
        # the residual rms comes from three sums of n terms, each within (n + 16) 2^-53 of its terms' absolute sum, which cancel to
        # zero here: what is left is below sqrt(3 (n + 16) 2^-53) of the target's rms
        y = (depth - t) / depth if kind == R.SCALED_POLYNOMIAL else depth - t
        assert fit['rms_true_angles'] <= math.sqrt(3 * (len(y) + 16) * 2.0 ** -53) * math.sqrt(np.mean(y * y))
    # against lstsq on the per-ray rows, and the class passed as a class
    ref = R.lstsq_fit(g, (depth - t) / depth if kind == R.SCALED_POLYNOMIAL else depth - t, exponent)
    fit = fit_bias(out, getattr(M, kind), np.asarray(exponent))
    assert np.abs(fit['w_true_angles'] - ref).max() <= 1e-9 * np.abs(ref).max()
    model = fitted_model(fit)
    assert type(model).__name__ == kind and model.w.dtype == torch.float64
    assert np.array_equal(model.w.detach().numpy().reshape(-1), fit['w_true_angles'])
    assert np.array_equal(model.exponent.detach().numpy().reshape(-1), exponent)
    assert np.array_equal(fitted_model(fit, 'est_angles').w.detach().numpy().reshape(-1), fit['w_est_angles'])


def test_fit_bias_singular_systems_give_nan(host):
    from depth_correction_amd.metrics import fit_bias
    face = np.zeros(1000, dtype=np.int32)
    t = np.full(1000, 5.0)
    depth = t + 0.01

    def fit(g, est, kind=R.POLYNOMIAL, e=(2.0, 4.0), n=1000):
        rc, out = _host_out(host, depth[:n].copy(), est, None, face[:n].copy(), t[:n].copy(), g, kind, list(e), 18, None)
        assert rc == 0
        return fit_bias(out, kind, list(e))
    rng = np.random.default_rng(0)
    g = rng.uniform(0.1, 1.4, size=1000)
    # every true angle zero: the basis vanishes; the estimated angles still give a system
    f = fit(np.zeros(1000), g.copy())
    assert np.isnan(f['w_true_angles']).all() and np.isnan(f['rms_true_angles']) and np.isfinite(f['w_est_angles']).all()
    assert 'true_angles' in f['message'] and 'est_angles' not in f['message']
    # one angle for every ray: two columns, rank one
    f = fit(np.full(1000, 0.7), None)
    assert np.isnan(f['w_true_angles']).all() and np.isnan(f['w_est_angles']).all() and 'singular' in f['message']
    # fewer rays than weights, and no ray at all
    assert np.isnan(fit(g[:1].copy(), None, n=1)['w_true_angles']).all()
    f = fit(g[:0].copy(), None, n=0)
    assert np.isnan(f['w_true_angles']).all() and f['n_true_angles'] == 0 and 'rays' in f['message']
    with pytest.raises(ValueError):
        fit_bias(np.zeros(7), R.POLYNOMIAL, [2.0])
    with pytest.raises(ValueError):
        fit_bias(np.zeros(R.out_count(18, 1)), 'Linear', [2.0])


# ---- finishing arithmetic, CSV, configuration --------------------------------------------------------------------------------------
def _reference_result(kind=R.SCALED_POLYNOMIAL, exponent=(2.0, 4.0), n_bins=18, empty_bins=False):
    import torch
    depth, est, mask, face, t, g = _synthetic(30000, seed=8)
    if empty_bins:
        mask = mask & ~((g > 0.5) & (g < 0.8))
    out = R.accumulate(depth, est, mask, face, t, g, kind, list(exponent), n_bins, 0.5)[0]
    return out, torch.as_tensor(out)


def test_bias_statistics_on_cpu_tensors():
    import torch
    from depth_correction_amd.metrics import BIAS_BIN_FIELDS, bias_statistics
    for empty in (False, True):
        out, tens = _reference_result(empty_bins=empty)
        got, want = bias_statistics(tens, 18), R.bin_statistics(out, 18)
        assert got['count'].device.type == 'cpu' and got['count'].dtype == torch.float64
        for f in BIAS_BIN_FIELDS:
            np.testing.assert_allclose(got[f].numpy(), want[f], rtol=1e-14, atol=0, equal_nan=True)
        assert bool(np.isnan(want['mean']).any()) == empty and np.array_equal(np.isnan(got['rms'].numpy()), want['count'] == 0)
        assert got['totals'] == dict(zip(('rays', 'masked', 'hits', 'used', 'beyond_gate'), out[:5]))
        rows = out[R.TOTALS:R.TOTALS + R.BIN_COLS * 18].reshape(18, R.BIN_COLS).sum(axis=0)
        o = got['overall']
        assert o['count'] == out[3] == rows[0]
        for key, val in (('mean_abs', rows[3] / rows[0]), ('rms', math.sqrt(rows[2] / rows[0])), ('rel_rms', math.sqrt(rows[5] / rows[0])),
                         ('angle_err_rms', math.sqrt(rows[7] / rows[8]))):
            assert isinstance(o[key], float) and abs(o[key] - val) <= 1e-14 * abs(val), key
    nothing = bias_statistics(torch.zeros(R.out_count(4, 1), dtype=torch.float64), 4)
    assert np.isnan(nothing['mean'].numpy()).all() and math.isnan(nothing['overall']['rms']) and nothing['totals']['used'] == 0
    with pytest.raises(ValueError):
        bias_statistics(torch.zeros(10, dtype=torch.float64), 18)


def test_csv_helpers(tmp_path):
    import torch
    from depth_correction_amd.eval import bias_eval_line, write_bias_curve_csv
    from depth_correction_amd.metrics import BIAS_BIN_FIELDS, bias_statistics, fit_bias
    out, tens = _reference_result()
    before = bias_statistics(tens, 18)
    before['out'] = tens
    res = dict(bins=18, bin_edges=torch.linspace(0.0, math.pi / 2, 19, dtype=torch.float64), before=before, after=None,
               fit_class=R.SCALED_POLYNOMIAL, fit_exponent=[2.0, 4.0])
    fit = fit_bias(res, R.SCALED_POLYNOMIAL, [2.0, 4.0])
    with pytest.raises(ValueError):
        fit_bias(res, R.POLYNOMIAL, [2.0, 4.0])                       # the sums were taken for another class
    line = bias_eval_line('room', res, fit)
    tok = line.split()
    assert line.endswith('\n') and len(tok) == 11 and tok[0] == 'room' and int(tok[1]) == out[3]
    assert abs(float(tok[2]) - before['overall']['mean_abs']) < 1e-9 and tok[5:8] == ['nan'] * 3
    assert abs(float(tok[8]) - before['overall']['angle_err_rms']) < 1e-9
    np.testing.assert_allclose([float(x) for x in tok[9].split(',')], fit['w_true_angles'], rtol=1e-8)
    np.testing.assert_allclose([float(x) for x in tok[10].split(',')], fit['w_est_angles'], rtol=1e-8)
    res['after'] = before
    assert bias_eval_line('room', res, fit).split()[5:8] == tok[2:5]
    path = tmp_path / 'sub' / 'curve.csv'
    write_bias_curve_csv(str(path), 'room', res)
    lines = path.read_text().splitlines()
    assert lines[0].startswith('# name bin angle_lo angle_hi count_before') and len(lines) == 19
    assert lines[0].split()[1:] == ['name', 'bin', 'angle_lo', 'angle_hi'] + ['%s_%s' % (f, p) for p in ('before', 'after') for f in BIAS_BIN_FIELDS]
    row = lines[5].split()
    assert row[:2] == ['room', '4'] and len(row) == 4 + 16 and abs(float(row[3]) - 5 * math.pi / 36) < 1e-8
    assert abs(float(row[5]) - float(before['mean'][4])) <= 1e-8 * abs(float(before['mean'][4])) and row[4:12] == row[12:20]


def test_config_and_file_names():
    from depth_correction_amd.config import Config, bias_eval_csv, map_eval_csv
    cfg = Config()
    assert cfg.bias_eval_csv is None and cfg.bias_eval_curve_csv is None and cfg.bias_eval_bins == 18
    assert cfg.bias_eval_max_residual is None and cfg.bias_eval_cull is True
    assert Config(bias_eval_bins=30, bias_eval_max_residual=0.5).copy().bias_eval_bins == 30
    assert bias_eval_csv('/tmp/log', 'val') == '/tmp/log/bias_eval_val.csv' and bias_eval_csv('', None) == 'bias_eval.csv'
    assert bias_eval_csv('log', 'test') == 'log/bias_eval_test.csv' and bias_eval_csv(None, 'train') == 'bias_eval_train.csv'
    assert os.path.dirname(bias_eval_csv('/x/y', 'test')) == os.path.dirname(map_eval_csv('/x/y', 'test'))


def test_operators_refuse_cpu_tensors():
    import torch
    from depth_correction_amd import ops
    from depth_correction_amd.mesh import MeshBVH
    bvh = MeshBVH(torch.zeros(1, dtype=torch.int32), torch.zeros((0, 2), dtype=torch.int32), torch.full((1,), -1, dtype=torch.int32),
                  torch.zeros((1, 6)), torch.zeros((1, 9), dtype=torch.float64))
    rays = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        ops.raycast_rays(bvh, rays, rays, [0, 4], torch.eye(4, dtype=torch.float64)[None])
    z = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        ops.bias_accumulate(z, None, None, torch.zeros(4, dtype=torch.int32), z, z, 'Polynomial', [2.0])
    assert ops.bias_out_count(18, 2) == R.out_count(18, 2) == 5 + 9 * 18 + 2 * 7


def test_eval_bias_refuses_what_it_cannot_do():
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import eval_bias, eval_map
    from depth_correction_amd.model import BaseModel

    class NoMesh(object):
        def __iter__(self):
            return iter(())

        def __str__(self):
            return 'no_mesh/seq'

    cfg = Config(device='cpu')
    with pytest.raises(ValueError) as bias_err:
        eval_bias(cfg, test_datasets=[NoMesh()], model=BaseModel())
    with pytest.raises(ValueError) as map_err:
        eval_map(cfg, test_datasets=[NoMesh()], model=BaseModel())
    assert str(bias_err.value) == str(map_err.value).replace('eval_map', 'eval_bias') and 'no get_mesh()' in str(bias_err.value)

    class WithMesh(NoMesh):
        def get_mesh(self):
            return object()

    with pytest.raises(RuntimeError, match='needs a GPU'):
        eval_bias(cfg, test_datasets=[WithMesh()], model=BaseModel())
