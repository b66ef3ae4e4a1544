"""bench.py on the GPU box, at a small size: a plain run prints the headline alone and --dump-outputs writes what the timed
path returned in its last step (the same files from run to run); --full adds the roofline, the side measurements and the
CPU baseline."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--gpus', '1', '--scans', '2', '--points', '20000', '--steps', '3', '--warmup', '1']


def _bench(*args, timeout=300):
    env = dict(os.environ)
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'DC_FORCE_DIST'):
        env.pop(key, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def _load(d):
    out = {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, '*.npy')))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


@pytest.mark.timeout(600)
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    line = _bench(*SMALL, '--dump-outputs', str(tmp_path / 'a'))
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in line
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    n = line['value'] * line['ms_per_step'] * 1e-3                       # points per step: the sequence's global cloud
    assert abs(n - round(n)) < 1e-6 * n and round(n) <= 2 * 20000
    assert line['roofline'] is None and line['cpu_baseline'] is None
    assert 'sustained_ms_per_step' not in line['config'] and 'knn_build_ms' not in line['config']
    a = _load(str(tmp_path / 'a'))
    assert sorted(a) == ['grad_w', 'loss', 'w']
    assert a['loss'].shape == (1,) and a['w'].shape == a['grad_w'].shape == (2,)
    np.testing.assert_allclose(a['loss'][0], line['config']['final_loss'], rtol=1e-12)
    assert np.all(np.isfinite(a['grad_w'])) and not np.array_equal(a['w'], [1e-3, 2e-3])     # four Adam steps moved the weights
    # the inputs are seeded: a second run computes the same
    _bench(*SMALL, '--dump-outputs', str(tmp_path / 'b'))
    b = _load(str(tmp_path / 'b'))
    for name in a:
        np.testing.assert_allclose(b[name], a[name], rtol=1e-12, atol=0, err_msg=name)


@pytest.mark.timeout(900)
def test_full_run_keeps_the_side_measurements(tmp_path):
    line = _bench(*SMALL, '--full', '--cpu-scans', '1', '--cpu-iters', '1', '--cpu-variants', '0', '--dump-outputs', str(tmp_path))
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    assert line['roofline'] is not None and line['roofline']['kernels']
    assert line['cpu_baseline'] is not None and line['cpu_baseline']['value'] > 0
    cfg = line['config']
    for key in ('knn_build_ms', 'setup_ms', 'setup_stages_ms', 'sustained_ms_per_step', 'cold_ms_per_step', 'fp64_cloud_step',
                'multi_sequence_step', 'same_step_other_forms', 'pose_mode_evaluation', 'train_iteration_ms', 'c1_forward_only',
                'online_correction', 'gpu_over_cpu'):
        assert key in cfg, key
    assert sorted(_load(str(tmp_path))) == ['grad_w', 'loss', 'w']


@pytest.mark.timeout(600)
def test_c4_run_dumps_what_train_returns(tmp_path):
    line = _bench('--workload', 'c4', '--c4-scans', '2', '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path))
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    out = _load(str(tmp_path))
    assert 'model_w' in out and out['pose_deltas'].shape == (1, 2, 6)
    assert all(np.all(np.isfinite(a)) for a in out.values())
