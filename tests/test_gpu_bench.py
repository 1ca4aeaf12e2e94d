"""bench.py emits ONE workload at every N (the N = 1 and N > 1 lines were different workloads, so the driver
could not form a scaling curve): the same metric, unit, scaling mode and keys from `--gpus 1` and from a 2-rank run - here a
small rehearsal (64 timesteps, 32^3 grid) with both ranks sharing the one GPU over the socket control plane."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(n, extra=(), steps=1, flags=('--no-cpu-baseline', '--no-secondary')):
    env = dict(os.environ, VINTERP_DIST_BACKEND='socket', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', str(n), '--records', '64', '--c3-grid', '32',
                        '--steps', str(steps), '--warmup', '1'] + list(flags) + list(extra),
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_one_workload_at_every_n():
    one, two = _bench(1), _bench(2)
    for line, n in ((one, 1), (two, 2)):
        assert line['metric'] == 'fit+eval timesteps/sec' and line['unit'] == 'timesteps/s'
        assert line['scaling'] == 'strong' and line['dtype'] == 'f64' and line['data'] == 'synthetic'
        assert line['n_gpus'] == n and line['steps'] == 1 and line['vs_baseline'] is None
        assert line['config']['timesteps'] == 64 and line['config']['timesteps_per_rank'] == 64 // n
        assert line['value'] > 0 and abs(line['value'] - 64 / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
        # the dominant part of the step - the fit - carries the roofline; the evaluation product is the second object
        rf, re_ = line['roofline'], line['roofline_eval']
        assert rf['bound'] == 'lds' and rf['achieved'] > 0 and 0 < rf['frac'] < 1 and rf['rounds_per_step'] > 0
        assert abs(rf['frac'] - rf['achieved'] / rf['peak']) <= 1e-12
        assert re_['bound'] == 'mfma' and re_['achieved'] > 0 and 0 < re_['frac'] < 1
        assert len(line['per_rank_step_s']) == n
    assert one['config']['workload'] == two['config']['workload']
    assert set(one) - {'cpu_baseline'} == set(two) - {'cpu_baseline'}
    assert set(one['roofline']) == set(two['roofline']) and set(one['roofline_eval']) == set(two['roofline_eval'])


def _load_dump(d):
    names = sorted(f for f in os.listdir(d) if f.endswith('.npy'))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in names}


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: --steps sets the timed steps, ms_per_step is their mean, nothing of --full is in the line; --dump-outputs
    writes the last step's fit and a sample of its densities in float64, every value finite, the same from run to run."""
    lines, dumps = [], []
    for i in range(2):
        d = str(tmp_path / ('out%d' % i))
        lines.append(_bench(1, ['--dump-outputs', d], steps=3))
        dumps.append(_load_dump(d))
    line = lines[0]
    assert line['steps'] == 3 and line['warmup'] == 1
    assert abs(line['value'] - 64 / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line
    assert not {'cpu_baseline', 'single_record', 'roofline_eval_fused', 'eval_many_timesteps', 'batched_records'} & set(line)
    a, b = dumps
    names = {'coeffs', 'chi_sq', 'alpha_curvature', 'ranks', 'covariance_sample', 'density_sample'}
    assert set(a) == names | {k + '_finite' for k in names} == set(b)
    assert a['coeffs'].shape == (64, 144) and a['covariance_sample'].shape == (64, 144, 144)
    assert a['density_sample'].shape == (16, 32**3)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in names:                                   # every value finite; the mask says where the path gave NaN
        assert a[k].dtype == np.float64 and a[k + '_finite'].dtype == np.float32
        assert a[k].shape == a[k + '_finite'].shape and np.all(np.isfinite(a[k]))
        assert np.all(a[k][a[k + '_finite'] == 0] == 0)
    assert a['density_sample_finite'].any() and a['coeffs_finite'].any()
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=0, err_msg=k)


def test_full_run_carries_the_secondary_objects():
    """--full (CPU baseline off here) adds the secondary objects of workload c3 at N = 1 to the same headline line."""
    line = _bench(1, ['--full', '--grid', '32', '--batched-records', '16'], flags=('--no-cpu-baseline',))
    assert line['metric'] == 'fit+eval timesteps/sec' and line['steps'] == 1
    for k in ('single_record', 'roofline_eval_fused', 'eval_many_timesteps', 'batched_records'):
        assert k in line, k
    assert line['cpu_baseline'] is None                  # --no-cpu-baseline
    assert line['single_record']['steps'] == 16 and line['roofline_eval_fused']['kernel_ms_hull_on'] > 0
