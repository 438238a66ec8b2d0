"""bench.py's plain run (what the headline needs, nothing else) and --dump-outputs: one timed window of exactly --steps batches,
the slots of the last timed batch written as float32, the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def test_plain_bench_times_steps_and_dumps_the_last_batch(dev, tmp_path):
    runs = []
    for k in range(2):
        d = _bench('--gpus', '1', '--steps', '3', '--warmup', '2', '--dump-outputs', str(tmp_path / f'run{k}'))
        assert d['steps'] == 3 and d['warmup'] == 2 and d['value'] > 0 and d['higher_is_better'] is True
        assert d['ms_per_step_windows']['n'] == 1
        assert d['ms_per_step'] == pytest.approx(1e3 * d['timed_region_s'] / 3, rel=1e-9)
        assert d['value'] == pytest.approx(d['config']['batch_per_gpu'] * (d['config']['burn_in'] + d['config']['rollout']) * 1e3 / d['ms_per_step'], rel=1e-9)
        for key in ('roofline', 'cpu_baseline', 'one_batch_latency_ms', 'encode_ms', 'ms_per_step_distribution'):
            assert key not in d, key   # --full only
        runs.append(np.load(tmp_path / f'run{k}' / 'slots.npy'))
    a, b = runs
    assert a.dtype == np.float32 and a.shape == (32, 6 + 50, 7, 128)
    assert np.isfinite(a).all() and np.abs(a[:, 6:]).max() > 0
    assert np.array_equal(a, b)
