"""bench.py end to end on a small cloud: a plain run stops after the headline, --full adds the roofline object."""
import json
import subprocess
import sys

import pytest

from conftest import ROOT


def _bench_line(*extra):
    r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--points', '200000', '--steps', '3', '--warmup', '1', *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().split('\n')[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    d = _bench_line()
    assert d['unit'] == 'points/s' and d['higher_is_better'] is True and d['dtype'] == 'f64' and d['steps'] == 3
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - 200000) < 0.01 * 200000
    assert d['roofline'] is None and d['cpu_baseline'] is None
    assert not {'streaming_kernels', 'variants', 'c3_end_to_end', 'merge_bb', 'parity_on_cpu_sample'} & set(d)


@pytest.mark.gpu
def test_full_run_adds_the_roofline():
    d = _bench_line('--full', '--no-extras', '--no-cpu-baseline')
    assert d['value'] > 0 and d['roofline']['kernel'] == 'k_fuse' and d['roofline']['kernel_ms'] > 0 and d['roofline']['sort_ms'] > 0
