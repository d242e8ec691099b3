"""``python bench.py`` without ``--full`` is the lean run: set-up, warm-up, the timed steps and the headline line, none of the
measurements that take runs of their own (they are ``--full`` only)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ('roofline', 'roofline_engine', 'roofline_chain', 'other_configs', 'cpu_baseline', 'parity', 'input_side', 'comm_timeline',
             'step_executed_tflop', 'step_executed_tflops', 'step_executed_frac', 'step_valid_rows_frac', 'step_executed_by_entry_point_gflop')


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_alone():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1'], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line['metric'] == 'joint_train utterances/sec' and line['unit'] == 'utterances/s' and line['dtype'] == 'f32'
    assert line['higher_is_better'] is True and line['full'] is False
    assert line['steps'] == 2 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0
    assert abs(line['value'] - 32 * 1e3 / line['ms_per_step']) <= 1e-3 * line['value'] + 0.01
    assert line['persistent_kernel_aborts'] == 0
    assert all(v == v for v in line['final_losses'].values())
    assert [k for k in FULL_ONLY if k in line] == []
