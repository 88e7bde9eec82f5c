"""The driver reads bench.py's LAST stdout line as the contract object (a 30 KB line left BENCH_r03 unparsed).

GPU test: the default-shaped `--full` run (ResNet-50 bf16 b=256, kernel profile + CPU baseline on) prints exactly one line that
starts with {"metric", it is the last line, it is compact, and it carries `roofline` (a single kernel, with `alone` beside
it) and `cpu_baseline`; the per-kernel / per-layer tables live in the detail file instead.
Reference metric: /root/reference/trainer.py:232 (B * world / step.avg)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_contract_line_is_last_compact_and_complete(tmp_path):
    env = dict(os.environ, CONVNET_AMD_EMULATE='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    detail = tmp_path / 'detail.json'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '3', '--full', '--cpu-steps',
                        '1', '--detail-out', str(detail)], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.split('\n') if l.strip()]
    last = lines[-1]
    assert last.startswith('{"metric"') and len(last) < 8192, (len(last), last[:300])
    assert sum(l.startswith('{"metric"') for l in lines) == 1
    rec = json.loads(last)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'transport_fallback'):
        assert k in rec, k
    assert rec['steps'] == 4 and rec['warmup'] == 3 and rec['n_gpus'] == 1 and rec['dtype'] == 'bf16'
    assert rec['transport_fallback'] is False
    assert abs(rec['value'] - 256 * 1e3 / rec['ms_per_step']) / rec['value'] < 1e-3
    roof = rec['roofline']
    assert 0.0 < roof['frac'] <= 1.0 and roof['bound'] in ('hbm', 'mfma') and roof['peak'] > 0
    assert abs(roof['frac'] - roof['achieved'] / roof['peak']) < 1e-3
    # one kernel, not a composite call label
    base = roof['kernel'].split(' (')[0].split(' [')[0]
    assert '+' not in base.split('<')[0] and ' + ' not in base, roof['kernel']
    assert roof['alone']['avg_us_per_launch'] > 0
    assert rec['cpu_baseline']['value'] > 0 and rec['cpu_baseline']['cores'] >= 1
    assert rec['cpu_baseline']['kind'] in ('port', 'reference')
    for k in ('kernels', 'kernels_overlapped', 'conv_layers'):
        assert k not in rec
    d = json.load(open(detail))
    assert d['kernels'] and d['kernels_overlapped'] and d['conv_layers'] and d['value'] == rec['value']


@pytest.mark.gpu
def test_contract_line_is_last_in_an_rccl_run_too(tmp_path):
    """A distributed run (here: a 1-rank RCCL group, the only one a 1-GPU box can build) brings RCCL's version banner into
    the process - five lines through C stdio that a piped stdout used to deliver BEHIND the contract line.  The line must
    still be the last one, and the only {"metric" line."""
    env = dict(os.environ, CONVNET_AMD_EMULATE='0', BENCH_FORCE_DIST='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29571')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '2', '--no-cpu-baseline',
                        '--no-kernel-profile'], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.split('\n') if l.strip()]
    assert lines[-1].startswith('{"metric"'), lines[-3:]
    assert sum(l.startswith('{"metric"') for l in lines) == 1
    rec = json.loads(lines[-1])
    assert rec['n_gpus'] == 1 and rec['transport_fallback'] is False and 'RCCL' in (rec['config']['transport'] or '')


def _bench_env():
    env = dict(os.environ, CONVNET_AMD_EMULATE='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    return env


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run (no --full) prints the headline line without the --full objects, runs exactly --steps timed steps, and
    --dump-outputs writes the last timed step's results as float32 / float64 .npy files (< 64 MB) that two runs with the
    same arguments reproduce bit for bit."""
    import numpy as np
    dumps = []
    for run in range(2):
        d = tmp_path / ('out%d' % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--batch', '32', '--steps', '3', '--warmup', '3',
                            '--dump-outputs', str(d)], env=_bench_env(), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.split('\n') if l.strip()]
        assert lines[-1].startswith('{"metric"') and sum(l.startswith('{"metric"') for l in lines) == 1
        rec = json.loads(lines[-1])
        assert rec['steps'] == 3 and rec['warmup'] == 3 and rec['higher_is_better'] is True and rec['dtype'] == 'bf16'
        assert rec['unit'] == 'images/sec' and abs(rec['value'] - 32 * 1e3 / rec['ms_per_step']) / rec['value'] < 1e-3
        assert rec['roofline'] is None and rec['cpu_baseline'] is None and 'detail_file' not in rec
        assert rec['step_issue']['host_ms_per_step'] is None and 'hbm_measured_whole_step' not in rec
        files = sorted(os.listdir(d))
        assert files == ['logits.npy', 'loss.npy', 'meters.npy', 'state_sample.npy'], files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrs = {f: np.load(d / f) for f in files}
        for f, a in arrs.items():
            assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        assert arrs['logits.npy'].shape == (32, 1000)
        assert arrs['loss.npy'].shape == (1,) and arrs['loss.npy'][0] > 0
        assert abs(arrs['meters.npy'][0] - rec['config']['final_loss']) <= 1e-4     # Trainer.train's mean loss, as in the line
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_bench_options_are_checked_before_any_gpu_work():
    """--full and --dump-outputs exist; --pmc (a --full figure) and a timed region of no steps are refused up front."""
    h = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert h.returncode == 0 and '--full' in h.stdout and '--dump-outputs' in h.stdout, h.stdout + h.stderr
    for bad in (['--pmc'], ['--steps', '0']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and 'error' in r.stderr, (bad, r.stderr[-1000:])
