"""bench.py driver contract: runs standalone, emits one valid JSON line."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra):
    proc = subprocess.run(
        [sys.executable, 'bench.py', '--steps', '2', '--warmup', '1', '--batch-size', '64'] + extra,
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=420,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize('model', ['mnist'])
def test_bench_json_contract(model):
    result = _run_bench(['--model', model])
    for key in (
        'metric',
        'value',
        'unit',
        'n_gpus',
        'steps',
        'warmup',
        'ms_per_step',
        'higher_is_better',
        'scaling',
        'vs_baseline',
        'dtype',
        'data',
        'config',
    ):
        assert key in result, key
    assert result['n_gpus'] == 1
    assert result['steps'] == 2
    assert result['data'] == 'synthetic'
    assert result['value'] > 0
    assert result['config']['parallelism'] == 'dp1'
    assert result['scaling'] == 'weak'


def test_bench_ddp_impl():
    result = _run_bench(['--impl', 'ddp'])
    assert result['config']['impl'] == 'ddp'


def test_bench_metric_stress_mode():
    """BASELINE config #5 plumbing: N per-step reducers tracked and
    reported in the JSON config."""
    result = _run_bench(['--metric-stress', '8'])
    assert result['config']['metric_stress'] == 8


def _run_bench_dump(out_dir, extra=()):
    import numpy as np

    result = _run_bench(['--dump-outputs', str(out_dir), *extra])
    assert sorted(f.name for f in out_dir.iterdir()) == ['grads.npy', 'loss.npy', 'params.npy']
    return result, {f.stem: np.load(f) for f in out_dir.iterdir()}


@pytest.fixture(scope='module')
def full_run(tmp_path_factory):
    """One `--full --dump-outputs` run, shared by the tests below."""
    return _run_bench_dump(tmp_path_factory.mktemp('full') / 'out', ['--full'])


def test_bench_full_flag(full_run):
    """--full (everything beyond the headline figure) still ends in the
    one result line with the same headline fields."""
    result, _ = full_run
    assert result['steps'] == 2
    assert result['metric'] == 'samples/s'
    assert result['ms_per_step'] > 0


def test_bench_dump_outputs(full_run, tmp_path):
    """--dump-outputs writes the last timed step's loss, parameters and
    gradients as float32 .npy files, and two runs with the same arguments
    (--full changes neither inputs nor the timed path) start from identical
    inputs, so they dump the same results."""
    import numpy as np

    _, a = full_run
    _, b = _run_bench_dump(tmp_path / 'out')
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for key in a:
        assert a[key].dtype == np.float32, key
        assert a[key].shape == b[key].shape, key
        assert np.isfinite(a[key]).all(), key
    assert a['loss'].shape == (1,)
    assert a['params'].size == a['grads'].size > 0
    assert np.abs(a['grads']).max() > 0
    # Identical inputs, and every reduction on the default timed path runs
    # in a fixed order, so two runs agree to fp32 rounding: a few ulps
    # (2^-23 ~ 1.2e-7 relative), with an absolute floor for entries that
    # cancel to nearly zero (values here are O(1e-3..1)).
    for key in a:
        np.testing.assert_allclose(a[key], b[key], rtol=1e-6, atol=1e-7, err_msg=key)


def _free_port():
    import socket

    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize('impl', ['flat', 'ddp'])
def test_bench_torchrun_w2(impl):
    """The driver's multi-GPU launch contract, exercised at world_size=2 on
    CPU/gloo: torch.distributed.run -> env:// rendezvous -> ONE JSON line
    with n_gpus=2 / dp2."""
    import torch

    env = dict(os.environ)
    if torch.cuda.is_available() and torch.cuda.device_count() < 2:
        # one GPU cannot host two ranks: hide it so both ranks take the
        # CPU/gloo path this test is about
        env.update(HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    proc = subprocess.run(
        [
            sys.executable,
            '-m',
            'torch.distributed.run',
            '--nnodes=1',
            '--nproc-per-node',
            '2',
            '--master-addr',
            '127.0.0.1',
            '--master-port',
            str(_free_port()),
            'bench.py',
            '--gpus',
            '2',
            '--steps',
            '2',
            '--warmup',
            '1',
            '--batch-size',
            '64',
            '--impl',
            impl,
        ],
        cwd=REPO,
        env=env,
        capture_output=True,
        text=True,
        timeout=420,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, proc.stdout  # rank 0 only
    result = json.loads(lines[0])
    assert result['n_gpus'] == 2
    assert result['config']['parallelism'] == 'dp2'
    assert result['config']['global_batch'] == 128
    assert result['value'] > 0
