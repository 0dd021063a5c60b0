"""bench.py's N > 1 flow on a one-GPU box: `--gpus 2` spawns two ranks itself (torch.distributed.run), both use cuda:0 and exchange
over gloo (VITAE_BENCH_ONE_GPU=1 — a plumbing mode, never a reported number).  Everything else is the real path: rank spawn,
data-parallel step with per-phase graphs and the bucketed exchange, barriers, max-over-ranks clock, rank-0 instrumentation while
the other rank waits, ONE JSON line from rank 0."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_print_one_line():
    env = dict(os.environ, VITAE_BENCH_ONE_GPU='1')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--full'],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['rccl_ranks'] == 2 and d['config']['global_batch'] == 8
    assert d['scaling'] == 'weak' and d['value'] > 0 and d['roofline'] is not None and d['cpu_baseline'] is None
    assert 'PLUMBING CHECK' in d['config']['parallelism']
    # the dual-leg flow: the host-issued exchange was timed and described; the native (RCCL in the graph) leg cannot run on a shared GPU
    assert d['config']['exchange']['route'].startswith('host-issued') and d['config']['exchange']['buckets'] >= 2
    assert 'skipped' in d['config']['also_exchange']


def test_bench_refuses_more_ranks_than_gpus():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'VITAE_BENCH_ONE_GPU')}
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--steps', '1'], capture_output=True,
                       text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and 'refusing' in (r.stderr + r.stdout)


def test_bench_times_both_exchange_routes_on_a_world_of_one():
    """at N > 1 bench.py times BOTH gradient-exchange routes in one invocation — torch.distributed collectives
    between per-phase graphs, and RCCL through the C ABI inside the one step graph — reports the faster as `value` and the other
    under config.also_exchange.  On a one-GPU box the same flow runs over a communicator of one rank (VITAE_FORCE_DDP=1)."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'VITAE_BENCH_ONE_GPU', 'RANK', 'LOCAL_RANK')}
    env['VITAE_FORCE_DDP'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '1', '--full', '--no-cpu-baseline',
                        '--profile-steps', '0'],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    a, b = d['config']['exchange'], d['config']['also_exchange']
    assert {a['route'].split(':')[0], b['route'].split(':')[0]} == {'host-issued', 'native'}, (a, b)
    nat = a if a['route'].startswith('native') else b
    assert nat['vitae_ddp_world_size'] == 1 and d['config']['rccl_ranks'] == 1
    assert a['ms_per_step'] <= b['ms_per_step'] and abs(d['ms_per_step'] - a['ms_per_step']) < 1e-3
    assert a['wire_dtype'] == 'bf16' and len(a['bucket_mbytes']) == a['buckets']
    # the diagnostics of the one hardware run: per-bucket all-reduce time (host-issued route), the step with the exchange off
    host = a if a['route'].startswith('host-issued') else b
    dg = host['diagnostics']
    assert 'error' not in dg, dg
    assert len(dg['allreduce_ms_per_bucket']) == host['buckets'] and dg['ms_per_step_exchange_off'] > 0
    assert 'exposed_exchange_ms_per_step' in dg and 'ms_per_step_exchange_off' in nat['diagnostics']


def test_bench_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run times exactly --steps steps of the headline workload and nothing else (the secondary
    measurements are behind --full); --dump-outputs writes float .npy files, and two runs with the same arguments write the same
    outputs up to float round-off."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'VITAE_BENCH_ONE_GPU', 'VITAE_FORCE_DDP', 'RANK', 'LOCAL_RANK')}
    dumps = []
    for run in range(2):
        out_dir = tmp_path / f'outputs{run}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                            '--dump-outputs', str(out_dir)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1 and d['dtype'] == 'bf16'
        assert d['unit'] == 'volumes/s' and d['higher_is_better'] is True and d['value'] > 0 and d['ms_per_step'] > 0
        assert d['roofline'] is None and d['cpu_baseline'] is None and 'parity' not in d
        assert d['config']['also_exchange'] is None and not [k for k in d['config'] if k.startswith('also_') and k != 'also_exchange']
        files = sorted(p.name for p in out_dir.iterdir())
        assert files == ['grads_sample.npy', 'losses.npy', 'params_sample.npy'], files
        arrays = {f: np.load(out_dir / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays['losses.npy'][5] > 0                      # the step's global gradient norm
        dumps.append(arrays)
    # round-off only: some gradients are summed with float atomics in an order that varies from run to run (measured: losses and
    # parameters bitwise equal, a few gradient elements apart by ~1e-7 relative)
    a, b = dumps
    np.testing.assert_allclose(b['losses.npy'], a['losses.npy'], rtol=1e-6, atol=0)
    for f in ('params_sample.npy', 'grads_sample.npy'):
        np.testing.assert_allclose(b[f], a[f], rtol=1e-5, atol=1e-6 * float(np.abs(a[f]).max()), err_msg=f)
