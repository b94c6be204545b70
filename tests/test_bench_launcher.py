"""bench.py --gpus N must start its own N ranks: the parent spawns a fresh torch.distributed.run
child before touching any GPU and relays rank 0's JSON line.  Exercised here with --dry-run (gloo on CPU, the rollout
launch replaced by a sleep): rendezvous, barrier, max-over-ranks time, summed env-steps, one JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, env=None):
    e = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *flags], capture_output=True, text=True,
                       env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks():
    d = _run('--gpus', '2', '--dry-run', '--full', '--steps', '3', '--warmup', '1')
    assert d['n_gpus'] == 2 and d['config']['world_size'] == 2 and d['config']['backend'] == 'gloo'
    assert d['steps'] == 3 and d['warmup'] == 1 and d['scaling'] == 'weak'
    # whole-job value: both ranks' env-steps over the max-over-ranks time
    per_launch = d['config']['env_steps_per_launch_per_gpu']
    assert abs(d['value'] - 2 * 3 * per_launch / (d['ms_per_step'] * 1e-3 * 3)) / d['value'] < 1e-6
    assert 'cpu_baseline' not in d and 'extra' not in d
    # BASELINE configs[2] split over the two ranks rides along with the weak-scaling headline
    c3 = d['cfg3_strong_scaling']
    assert c3['global_num_envs'] == 65536 and c3['num_envs_per_gpu'] == 32768 and c3['scaling'] == 'strong'
    assert c3['value'] > 0 and c3['steps'] == 3


def test_cfg3_is_split_over_the_ranks():
    d = _run('--gpus', '2', '--dry-run', '--full', '--steps', '2', '--warmup', '0', '--workload', 'cfg3')
    assert d['config']['global_num_envs'] == 65536 and d['config']['num_envs_per_gpu'] == 32768
    assert d['scaling'] == 'strong' and d['config']['baseline_config'] == 'BASELINE.json configs[2]'
    assert abs(d['cfg3_strong_scaling']['value'] - d['value']) / d['value'] < 1e-9   # the same region, not timed twice


def test_single_process_default_and_cpu_baseline_legs():
    d = _run('--dry-run', '--full', '--steps', '2', '--warmup', '1')
    assert d['n_gpus'] == 1 and d['config']['world_size'] == 1
    assert str(d['config']['batch_steps_per_launch']) in d['config']['workload']
    cb = d['cpu_baseline']
    assert cb['kind'] == 'port' and cb['value'] > 0 and cb['cores'] >= 1
    assert cb['c_port_1thread']['value'] > 0 and cb['c_port_allcores']['value'] > 0


def test_worker_under_an_external_torchrun():
    """the driver's own launch line for N > 1: python -m torch.distributed.run ... bench.py --gpus N"""
    from bench import free_port
    e = dict(os.environ)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', str(free_port()),
                        os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dry-run', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    assert json.loads(lines[0])['n_gpus'] == 2


def test_world_size_8_with_an_uneven_global_batch():
    """the 8-GPU shape north_star names, on gloo: 65 537 envs do not divide by 8 — every rank gets a contiguous block,
    the blocks tile the batch, the line's key numbers carry the strong-scaling value"""
    d = _run('--gpus', '8', '--dry-run', '--full', '--steps', '2', '--warmup', '0', '--workload', 'cfg3',
             '--num-envs', '65537')
    assert d['n_gpus'] == 8 and d['config']['world_size'] == 8 and d['scaling'] == 'strong'
    assert d['config']['global_num_envs'] == 65537
    assert d['config']['num_envs_per_gpu'] == 8193            # rank 0's block: the remainder goes to the first ranks
    assert d['value'] > 0 and d['key']['cfg3_strong_scaling_eps'] > 0
    from wurm_amd.sharding import shard_range
    blocks = [shard_range(65537, r, 8) for r in range(8)]
    assert blocks[0][0] == 0 and sum(n for _, n in blocks) == 65537
    assert all(blocks[i][0] + blocks[i][1] == blocks[i + 1][0] for i in range(7))
    assert max(n for _, n in blocks) - min(n for _, n in blocks) == 1
    # every rank's own record rides in the line (device, shard, communicator init, launch time): VERDICT r04 #9
    ranks = d['ranks']
    assert [r['rank'] for r in ranks] == list(range(8))
    assert [(r['env_offset'], r['num_envs']) for r in ranks] == blocks
    assert all(r['comm_init_s'] >= 0 and r['avg_launch_ms'] > 0 for r in ranks)


def test_plain_run_times_the_headline_only():
    """without --full the line carries the headline region and nothing that takes runs of its own"""
    d = _run('--dry-run', '--steps', '3', '--warmup', '1')
    assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0
    assert d['metric'] == 'env_steps_per_s' and d['unit'] == 'env-steps/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'i32'
    assert 'cfg3_strong_scaling' not in d and 'cpu_baseline' not in d and 'extra' not in d
    assert d['key']['cfg3_strong_scaling_eps'] is None


def test_dump_outputs_keeps_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    """dump_outputs() on host tensors of a rollout's shapes: float32 files, the byte budget, the same sample twice"""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 300_000)
    T, N = 40, 64
    g = torch.Generator().manual_seed(0)
    out = {'observations': torch.rand((T, N, 3, 5, 5), generator=g), 'rewards': torch.rand((T, N), generator=g),
           'dones': torch.rand((T, N), generator=g) < 0.5, 'self_collision': torch.zeros((T, N), dtype=torch.bool),
           'edge_collision': torch.ones((T, N), dtype=torch.bool)}
    state = torch.rand((N, 3, 9, 9), generator=g)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), out, state)
    files = sorted(p.name for p in (tmp_path / 'a').iterdir())
    assert files == ['dones.npy', 'edge_collision.npy', 'observations.npy', 'rewards.npy', 'self_collision.npy',
                     'state.npy']
    assert sum(p.stat().st_size for p in (tmp_path / 'a').iterdir()) <= 300_000 + 6 * 128
    a = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    for f in files:
        assert a[f[:-4]].dtype == np.float32
        assert np.array_equal(a[f[:-4]], np.load(tmp_path / 'b' / f))
    rows = a['rewards'].shape[0]
    assert 0 < rows < T * N and a['observations'].shape == (rows, 3, 5, 5)
    # the sampled rows are the same rows in every per-step file
    flat_r, flat_o = out['rewards'].reshape(-1).numpy(), out['observations'].reshape(T * N, -1).numpy()
    idx = np.flatnonzero(np.isin(flat_r, a['rewards']))
    assert len(idx) == rows and np.array_equal(flat_o[idx], a['observations'].reshape(rows, -1))
    assert a['state'].shape == (N, 3, 9, 9) and np.array_equal(a['state'], state.numpy())  # (fits: kept whole)


@pytest.mark.gpu
def test_dump_outputs_on_the_gpu_are_identical_from_run_to_run(tmp_path):
    """two runs with the same arguments dump the same arrays (the inputs are seeded), under 64 MB in all"""
    import numpy as np
    for d in ('a', 'b'):
        line = _run('--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / d))
        assert line['steps'] == 2 and 'extra' not in line
    files = sorted(p.name for p in (tmp_path / 'a').iterdir())
    assert 'observations.npy' in files and 'rewards.npy' in files and 'state.npy' in files
    assert sum(p.stat().st_size for p in (tmp_path / 'a').iterdir()) < 64 * 10**6
    for f in files:
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    assert np.load(tmp_path / 'a' / 'state.npy').shape == (512, 3, 9, 9)
