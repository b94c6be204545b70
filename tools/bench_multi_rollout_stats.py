#!/usr/bin/env python3
"""What the logging of the fused multi-agent training loop costs: one window of examples/a2c_multi_species.py
(`act_window(..., info=True)` + `FusedA2CPopulation.update` + logging), timed three ways in the same process on the same
device, alternating, with HIP events after warm-up:

    stats   `MultiRolloutStats.update(out)`: two launches, every per-agent log column and its smoothed version
    torch   the reference's log lines (experiments/multiagent.py:486-505) restated as torch masked means over the window's
            (T, K, N) tensors, smoothed with the tracker's weights, all of it left on the device (about forty torch kernels;
            an empty mask gives NaN as in the reference)
    none    no logging at all

MultiSnake 512 x 12 x 12 x 2 snakes 'partial_2' and 4096 x 25 x 25 x 4 snakes 'partial_5', two species, T in {5, 20}.  The
three loops advance their own env and learner from the same seed, so each times the same work.  One JSON line per
(config, T), appended to profiles/r21_multi_rollout_stats.jsonl (or --out).  Needs the GPU.

    tools/bench_multi_rollout_stats.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, MultiRolloutStats  # noqa: E402

CONFIGS = [dict(num_envs=512, size=12, num_snakes=2, n=2), dict(num_envs=4096, size=25, num_snakes=4, n=5)]
SPECIES = 2
EPS32 = 1.1920928955078125e-07


def torch_log_lines(out, T, K, N, alpha, state):
    """multiagent.py:493-502 for every agent and step of the window at once, and the tracker over the T steps"""
    view = lambda name: out[name].view(T, K, N)
    done = view('dones')
    alive = ~done
    n_alive, n_done = alive.sum(-1, dtype=torch.float64), done.sum(-1, dtype=torch.float64)
    p = out['probs'].view(T, K, N, 4)
    entropy = -(p * torch.log(p.clamp(EPS32, 1 - EPS32))).sum(-1)
    over = lambda x, mask, n: (x * mask).sum(-1, dtype=torch.float64) / n
    size = view('size')
    table = torch.stack([over(view('rewards'), alive, n_alive), over(entropy, alive, n_alive),
                         over(view('food'), alive, n_alive), view('edge_collision').float().mean(-1, dtype=torch.float64),
                         view('snake_collision').float().mean(-1, dtype=torch.float64),
                         over(view('boost'), alive, n_alive), over(size, alive, n_alive),
                         done.float().mean(-1, dtype=torch.float64), over(size, done, n_done)])          # (9, T, K)
    weights = alpha * (1 - alpha) ** torch.arange(T - 1, -1, -1, dtype=torch.float64, device=table.device)
    state['smooth'] = (1 - alpha) ** T * state['smooth'] + (weights[None, :, None] * table).sum(1)
    state['episodes'] += out['all_done'].sum()


def make_window(kind, cfg, T, dev):
    """one training window with the logging `kind`, as a callable"""
    N, K, n = cfg['num_envs'], cfg['num_snakes'], cfg['n']
    E = 3 * (2 * n + 1) ** 2
    env = MultiSnake(num_envs=N, num_snakes=K, size=cfg['size'], observation_mode=f'partial_{n}', device=dev,
                     boost=False, food_mode='random_rate', respawn_mode='any', seed=0)
    agents = []
    for p in range(SPECIES):
        torch.manual_seed(p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(dev))
    learner = FusedA2CPopulation(agents, lr=1e-3, gamma=0.99, entropy_coef=0.01)
    box = {'state': env.reset()}
    stats = MultiRolloutStats(env) if kind == 'stats' else None
    logged = {'smooth': torch.zeros((9, K), dtype=torch.float64, device=dev),
              'episodes': torch.zeros((), dtype=torch.long, device=dev)}

    def window():
        state = box['state']
        out = env.act_window(learner.params, state, T, info=kind != 'none')
        learner.update(torch.stack(list(state.values())).reshape(K * N, E), out)
        box['state'] = out['state']
        if kind == 'stats':
            stats.update(out)
        elif kind == 'torch':
            torch_log_lines(out, T, K, N, 0.025, logged)
    return window


def time_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_multi_rollout_stats.jsonl'))
    ap.add_argument('--steps', type=int, nargs='+', default=[5, 20])
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_multi_rollout_stats.py needs the GPU: a time taken anywhere else says nothing')
    dev, kinds = 'cuda:0', ('stats', 'torch', 'none')
    for cfg in CONFIGS:
        for T in a.steps:
            windows = {k: make_window(k, cfg, T, dev) for k in kinds}
            launches = {}
            for k in kinds:
                for _ in range(a.warmup):
                    windows[k]()
                torch.cuda.synchronize()
                before = _lib.lib().wurm_launch_count()
                windows[k]()
                launches[k] = _lib.lib().wurm_launch_count() - before  # (the library's own kernels: torch's are not counted)
            times = {k: [] for k in kinds}
            for _ in range(a.reps):          # alternating: drift of the machine lands on all three
                for k in kinds:
                    times[k].append(time_ms(windows[k], a.inner))
            med = {k: statistics.median(v) for k, v in times.items()}
            row = dict(what='multi_rollout_stats_window', device=torch.cuda.get_device_name(0), num_envs=cfg['num_envs'],
                       size=cfg['size'], num_snakes=cfg['num_snakes'], observation=f"partial_{cfg['n']}", species=SPECIES,
                       steps=T, library_launches_per_window=launches,
                       **{f'{k}_ms': round(med[k], 4) for k in kinds},
                       **{f'{k}_ms_range': [round(min(times[k]), 4), round(max(times[k]), 4)] for k in kinds},
                       stats_minus_none_ms=round(med['stats'] - med['none'], 4),
                       torch_minus_none_ms=round(med['torch'] - med['none'], 4),
                       stats_over_torch=round(med['stats'] / med['torch'], 3), reps=a.reps, windows_per_rep=a.inner)
            print(json.dumps(row), flush=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
