#!/usr/bin/env python3
"""What the logging of the fused training loop costs: one window (rollout + update + statistics) of
examples/a2c_fused_learner.py (P = 1) or examples/a2c_population.py (P > 1), timed three ways in the same process on the
same device, alternating, with HIP events after warm-up:

    stats   `RolloutStats.update(out)`: two launches, every log column
    sums    the two torch sums the examples had before (`reward_rate`, `done_rate` only), added to a device total
    none    no logging at all

SingleSnake 512 x 9 x 9 partial_2 per member, T in {5, 20}, P in {1, 16}.  The three loops advance their own env and
learner from the same seed, so each times the same work.  One JSON line per (T, P), appended to
profiles/r15_rollout_stats.jsonl (or --out).  Needs the GPU.

    tools/bench_rollout_stats.py
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
from wurm_amd.envs import SingleSnake  # noqa: E402
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation, RolloutStats  # noqa: E402


def make_window(kind, P, M, T, dev):
    """one training window of P members x M envs with the logging `kind`, as a callable"""
    env = SingleSnake(num_envs=P * M, size=9, observation_mode='partial_2', device=dev, seed=0)
    box = {'state': env.reset()}
    agents = []
    for p in range(P):
        torch.manual_seed(p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75).to(dev))
    if P == 1:
        learner = FusedA2CLearner(agents[0], lr=1e-3, gamma=0.99, entropy_coef=0.01)
        population = None
    else:
        learner = FusedA2CPopulation(agents, lr=1e-3, gamma=0.99, entropy_coef=0.01)
        population = P
    stats = RolloutStats(env, population=population) if kind == 'stats' else None
    totals = torch.zeros((2, P), dtype=torch.float64, device=dev)

    def window():
        out = env.policy_rollout(learner.params, box['state'], T, check=False, population=population)
        learner.update(box['state'], out)
        box['state'] = out['state']
        if kind == 'stats':
            stats.update(out)
        elif kind == 'sums' and P == 1:    # the expression of the examples before RolloutStats
            totals[:, 0] += torch.stack([out['rewards'].sum(dtype=torch.float64), out['dones'].sum(dtype=torch.float64)])
        elif kind == 'sums':
            totals.add_(torch.stack([out['rewards'].view(T, P, M).sum(dim=(0, 2), dtype=torch.float64),
                                     out['dones'].view(T, P, M).sum(dim=(0, 2), dtype=torch.float64)]))
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_rollout_stats.jsonl'))
    ap.add_argument('--envs', type=int, default=512, help='envs per member')
    ap.add_argument('--members', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--steps', type=int, nargs='+', default=[5, 20])
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rollout_stats.py needs the GPU: a time taken anywhere else says nothing')
    dev, M, kinds = 'cuda:0', a.envs, ('stats', 'sums', 'none')
    for T in a.steps:
        for P in a.members:
            windows = {k: make_window(k, P, M, T, dev) for k in kinds}
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
            row = dict(what='rollout_stats_window', device=torch.cuda.get_device_name(0), size=9, observation='partial_2',
                       envs_per_member=M, members=P, steps=T, library_launches_per_window=launches,
                       **{f'{k}_ms': round(med[k], 4) for k in kinds},
                       **{f'{k}_ms_range': [round(min(times[k]), 4), round(max(times[k]), 4)] for k in kinds},
                       stats_minus_none_ms=round(med['stats'] - med['none'], 4),
                       sums_minus_none_ms=round(med['sums'] - med['none'], 4),
                       stats_over_sums=round(med['stats'] / med['sums'], 3), reps=a.reps, windows_per_rep=a.inner)
            print(json.dumps(row), flush=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
