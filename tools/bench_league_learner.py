"""Times `FusedA2CPopulation.update(state, out, plan=plan)` — A policies learning from one league window, each from the
columns its line-up gives it — against what it stands beside, in one process, alternating, with HIP events:

  (a) the same work without it: per policy an `index_select` of the start observations and of the window's four tensors
      by the policy's list, then a `FusedA2CLearner.update` on the copies — A x 5 copies and 3 A launches.  The lists are
      split on the host beforehand and not timed.
  (b) with the block line-up `lineup[k, :] = k * P // K`, `FusedA2CPopulation.update` of the same window WITHOUT a plan
      (members = consecutive blocks): the same grid and arithmetic, so the difference is the price of the indirection
      and of sizing the members on the device.  P has to divide K, so this runs at P = 2 (and 4 where K = 4).

The windows are synthetic (the learner takes tensors): R = num_snakes x num_envs columns of crops of zeros and ones.
Line-ups: 'balanced' draws every row's policy uniformly; 'skewed' gives policy a a share proportional to 2^-a, so
policy 0 plays about half the rows and the last ones a handful — the grid is sized by A, not by rows per policy, and
most of a small member's workgroups return at once.

Writes profiles/r27_league_learner.jsonl: one line per (shape, A, T, line-up, what) with the median and the range over
the repeats in microseconds per update of all A policies.

    python tools/bench_league_learner.py [--repeats 7] [--sample-ms 60] [--out profiles/r27_league_learner.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import MultiSnake, _multi_league  # noqa: E402
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation  # noqa: E402

# (num_envs, size, num_snakes, observation n)
SHAPES = [(512, 12, 2, 2), (4096, 25, 4, 5)]
POLICIES = (2, 16)
STEPS = (5, 20)
KEYS = ('observations', 'actions', 'rewards', 'dones')


def timed(fn, iters):
    """microseconds per call of `fn` over `iters` calls between two HIP events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def agents(A, E):
    return [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to('cuda') for _ in range(A)]


def window(R, T, E, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    rand = lambda *shape: torch.rand(shape, generator=g, device='cuda')
    out = {'observations': (rand(T, R, E) < 0.3).float(), 'actions': (rand(T, R) * 4).long().clamp_(0, 3),
           'rewards': (rand(T, R) < 0.1).float() - (rand(T, R) < 0.05).float(), 'dones': rand(T, R) < 0.05}
    return (rand(R, E) < 0.3).float(), out


def draw_lineup(kind, K, N, A, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'balanced':
        return torch.randint(A, (K, N), generator=g)
    weights = torch.tensor([2.0 ** -a for a in range(A)])
    return torch.multinomial(weights, K * N, replacement=True, generator=g).view(K, N)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sample-ms', type=float, default=60.0, help='about this much device time per sample')
    ap.add_argument('--out', default=os.path.join('profiles', 'r27_league_learner.jsonl'))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_league_learner needs the GPU: nothing is timed without one')
    count = _lib.lib().wurm_launch_count
    lines = []

    def run(tags, what):
        """what: (name, fn) pairs; alternating samples, one line each"""
        iters, launches = {}, {}
        for name, fn in what:   # warm-up (code objects, the allocator, the workspaces), launches, and how many calls fill a sample
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            before = count()
            fn()
            launches[name] = count() - before
            iters[name] = int(min(400, max(5, args.sample_ms * 1e3 / timed(fn, 5))))
        samples = {name: [] for name, _ in what}
        for _ in range(args.repeats):
            for name, fn in what:
                samples[name].append(timed(fn, iters[name]))
        for name, _ in what:
            xs = samples[name]
            line = dict(tags, what=name, unit='us per update of all policies', median=round(statistics.median(xs), 1),
                        min=round(min(xs), 1), max=round(max(xs), 1), repeats=args.repeats,
                        calls_per_sample=iters[name], library_launches_per_update=launches[name])
            lines.append(line)
            print(json.dumps(line), flush=True)

    for N, S, K, n in SHAPES:
        E, R = 3 * (2 * n + 1) ** 2, K * N
        shape = f'{N}x{S}x{S}x{K} partial_{n}'
        env = MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=f'partial_{n}', device='cuda', boost=False,
                         food_mode='random_rate', respawn_mode='any', seed=1)   # (for league_plan: the window is synthetic)
        for T in STEPS:
            state, out = window(R, T, E, seed=T)
            for A in POLICIES:                                    # ---- (a) against per-policy copies and learners
                for kind in ('balanced', 'skewed'):
                    torch.manual_seed(0)
                    plan = env.league_plan(draw_lineup(kind, K, N, A, seed=A).to('cuda'), A)
                    offsets = plan.offsets.tolist()
                    lists = [plan.order[offsets[a]:offsets[a + 1]].long() for a in range(A)]
                    pop = FusedA2CPopulation(agents(A, E), entropy_coef=0.01)
                    singles = [FusedA2CLearner(agent, entropy_coef=0.01) for agent in agents(A, E)]

                    def league():
                        pop.update(state, out, plan=plan)

                    def per_policy():
                        for single, idx in zip(singles, lists):
                            if len(idx):
                                single.update(state.index_select(0, idx), {k: out[k].index_select(1, idx) for k in KEYS})

                    rows = [len(idx) for idx in lists]
                    run({'shape': shape, 'rows': R, 'policies': A, 'steps': T, 'lineup': kind, 'rows_per_policy_min': min(rows),
                         'rows_per_policy_max': max(rows)},
                        [('league_update', league), ('index_select_and_learner_per_policy', per_policy)])
            for P in (p for p in (2, 4) if K % p == 0 and p <= K):  # ---- (b) against the population on the block line-up
                plan = env.league_plan(_multi_league.block_lineup(K, N, P, 'cuda'), P)
                torch.manual_seed(0)
                with_plan, without = (FusedA2CPopulation(agents(P, E), entropy_coef=0.01) for _ in range(2))
                run({'shape': shape, 'rows': R, 'policies': P, 'steps': T, 'lineup': 'block', 'rows_per_policy_min': R // P,
                     'rows_per_policy_max': R // P},
                    [('league_update', lambda: with_plan.update(state, out, plan=plan)),
                     ('population_update_without_plan', lambda: without.update(state, out))])
            del state, out
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
