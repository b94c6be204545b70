"""Times the league paths of MultiSnake against what they stand beside, in one process, alternating, with HIP events:

  * `act_league` with the block line-up `lineup[k, :] = k * P // K` against `act` at the same shape — the same work, the
    rows found through an index list instead of a range;
  * a step of `league_window` with R distinct matchups in ONE env object of N envs against a step of R env objects of
    N / R envs each through `act_window`, each with its matchup's rows of `params` — the same envs, the same policies.

Writes profiles/r26_multi_league.jsonl: one line per (shape, what) with the median and the range over the repeats, in
microseconds (per call, and per step of the whole batch of N envs).

    python tools/bench_multi_league.py [--repeats 9] [--iters 300] [--window 10] [--out profiles/r26_multi_league.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent, pack_policy_params  # noqa: E402
from wurm_amd.envs import MultiSnake, _multi_league  # noqa: E402

# (num_envs, size, num_snakes, observation n, species of the block line-up, matchups R of the window comparison)
SHAPES = [(512, 12, 2, 2, 2, (8, 64)), (4096, 25, 4, 5, 2, (8, 64))]
POLICIES = 16   # the league the matchups are drawn from


def timed(fn, iters):
    """microseconds per call of `fn` over `iters` calls between two HIP events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def make_env(N, S, K, n, seed=1):
    return MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=f'partial_{n}', device='cuda', boost=False,
                      food_mode='random_rate', respawn_mode='any', seed=seed)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--window', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'r26_multi_league.jsonl'))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_multi_league needs the GPU: nothing is timed without one')
    count = _lib.lib().wurm_launch_count
    lines = []

    def run(shape, what, extra=None):
        """what: (name, fn, iters, steps per call); alternating samples, one line each"""
        for _, fn, _, _ in what:   # warm-up: code objects, the allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _, _, _ in what}
        for _ in range(args.repeats):
            for name, fn, iters, per in what:
                samples[name].append(timed(fn, iters) / per)
        for name, _, iters, per in what:
            xs = samples[name]
            line = {'shape': shape, 'what': name, 'unit': 'us', 'median': round(statistics.median(xs), 2),
                    'min': round(min(xs), 2), 'max': round(max(xs), 2), 'repeats': args.repeats,
                    'calls_per_sample': iters * per}
            line.update((extra or {}).get(name, {}))
            lines.append(line)
            print(json.dumps(line), flush=True)

    for N, S, K, n, P, matchups in SHAPES:
        E = 3 * (2 * n + 1) ** 2
        shape = f'{N}x{S}x{S}x{K} partial_{n}'
        torch.manual_seed(0)
        params = torch.stack([pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E))
                              for _ in range(POLICIES)]).to('cuda')
        env = make_env(N, S, K, n)
        state = env.reset()
        block = env.league_plan(_multi_league.block_lineup(K, N, P, 'cuda'), P)
        species = params[:P].contiguous()
        run(shape, [('act', lambda: env.act(species, state), args.iters, 1),
                    ('act_league_block_lineup', lambda: env.act_league(species, state, block), args.iters, 1)],
            {name: {'num_species': P} for name in ('act', 'act_league_block_lineup')})

        T, iters = args.window, max(1, args.iters // (4 * args.window))
        for R in matchups:
            g = torch.Generator().manual_seed(R)
            teams = torch.stack([torch.randperm(POLICIES, generator=g)[:K] for _ in range(R)])   # (R, K): matchup r's policies
            M = N // R
            lineup = teams.t().repeat_interleave(M, dim=1).contiguous().to('cuda')                  # env i plays matchup i // M
            league = make_env(N, S, K, n)
            plan = league.league_plan(lineup, POLICIES)
            box = {'state': league.reset()}
            parts = [make_env(M, S, K, n, seed=2 + r) for r in range(R)]
            part_params = [params[teams[r].to('cuda')].contiguous() for r in range(R)]             # one row per snake
            part_state = [e.reset() for e in parts]

            def league_window():
                box['state'] = league.league_window(params, box['state'], T, plan)['state']

            def object_windows():
                for r, e in enumerate(parts):
                    part_state[r] = e.act_window(part_params[r], part_state[r], T, num_species=K)['state']

            torch.cuda.synchronize()
            before = count()
            league_window()
            one = (count() - before) / T
            before = count()
            object_windows()
            many = (count() - before) / T
            names = (f'league_window_step_{R}_matchups', f'act_window_step_{R}_objects_of_{M}_envs')
            run(shape, [(names[0], league_window, iters, T), (names[1], object_windows, iters, T)],
                {names[0]: {'matchups': R, 'policies': POLICIES, 'library_launches_per_step': one},
                 names[1]: {'matchups': R, 'policies': POLICIES, 'library_launches_per_step': many}})
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
