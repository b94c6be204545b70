"""Times the league's matchmaking on the device against the path it stands beside, in one process, alternating, with HIP
events:

  * `league_draw` (one launch for the draw, the plan builder's launches behind it) and `league_plan(sync=False)` alone,
    against the host path: `draw_lineup` on the CPU with a torch.Generator (examples/league_eval.py), the copy to the
    device, `league_plan` with its torch sort and the range check it reads back;
  * a window of examples/league_selfplay.py — `league_window`, `FusedA2CPopulation.update(plan=...)`, `LeagueTable.update`
    — with a redraw in front of EVERY window, both ways.

The host path occupies the host, not only the stream: its figure is what the loop waits for it, measured between two events
on an otherwise idle stream.  Writes profiles/r29_league_draw.jsonl: one line per (shape, policies, what) with the median
and the range over the repeats, in microseconds per call.

    python tools/bench_league_draw.py [--repeats 9] [--iters 100] [--window 10] [--out profiles/r29_league_draw.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.league_eval import draw_lineup  # noqa: E402
from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, LeagueTable  # noqa: E402

# (num_envs, size, num_snakes, observation n)
SHAPES = [(512, 12, 2, 2), (4096, 25, 4, 5)]
POLICIES = (16, 256)


def timed(fn, iters):
    """microseconds per call of `fn` over `iters` calls between two HIP events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--window', type=int, default=10, help='steps of the self-play window')
    ap.add_argument('--out', default=os.path.join('profiles', 'r29_league_draw.jsonl'))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_league_draw needs the GPU: nothing is timed without one')
    count = _lib.lib().wurm_launch_count
    lines = []

    def run(shape, A, what):
        """what: (name, fn, iters); alternating samples, one line each"""
        launches = {}
        for name, fn, _ in what:   # warm-up: code objects, the allocator
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            before = count()
            fn()
            launches[name] = count() - before
        torch.cuda.synchronize()
        samples = {name: [] for name, _, _ in what}
        for _ in range(args.repeats):
            for name, fn, iters in what:
                samples[name].append(timed(fn, iters))
        for name, _, iters in what:
            xs = samples[name]
            line = {'shape': shape, 'policies': A, 'what': name, 'unit': 'us', 'median': round(statistics.median(xs), 2),
                    'min': round(min(xs), 2), 'max': round(max(xs), 2), 'repeats': args.repeats, 'calls_per_sample': iters,
                    'library_launches': launches[name]}
            lines.append(line)
            print(json.dumps(line), flush=True)

    for N, S, K, n in SHAPES:
        E = 3 * (2 * n + 1) ** 2
        shape = f'{N}x{S}x{S}x{K} partial_{n}'
        for A in POLICIES:
            env = MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=f'partial_{n}', device='cuda', boost=False,
                             food_mode='random_rate', respawn_mode='any', seed=1)
            g = torch.Generator().manual_seed(0)
            lineup = draw_lineup(A, K, N, False, g).to('cuda')
            tickets = torch.arange(A, 0, -1, dtype=torch.int32, device='cuda')

            def host_path():
                return env.league_plan(draw_lineup(A, K, N, False, g).to('cuda'), A)

            run(shape, A, [('host draw_lineup + copy + league_plan', host_path, max(1, args.iters // 4)),
                           ('league_draw', lambda: env.league_draw(A), args.iters),
                           ('league_draw with tickets', lambda: env.league_draw(A, tickets=tickets), args.iters),
                           ('league_plan(sync=True) alone', lambda: env.league_plan(lineup, A), args.iters),
                           ('league_plan(sync=False) alone', lambda: env.league_plan(lineup, A, sync=False), args.iters)])

            # the self-play window with a redraw in front of every window
            T = args.window

            def loop(device_draw):
                torch.manual_seed(0)   # (a population takes its agents' parameters into its own buffer: a set each)
                agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to('cuda') for _ in range(A)]
                pop, table = FusedA2CPopulation(agents, lr=1e-3, gamma=0.99, entropy_coef=0.01), LeagueTable(A, env.device)
                box = {'state': env.reset()}

                def window():
                    plan = env.league_draw(A) if device_draw else host_path()
                    out = env.league_window(pop.params, box['state'], T, plan, info=True)
                    pop.update(box['state'], out, plan=plan)
                    table.update(plan, out)
                    box['state'] = out['state']
                return window

            iters = max(1, args.iters // (2 * T))
            run(shape, A, [(f'selfplay window of {T} steps, host redraw', loop(False), iters),
                           (f'selfplay window of {T} steps, device redraw', loop(True), iters)])
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
