"""Times `MultiSnake.act` and a step of `MultiSnake.act_window` against the torch acting path they replace — per agent a
`FeedforwardAgent` forward, `Categorical(probs).sample()` and `.clone().long()` (experiments/multiagent.py:354-364) — in the
same process, alternating, with HIP events.  Writes profiles/r19_multi_act.jsonl: one line per (shape, what) with the
median and the range over the repeats, in microseconds.

    python tools/bench_multi_act.py [--repeats 9] [--iters 500] [--out profiles/r19_multi_act.jsonl]
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
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation  # noqa: E402

# (num_envs, size, num_snakes, observation n, species)
SHAPES = [(4096, 25, 4, 5, 2), (512, 12, 2, 2, 2)]


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
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'r19_multi_act.jsonl'))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_multi_act needs the GPU: nothing is timed without one')
    count = _lib.lib().wurm_launch_count
    lines = []
    for N, S, K, n, P in SHAPES:
        E = 3 * (2 * n + 1) ** 2
        torch.manual_seed(0)
        env = MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=f'partial_{n}', device='cuda', boost=False,
                         food_mode='random_rate', respawn_mode='any', seed=1)
        agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to('cuda') for _ in range(P)]
        params = FusedA2CPopulation(agents).params
        state = env.reset()
        box = {'state': state}

        def act():
            env.act(params, box['state'])

        def torch_act():   # multiagent.py:354-364
            with torch.no_grad():
                for i, (agent, obs) in enumerate(box['state'].items()):
                    probs, _ = agents[i * P // K](obs.reshape(N, E))
                    torch.distributions.Categorical(probs).sample().clone().long()

        def window():
            box['state'] = env.act_window(params, box['state'], args.window)['state']

        def torch_window():
            with torch.no_grad():
                for _ in range(args.window):
                    actions = {}
                    for i, (agent, obs) in enumerate(box['state'].items()):
                        probs, _ = agents[i * P // K](obs.reshape(N, E))
                        actions[agent] = torch.distributions.Categorical(probs).sample().clone().long()
                    obs, _, dones, _ = env.step(actions)
                    env.reset(dones['__all__'], return_observations=False)
                    box['state'] = obs

        what = [('act', act, args.iters, 1), ('torch_act', torch_act, args.iters, 1),
                ('act_window_step', window, max(1, args.iters // args.window), args.window),
                ('torch_loop_step', torch_window, max(1, args.iters // args.window), args.window)]
        for _, fn, _, _ in what:   # warm-up: code objects, the allocator, torch's kernels
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        before = count()
        window()
        launches = (count() - before) / args.window
        samples = {name: [] for name, _, _, _ in what}
        for _ in range(args.repeats):   # alternating: one sample of each per round
            for name, fn, iters, per in what:
                samples[name].append(timed(fn, iters) / per)
        for name, _, iters, per in what:
            xs = samples[name]
            line = {'shape': f'{N}x{S}x{S}x{K} partial_{n}', 'num_species': P, 'what': name, 'unit': 'us',
                    'median': round(statistics.median(xs), 2), 'min': round(min(xs), 2), 'max': round(max(xs), 2),
                    'repeats': args.repeats, 'calls_per_sample': iters * per}
            if name == 'act_window_step':
                line['library_launches_per_step'] = launches
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
