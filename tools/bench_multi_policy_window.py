"""Times `MultiSnake.policy_window` (one launch per window) against `MultiSnake.act_window` (two launches per step) in the
same process, alternating repeat by repeat, with HIP events.  Two envs of equal configuration and seed, one per path, each
fed its own last observations; T in {5, 20}, two species, with and without info=True.  Writes
profiles/r23_multi_policy_window.jsonl: one line per (shape, T, info, what) with the median and the range over the repeats,
in milliseconds per window and microseconds per step.  A figure between two events is the time of the whole loop as the
stream saw it — host work included wherever the stream ran dry — which is exactly what the caller of a window pays.

    python tools/bench_multi_policy_window.py [--repeats 9] [--iters 40] [--out profiles/r23_multi_policy_window.jsonl]
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

# (num_envs, size, num_snakes, observation n, species): the reference's test shape, and the training shape with the largest
# crop the kernel fuses
SHAPES = [(512, 12, 2, 2, 2), (4096, 25, 4, 3, 2)]
WINDOWS = (5, 20)


def timed(fn, iters):
    """milliseconds per call of `fn` over `iters` calls between two HIP events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--iters', type=int, default=40, help='windows per sample')
    ap.add_argument('--out', default=os.path.join('profiles', 'r23_multi_policy_window.jsonl'))
    args = ap.parse_args(argv)
    if args.repeats < 9:
        raise SystemExit('bench_multi_policy_window: at least 9 alternating repeats')
    if not torch.cuda.is_available():
        raise SystemExit('bench_multi_policy_window needs the GPU: nothing is timed without one')
    count = _lib.lib().wurm_launch_count
    lines = []
    for N, S, K, n, P in SHAPES:
        E = 3 * (2 * n + 1) ** 2
        torch.manual_seed(0)
        agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to('cuda') for _ in range(P)]
        params = FusedA2CPopulation(agents).params
        envs, box = {}, {}
        for name in ('policy_window', 'act_window'):
            envs[name] = MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=f'partial_{n}', device='cuda',
                                    boost=False, food_mode='random_rate', respawn_mode='any', seed=1)
            box[name] = envs[name].reset()
        assert envs['policy_window'].policy_window_fused(P)
        for T in WINDOWS:
            for info in (False, True):
                def run(name):
                    box[name] = getattr(envs[name], name)(params, box[name], T, info=info)['state']

                launches = {}
                for name in envs:   # warm-up: code objects, the allocator
                    for _ in range(3):
                        run(name)
                    torch.cuda.synchronize()
                    before = count()
                    run(name)
                    launches[name] = count() - before
                samples = {name: [] for name in envs}
                for _ in range(args.repeats):   # alternating: one sample of each per round
                    for name in envs:
                        samples[name].append(timed(lambda: run(name), args.iters))
                for name in envs:
                    xs = samples[name]
                    med = statistics.median(xs)
                    line = {'shape': f'{N}x{S}x{S}x{K} partial_{n}', 'num_species': P, 'T': T, 'info': info, 'what': name,
                            'ms_per_window': {'median': round(med, 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4)},
                            'us_per_step': {'median': round(med * 1e3 / T, 2), 'min': round(min(xs) * 1e3 / T, 2),
                                            'max': round(max(xs) * 1e3 / T, 2)},
                            'library_launches_per_window': launches[name], 'repeats': args.repeats,
                            'windows_per_sample': args.iters}
                    lines.append(line)
                    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
