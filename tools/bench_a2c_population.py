#!/usr/bin/env python3
"""Time of one training window (rollout + update) of a POPULATION of P agents with M envs each — one env object, one
`policy_rollout(..., population=P)`, one `FusedA2CPopulation.update`: four launches — against the same P members as P
separate env objects and `FusedA2CLearner`s stepped one after the other (4 P launches), in the same process on the same
device, with HIP events after warm-up.  SingleSnake 9 x 9 partial_2, M = 512, T in {5, 20}, P in {1, 4, 16}.  One JSON line
per (T, P), appended to profiles/r14_a2c_population.jsonl (or --out).  Needs the GPU.

    tools/bench_a2c_population.py
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
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation  # noqa: E402


def agents(P, E, dev):
    out = []
    for p in range(P):
        torch.manual_seed(p)
        out.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(dev))
    return out


def time_ms(fn, reps, inner):
    """median and range over `reps` event-timed runs of `inner` windows each, in ms per window"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_a2c_population.jsonl'))
    ap.add_argument('--envs', type=int, default=512, help='envs per member')
    ap.add_argument('--members', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--steps', type=int, nargs='+', default=[5, 20])
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    a = ap.parse_args()
    dev, M, size, mode, E = 'cuda:0', a.envs, 9, 'partial_2', 75
    lrs = [1e-3 * (1 + p % 4) for p in range(max(a.members))]
    for T in a.steps:
        for P in a.members:
            # the population: one env object of P M envs
            env = SingleSnake(num_envs=P * M, size=size, observation_mode=mode, device=dev, seed=0)
            pop = FusedA2CPopulation(agents(P, E, dev), lr=lrs[:P], gamma=0.99, entropy_coef=0.01)
            box = {'state': env.reset()}

            def pop_window():
                out = env.policy_rollout(pop.params, box['state'], T, check=False, population=P)
                pop.update(box['state'], out)
                box['state'] = out['state']

            # the same members as P env objects and P learners, one after the other
            envs = [SingleSnake(num_envs=M, size=size, observation_mode=mode, device=dev, seed=0, env_offset=p * M)
                    for p in range(P)]
            learners = [FusedA2CLearner(ag, lr=lrs[p], gamma=0.99, entropy_coef=0.01)
                        for p, ag in enumerate(agents(P, E, dev))]
            states = [e.reset() for e in envs]

            def separate_window():
                for p in range(P):
                    out = envs[p].policy_rollout(learners[p].params, states[p], T, check=False)
                    learners[p].update(states[p], out)
                    states[p] = out['state']

            for fn in (pop_window, separate_window):
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            # both loops have run the same number of windows from the same start: they hold the same weights
            same = all(torch.equal(pop.params[p], learners[p].params) for p in range(P))
            before = _lib.lib().wurm_launch_count()
            pop_window()
            launches = _lib.lib().wurm_launch_count() - before
            separate_window()
            sep = time_ms(separate_window, a.reps, a.inner)
            one = time_ms(pop_window, a.reps, a.inner)
            sep2 = time_ms(separate_window, a.reps, a.inner)   # the baseline again, behind: drift shows as a difference
            row = dict(what='a2c_population_window', device=torch.cuda.get_device_name(0), size=size, observation=mode,
                       envs_per_member=M, members=P, steps=T, launches_per_window=launches, members_bit_equal=same,
                       population_ms=round(one[0], 4), population_ms_range=[round(one[1], 4), round(one[2], 4)],
                       separate_ms=round(sep[0], 4), separate_ms_range=[round(sep[1], 4), round(sep[2], 4)],
                       separate_again_ms=round(sep2[0], 4), speedup=round(sep[0] / one[0], 3),
                       env_steps_per_s_population=round(P * M * T / (one[0] * 1e-3)),
                       env_steps_per_s_separate=round(P * M * T / (sep[0] * 1e-3)), reps=a.reps, windows_per_rep=a.inner)
            print(json.dumps(row), flush=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
