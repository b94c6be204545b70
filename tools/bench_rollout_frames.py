#!/usr/bin/env python3
"""What recording the frames of a fused window costs (`env.record_start` / `env.record_frames`), in one process on one
device, with HIP events after warm-up.  Needs the GPU.

SingleSnake 512 x 9 x 9 'partial_2', windows of T = 20 steps of `policy_rollout`.  Three loops alternate, rep by rep, so
that drift of the device hits all of them alike; each rep times `--inner` windows between two events:
    recorded   record_start(k = 16 envs) + policy_rollout + record_frames        the feature
    plain      policy_rollout alone (the path as it was before; untouched)       what the feature is added to
    per_call   T iterations of `_get_rgb(); step(a); reset(done)` on precomputed actions (no policy in the loop): what a
               user who wanted frames had to fall back to — every env's frame, every step
One JSON line per loop (median and range of ms per window over the reps), appended to profiles/r18_rollout_frames.jsonl
(or --out).

    tools/bench_rollout_frames.py
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
from wurm_amd.agents import FeedforwardAgent, pack_policy_params  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402

DEV = 'cuda:0'


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def launches(fn):
    before = _lib.lib().wurm_launch_count()
    fn()
    return _lib.lib().wurm_launch_count() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_rollout_frames.jsonl'))
    ap.add_argument('--num-envs', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--select', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/bench_rollout_frames.py measures on the GPU: no HIP device visible')
    N, T, k = a.num_envs, a.steps, a.select
    torch.manual_seed(0)
    params = pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75).to(DEV))
    select = torch.arange(k, device=DEV)

    def fused(record):
        env = SingleSnake(num_envs=N, size=9, observation_mode='partial_2', device=DEV, seed=0)
        box = {'state': env.reset()}

        def window():
            rec = env.record_start(select) if record else None
            out = env.policy_rollout(params, box['state'], T, check=False)
            box['state'] = out['state']
            if record:
                box['clip'] = env.record_frames(rec, out['actions'])
        return window

    def per_call():
        env = SingleSnake(num_envs=N, size=9, observation_mode='partial_2', device=DEV, seed=0)
        tape = torch.randint(4, (T, N), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
        box = {}

        def window():
            for t in range(T):
                box['rgb'] = env._get_rgb()
                _, _, done, _ = env.step(tape[t].clone())
                env.reset(done, return_observations=False)
        return window

    loops = {'recorded': fused(True), 'plain': fused(False), 'per_call': per_call()}
    for fn in loops.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    counts = {name: launches(fn) for name, fn in loops.items()}
    times = {name: [] for name in loops}
    for _ in range(a.reps):
        for name, fn in loops.items():
            times[name].append(timed(fn, a.inner))
    rows = []
    for name in loops:
        t = times[name]
        rows.append(dict(what='rollout_frames', loop=name, device=torch.cuda.get_device_name(0), num_envs=N, size=9,
                         observation='partial_2', steps=T, selected=k if name == 'recorded' else (N if name == 'per_call' else 0),
                         library_launches_per_window=counts[name], window_ms=round(statistics.median(t), 5),
                         window_ms_range=[round(min(t), 5), round(max(t), 5)], reps=a.reps, windows_per_rep=a.inner,
                         warmup_windows=a.warmup))
    with open(a.out, 'a') as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
