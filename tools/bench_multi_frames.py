#!/usr/bin/env python3
"""What recording the frames of a MultiSnake window costs (`env.record_start` / `env.record_frames`), in one process on one
device, with HIP events after warm-up.  Needs the GPU.

Two shapes: 512 envs of 2 snakes on 12 x 12 with 'partial_2' (the reference's test shape) and 4096 envs of 4 snakes on
25 x 25 with 'partial_5' (its training shape); windows of T = 20 steps, k = 4 recorded envs.  Three loops alternate, rep by
rep, so that drift of the device hits all of them alike; each rep times `--inner` windows between two events:
    plain      act_window alone (the path as it was before; untouched)           what the feature is added to
    recorded   record_start(k envs) + act_window + record_frames                 the feature
    per_call   T iterations of `_get_env_images(); step(a); reset(all_done)` on precomputed actions (no policy in the
               loop): what a user who wanted frames had to fall back to — every env's image, every step
One JSON line per loop and shape (median and range of ms per window over the reps), appended to
profiles/r22_multi_frames.jsonl (or --out).

    tools/bench_multi_frames.py
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
from wurm_amd.envs import MultiSnake, _multi_act  # noqa: E402

DEV = 'cuda:0'
SHAPES = ((512, 12, 2, 'partial_2'), (4096, 25, 4, 'partial_5'))


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


def measure(N, S, K, mode, T, k, a):
    n = int(mode.split('_')[1])
    E = 3 * (2 * n + 1) ** 2
    params = (torch.randn((1, _multi_act.num_policy_params(E)), generator=torch.Generator().manual_seed(0)) * 0.1).to(DEV)
    select = torch.arange(k, device=DEV)
    make = lambda: MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=mode, device=DEV, boost=False,
                              food_mode='random_rate', respawn_mode='any', seed=0)

    def fused(record):
        env = make()
        box = {'state': env.reset()}

        def window():
            rec = env.record_start(select) if record else None
            out = env.act_window(params, box['state'], T)
            box['state'] = out['state']
            if record:
                box['clip'] = env.record_frames(rec, out['actions'])
        return window

    def per_call():
        env = make()
        tape = torch.randint(4, (T, K, N), device=DEV, generator=torch.Generator(DEV).manual_seed(0))
        box = {}

        def window():
            for t in range(T):
                box['rgb'] = env._get_env_images()
                _, _, dones, _ = env.step({f'agent_{i}': tape[t, i] for i in range(K)})
                env.reset(dones['__all__'], return_observations=False)
        return window

    loops = {'plain': fused(False), 'recorded': fused(True), 'per_call': per_call()}
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
        rows.append(dict(what='multi_frames', loop=name, device=torch.cuda.get_device_name(0), num_envs=N, size=S,
                         num_snakes=K, observation=mode, steps=T,
                         selected=k if name == 'recorded' else (N if name == 'per_call' else 0),
                         library_launches_per_window=counts[name], window_ms=round(statistics.median(t), 5),
                         window_ms_range=[round(min(t), 5), round(max(t), 5)], reps=a.reps, windows_per_rep=a.inner,
                         warmup_windows=a.warmup))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_multi_frames.jsonl'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--select', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=10)
    a = ap.parse_args()
    if a.reps < 9:
        sys.exit('tools/bench_multi_frames.py: at least 9 alternating repeats')
    if not torch.cuda.is_available():
        sys.exit('tools/bench_multi_frames.py measures on the GPU: no HIP device visible')
    with open(a.out, 'a') as f:
        for N, S, K, mode in SHAPES:
            for row in measure(N, S, K, mode, a.steps, a.select, a):
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
