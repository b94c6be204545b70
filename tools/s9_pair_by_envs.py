#!/usr/bin/env python3
"""rollout_s9_kernel, pair form against one-wave form, and trio form (a second render wave) against pair form, by batch size
(SingleSnake N x 9 x 9 'partial_2', T batch-steps per launch): one process, the same env object and buffers, the form switched
by WURM_S9_PAIR_MAX_ENVS and WURM_S9_TRIO_MIN_STEPS between rounds that alternate.  Per N and form: the rounds' times per
launch (each round the mean of --launches launches between two events), their median and spread (max - min over the
median); the pair form "wins" at N if its slowest round beats the one-wave form's fastest by more than the larger spread,
the trio form if its slowest round beats the pair form's fastest likewise.  (The trio form exists where the helper renders
the crops: --steps at least WURM_S9_CROP_HELPER_MIN_STEPS.)  Prints one JSON document.
    python tools/s9_pair_by_envs.py [--envs 128,256,512,1024,2048,4096] [--steps 1024] [--rounds 5] [--launches 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from wurm_amd import _lib  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--envs', default='128,256,512,1024,2048,4096')
ap.add_argument('--steps', type=int, default=1024)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--launches', type=int, default=10)
args = ap.parse_args()
KNOB, TRIO_KNOB = 'WURM_S9_PAIR_MAX_ENVS', 'WURM_S9_TRIO_MIN_STEPS'
_lib.set_option('WURM_S9_TRIO_MAX_ENVS', 1 << 40)
dev = torch.device('cuda:0')
rows = []
for N in [int(v) for v in args.envs.split(',')]:
    env = SingleSnake(num_envs=N, size=9, observation_mode='partial_2', device=dev, seed=0)
    actions = torch.randint(4, (args.steps, N), device=dev, dtype=torch.int64)
    times = {1: [], 2: [], 3: []}
    for r in range(args.rounds + 1):        # (round 0 warms both forms up)
        for waves in (1, 2, 3):
            _lib.set_option(KNOB, 0 if waves == 1 else 1 << 40)
            _lib.set_option(TRIO_KNOB, 1 if waves == 3 else -1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                env.rollout(actions)
            t1.record()
            torch.cuda.synchronize()
            assert _lib.lib().wurm_single_last_waves_per_env() == waves
            if r > 0:
                times[waves].append(t0.elapsed_time(t1) / args.launches)
    row = {'envs': N, 'steps': args.steps}
    for waves, name in ((1, 'one_wave'), (2, 'pair'), (3, 'trio')):
        ts = sorted(times[waves])
        med = ts[len(ts) // 2]
        row[name] = {'ms_per_launch': [round(t, 5) for t in times[waves]], 'median_ms': round(med, 5),
                     'spread': round((ts[-1] - ts[0]) / med, 5), 'env_steps_per_s': round(N * args.steps / med * 1e3)}
    spread = max(row['one_wave']['spread'], row['pair']['spread'])
    gain = min(times[1]) / max(times[2]) - 1.0          # slowest pair round over fastest one-wave round
    row['gain_worst_case'] = round(gain, 5)
    row['gain_median'] = round(row['one_wave']['median_ms'] / row['pair']['median_ms'] - 1.0, 5)
    row['pair_wins'] = bool(gain > spread)
    trio_spread = max(row['pair']['spread'], row['trio']['spread'])
    trio_gain = min(times[2]) / max(times[3]) - 1.0     # slowest trio round over fastest pair round
    row['trio_gain_worst_case'] = round(trio_gain, 5)
    row['trio_gain_median'] = round(row['pair']['median_ms'] / row['trio']['median_ms'] - 1.0, 5)
    row['trio_wins'] = bool(trio_gain > trio_spread)
    rows.append(row)
    print(f"# N {N:5d}: one wave {row['one_wave']['median_ms']:.4f} ms  pair {row['pair']['median_ms']:.4f} ms  "
          f"gain {100 * row['gain_median']:+.2f} % (worst case {100 * gain:+.2f} %, spread {100 * spread:.2f} %)  "
          f"trio {row['trio']['median_ms']:.4f} ms  gain over pair {100 * row['trio_gain_median']:+.2f} % (worst case {100 * trio_gain:+.2f} %, "
          f"spread {100 * trio_spread:.2f} %)", file=sys.stderr, flush=True)
    del env, actions
for k in (KNOB, TRIO_KNOB, 'WURM_S9_TRIO_MAX_ENVS'):
    _lib.set_option(k, None)
print(json.dumps({'kernel': 'rollout_s9_kernel<partial>', 'rounds': args.rounds, 'launches_per_round': args.launches,
                  'default_' + KNOB: _lib.get_option(KNOB),
                  'default_WURM_S9_TRIO_MAX_ENVS': _lib.get_option('WURM_S9_TRIO_MAX_ENVS'), 'rows': rows}, indent=1))
