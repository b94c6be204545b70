#!/usr/bin/env python3
"""rollout_s9_kernel's pair form, the crop in the stepping wave against the crop in the helper wave, by launch length
(SingleSnake N x 9 x 9 'partial_2', T batch-steps per launch): one process, the same env object and buffers, the form
switched by WURM_S9_CROP_HELPER_MIN_STEPS between rounds that alternate.  Per T and form: the rounds' times per launch (each
round the mean of --launches launches between two events), their median and spread (max - min over the median); the
helper's crop "wins" at T if its slowest round beats the other form's fastest by more than the larger spread.  The trio form
(a second render wave, WURM_S9_TRIO_MIN_STEPS) alternates with the two and is set against the helper's crop in the same way.
Prints one JSON document.
    python tools/s9_crop_by_steps.py [--envs 512] [--steps 64,128,256,512,1024] [--rounds 5] [--launches 20]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from wurm_amd import _lib  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=512)
ap.add_argument('--steps', default='64,128,256,512,1024')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--launches', type=int, default=20)
args = ap.parse_args()
KNOB, TRIO_KNOB = 'WURM_S9_CROP_HELPER_MIN_STEPS', 'WURM_S9_TRIO_MIN_STEPS'
_lib.set_option('WURM_S9_TRIO_MAX_ENVS', 1 << 40)
dev = torch.device('cuda:0')
_lib.set_option('WURM_S9_PAIR_MAX_ENVS', 1 << 40)
N, rows = args.envs, []
env = SingleSnake(num_envs=N, size=9, observation_mode='partial_2', device=dev, seed=0)
for T in [int(v) for v in args.steps.split(',')]:
    actions = torch.randint(4, (T, N), device=dev, dtype=torch.int64)
    times = {0: [], 1: [], 2: []}      # by the number of waves that render beside the stepper
    for r in range(args.rounds + 1):        # (round 0 warms both forms up)
        for wave in (0, 1, 2):
            _lib.set_option(KNOB, 1 if wave else -1)
            _lib.set_option(TRIO_KNOB, 1 if wave == 2 else -1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                env.rollout(actions)
            t1.record()
            torch.cuda.synchronize()
            assert _lib.lib().wurm_single_last_waves_per_env() == max(2, 1 + wave) and _lib.lib().wurm_single_last_crop_wave() == min(wave, 1)
            if r > 0:
                times[wave].append(t0.elapsed_time(t1) / args.launches)
    row = {'envs': N, 'steps': T}
    for wave, name in ((0, 'crop_in_stepper'), (1, 'crop_in_helper'), (2, 'trio')):
        ts = sorted(times[wave])
        med = ts[len(ts) // 2]
        row[name] = {'ms_per_launch': [round(t, 5) for t in times[wave]], 'median_ms': round(med, 5),
                     'spread': round((ts[-1] - ts[0]) / med, 5), 'env_steps_per_s': round(N * T / med * 1e3)}
    spread = max(row['crop_in_stepper']['spread'], row['crop_in_helper']['spread'])
    gain = min(times[0]) / max(times[1]) - 1.0          # slowest helper round over fastest stepper round
    row['gain_worst_case'] = round(gain, 5)
    row['gain_median'] = round(row['crop_in_stepper']['median_ms'] / row['crop_in_helper']['median_ms'] - 1.0, 5)
    row['helper_wins'] = bool(gain > spread)
    trio_spread = max(row['crop_in_helper']['spread'], row['trio']['spread'])
    trio_gain = min(times[1]) / max(times[2]) - 1.0     # slowest trio round over fastest helper round
    row['trio_gain_worst_case'] = round(trio_gain, 5)
    row['trio_gain_median'] = round(row['crop_in_helper']['median_ms'] / row['trio']['median_ms'] - 1.0, 5)
    row['trio_wins'] = bool(trio_gain > trio_spread)
    rows.append(row)
    print(f"# T {T:5d}: stepper {row['crop_in_stepper']['median_ms']:.4f} ms  helper {row['crop_in_helper']['median_ms']:.4f} ms  "
          f"gain {100 * row['gain_median']:+.2f} % (worst case {100 * gain:+.2f} %, spread {100 * spread:.2f} %)  "
          f"trio {row['trio']['median_ms']:.4f} ms  gain over helper {100 * row['trio_gain_median']:+.2f} % (worst case {100 * trio_gain:+.2f} %, "
          f"spread {100 * trio_spread:.2f} %)", file=sys.stderr, flush=True)
    del actions
_lib.set_option(KNOB, None)
_lib.set_option(TRIO_KNOB, None)
_lib.set_option('WURM_S9_TRIO_MAX_ENVS', None)
_lib.set_option('WURM_S9_PAIR_MAX_ENVS', None)
print(json.dumps({'kernel': 'rollout_s9_kernel<partial, pair>', 'rounds': args.rounds, 'launches_per_round': args.launches,
                  'default_' + KNOB: _lib.get_option(KNOB),
                  'default_' + TRIO_KNOB: _lib.get_option(TRIO_KNOB), 'rows': rows}, indent=1))
