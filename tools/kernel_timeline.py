#!/usr/bin/env python3
"""In-kernel timeline of the per-call lane kernels (SingleSnake N x 9 x 9 'partial_2').

Needs the instrumented build of the library (s_memtime stamps, wurm_amd/csrc/wurm_device.hpp WURM_TL):
    make -C wurm_amd/csrc timeline          # -> wurm_amd/libwurm_hip_timeline.so (cross-compiles without a GPU)
    WURM_HIP_LIBRARY=$PWD/wurm_amd/libwurm_hip_timeline.so python tools/kernel_timeline.py [--kernel resident|lane_step]
                                                            [--envs 65536] [--epw 32] [--form ref|noobs]
    ... python tools/kernel_timeline.py --kernel s9 [--envs 512] [--steps 1024] [--pair 0|1] [--crop-helper 0|1] [--render-waves 1|2]
Every wave overwrites the first 64 bytes of its own observation block with eight stamps once its stores have drained; this
script reads them back from the observation `step` returned and prints, per segment between two stamps, the distribution
over the waves in s_memtime ticks — counters of different XCDs are not synchronised, so only differences within one wave
are used.  The observations of a timeline run are garbage by construction.

--kernel s9: the stepping wave of rollout_s9_kernel (the headline rollout, --envs x 9 x 9 'partial_2', --steps batch-steps per
launch), one wave form (--pair 0) or pair form (--pair 1).  Its stamps are TOTALS over the launch's 64-step chunks.
--crop-helper 1 (with --pair 1, --steps above 64): the pair form whose helper wave renders the crops; the helper's own laps,
which it leaves over the crop of step 1, are printed too: its rendering time per chunk against the stepper's stepping time
per chunk, and what each wave waits at the chunk barrier.  (A library built with -DWURM_S9_CROP_SPP1 as well renders one
step per pass whatever the window: the measurement the two-steps-per-pass renderer rests on.)
--render-waves 2 (with --crop-helper 1, --steps above 128): the trio form, whose wave 2 renders most of each chunk beside the
helper; wave 2 leaves its laps over the crop of step 2 and gets a section of its own."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--kernel', default='resident', choices=['resident', 'lane_step', 'grid', 's9'])
ap.add_argument('--size', type=int, default=36, help='--kernel grid: the grid size (cfg5: 8192 envs of 36 x 36, default observation)')
ap.add_argument('--envs', type=int, default=None, help='default 65536; --kernel s9: 512')
ap.add_argument('--epw', type=int, default=0)
ap.add_argument('--form', default='ref', choices=['ref', 'noobs'])
ap.add_argument('--iters', type=int, default=12)
ap.add_argument('--steps', type=int, default=1024, help='--kernel s9: batch-steps per launch')
ap.add_argument('--pair', type=int, default=0, choices=[0, 1], help='--kernel s9: the pair form (two waves per env)')
ap.add_argument('--crop-helper', type=int, default=0, choices=[0, 1], help='--kernel s9 --pair 1: the helper wave renders the crops')
ap.add_argument('--render-waves', type=int, default=1, choices=[1, 2], help='--kernel s9 --crop-helper 1: 2 = the trio form, a second render wave')
args = ap.parse_args()
if 'timeline' not in os.environ.get('WURM_HIP_LIBRARY', ''):
    sys.exit('set WURM_HIP_LIBRARY to the instrumented library (see the docstring)')
N = args.envs if args.envs is not None else (512 if args.kernel == 's9' else 65536)


def s9_timeline():
    """slots of rollout_s9_kernel's stepper (single_kernels.hpp): 0 entry, 7 end (stores drained); totals over the chunks:
    5 state load + setup, 1 wait for the chunk's inputs (one wave: the tape load, which also drains the previous chunk's
    observation stores; pair: the barrier and the LDS reads), 2 prologue arithmetic (one wave only), 3 step loop, 4 flush
    (one wave: the record stores issued; pair: the record's LDS write and the barrier, that is the stepper's wait for the helper).
    Slots of the helper with --crop-helper 1: 1 tape load, draw and record stores (and, first, B0), 2 rendering of the chunk
    before, 3 wait at the chunk barrier, 4 rendering of the last chunk, after the stepper has finished; the trio form's render
    waves also 5: rebuilding the crop words and body masks of a chunk (all chunks; slots 2 and 4 are the passes alone then)"""
    import numpy as np
    import torch
    from wurm_amd import _lib
    from wurm_amd.envs import SingleSnake
    N_ = N
    T = args.steps
    env = SingleSnake(num_envs=N_, size=9, observation_mode='partial_2', device='cuda', seed=0)
    _lib.set_option('WURM_S9_PAIR_MAX_ENVS', (1 << 40) if args.pair else 0)
    _lib.set_option('WURM_S9_CROP_HELPER_MIN_STEPS', 1 if args.crop_helper else -1)
    _lib.set_option('WURM_S9_TRIO_MAX_ENVS', 1 << 40)
    _lib.set_option('WURM_S9_TRIO_MIN_STEPS', 1 if args.render_waves == 2 else -1)
    assert not args.crop_helper or (args.pair and T > 64), '--crop-helper 1 needs --pair 1 and more than one chunk'
    assert args.render_waves == 1 or (args.crop_helper and T > 128), '--render-waves 2 needs --crop-helper 1 and more than two chunks'
    helper_rows, wave2_rows = [], []
    g = torch.Generator(device='cuda').manual_seed(1)
    rows = []
    for it in range(args.iters):
        out = env.rollout(torch.randint(0, 4, (T, N_), device='cuda', generator=g))
        torch.cuda.synchronize()
        assert _lib.lib().wurm_single_last_waves_per_env() == (3 if args.render_waves == 2 else 1 + args.pair)
        assert _lib.lib().wurm_single_last_crop_wave() == args.crop_helper
        obs = out['observations']
        if it >= 4:
            rows.append(obs[0].reshape(N_, -1)[:, :16].contiguous().view(torch.int64).cpu().numpy().astype(np.int64))
            if args.crop_helper:
                helper_rows.append(obs[1].reshape(N_, -1)[:, :16].contiguous().view(torch.int64).cpu().numpy().astype(np.int64))
            if args.render_waves == 2:
                wave2_rows.append(obs[2].reshape(N_, -1)[:, :16].contiguous().view(torch.int64).cpu().numpy().astype(np.int64))
    st = np.concatenate(rows)
    life = st[:, 7] - st[:, 0]
    st, life = st[(life > 0) & (life < 10 ** 9)], life[(life > 0) & (life < 10 ** 9)]
    form = 'trio form, crops by the helper and wave 2' if args.render_waves == 2 else 'pair form, crops by the helper' if args.crop_helper else 'pair form' if args.pair else 'one-wave form'
    print(f'rollout_s9_kernel, {N_} envs x {T} steps, {form}: {len(life)} stepper samples; '
          f's_memtime ticks, totals over {(T + 63) // 64} chunks')
    named = [(5, 'state load + setup'), (1, 'wait for the chunk inputs'), (2, 'prologue arithmetic'), (3, 'step loop'),
             (4, 'flush / hand-over')]
    for k, name in named:
        c = st[:, k]
        print(f'  {name:>26s} p10 {int(np.percentile(c, 10)):7d}  p50 {int(np.median(c)):7d}  p90 {int(np.percentile(c, 90)):7d}  '
              f'max {int(c.max()):7d}   {100.0 * np.median(c) / np.median(life):5.1f} % of p50 life')
    rest = life - sum(st[:, k] for k, _ in named)
    print(f'  {"state store + drain":>26s} p10 {int(np.percentile(rest, 10)):7d}  p50 {int(np.median(rest)):7d}  '
          f'p90 {int(np.percentile(rest, 90)):7d}  max {int(rest.max()):7d}   {100.0 * np.median(rest) / np.median(life):5.1f} % of p50 life')
    print(f'  wave lifetime: p10 {int(np.percentile(life, 10))}  p50 {int(np.median(life))}  p90 {int(np.percentile(life, 90))}  max {int(life.max())}')
    per_chunk = 100.0 * np.median(st[:, 1] + st[:, 2] + st[:, 4]) / np.median(life)
    print(f'  per-chunk work around the step loop (wait + prologue + flush): {per_chunk:.1f} % of p50 life')
    if not args.crop_helper:
        return
    C = (T + 63) // 64
    hs = np.concatenate(helper_rows)
    hl = hs[:, 7] - hs[:, 0]
    hs, hl = hs[(hl > 0) & (hl < 10 ** 9)], hl[(hl > 0) & (hl < 10 ** 9)]
    print(f'helper wave: {len(hl)} samples')
    for k, name in [(1, 'tape, draw, records (+ B0)'), (2, 'rendering, chunks 0 .. C-2'), (3, 'wait at the chunk barrier'),
                    (4, 'rendering, last chunk'), (5, 'rebuild, all chunks')]:
        c = hs[:, k]
        print(f'  {name:>26s} p10 {int(np.percentile(c, 10)):7d}  p50 {int(np.median(c)):7d}  p90 {int(np.percentile(c, 90)):7d}  '
              f'max {int(c.max()):7d}   {100.0 * np.median(c) / np.median(hl):5.1f} % of p50 life')
    print(f'  wave lifetime: p10 {int(np.percentile(hl, 10))}  p50 {int(np.median(hl))}  p90 {int(np.percentile(hl, 90))}  max {int(hl.max())}')
    print(f'per chunk, p50: the stepper steps {int(np.median(st[:, 3])) // C} ticks, the helper renders '
          f'{int(np.median(hs[:, 2])) // max(C - 1, 1)} and does its other work in {int(np.median(hs[:, 1])) // C}; '
          f'the stepper\'s hand-over and barrier wait is {100.0 * np.median(st[:, 4]) / np.median(life):.1f} % of its life, '
          f'the helper\'s barrier wait {100.0 * np.median(hs[:, 3]) / np.median(hl):.1f} % of its own')
    print(f'stepper\'s hand-over and barrier wait: p50 {int(np.median(st[:, 4]))}  p90 {int(np.percentile(st[:, 4], 90))} ticks; '
          f'last chunk after the stepper has finished: helper p50 {int(np.median(hs[:, 4]))}  p90 {int(np.percentile(hs[:, 4], 90))}')
    if args.render_waves != 2:
        return
    ws = np.concatenate(wave2_rows)
    wl = ws[:, 7] - ws[:, 0]
    ws, wl = ws[(wl > 0) & (wl < 10 ** 9)], wl[(wl > 0) & (wl < 10 ** 9)]
    print(f'wave 2 (renders only): {len(wl)} samples')
    for k, name in [(1, 'B0 and loop overhead'), (2, 'rendering, chunks 0 .. C-2'), (3, 'wait at the chunk barrier'),
                    (4, 'rendering, last chunk'), (5, 'rebuild, all chunks')]:
        c = ws[:, k]
        print(f'  {name:>26s} p10 {int(np.percentile(c, 10)):7d}  p50 {int(np.median(c)):7d}  p90 {int(np.percentile(c, 90)):7d}  '
              f'max {int(c.max()):7d}   {100.0 * np.median(c) / np.median(wl):5.1f} % of p50 life')
    print(f'  wave lifetime: p10 {int(np.percentile(wl, 10))}  p50 {int(np.median(wl))}  p90 {int(np.percentile(wl, 90))}  max {int(wl.max())}')
    print(f'per chunk, p50: wave 2 renders {int(np.median(ws[:, 2])) // max(C - 1, 1)} ticks and waits at the barrier '
          f'{int(np.median(ws[:, 3])) // C}; the helper renders and works {(int(np.median(hs[:, 2])) + int(np.median(hs[:, 1]))) // C} '
          f'and waits {int(np.median(hs[:, 3])) // C}; the stepper steps {int(np.median(st[:, 3])) // C}')
    print(f'per chunk, p50: the helper rebuilds in {int(np.median(hs[:, 5])) // C} ticks, wave 2 in {int(np.median(ws[:, 5])) // C} '
          f'(0: a library whose render waves leave no such lap)')


if args.kernel == 's9':
    s9_timeline()
    sys.exit(0)
if args.kernel == 'grid':
    os.environ['WURM_GRID_STEP_MIN_CELLS'] = '0'
    names = ['entry', 'grid in LDS', 'action', 'stepped', 'outputs', 'obs issued', 'state stored', 'drained']
    epw = 1
elif args.kernel == 'resident':
    os.environ['WURM_RESIDENT_MIN_ENVS'] = '0'
    nw = 2 if args.form == 'ref' else 1
    epw = args.epw or (64 // nw if N >= 32768 else (32 // nw if N >= 8192 else 16))
    os.environ['WURM_RESIDENT_EPW'] = str(epw)
    names = ['entry', 'loaded', 'stepped', 'outputs', 'state', 'bits', 'crops issued', 'drained']
else:
    os.environ['WURM_RESIDENT_MIN_ENVS'] = str(10 ** 9)
    os.environ['WURM_LANE_STEP_MIN_ENVS'] = '0'
    epw = 16 if N >= 49152 else (8 if N >= 24576 else 4)
    names = ['entry', 'state read', 'validated', 'moved', 'cells+outputs', 'rebuilt', 'crops issued', 'drained']

import numpy as np  # noqa: E402
import torch  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402

S_, mode_ = (args.size, 'default') if args.kernel == 'grid' else (9, 'partial_2')
E_ = 3 * S_ * S_ if args.kernel == 'grid' else 75
env = SingleSnake(num_envs=N, size=S_, observation_mode=mode_, device='cuda', seed=0)
g = torch.Generator(device='cuda').manual_seed(1)
nw_ = N // epw
segs, life = [], []
for it in range(args.iters):
    a = torch.randint(0, 4, (N,), device='cuda', generator=g)
    obs, r, d, info = env.step(a)
    env.reset(d) if args.form == 'ref' else env.reset(d, return_observations=False)
    torch.cuda.synchronize()
    if it < 4:
        continue
    st = obs.detach().reshape(-1)[:nw_ * epw * E_].reshape(nw_, epw * E_)[:, :16].contiguous().view(torch.int64)
    st = st.cpu().numpy().astype(np.int64)
    ok = (st[:, 7] > st[:, 0]) & (st[:, 7] - st[:, 0] < 10 ** 7)
    st = st[ok]
    segs.append(st[:, 1:] - st[:, :-1])
    life.append(st[:, 7] - st[:, 0])
seg, life = np.concatenate(segs), np.concatenate(life)
print(f'{args.kernel} kernel, {N} envs, {epw} envs per wave, form {args.form}: {len(life)} wave samples; s_memtime ticks')
for k in range(7):
    c = seg[:, k]
    print(f'  {names[k]:>14s} -> {names[k + 1]:14s} p10 {int(np.percentile(c, 10)):6d}  p50 {int(np.median(c)):6d}  '
          f'p90 {int(np.percentile(c, 90)):6d}  max {int(c.max()):6d}   {100.0 * np.median(c) / np.median(life):5.1f} % of p50 life')
print(f'  wave lifetime: p10 {int(np.percentile(life, 10))}  p50 {int(np.median(life))}  p90 {int(np.percentile(life, 90))}  max {int(life.max())}')
