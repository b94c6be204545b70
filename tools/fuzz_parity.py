#!/usr/bin/env python3
"""Randomised parity fuzz on the GPU box: random shapes, observation modes, dynamics and seeds; HIP (C ABI) vs the CPU
oracle, bit-exact on every output of every step, per-call and rollout entry points.  Not part of the default test
suite (run time is the argument); failures print the configuration that reproduces them.

    python tools/fuzz_parity.py --seconds 120 [--seed 0]"""
import argparse
import os
import sys
import time
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oracle import oracle as _o  # noqa: E402
from tests.backends import OracleBackend  # noqa: E402
from tests.hip_backend import HipBackend  # noqa: E402
from wurm_amd import _lib  # noqa: E402


def same(a, b, what):
    if a is None and b is None:
        return
    x, y = np.asarray(a), np.asarray(b)
    if x.dtype.kind == 'f':
        x, y = np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32)
    assert x.shape == y.shape, f'{what}: shapes {x.shape} {y.shape}'
    bad = np.argwhere(x != y)
    assert len(bad) == 0, f'{what}: {len(bad)} mismatches, first {bad[0].tolist()}'


def fuzz_single(rng):
    S = int(rng.choice([9, 9, 10, 11, 12, 13, 16, 20, 25, 31, 36, 40, 48, 57, 64]))
    N = int(rng.randint(1, 70 if S <= 16 else 12))
    T = int(rng.randint(5, 120 if S <= 16 else 40))
    modes = ['default', 'raw', 'one_channel', 'positions', f'partial_{rng.randint(1, 7)}', 'none']
    mode = modes[rng.randint(len(modes))]
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'single S={S} N={N} T={T} mode={mode} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    eo, eh = np.zeros((N, 3, S, S), np.float32), np.zeros((N, 3, S, S), np.float32)
    o.single_reset(eo, np.ones(N), 'none'); h.single_reset(eh, np.ones(N), 'none')
    same(eo, eh, desc + ' fresh')
    dtype = np.int64 if rng.rand() < 0.7 else np.int32
    if rng.rand() < 0.5:   # per-call loop with occasional skipped resets
        skip = rng.rand() < 0.5 and not mode.startswith('partial')
        for t in range(T):
            a = rng.randint(0, 4, N).astype(dtype)
            ao, ah = a.copy(), a.copy()
            ro, rh = o.single_step(eo, ao, mode), h.single_step(eh, ah, mode)
            same(ao, ah, f'{desc} actions t={t}'); same(eo, eh, f'{desc} state t={t}')
            for x, y, w in zip(ro, rh, 'obs reward done sc ec'.split()):
                same(x, y, f'{desc} {w} t={t}')
            if skip and t % 4 == 3:
                o._next(); h._next()
            else:
                same(o.single_reset(eo, ro[2], mode), h.single_reset(eh, rh[2], mode), f'{desc} reset obs t={t}')
                same(eo, eh, f'{desc} reset state t={t}')
    else:
        a = rng.randint(0, 4, (T, N)).astype(dtype)
        ao, ah = a.copy(), a.copy()
        # (round 6: from which size on the clock-grid rollout serves a launch depends on the observation mode — half of the cases
        # with the shipped thresholds, half with the kernel forced from 12 x 12 on)
        old = _lib.set_option('WURM_GRID_ROLLOUT_MIN_SIZE', 12 if rng.rand() < 0.5 else -1)
        try:
            ro, rh = o.single_rollout(eo, ao, mode), h.single_rollout(eh, ah, mode)
        finally:
            _lib.set_option('WURM_GRID_ROLLOUT_MIN_SIZE', old)
        for k in ro:
            same(ro[k], rh[k], f'{desc} rollout {k}')
        same(ao, ah, desc + ' rollout actions'); same(eo, eh, desc + ' rollout state')
    return desc


def fuzz_fused(rng):
    """wurm_single_step_reset / wurm_grid_step_reset: random mixes of the two groupings ([postponed reset, step, observe]
    and [step, observe, reset]), with and without the reset observation, an occasional iteration without any reset
    (irregular states), hostile action values — against the oracle's step / reset pair with the same counters."""
    grid = rng.rand() < 0.2
    S = int(rng.choice([9, 9, 10, 11, 12, 14, 20, 25, 36, 48, 64]))
    N = int(rng.randint(1, 70 if S <= 16 else 10))
    T = int(rng.randint(5, 80 if S <= 16 else 30))
    if grid:
        mode = ['default', 'raw', 'positions', 'none'][rng.randint(4)]
        start = (int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1)))
    else:
        mode = ['default', 'raw', 'one_channel', 'positions', f'partial_{rng.randint(1, 7)}', 'none'][rng.randint(6)]
        start = None
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'fused grid={grid} S={S} N={N} T={T} mode={mode} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    C = 2 if grid else 3
    eo = np.zeros((N, C, S, S), np.float32)
    if grid:
        o.grid_reset(eo, np.ones(N), start, 'none')
    else:
        o.single_reset(eo, np.ones(N), 'none')
    eh = eo.copy()
    call, prev, prev_call = 10, None, None
    dtype = np.int64 if rng.rand() < 0.7 else np.int32
    for t in range(T):
        a = rng.randint(0, 4, N).astype(dtype)
        if rng.rand() < 0.1:
            a[rng.rand(N) < 0.3] = rng.randint(-9, 9)
        ao, ah = a.copy(), a.copy()
        style = rng.randint(4)  # 0: post reset, 1: pre (deferred) reset, 2: deferred + obs_after, 3: no reset at all
        kw = dict(call=call, grid=start)
        if style == 0:
            kw.update(post_reset=True, want_obs_after=bool(rng.rand() < 0.5), pre_done=prev, pre_call=prev_call)
        elif style in (1, 2):
            kw.update(pre_done=prev, pre_call=prev_call, want_obs_after=(style == 2))
        ro, rh = o.single_step_reset(eo, ao, mode, **kw), h.single_step_reset(eh, ah, mode, **kw)
        same(ao, ah, f'{desc} actions t={t}'); same(eo, eh, f'{desc} state t={t} style={style}')
        for k in ro:
            same(ro[k], rh[k], f'{desc} {k} t={t} style={style}')
        if style == 0 or style == 3:
            prev, prev_call = None, None          # reset applied (0) or skipped altogether (3)
        else:
            prev, prev_call = ro['done'], call + 1  # the caller postponed reset(done): the next launch applies it
        call += 2
    return desc


def fuzz_resident(rng):
    """wurm_single_step_reset on the resident mirror (wurm_single_call.resident, lane_resident.hpp), eager and lazy: random
    batch sizes around the envs-per-wave settings, deferred resets with and without the reset observation, iterations
    without any reset (finished envs stepped again), hostile actions, hand-edited states and calls that cannot use the
    mirror (post_reset) in between; `envs` compared whenever the lazy form writes them out."""
    S = int(rng.choice([9, 9, 9, 10, 11, 12, 14, 20, 25, 36]))
    if S == 9:    # lane_resident.hpp: 32 bytes per env
        N = int(rng.choice([1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 100, 129, 200, 257]))
        mode = ['partial_2', 'partial_2', 'none', 'one_channel', 'one_channel', 'default', 'positions', 'partial_0', 'partial_1',
                'raw', 'raw', 'partial_3', 'partial_3'][rng.randint(13)]
    elif S <= 11:  # lane_wide_resident.hpp (round 6): 48 bytes per env, kept by lazy calls only; the modes it does not serve
        N = int(rng.choice([1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 100, 129, 200]))   # ('raw', 'partial_1'): no mirror at all
        mode = ['partial_2', 'partial_2', 'none', 'one_channel', 'default', 'default', 'positions', 'partial_3', 'raw', 'partial_1'][rng.randint(10)]
    else:         # grid_rollout.hip: the clock grid + a record per env, every observation mode
        N = int(rng.randint(1, 24))
        mode = ['default', 'raw', 'one_channel', 'positions', f'partial_{rng.randint(1, 7)}', 'none'][rng.randint(6)]
    T = int(rng.randint(5, 70))
    lazy = bool(rng.rand() < 0.6)
    epw = int(rng.choice([0, 16, 32, 64]))
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'resident S={S} N={N} T={T} mode={mode} lazy={lazy} epw={epw} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    _lib.set_option('WURM_RESIDENT_EPW', epw if epw else None)
    try:
        o, h = OracleBackend(seed, off), HipBackend(seed, off)
        eo = np.zeros((N, 3, S, S), np.float32)
        o.single_reset(eo, np.ones(N), 'none')
        eh = eo.copy()
        mirror = {'valid': 0, 'lazy': lazy}
        call, prev, prev_call = 10, None, None
        dtype = np.int64 if rng.rand() < 0.7 else np.int32
        for t in range(T):
            a = rng.randint(0, 4, N).astype(dtype)
            if rng.rand() < 0.1:
                a[rng.rand(N) < 0.3] = rng.randint(-9, 9)
            ao, ah = a.copy(), a.copy()
            style = int(rng.choice([0, 1, 1, 2, 2, 2, 3]))  # 0: post reset (no mirror), 1 / 2: deferred (+ obs_after), 3: none
            edit = rng.rand() < 0.08
            mirror['sync'] = bool(not lazy or edit or rng.rand() < 0.3 or t == T - 1)
            kw = dict(call=call)
            if style == 0:
                kw.update(post_reset=True, want_obs_after=bool(rng.rand() < 0.5), pre_done=prev, pre_call=prev_call)
            elif style in (1, 2):
                kw.update(pre_done=prev, pre_call=prev_call, want_obs_after=(style == 2))
            ro = o.single_step_reset(eo, ao, mode, **kw)
            rh = h.single_step_reset(eh, ah, mode, resident=mirror, **kw)
            same(ao, ah, f'{desc} actions t={t}')
            if mirror['sync'] or style == 0:
                same(eo, eh, f'{desc} state t={t} style={style}')
            for k in ro:
                same(ro[k], rh[k], f'{desc} {k} t={t} style={style}')
            if style == 0 or style == 3:
                prev, prev_call = None, None
            else:
                prev, prev_call = ro['done'], call + 1
            if edit:  # the caller edits the state (and says so): an extra food, a food removed, a body value broken
                i = int(rng.randint(N))
                eo[i, 0, int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))] = 1
                if rng.rand() < 0.5:
                    eo[int(rng.randint(N)), 0] = 0
                if rng.rand() < 0.3:
                    eo[int(rng.randint(N)), 2, int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))] += 2
                eh[...] = eo
                mirror['valid'] = 0
            call += 2
    finally:
        _lib.set_option('WURM_RESIDENT_EPW', None)
    return desc


def fuzz_lean(rng):
    """The shapes the lean / 9x9 rollout kernels take: chained launches, tape lengths around the 64-step chunk, action
    values outside 0..3, an occasional per-call step without reset in between (irregular states -> generic path)."""
    S = int(rng.choice([9, 9, 9, 10, 11]))
    N = int(rng.choice([1, 3, 17, 64, 65, 200]))
    mode = ['partial_0', 'partial_1', 'partial_2', 'partial_2', 'partial_3', 'none'][rng.randint(6)]
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 40))
    desc = f'lean S={S} N={N} mode={mode} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    eo, eh = np.zeros((N, 3, S, S), np.float32), np.zeros((N, 3, S, S), np.float32)
    o.single_reset(eo, np.ones(N), 'none'); h.single_reset(eh, np.ones(N), 'none')
    o.call = h.call = int(rng.randint(1 << 50))
    for launch in range(int(rng.randint(1, 4))):
        T = int(rng.choice([1, 2, 30, 63, 64, 65, 127, 128, 129, 200]))
        dtype = np.int64 if rng.rand() < 0.7 else np.int32
        a = rng.randint(0, 4, (T, N)).astype(dtype)
        if rng.rand() < 0.3:
            wild = rng.rand(T, N) < 0.2
            a[wild] = rng.randint(-50, 50, int(wild.sum()))
        ao, ah = a.copy(), a.copy()
        ro, rh = o.single_rollout(eo, ao, mode), h.single_rollout(eh, ah, mode)
        for k in ro:
            same(ro[k], rh[k], f'{desc} launch {launch} T={T} {k}')
        same(ao, ah, f'{desc} launch {launch} actions'); same(eo, eh, f'{desc} launch {launch} state')
        if rng.rand() < 0.3:   # leave some envs done-but-not-reset for the next launch
            a1 = rng.randint(0, 4, N).astype(np.int64)
            for _ in range(int(rng.randint(1, 6))):
                o.single_step(eo, a1.copy(), 'none'); h.single_step(eh, a1.copy(), 'none')
            same(eo, eh, f'{desc} un-reset steps')
    return desc


def fuzz_lane(rng):
    """The one-env-per-LANE rollout (lane_rollout.hpp), forced at small batch sizes: random envs-per-wave, ragged batches,
    tape lengths around the chunk / action-batch sizes, hostile action values, chained launches, un-reset envs and
    hand-edited states between launches (they must fall back to the generic path inside the launch)."""
    epw = int(rng.choice([4, 8, 16, 32, 64]))
    N = int(rng.choice([1, 3, epw - 1, epw, epw + 1, 2 * epw + 5, 3 * epw, 200]))
    # (round 4: one_channel / default through bit planes, positions / partial_0 / partial_1 float by float; round 5: partial_3
    # through 7 x 7 bit planes, raw through a byte slab; partial_4 is routed to the one-env-per-wave kernels inside the same
    # entry point)
    mode = ['partial_2', 'partial_2', 'none', 'one_channel', 'one_channel', 'default', 'default', 'positions', 'partial_0',
            'partial_1', 'partial_3', 'partial_3', 'raw', 'raw', 'partial_4'][rng.randint(15)]
    # (round 6: a third of the cases on 10 x 10 / 11 x 11 — lane_wide.hpp: 8 / 16 / 32 envs per wave; 'default', 'one_channel',
    # 'partial_2', 'partial_3', none through its bit planes, every other mode through the one-env-per-wave kernels)
    S = int(rng.choice([9, 9, 10, 11]))
    if S != 9:
        epw = int(rng.choice([8, 16, 32]))
        N = int(rng.choice([1, 3, epw - 1, epw, epw + 1, 2 * epw + 5, 3 * epw, 200]))
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 40))
    desc = f'lane S={S} epw={epw} N={N} mode={mode} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    eo, eh = np.zeros((N, 3, S, S), np.float32), np.zeros((N, 3, S, S), np.float32)
    o.single_reset(eo, np.ones(N), 'none'); h.single_reset(eh, np.ones(N), 'none')
    o.call = h.call = int(rng.randint(1 << 50))
    old = {'WURM_LANE_ROLLOUT_MIN_ENVS': _lib.set_option('WURM_LANE_ROLLOUT_MIN_ENVS', 0),
           'WURM_LANE_ROLLOUT_EPW': _lib.set_option('WURM_LANE_ROLLOUT_EPW', epw)}
    try:
        tc = 64 // epw
        for launch in range(int(rng.randint(1, 4))):
            T = int(rng.choice([1, 2, tc - 1, tc, tc + 1, 16 * tc - 1, 16 * tc, 16 * tc + 1, 30, 64, 100, 200]))
            T = max(T, 1)
            dtype = np.int64 if rng.rand() < 0.7 else np.int32
            a = rng.randint(0, 4, (T, N)).astype(dtype)
            if rng.rand() < 0.3:
                wild = rng.rand(T, N) < 0.2
                a[wild] = rng.randint(-50, 50, int(wild.sum()))
            ao, ah = a.copy(), a.copy()
            ro, rh = o.single_rollout(eo, ao, mode), h.single_rollout(eh, ah, mode)
            for k in ro:
                same(ro[k], rh[k], f'{desc} launch {launch} T={T} {k}')
            same(ao, ah, f'{desc} launch {launch} actions'); same(eo, eh, f'{desc} launch {launch} state')
            r = rng.rand()
            if r < 0.25:   # leave some envs done-but-not-reset for the next launch
                a1 = rng.randint(0, 4, N).astype(np.int64)
                for _ in range(int(rng.randint(1, 6))):
                    o.single_step(eo, a1.copy(), 'none'); h.single_step(eh, a1.copy(), 'none')
                same(eo, eh, f'{desc} un-reset steps')
            elif r < 0.4:  # hand-edit a few envs: extra food, head wiped, body value removed
                for e in rng.randint(0, N, size=min(N, 3)):
                    kind = rng.randint(3)
                    if kind == 0:
                        eo[e, 0, rng.randint(1, S - 1), rng.randint(1, S - 1)] = 1
                    elif kind == 1:
                        eo[e, 1] = 0
                    else:
                        eo[e, 2][eo[e, 2] == 2] = 0
                eh[...] = eo
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    return desc


def fuzz_policy(rng):
    S, n = int(rng.choice([9, 9, 10, 11])), int(rng.randint(0, 4))
    N, T = int(rng.choice([1, 5, 33, 64, 100])), int(rng.choice([1, 7, 64, 65, 130]))
    E = 3 * (2 * n + 1) ** 2
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 40))
    params = (rng.randn(_o.policy_param_count(E)) * float(rng.choice([0.05, 0.3, 1.0, 3.0]))).astype(np.float32)
    desc = f'policy S={S} n={n} N={N} T={T} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    eo = np.zeros((N, 3, S, S), np.float32)
    obs0 = o.single_reset(eo, np.ones(N), f'partial_{n}')
    eh = eo.copy()
    o.call = h.call = int(rng.randint(1 << 50))
    for launch in range(2):
        ro, rh = o.single_policy_rollout(eo, obs0, params, T, n), h.single_policy_rollout(eh, obs0, params, T, n)
        assert (rh['status'] == 0).all(), desc + ' status'
        for k in ro:
            same(ro[k], rh[k], f'{desc} launch {launch} {k}')
        same(eo, eh, f'{desc} launch {launch} state')
        obs0 = ro['obs'][-1]
    return desc


def fuzz_policy_wide(rng):
    """policy_wide_kernel (wurm_single_policy_rollout_mode, wurm_grid_policy_rollout) over its whole domain: sizes with
    weight on the edges of the cells-per-lane buckets, every crop and 'positions', batches up to 2 100 envs (every
    workgroup shape), start states from tests/policy_states.py or a fresh reset, large keys, two chained launches.
    WURM_POLICY_WIDE = 1 keeps the old kernels' shapes (S <= 11, n <= 3) on this kernel too."""
    from tests import policy_states as ps
    from tests.test_policy_rollout_wide import hip_rollout, oracle_composed
    snake = rng.rand() < 0.7
    edges = [9, 11, 12, 16, 17, 22, 23, 32, 33, 39, 40, 45, 46, 55, 56, 64]
    S = int(rng.choice(edges)) if rng.rand() < 0.6 else int(rng.randint(9 if snake else 5, 65))
    n = int(rng.randint(0, 7))
    mode = f'partial_{n}' if snake and rng.rand() < 0.75 else 'positions'
    E = 4 if mode == 'positions' else 3 * (2 * n + 1) ** 2
    N = int(rng.choice([1, 5, 64, 100, 300, 1100, 2100]))
    T = int(rng.choice([1, 3, 7] if N >= 300 else [1, 7, 64, 65, 130]))
    T = max(1, min(T, 1000000 // (N * E)))   # the oracle is the cost: about 0.2 s per million weights times inputs
    kind = ['filled', 'fresh', 'crowded'][int(rng.choice(3, p=[0.5, 0.35, 0.15]))]
    if kind == 'crowded' and (not snake or S > 47):
        kind = 'filled'
    scale = float(rng.choice([0.05, 0.3, 1.0, 3.0]))
    seed, off, call = int(rng.randint(1 << 62)), int(rng.randint(1 << 44)), int(rng.randint(1 << 50))
    desc = f'policy_wide {"snake" if snake else "grid"} S={S} mode={mode} N={N} T={T} states={kind} scale={scale} seed={seed} off={off} call={call}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    grid = None if snake else (int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1)))
    if snake:
        if kind == 'fresh':
            eo = np.zeros((N, 3, S, S), np.float32)
            _o.single_reset(eo, np.ones(N, np.uint8), 'none', seed, 0, off)
        else:
            eo = ps.crowded_snake_states(N, S, rng) if kind == 'crowded' else ps.snake_states(N, S, rng, fill=float(rng.rand()))
        obs0 = _o.single_observe(eo, mode)
    else:
        if kind == 'fresh':
            eo = np.zeros((N, 2, S, S), np.float32)
            _o.grid_reset(eo, np.ones(N, np.uint8), grid, 'none', seed, 0, off)
        else:
            eo = ps.grid_states(N, S, rng)
        obs0 = _o.grid_observe(eo, 'positions')
    obs0 = np.asarray(obs0, np.float32).reshape(N, E)
    params = (rng.randn(_o.policy_param_count(E)) * scale).astype(np.float32)
    eh = eo.copy()
    old = _lib.set_option('WURM_POLICY_WIDE', 1)
    try:
        for launch in range(2):
            if snake and mode != 'positions':
                ro = _o.single_policy_rollout(eo, obs0, params, T, n, seed, call, off)
            else:
                ro = oracle_composed(eo, obs0, params, T, seed, call, off, mode, grid)
            rh = hip_rollout(eh, obs0, params, T, seed, call, off, mode, grid)
            assert _lib.lib().wurm_policy_last_route() == b'policy_wide', desc + ' route'
            assert (rh.pop('status') == 0).all(), desc + ' status'
            for k in ro:
                same(ro[k], rh[k], f'{desc} launch {launch} {k}')
            same(eo, eh, f'{desc} launch {launch} state')
            obs0, call = ro['obs'][-1], call + 2 * T
    finally:
        _lib.set_option('WURM_POLICY_WIDE', old)
    return desc


def fuzz_grid(rng):
    S = int(rng.choice([5, 7, 9, 12, 20, 33, 64]))
    N, T = int(rng.randint(1, 40)), int(rng.randint(5, 80))
    mode = ['default', 'raw', 'positions', 'none'][rng.randint(4)]
    start = (int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1)))
    seed = int(rng.randint(1 << 30))
    desc = f'grid S={S} N={N} T={T} mode={mode} start={start} seed={seed}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed), HipBackend(seed)
    eo, eh = np.zeros((N, 2, S, S), np.float32), np.zeros((N, 2, S, S), np.float32)
    o.grid_reset(eo, np.ones(N), start, 'none'); h.grid_reset(eh, np.ones(N), start, 'none')
    a = rng.randint(0, 4, (T, N)).astype(np.int64)
    ro, rh = o.grid_rollout(eo, a.copy(), start, mode), h.grid_rollout(eh, a.copy(), start, mode)
    for k in ro:
        same(ro[k], rh[k], f'{desc} {k}')
    same(eo, eh, desc + ' state')
    return desc


def fuzz_grid_lane(rng):
    """SimpleGridworld rollouts through the one-env-per-lane kernel (gridworld_lane.hip), forced at small batch sizes: every
    envs-per-wave of the image modes (runs composed in LDS and runs beyond the slab budget), ragged and odd batches, chained
    launches, hand-made states between launches that must go to the one-env-per-wave kernel in the second launch (two
    foods, no agent, food under the agent) and ones that stay in the domain (no food, food or agent on the border ring)."""
    S = int(rng.choice([5, 7, 9, 9, 9, 12, 20, 33, 64]))
    epw = int(rng.choice([-1, 4, 8, 16, 32, 64]))
    N = int(rng.choice([1, 3, 63, 64, 65, 131, 200, 257])) if S <= 20 else int(rng.randint(1, 40))
    mode = ['default', 'default', 'raw', 'raw', 'positions', 'none'][rng.randint(6)]
    start = (int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1)))
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 40))
    desc = f'grid_lane S={S} N={N} epw={epw} mode={mode} start={start} seed={seed} off={off}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    eo, eh = np.zeros((N, 2, S, S), np.float32), np.zeros((N, 2, S, S), np.float32)
    o.grid_reset(eo, np.ones(N), start, 'none'); h.grid_reset(eh, np.ones(N), start, 'none')
    o.call = h.call = int(rng.randint(1 << 50))
    old = {'WURM_LANE_ROLLOUT_MIN_ENVS': _lib.set_option('WURM_LANE_ROLLOUT_MIN_ENVS', 0),
           'WURM_LANE_STEP_MIN_ENVS': _lib.set_option('WURM_LANE_STEP_MIN_ENVS', 0),
           'WURM_GRIDWORLD_LANE_EPW': _lib.set_option('WURM_GRIDWORLD_LANE_EPW', epw)}
    try:
        for launch in range(int(rng.randint(1, 4))):
            T = int(rng.choice([1, 2, 3, 4, 5, 8, 17, 40, 90]))
            a = rng.randint(0, 4, (T, N)).astype(np.int64 if rng.rand() < 0.7 else np.int32)
            if rng.rand() < 0.3:
                wild = rng.rand(T, N) < 0.2
                a[wild] = rng.randint(-50, 50, int(wild.sum()))
            ro, rh = o.grid_rollout(eo, a.copy(), start, mode), h.grid_rollout(eh, a.copy(), start, mode)
            assert _lib.lib().wurm_single_last_route().decode() == 'gridworld_lane', desc
            for k in ro:
                same(ro[k], rh[k], f'{desc} launch {launch} T={T} {k}')
            same(eo, eh, f'{desc} launch {launch} state')
            for _ in range(int(rng.randint(0, 4))):   # hand-made states for the next launch
                i, kind = int(rng.randint(N)), int(rng.randint(6))
                y, x = int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))
                if kind == 0:
                    eo[i, 0, y, x] = 1                                   # (maybe) a second food
                elif kind == 1:
                    eo[i, 1] = 0                                         # no agent
                elif kind == 2:
                    eo[i, 0] = eo[i, 1]                                  # the food under the agent
                elif kind == 3:
                    eo[i, 0] = 0                                         # no food
                elif kind == 4:
                    eo[i, 0] = 0; eo[i, 0, 0, x] = 1                     # the only food on the border ring
                else:
                    eo[i, 1] = 0; eo[i, 1, y, 0] = 1                     # the agent on the border ring
                eh[i] = eo[i]
        # ... and the per-call step of the same file (gridworld_lane_step_kernel): the deferred form with / without the reset
        # observation, iterations without any reset, from whatever state the launches above left
        # (round 6) half of the cases on the caller's mirror of one record per env (wurm_grid_resident_bytes), lazy or eager,
        # written out only now and then; hand-made states in between (some outside the lane kernel's domain: the mirror is then
        # refused, resident_valid == 2, until the next edit clears it)
        call, prev, prev_call = int(rng.randint(1 << 40)) * 2, None, None
        res = {'lazy': bool(rng.rand() < 0.6), 'sync': True} if rng.rand() < 0.5 else None
        synced = True
        for t in range(int(rng.randint(0, 25))):
            a = rng.randint(0, 4, N).astype(np.int64 if rng.rand() < 0.7 else np.int32)
            style = int(rng.randint(1, 4))   # 1: deferred reset, 2: deferred + obs_after, 3: no reset at all
            kw = dict(call=call, grid=start)
            if style in (1, 2):
                kw.update(pre_done=prev, pre_call=prev_call, want_obs_after=(style == 2))
            if res is not None:
                res['sync'] = bool(rng.rand() < 0.5)
                kw['resident'] = res
            ro = o.single_step_reset(eo, a.copy(), mode, **{k: v for k, v in kw.items() if k != 'resident'})
            rh = h.single_step_reset(eh, a.copy(), mode, **kw)
            synced = res is None or not res['lazy'] or res['sync'] or res.get('valid') != 1
            how = 'no mirror' if res is None else f"mirror lazy={res['lazy']} valid={res.get('valid')} sync={res['sync']}"
            if synced:
                same(eo, eh, f'{desc} per call t={t} style={style} state ({how})')
            for k in ro:
                same(ro[k], rh[k], f'{desc} per call t={t} style={style} {k} ({how})')
            prev, prev_call = (None, None) if style == 3 else (ro['done'], call + 1)
            call += 2
            if synced and rng.rand() < 0.2:   # the caller edits the state it can see, and says so
                i, kind = int(rng.randint(N)), int(rng.randint(4))
                y, x = int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))
                if kind == 0:
                    eo[i, 0, y, x] = 1
                elif kind == 1:
                    eo[i, 1] = 0
                elif kind == 2:
                    eo[i, 0] = eo[i, 1]
                else:
                    eo[i, 0] = 0
                eh[i] = eo[i]
                if res is not None:
                    res['valid'] = 0
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    return desc


# (round 6) the shapes with kernels of their own — K, S and the crop radius compiled in (multi_device.hpp: shape_constants)
SPECIAL_SHAPES = [(4, 25, 'partial_5'), (4, 25, 'full'), (10, 36, 'full'), (2, 12, 'full')]


def fuzz_multi(rng):
    S = int(rng.choice([8, 10, 12, 14, 18, 25, 30, 36, 44]))
    K = int(rng.choice([1, 2, 2, 3, 4, 4, 5, 8, 10, 16]))
    while 2 * K * S * S + 8 * S * S > 60000:
        K = max(1, K // 2)
    mode = ['full', f'partial_{rng.randint(1, 6)}'][rng.randint(2)]
    if rng.rand() < 0.3:
        K, S, mode = SPECIAL_SHAPES[rng.randint(len(SPECIAL_SHAPES))]
    N, T = int(rng.randint(1, 20 if S <= 18 else 6)), int(rng.randint(5, 60 if S <= 18 else 25))
    cfg = dict(boost=bool(rng.rand() < 0.8), food_on_death_prob=float(rng.choice([0.0, 0.2, 0.5, 0.9, 1.0])),
               boost_cost_prob=float(rng.choice([0.0, 0.25, 0.5, 1.0])), food_mode=['only_one', 'random_rate'][rng.randint(2)],
               food_rate=float(rng.choice([5e-4, 5e-3, 5e-2])), reward_on_death=float(rng.choice([-1, -2, 0])),
               respawn_mode=['all', 'any'][rng.randint(2)], colour_mode=['random', 'fixed'][rng.randint(2)])
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'multi S={S} K={K} N={N} T={T} mode={mode} seed={seed} off={off} cfg={cfg}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    so, sh = _o.multi_empty_state(N, K, S), _o.multi_empty_state(N, K, S)
    so['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
    sh['colours'][...] = h.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
    o._next(); h._next()
    fo, fh = o.multi_reset(so, np.ones(N), cfg), h.multi_reset(sh, np.ones(N), cfg)
    assert fo == fh, f'{desc}: spawn failures {fo} vs {fh}'
    for k in so:
        same(so[k], sh[k], f'{desc} fresh {k}')
    a = rng.randint(0, 8, (T, K, N)).astype(np.int64)
    if rng.rand() < 0.5:
        for t in range(T):
            ro, rh = o.multi_step(so, a[t], cfg, mode), h.multi_step(sh, a[t], cfg, mode)
            for k in ro:
                same(ro[k], rh[k], f'{desc} {k} t={t}')
            for k in so:
                same(so[k], sh[k], f'{desc} state {k} t={t}')
            done_env = ro['all_done'] if rng.rand() < 0.8 else (rng.rand(N) < 0.2)
            o.multi_reset(so, done_env, cfg, mode=mode); h.multi_reset(sh, done_env, cfg, mode=mode)
            for k in so:
                same(so[k], sh[k], f'{desc} reset {k} t={t}')
            same(o.last_reset_obs, h.last_reset_obs, f'{desc} reset obs t={t}')
            if rng.rand() < 0.06:   # hand-made: food anywhere inside the ring — under a body or a head too —, sometimes ON the ring
                lo, hi = (0, S) if rng.rand() < 0.2 else (1, S - 1)
                so['foods'][int(rng.randint(N)), 0, int(rng.randint(lo, hi)), int(rng.randint(lo, hi))] = 1
                sh['foods'][...] = so['foods']
    else:
        ro, rh = o.multi_rollout(so, a, cfg, mode), h.multi_rollout(sh, a, cfg, mode)
        for k in ro:
            same(ro[k], rh[k], f'{desc} rollout {k}')
        for k in so:
            same(so[k], sh[k], f'{desc} rollout state {k}')
    same(o.multi_check(so), h.multi_check(sh), desc + ' check')
    return desc


def fuzz_multi_resident(rng):
    """wurm_multi_step_reset on the resident mirror (wurm_multi_call.resident), eager and lazy: random K / S (one env per
    wave and per workgroup), dynamics and observation modes; postponed resets with the step's own mask, arbitrary masks, no
    reset at all; the fp32 state compared whenever the lazy form writes it out; hand-edited food in between."""
    S = int(rng.choice([8, 10, 12, 14, 18, 25, 30, 36, 44]))
    K = int(rng.choice([1, 2, 2, 3, 4, 4, 5, 8, 10, 16]))
    while 2 * K * S * S + 8 * S * S > 60000:
        K = max(1, K // 2)
    mode = ['full', f'partial_{rng.randint(1, 6)}', 'none'][rng.randint(3)]
    if rng.rand() < 0.3:
        K, S, mode = SPECIAL_SHAPES[rng.randint(len(SPECIAL_SHAPES))]
    N, T = int(rng.randint(1, 20 if S <= 18 else 6)), int(rng.randint(5, 60 if S <= 18 else 25))
    cfg = dict(boost=bool(rng.rand() < 0.8), food_on_death_prob=float(rng.choice([0.0, 0.2, 0.5, 0.9, 1.0])),
               boost_cost_prob=float(rng.choice([0.0, 0.25, 0.5, 1.0])), food_mode=['only_one', 'random_rate'][rng.randint(2)],
               food_rate=float(rng.choice([5e-4, 5e-3, 5e-2])), reward_on_death=float(rng.choice([-1, -2, 0])),
               respawn_mode=['all', 'any'][rng.randint(2)], colour_mode=['random', 'fixed'][rng.randint(2)])
    lazy = bool(rng.rand() < 0.6)
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'multi_resident S={S} K={K} N={N} T={T} mode={mode} lazy={lazy} seed={seed} off={off} cfg={cfg}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    old = _lib.set_option('WURM_RESIDENT_MIN_ENVS', 0)
    try:
        o, h = OracleBackend(seed, off), HipBackend(seed, off)
        so = _o.multi_empty_state(N, K, S)
        so['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
        o.call = 1
        o.multi_reset(so, np.ones(N), cfg)
        sh = {k: v.copy() for k, v in so.items()}
        mirror = {'valid': 0, 'lazy': lazy}
        call, prev, prev_call = 2, None, 0
        for t in range(T):
            a = rng.randint(0, 8, size=(K, N)).astype(np.int64)
            if prev is not None:
                o.call = prev_call
                o.multi_reset(so, prev, cfg)
            o.call = call
            ro = o.multi_step(so, a, cfg, mode)
            edit = rng.rand() < 0.06
            mirror['sync'] = bool(not lazy or edit or rng.rand() < 0.3 or t == T - 1)
            rh = h.multi_step_reset(sh, a, cfg, mode, call=call, pre_done=prev, pre_call=prev_call,
                                    want_obs_after=bool(rng.rand() < 0.5) and mode != 'none', resident=mirror)
            for k in so:
                if mirror['sync'] or k not in ('foods', 'heads', 'bodies'):
                    same(so[k], sh[k], f'{desc} state {k} t={t}')
            for k in ro:
                same(ro[k], rh[k], f'{desc} {k} t={t}')
            # check_consistency's mask out of the step launch (wurm_multi_call.check_mask): where it vouches, the checker's
            got = mirror['masks'][0].cpu().numpy().astype(np.int64)
            want_m = np.asarray(o.multi_check(so)).astype(np.int64)
            known = got != -1
            same(got[known], want_m[known], f'{desc} check_mask t={t}')
            if 'obs_after' in rh:
                tmp = {k: v.copy() for k, v in so.items()}
                o.call = call + 1
                o.multi_reset(tmp, ro['all_done'], cfg, mode=mode)
                same(o.last_reset_obs, rh['obs_after'], f'{desc} obs_after t={t}')
                got = mirror['masks'][1].cpu().numpy().astype(np.int64)
                want_m = np.asarray(o.multi_check(tmp)).astype(np.int64)
                known = got != -1
                same(got[known], want_m[known], f'{desc} check_mask_after t={t}')
            u = rng.rand()
            if u < 0.15:
                prev = None
            elif u < 0.3:
                prev, prev_call = (rng.rand(N) < 0.3).astype(np.uint8), call + 1
            else:
                prev, prev_call = ro['all_done'], call + 1
            call += 2
            if edit:
                # (hand-made: food anywhere inside the ring — under a body or a head too; one time in five ON the ring)
                lo, hi = (0, S) if rng.rand() < 0.2 else (1, S - 1)
                so['foods'][int(rng.randint(N)), 0, int(rng.randint(lo, hi)), int(rng.randint(lo, hi))] = 1
                sh['foods'][...] = so['foods']
                mirror['valid'] = 0
    finally:
        _lib.set_option('WURM_RESIDENT_MIN_ENVS', old)
    return desc


def fuzz_multi_group(rng):
    """wurm_multi_rollout through multi_rollout_group_kernel (round 4: G envs per workgroup, per-agent class codes, work
    sharing; 6 .. 10 snakes: 32-bit codes, one buffer) in every compiled shape, and wurm_multi_step_reset with the grouped
    writer of the per-call kernel: 'full' observations, random K / S / N / T and dynamics, chained launches."""
    K = int(rng.choice([1, 2, 3, 4, 4, 5, 6, 8, 10]))
    S = int(rng.choice([8, 10, 12, 14, 18, 25, 27, 30, 36]))
    while 2 * K * S * S + 8 * S * S > 60000:
        S -= 4
    if rng.rand() < 0.3:
        K, S = [(4, 25), (10, 36), (2, 12)][rng.randint(3)]
    N = int(rng.choice([1, 3, 7, 8, 9, 15, 16, 17, 33])) if S <= 18 else int(rng.randint(1, 12))
    cfg = dict(boost=bool(rng.rand() < 0.8), food_on_death_prob=float(rng.choice([0.0, 0.2, 0.5, 0.9, 1.0])),
               boost_cost_prob=float(rng.choice([0.0, 0.25, 0.5, 1.0])), food_mode=['only_one', 'random_rate'][rng.randint(2)],
               food_rate=float(rng.choice([5e-4, 5e-3, 5e-2])), reward_on_death=float(rng.choice([-1, -2, 0])),
               respawn_mode=['all', 'any'][rng.randint(2)], colour_mode=['random', 'fixed'][rng.randint(2)])
    shape = int(rng.choice([0, 8215, 8416, 4414, 8424])) if K <= 5 else int(rng.choice([0, 5014, 4514, 3014]))
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'multi_group S={S} K={K} N={N} shape={shape} seed={seed} off={off} cfg={cfg}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    o, h = OracleBackend(seed, off), HipBackend(seed, off)
    so, sh = _o.multi_empty_state(N, K, S), _o.multi_empty_state(N, K, S)
    so['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
    sh['colours'][...] = so['colours']
    o._next(); h._next()
    fo, fh = o.multi_reset(so, np.ones(N), cfg), h.multi_reset(sh, np.ones(N), cfg)
    assert fo == fh, f'{desc}: spawn failures {fo} vs {fh}'
    old = {'WURM_MULTI_GROUP_MIN_ENVS': _lib.set_option('WURM_MULTI_GROUP_MIN_ENVS', 0),
           'WURM_MULTI_GROUP_SHAPE': _lib.set_option('WURM_MULTI_GROUP_SHAPE', shape)}
    try:
        for launch in range(int(rng.randint(1, 4))):
            T = int(rng.choice([1, 2, 5, 16, 30, 63, 64, 65, 100]) if S <= 18 else rng.choice([1, 2, 9, 20]))
            a = rng.randint(0, 8, (T, K, N)).astype(np.int64)
            ro, rh = o.multi_rollout(so, a, cfg, 'full'), h.multi_rollout(sh, a, cfg, 'full')
            for k in ro:
                same(ro[k], rh[k], f'{desc} launch {launch} T={T} {k}')
            for k in so:
                same(so[k], sh[k], f'{desc} launch {launch} state {k}')
            if rng.rand() < 0.5:   # a few per-call iterations in between (the grouped writer of multi_step_kernel)
                for t in range(int(rng.randint(1, 6))):
                    at = rng.randint(0, 8, (K, N)).astype(np.int64)
                    po, ph = o.multi_step(so, at, cfg, 'full'), h.multi_step(sh, at, cfg, 'full')
                    for k in po:
                        same(po[k], ph[k], f'{desc} per call {k} t={t}')
                    o.multi_reset(so, po['all_done'], cfg, mode='full'); h.multi_reset(sh, ph['all_done'], cfg, mode='full')
                    same(o.last_reset_obs, h.last_reset_obs, f'{desc} per call reset obs t={t}')
                    for k in so:
                        same(so[k], sh[k], f'{desc} per call state {k} t={t}')
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    return desc


def fuzz_multi_mirror_class(rng):
    """MultiSnake through the host class with the resident mirror on: fused rollouts (wurm_multi_rollout_resident — the
    grouped writer, the one-wave rollout, or the two-wave form that does not keep the mirror) and per-call steps take turns
    on one env object, the state tensors are looked at, held and edited in place in between; every output and the state at
    the looks against the oracle."""
    import torch
    from wurm_amd.envs import MultiSnake
    case = int(os.environ.get('WURM_FUZZ_REPLAY_CASE', 0)) or int(rng.randint(1, 1 << 30))
    rng = np.random.RandomState(case)   # (everything below is drawn from the case's own stream: `--replay multi_mirror_class:<case>`)
    verbose = bool(os.environ.get('WURM_FUZZ_VERBOSE'))
    S = int(rng.choice([8, 10, 12, 14, 18, 25, 30, 36]))
    K = int(rng.choice([1, 2, 3, 4, 4, 5, 8, 10, 12]))
    while 2 * K * S * S + 8 * S * S > 60000 or 16 * K > (S - 4) * (S - 4):   # (and room to place every snake: the constructor raises)
        K = max(1, K // 2)
    N = int(rng.randint(1, 24 if S <= 18 else 8))
    mode = ['full', 'full', f'partial_{rng.randint(1, 6)}'][rng.randint(3)]
    cfg = dict(boost=bool(rng.rand() < 0.8), food_on_death_prob=float(rng.choice([0.0, 0.2, 0.5, 0.9, 1.0])),
               boost_cost_prob=float(rng.choice([0.0, 0.25, 0.5, 1.0])), food_mode=['only_one', 'random_rate'][rng.randint(2)],
               food_rate=float(rng.choice([5e-4, 5e-3, 5e-2])), reward_on_death=float(rng.choice([-1, -2, 0])),
               respawn_mode=['all', 'any'][rng.randint(2)], colour_mode=['random', 'fixed'][rng.randint(2)])
    group = bool(rng.rand() < 0.7)
    seed, off = int(rng.randint(1 << 30)), int(rng.randint(1 << 20))
    desc = f'multi_mirror_class case={case} S={S} K={K} N={N} mode={mode} group={group} seed={seed} off={off} cfg={cfg}'
    if os.environ.get('WURM_FUZZ_VERBOSE'):
        print('start:', desc, flush=True)
    with _lib.knobs(WURM_RESIDENT_MIN_ENVS=0, WURM_MULTI_GROUP_MIN_ENVS=0 if group else 1 << 40):
        env = MultiSnake(N, K, S, device='cuda:0', seed=seed, env_offset=off, observation_mode=mode, boost=cfg['boost'],
                         food_on_death_prob=cfg['food_on_death_prob'], boost_cost_prob=cfg['boost_cost_prob'],
                         food_mode=cfg['food_mode'], food_rate=cfg['food_rate'], respawn_mode=cfg['respawn_mode'],
                         reward_on_death=cfg['reward_on_death'], agent_colours=cfg['colour_mode'])
        o = OracleBackend(seed, off)
        st = _o.multi_empty_state(N, K, S)
        st['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
        o.call = 1
        o.multi_reset(st, np.ones(N), cfg)
        alias = None
        for op in range(int(rng.randint(4, 12))):
            u = rng.rand()
            if verbose:
                print(f'  op {op}: u={u:.3f} mirror={env.mirror_state()} pending={env._pending}', flush=True)
            if u < 0.45:
                T = int(rng.randint(1, 12))
                a = rng.randint(0, 8, size=(T, K, N)).astype(np.int64)
                out = env.rollout(torch.from_numpy(a).cuda())
                ref = o.multi_rollout(st, a, cfg, mode)
                same(out['observations'].cpu().numpy().reshape(ref['obs'].shape), ref['obs'], f'{desc} op {op} rollout obs')
                same(out['all_done'].cpu().numpy().astype(np.uint8), ref['all_done'], f'{desc} op {op} rollout all_done')
                same(out['rewards'].cpu().numpy().transpose(0, 2, 1).reshape(T, -1), ref['rewards'].reshape(T, -1),
                     f'{desc} op {op} rollout rewards')
            elif u < 0.8:
                for t in range(int(rng.randint(1, 6))):
                    a = rng.randint(0, 8, size=(K, N)).astype(np.int64)
                    ac = torch.from_numpy(a).cuda()
                    obs, rew, dones, info = env.step({f'agent_{i}': ac[i] for i in range(K)})
                    r = o.multi_step(st, a, cfg, mode)
                    for i in range(K):
                        same(obs[f'agent_{i}'].cpu().numpy(), r['obs'][i], f'{desc} op {op} step {t} obs {i}')
                        same(rew[f'agent_{i}'].cpu().numpy(), r['rewards'].reshape(N, K)[:, i], f'{desc} op {op} step {t} reward {i}')
                    same(dones['__all__'].cpu().numpy().astype(np.uint8), r['all_done'], f'{desc} op {op} step {t} all_done')
                    how = int(rng.randint(5))   # the reset: postponed, with its observations, eager (not the step's own tensor), none,
                    # with its observations after the observation mode was changed (VERDICT r04's repro)
                    if how == 4:
                        mode = 'full' if mode != 'full' else f'partial_{rng.randint(1, 6)}'
                        env.observation_mode = mode
                        how = 1
                    if how == 0:
                        env.reset(dones['__all__'], return_observations=False)
                        o.multi_reset(st, r['all_done'], cfg)
                    elif how == 1:
                        back = env.reset(dones['__all__'])
                        o.multi_reset(st, r['all_done'], cfg, mode=mode)
                        for i in range(K):
                            same(back[f'agent_{i}'].cpu().numpy(), o.last_reset_obs[i], f'{desc} op {op} step {t} reset obs {i}')
                    elif how == 2:
                        env.reset(dones['__all__'].clone(), return_observations=False)
                        o.multi_reset(st, r['all_done'], cfg)
                    if rng.rand() < 0.15:       # experiments/speeds.py:37
                        ok = bool((o.multi_check(st) == 0).all())
                        try:
                            env.check_consistency()
                            assert ok, f'{desc} op {op} step {t}: check_consistency passed, the oracle finds a fault'
                        except RuntimeError:
                            assert not ok, f'{desc} op {op} step {t}: check_consistency raised, the oracle finds none'
            elif u < 0.9:
                same(env.foods.cpu().numpy(), st['foods'], f'{desc} op {op} look foods')
                same(env.bodies.cpu().numpy(), st['bodies'], f'{desc} op {op} look bodies')
                same(env.heads.cpu().numpy(), st['heads'], f'{desc} op {op} look heads')
                alias = env.foods
            elif u < 0.94:              # round 5: an attribute assigned between calls (reference tests/test_multi_snake_env.py:
                # 180,288,401-403,618; experiments/multiagent.py:340,345) — with a reset possibly postponed in front of it
                which = int(rng.randint(4))
                if which == 0:
                    cfg['respawn_mode'] = 'any' if cfg['respawn_mode'] == 'all' else 'all'
                    env.respawn_mode = cfg['respawn_mode']
                elif which == 1:
                    cfg['food_rate'] = float(rng.choice([5e-4, 5e-3, 5e-2, 0.4]))
                    env.food_rate = cfg['food_rate']
                elif which == 2:
                    cfg['food_on_death_prob'] = float(rng.choice([0.0, 0.33, 1.0]))
                    env.food_on_death_prob = cfg['food_on_death_prob']
                else:
                    mode = ['full', f'partial_{rng.randint(1, 6)}'][rng.randint(2)]
                    env.observation_mode = mode
            elif alias is not None:     # an in-place edit through a tensor the caller holds (no look first: while the caller
                # holds a state tensor no reset is postponed — round 5, _alias_free — so the edit lands where the reference's would)
                assert env.foods.data_ptr() == alias.data_ptr()
                e, y, x = int(rng.randint(N)), int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))
                occupied = st['bodies'].reshape(N, K, S, S)[e, :, y, x].sum() + st['heads'].reshape(N, K, S, S)[e, :, y, x].sum()
                if occupied == 0:
                    alias[e, 0, y, x] = 1.0
                    st['foods'][e, 0, y, x] = 1.0
        same(env.foods.cpu().numpy(), st['foods'], f'{desc} final foods')
        same(env.heads.cpu().numpy(), st['heads'], f'{desc} final heads')
        same(env.bodies.cpu().numpy(), st['bodies'], f'{desc} final bodies')
        same(env.dones.cpu().numpy().astype(np.uint8), st['dones'], f'{desc} final dones')
        same(env.orientations.cpu().numpy(), st['orientations'], f'{desc} final orientations')


def fuzz_single_mirror_class(rng):
    """SingleSnake through the host class, the same random sequence of operations on two env objects — the resident mirror
    forced on (WURM_RESIDENT_MIN_ENVS=0: the 32-byte records of 9 x 9, the clock-grid image from 12 x 12 on) and off (the
    per-call kernels, themselves checked against the oracle by the other families): steps with every flavour of reset,
    fused rollouts, looks at `envs`, in-place edits through a held alias (with and without a look in between),
    check_consistency(), a changed observation mode; every output and the state must be identical."""
    import torch
    from wurm_amd.envs import SingleSnake
    case = int(os.environ.get('WURM_FUZZ_REPLAY_CASE', 0)) or int(rng.randint(1, 1 << 30))
    rng = np.random.RandomState(case)
    verbose = bool(os.environ.get('WURM_FUZZ_VERBOSE'))
    S = int(rng.choice([9, 9, 9, 12, 16, 25, 36]))
    N = int(rng.randint(1, 400 if S == 9 else 48))
    modes = ['partial_2', 'one_channel', 'default', 'positions', 'partial_1'] if S == 9 else \
        ['default', 'partial_2', 'partial_5', 'one_channel', 'raw', 'positions']
    mode = modes[rng.randint(len(modes))]
    lazy_reset = bool(rng.rand() < 0.8)
    seed = int(rng.randint(1 << 30))
    nops = int(rng.randint(5, 25))
    desc = f'single_mirror_class case={case} S={S} N={N} mode={mode} lazy_reset={lazy_reset} seed={seed}'
    if verbose:
        print('start:', desc, flush=True)
    plan = []
    for _ in range(nops):
        u = rng.rand()
        if u < 0.5:
            plan.append(('steps', [(rng.randint(-1, 5, N), int(rng.randint(6)), modes[rng.randint(len(modes))])
                                   for _ in range(int(rng.randint(1, 6)))]))
        elif u < 0.65:
            T = int(rng.randint(1, 20))
            plan.append(('rollout', rng.randint(-1, 5, (T, N)), bool(rng.rand() < 0.8)))
        elif u < 0.75:
            plan.append(('look',))
        elif u < 0.8:
            plan.append(('hold',))
        elif u < 0.92:
            plan.append(('edit', int(rng.randint(N)), int(rng.randint(1 << 30)), bool(rng.rand() < 0.5)))
        elif u < 0.97:
            plan.append(('check',))
        else:
            plan.append(('mode', modes[rng.randint(len(modes))]))

    def run(mirror):
        out = []
        with _lib.knobs(WURM_RESIDENT_MIN_ENVS=0 if mirror else 10 ** 9):
            env = SingleSnake(N, S, observation_mode=mode, device='cuda:0', seed=seed, lazy_reset=lazy_reset)
            alias = None
            for i, op in enumerate(plan):
                if verbose and mirror:
                    print(f'  op {i}: {op[0]} mirror={env.mirror_state()}', flush=True)
                if op[0] == 'steps':
                    for a_np, how, other in op[1]:
                        a = torch.from_numpy(a_np).cuda()
                        obs, r, d, info = env.step(a)
                        if how == 4:    # round 5 (VERDICT r04's repro): the observation mode changes between step and reset(d)
                            env.observation_mode = other
                            how = 0
                        elif how == 5:  # ... or lazy_reset does
                            env.lazy_reset = not env.lazy_reset
                            how = 0
                        # (how == 3: no reset at all — finished envs are stepped again, and the mirror stays current with
                        # nothing postponed: the state in which a look must not forget an edit)
                        back = env.reset(d) if how == 0 else env.reset(d.clone()) if how == 1 else \
                            env.reset(d, return_observations=False) if how == 2 else None
                        out.append([x.clone() for x in (obs, r, d, info['self_collision'], info['edge_collision'], a)] +
                                   ([back.clone()] if back is not None else []))
                elif op[0] == 'rollout':
                    a = torch.from_numpy(op[1]).cuda()
                    res = env.rollout(a, return_observations=op[2])
                    out.append([a.clone()] + [v.clone() for v in res.values() if v is not None])
                elif op[0] == 'look':
                    out.append([env.envs.clone()])
                elif op[0] == 'hold':
                    alias = env.envs
                elif op[0] == 'edit' and alias is not None:
                    e, r2 = op[1], np.random.RandomState(op[2])
                    if not op[3]:
                        assert env.envs.data_ptr() == alias.data_ptr()   # (a look first)
                    else:
                        env.reset(torch.zeros(N, dtype=torch.bool, device='cuda:0'), return_observations=False)  # (flushes a postponed reset; no look)
                    st = alias[e].cpu().numpy()
                    free = np.argwhere((st[2, 1:-1, 1:-1] == 0) & (st[1, 1:-1, 1:-1] == 0)) + 1
                    if len(free):
                        y, x = free[r2.randint(len(free))]
                        alias[e, 0] = 0                  # the food of env e moves: version counter bumps
                        alias[e, 0, int(y), int(x)] = 1
                    out.append([alias.clone()])
                elif op[0] == 'check':
                    try:        # (an env stepped on after it finished is inconsistent: both objects must say so)
                        env.check_consistency()
                        out.append([torch.zeros(1)])
                    except RuntimeError:
                        out.append([torch.ones(1)])
                elif op[0] == 'mode':
                    env.observation_mode = op[1]
            out.append([env.envs.clone()])
        return out

    a, b = run(True), run(False)
    assert len(a) == len(b), desc
    for i, (xa, xb) in enumerate(zip(a, b)):
        assert len(xa) == len(xb), f'{desc} record {i}'
        for j, (x, y) in enumerate(zip(xa, xb)):
            assert x.shape == y.shape and torch.equal(x, y), f'{desc} record {i} output {j}: {int((x != y).sum())} mismatches'


FAMILIES = {'single': fuzz_single, 'fused': fuzz_fused, 'resident': fuzz_resident, 'lean': fuzz_lean, 'lane': fuzz_lane,
            'policy': fuzz_policy, 'policy_wide': fuzz_policy_wide, 'grid': fuzz_grid, 'grid_lane': fuzz_grid_lane, 'multi': fuzz_multi, 'multi_resident': fuzz_multi_resident,
            'multi_group': fuzz_multi_group, 'multi_mirror_class': fuzz_multi_mirror_class,
            'single_mirror_class': fuzz_single_mirror_class}
WEIGHTS = {'single': 0.08, 'fused': 0.08, 'resident': 0.13, 'lean': 0.04, 'lane': 0.15, 'policy': 0.03, 'policy_wide': 0.05, 'grid': 0.03, 'grid_lane': 0.07,
           'multi': 0.10, 'multi_resident': 0.08, 'multi_group': 0.12, 'multi_mirror_class': 0.07, 'single_mirror_class': 0.07}


def library_sha256():
    import hashlib
    from wurm_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=60)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default=None, help='comma-separated families (default: all, by weight)')
    ap.add_argument('--replay', default=None, help='family:case — one case of a family that draws from its own stream (multi_mirror_class, single_mirror_class)')
    ap.add_argument('--summary', default=None,
                    help='append a JSON record of this run (library sha256, seed, cases per family, forced thresholds, '
                         'mismatches) to this file, e.g. profiles/r03_fuzz_summary.json')
    ap.add_argument('--save-failures', default=None, help='directory: a failing case leaves the generator state in front of it there (fuzz_fail_<seed>_<n>.pkl)')
    ap.add_argument('--replay-state', default=None, help='such a file: re-run exactly that case')
    ap.add_argument('--repeat', type=int, default=1)
    args = ap.parse_args()
    rng = np.random.RandomState(args.seed)
    if args.replay:
        fam, case = args.replay.split(':')
        os.environ['WURM_FUZZ_REPLAY_CASE'] = case
        os.environ['WURM_FUZZ_VERBOSE'] = '1'
        FAMILIES[fam](rng)
        print('replay: no mismatch')
        sys.exit(0)
    if args.replay_state:
        # a case that failed in an earlier run, from the generator state saved in front of it: the same case, --repeat times
        import pickle
        kind, st = pickle.load(open(args.replay_state, 'rb'))
        bad = 0
        for r in range(args.repeat):
            rng.set_state(st)
            try:
                desc = FAMILIES[kind](rng)
            except AssertionError as e:
                bad += 1
                print(f'run {r}: MISMATCH: {str(e)[:600]}', flush=True)
            else:
                if r == 0:
                    print('run 0: ok —', desc, flush=True)
        print(f'replay of one {kind} case: {bad} of {args.repeat} runs mismatched')
        sys.exit(1 if bad else 0)
    kinds = [k for k in FAMILIES if args.only is None or k in args.only.split(',')]
    t0, n, fails, messages = time.time(), {k: 0 for k in kinds}, 0, []
    while time.time() - t0 < args.seconds:
        w = np.array([WEIGHTS[k] for k in kinds])
        kind = kinds[rng.choice(len(kinds), p=w / w.sum())]
        state_before = rng.get_state()
        try:
            FAMILIES[kind](rng)
            n[kind] += 1
        except AssertionError as e:
            fails += 1
            messages.append(str(e)[:600])
            print('MISMATCH:', str(e)[:600])
            if args.save_failures:   # the generator state in front of the case: --replay-state re-runs exactly this case
                import pickle
                os.makedirs(args.save_failures, exist_ok=True)
                pickle.dump((kind, state_before), open(os.path.join(args.save_failures, f'fuzz_fail_{args.seed}_{fails}.pkl'), 'wb'))
        except Exception:
            fails += 1
            messages.append(traceback.format_exc()[-600:])
            traceback.print_exc()
        if fails >= 5:
            break
    elapsed = time.time() - t0
    print(f'fuzz done: {n} cases, {fails} failures, {elapsed:.0f} s')
    if args.summary:
        import json
        rec = {'library_sha256': library_sha256(), 'seed': args.seed, 'seconds': round(elapsed, 1), 'cases': n,
               'total_cases': sum(n.values()), 'mismatches': fails, 'messages': messages,
               'forced_thresholds': {k: os.environ[k] for k in ('WURM_LANE_STEP_MIN_ENVS', 'WURM_GRID_STEP_MIN_CELLS',
                                                                 'WURM_LANE_ROLLOUT_MIN_ENVS', 'WURM_LANE_ROLLOUT_EPW',
                                                                 'WURM_RESIDENT_MIN_ENVS', 'WURM_MULTI_GROUP_MIN_ENVS')
                                     if k in os.environ},
               'bar': 'bit-exact HIP (C ABI) vs oracle on every output of every step'}
        runs = []
        if os.path.exists(args.summary):
            try:
                runs = json.load(open(args.summary))['runs']
            except Exception:
                runs = []
        runs.append(rec)
        json.dump({'what': 'tools/fuzz_parity.py runs on the GPU box (one record per run)', 'runs': runs,
                   'total_cases': sum(r['total_cases'] for r in runs),
                   'total_mismatches': sum(r['mismatches'] for r in runs)}, open(args.summary, 'w'), indent=1)
    sys.exit(1 if fails else 0)
