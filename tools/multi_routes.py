#!/usr/bin/env python3
"""Which kernel serves which MultiSnake call — seen from OUTSIDE the library, to compare two builds of it.

  run      one launch of the library per case of tests/test_multi_dispatch_table.py (its CASES, its run_case), in order,
           and the too-large case that launches nothing; prints one line per case.  A target for
               rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python3 tools/multi_routes.py run [--root TREE]
           (no counters, no other tracing).  --root: the checkout whose wurm_amd / tests / oracle are imported (another
           revision, built); the cases are always this checkout's.
  lanes    the same for the one-env-per-lane kernels of SingleSnake / SimpleGridworld: the cases of tests/test_dispatch_table.py
           that take a lane row (its own functions: oracle parity and the route's name are asserted), then launches on both
           sides of every switch from one wave per workgroup to four, a per-call step and a rollout at 10 x 10, and a
           SimpleGridworld rollout of 6 144 envs.  Compared with --pattern lane_.
  learner  the same for the fused A2C learner: `grad`, `apply` and `update` of FusedA2CLearner at (N, T, E) = (1, 1, 4),
           (300, 5, 75), (65, 20, 507) and of FusedA2CPopulation at (P, M) = (1, 5), (3, 2), (2, 300) (T = 5, E = 75), each
           with n-step and with GAE returns: N on both sides of the 256 workgroups of the main kernel, the smallest and the
           largest E.  Compared with --pattern a2c_ff_.
  host     the same for the MultiSnake CLASS (a refactor of its host layer): a per-call and rollout script on a mirrored
           (40 x 3 x 12, resident_mirror=True) and an unmirrored shape — both reset forms, check_consistency(), a state
           attribute read and edited, rollouts with and without observations.  Compared with the default pattern.
  compare  two such kernel traces, row by row in order of Start_Timestamp over the library's kernels whose name contains
           --pattern (default wurm::multi_; the backend's torch copies and fills are dropped by name): kernel name, grid
           size (x, and y / z where they are not 1), workgroup size, LDS size.  Exit status 1 on a difference.
               python3 tools/multi_routes.py compare [--pattern P] BASE_kernel_trace.csv HEAD_kernel_trace.csv > profiles/rNN_multi_routes.txt"""
import argparse
import csv
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(root):
    sys.path.insert(0, os.path.abspath(root))
    spec = importlib.util.spec_from_file_location('multi_dispatch_cases', os.path.join(HERE, 'tests', 'test_multi_dispatch_table.py'))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    from tests.hip_backend import HipBackend
    from wurm_amd import _lib
    lib = _lib.lib()
    named = hasattr(lib, 'wurm_multi_last_route')
    for case, cid in zip(cases.CASES, cases.IDS):
        n0 = lib.wurm_launch_count()
        got, want = cases.run_case(HipBackend, case)
        same = all(a.tobytes() == b.tobytes() for (_, a), (_, b) in zip(got, want))
        print(f'{cid:60s} launches {lib.wurm_launch_count() - n0}  oracle {"same" if same else "DIFFERENT"}  '
              f'route {lib.wurm_multi_last_route().decode() if named else "-":32s} expected {case[-1]}', flush=True)
    if named:
        cases.test_an_env_too_large_for_the_lds_is_unsupported_and_launches_nothing(HipBackend)
        print('too large: unsupported, no launch')


def run_lanes(root):
    sys.path.insert(0, os.path.abspath(root))
    spec = importlib.util.spec_from_file_location('dispatch_cases', os.path.join(HERE, 'tests', 'test_dispatch_table.py'))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    import numpy as np
    from tests.hip_backend import HipBackend
    from wurm_amd._lib import knobs
    for row in cases.ROLLOUT_ROWS:
        if row[-1].startswith('lane'):
            cases.test_rollout_rows(HipBackend, *row)
            print('rollout row', row, cases._route(), flush=True)
    for row in cases.STEP_ROWS:
        if row[-1].startswith('lane'):
            cases.test_step_rows(HipBackend, *row)
            print('step row', row, cases._route(), flush=True)
    cases.test_gridworld_calls_are_generic_and_large_rollouts_take_the_lane_row(HipBackend)
    print('gridworld rows', flush=True)

    h = HipBackend(seed=1)

    def fresh(N, S):
        envs = np.zeros((N, 3, S, S), np.float32)
        h.single_reset(envs, np.ones(N, np.uint8), 'none')
        return envs

    def rollout(N, S, mode, T=3, **kn):
        with knobs(WURM_LANE_ROLLOUT_MIN_ENVS=0, **kn):
            h.single_rollout(fresh(N, S), np.zeros((T, N), np.int64), mode)
        print('rollout', N, S, mode, kn, cases._route(), flush=True)

    def percall(N, S, mode, **kn):  # on the mirror: its build launch, then the step with both observations
        with knobs(**kn):
            h.single_step_reset(fresh(N, S), np.zeros(N, np.int64), mode, call=1, want_obs_after=True, resident={'valid': 0, 'lazy': True})
        print('per-call step', N, S, mode, kn, cases._route(), flush=True)

    for N in (8188, 8192):                                  # 2 047 / 2 048 waves of a rollout
        rollout(N, 9, 'partial_2', WURM_LANE_ROLLOUT_EPW=4)
        rollout(N, 9, 'raw', WURM_LANE_ROLLOUT_EPW=4)       # (four waves: past 64 KB of LDS)
    rollout(16376, 10, 'partial_2', WURM_LANE_ROLLOUT_EPW=8)
    rollout(16384, 10, 'partial_2', WURM_LANE_ROLLOUT_EPW=8)
    for N in (16368, 16384):                                # 1 023 / 1 024 waves of a per-call kernel
        percall(N, 9, 'partial_2', WURM_RESIDENT_EPW=16)
        percall(N, 9, 'raw', WURM_RESIDENT_EPW=16)
        percall(N, 10, 'default', WURM_RESIDENT_EPW=16)
    for N in (8192, 8196, 24576, 49152):                    # lane_step_kernel: one wave up to 8 192 envs; 4, 8, 16 envs per wave
        with knobs(WURM_LANE_STEP_MIN_ENVS=0):
            h.single_step(fresh(N, 9 if N != 8196 else 10), np.zeros(N, np.int64), 'partial_2')
        print('step', N, cases._route(), flush=True)
    g = np.zeros((6144, 2, 9, 9), np.float32)
    h.grid_reset(g, np.ones(6144, np.uint8), (4, 4), 'default')
    for mode in ('default', 'raw', 'positions'):
        h.grid_rollout(g, np.zeros((3, 6144), np.int64), (4, 4), mode)
        print('gridworld rollout', 6144, mode, cases._route(), flush=True)
    with knobs(WURM_LANE_STEP_MIN_ENVS=0):
        h.grid_step(g, np.zeros(6144, np.int64), 'default')
    print('gridworld step', 6144, cases._route(), flush=True)


def run_learner(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from wurm_amd import _lib
    from wurm_amd.agents import FeedforwardAgent
    from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation
    dev, lib = 'cuda:0', _lib.lib()

    def agent(E):
        return FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(dev)

    def issue(what, learner, N, T, E):
        g = torch.Generator().manual_seed(N + T + E)
        state = torch.rand((N, E), generator=g).to(dev)
        out = dict(observations=torch.rand((T, N, E), generator=g).to(dev), actions=torch.randint(4, (T, N), generator=g).to(dev),
                   rewards=torch.rand((T, N), generator=g).to(dev), dones=(torch.rand((T, N), generator=g) < 0.2).to(dev))
        n0 = lib.wurm_launch_count()
        grad, _ = learner.grad(state, out)
        learner.apply(grad)
        learner.update(state, out)
        torch.cuda.synchronize()
        print(f'{what:44s} launches {lib.wurm_launch_count() - n0}  step {learner.step}', flush=True)

    for gae in (dict(), dict(use_gae=True, gae_lambda=0.95)):
        for N, T, E in ((1, 1, 4), (300, 5, 75), (65, 20, 507)):
            issue(f'learner N={N} T={T} E={E} gae={bool(gae)}', FusedA2CLearner(agent(E), **gae), N, T, E)
        for P, M in ((1, 5), (3, 2), (2, 300)):
            pop = FusedA2CPopulation([agent(75) for _ in range(P)], lr=[1e-3 * (1 + p) for p in range(P)], **gae)
            issue(f'population P={P} M={M} T=5 E=75 gae={bool(gae)}', pop, P * M, 5, 75)


def run_host(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from wurm_amd import _lib
    from wurm_amd.envs import MultiSnake
    lib, N, K, S = _lib.lib(), 40, 3, 12
    acts = torch.randint(8, (24, K, N), generator=torch.Generator().manual_seed(3)).cuda()
    keys = ['agent_%d' % i for i in range(K)]
    for mirror in (True, False):
        env = MultiSnake(N, K, S, device='cuda:0', seed=7, resident_mirror=mirror, food_mode='random_rate', respawn_mode='any')
        n0 = lib.wurm_launch_count()
        for t in range(12):
            d = env.step(dict(zip(keys, acts[t])))[2]['__all__']
            if t < 4:
                env.reset(d, return_observations=False)
            else:
                env.reset(d)
            if t >= 8:
                env.check_consistency()
        b = env.bodies
        env.step(dict(zip(keys, acts[12])))
        b[0, 0, 0, 0] = 0.0
        env.step(dict(zip(keys, acts[13])))
        del b
        env.rollout(acts[14:17])
        env.step(dict(zip(keys, acts[17])))
        env.rollout(acts[18:21], return_observations=False)
        env.check_consistency()
        torch.cuda.synchronize()
        print(f'MultiSnake {N} x {K} x {S} resident_mirror={mirror}: launches {lib.wurm_launch_count() - n0}  '
              f'{env.mirror_state()["state"]}', flush=True)


def rows(path, pattern):
    out = []
    with open(path) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp'])):  # (the file is not in order of dispatch)
            if pattern in r['Kernel_Name']:
                grid = [int(r['Grid_Size_' + d]) for d in 'XYZ']
                while len(grid) > 1 and grid[-1] == 1:
                    grid.pop()
                out.append((re.sub(r'\(wurm::\w+\)', '', r['Kernel_Name'].replace('void ', '')).replace('wurm::', ''),
                            'x'.join(map(str, grid)), int(r['Workgroup_Size_X']), int(r['LDS_Block_Size'])))
    return out


def compare(base, head, pattern):
    b, h = rows(base, pattern), rows(head, pattern)
    print(f'# kernels named *{pattern}* of two rocprofv3 --kernel-trace runs of tools/multi_routes.py, in order of dispatch: {len(b)} / {len(h)} rows')
    print(f'# {"#":>3s} {"same":4s} {"grid":>9s} {"wg":>4s} {"lds":>7s}  kernel (base; head beside it where it differs)')
    bad = len(b) != len(h)
    for i in range(max(len(b), len(h))):
        x, y = b[i] if i < len(b) else None, h[i] if i < len(h) else None
        bad |= x != y
        k, g, w, l = x or y
        print(f'{i:5d} {"yes" if x == y else "NO":4s} {g:>9s} {w:4d} {l:7d}  {k}' + ('' if x == y else f'   |   head: {y}'))
    print(f'# {"every row equal" if not bad else "DIFFERENT"}')
    return int(bad)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['run', 'lanes', 'learner', 'host', 'compare'])
    ap.add_argument('traces', nargs='*')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--pattern', default='wurm::multi_', help='compare: the rows whose kernel name contains this')
    a = ap.parse_intermixed_args()
    sys.exit(compare(*a.traces, a.pattern) if a.what == 'compare' else {'run': run, 'lanes': run_lanes, 'learner': run_learner, 'host': run_host}[a.what](a.root))
