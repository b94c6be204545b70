#!/usr/bin/env python3
"""Throughput of the fused acting loop on the shapes beyond 9-11 x 9-11 'partial_n <= 3' (policy_wide.hpp) beside the
unfused per-step loop of the reference's experiment on the same shape (experiments/main.py:207-227: torch forward of
FeedforwardAgent + Categorical sample + env.step + env.reset(done), one iteration per step).  Env-steps/s, one JSON line
per (shape, batch, loop).  usage: bench_policy_wide.py [--envs 512 8192] [--steps 64] [--shapes snake20p2 ...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.distributions import Categorical  # noqa: E402
from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent, pack_policy_params  # noqa: E402
from wurm_amd.envs import SimpleGridworld, SingleSnake  # noqa: E402

SHAPES = {  # name: (env class, size, observation mode, inputs)
    'snake20p2': ('snake', 20, 'partial_2', 75),
    'snake36p5': ('snake', 36, 'partial_5', 363),
    'snake64p6': ('snake', 64, 'partial_6', 507),
    'grid9pos': ('grid', 9, 'positions', 4),
}


def make(kind, N, S, mode):
    if kind == 'snake':
        return SingleSnake(num_envs=N, size=S, observation_mode=mode, device='cuda', seed=0)
    return SimpleGridworld(num_envs=N, size=S, observation_mode=mode, device='cuda', seed=0, start_location=(S // 2, S // 2))


def fused(kind, N, S, mode, E, T, reps):
    torch.manual_seed(0)
    env = make(kind, N, S, mode)
    params = pack_policy_params(FeedforwardAgent(4, 2, 64, E).to('cuda'))
    state = env.reset()
    state = env.policy_rollout(params, state, T, check=False)['state']
    route = _lib.lib().wurm_policy_last_route().decode()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = env.policy_rollout(params, state, T, check=False)
        state = out['state']
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'env_steps_per_s': N * T * reps / dt, 'ms_per_launch': dt / reps * 1e3, 'route': route,
            'done_rate': float(out['dones'].float().mean())}


@torch.no_grad()
def unfused(kind, N, S, mode, E, T):
    torch.manual_seed(0)
    env = make(kind, N, S, mode)
    agent = FeedforwardAgent(4, 2, 64, E).to('cuda')
    state = env.reset()

    def one(state):
        probs, _ = agent(state.reshape(N, -1))
        action = Categorical(probs).sample()
        state, _, done, _ = env.step(action)
        env.reset(done)
        return state
    for _ in range(8):
        state = one(state)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(T):
        state = one(state)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'env_steps_per_s': N * T / dt, 'ms_per_step': dt / T * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='+', default=[512, 8192])
    ap.add_argument('--steps', type=int, default=64, help='steps per fused launch, and timed steps of the unfused loop')
    ap.add_argument('--reps', type=int, default=4, help='timed fused launches')
    ap.add_argument('--shapes', nargs='+', default=list(SHAPES))
    a = ap.parse_args()
    for name in a.shapes:
        kind, S, mode, E = SHAPES[name]
        for N in a.envs:
            f = fused(kind, N, S, mode, E, a.steps, a.reps)
            u = unfused(kind, N, S, mode, E, a.steps)
            print(json.dumps({'shape': name, 'env': kind, 'size': S, 'mode': mode, 'num_envs': N, 'steps': a.steps,
                              'fused': f, 'unfused': u, 'speedup': f['env_steps_per_s'] / u['env_steps_per_s']}),
                  flush=True)


if __name__ == '__main__':
    main()
