#!/usr/bin/env python3
"""examples/a2c_fused_learner.py for a POPULATION: P independent agents — a sweep over learning rates here, the normal use
of the reference's experiments/main.py (`--r`, `--lr`, `--gamma`, `--entropy`) — in ONE env object of P x num_envs envs.
Member p owns the envs [p num_envs, (p + 1) num_envs), its own weights, Adam state and hyper-parameters; per window the
host issues one rollout launch (`env.policy_rollout(pop.params, state, T, population=P)`) and the three learner launches of
`FusedA2CPopulation.update` for all members together.  Each member computes, bit for bit, what its own run of
a2c_fused_learner.py (the same seed, `env_offset` = p num_envs) computes.  The P losses are read back once per log line,
and so are every member's log columns (`wurm_amd.rl.RolloutStats(env, population=P)`: the reference's columns and the
return, length and final size of the episodes that ended, per member, two more launches per window).

    python examples/a2c_population.py --num-envs 512 --steps 20000 --lrs 3e-4 1e-3 3e-3 1e-2
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, RolloutStats  # noqa: E402


def run(num_envs=512, size=9, observation='partial_2', steps=20000, update_steps=5, gamma=0.99, lrs=(3e-4, 1e-3, 3e-3),
        entropy=0.01, log_interval=2000, seed=0, device='cuda', verbose=True, gae_lambda=None):
    """num_envs: per member.  Returns one list of log rows per member."""
    P = len(lrs)
    env = SingleSnake(num_envs=P * num_envs, size=size, observation_mode=observation, device=device, seed=seed)
    state = env.reset()
    models = []
    for p in range(P):
        torch.manual_seed(seed + p)
        models.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=state[0].numel()).to(device))
    pop = FusedA2CPopulation(models, lr=list(lrs), gamma=gamma, entropy_coef=entropy, max_grad_norm=0.5,
                             use_gae=gae_lambda is not None, gae_lambda=gae_lambda)
    stats = RolloutStats(env, population=P)                               # every member's log columns, on the device
    history, t0 = [[] for _ in range(P)], time.perf_counter()
    for i_step in range(update_steps, steps + 1, update_steps):
        out = env.policy_rollout(pop.params, state, update_steps, check=False, population=P)
        res = pop.update(state, out)
        state = out['state']
        stats.update(out)
        if i_step % log_interval < update_steps or i_step + update_steps > steps:
            dt = time.perf_counter() - t0
            loss = (res['value_loss'] + res['policy_loss'] - entropy * res['entropy']).cpu().tolist()  # one copy for all P
            for p, member in enumerate(stats.read()):                                                  # and one for these
                row = dict(member=p, lr=lrs[p], step=i_step, env_steps_per_s=i_step * P * num_envs / dt, loss=loss[p])
                # since the last line (the episode columns are left out of a line before which no episode ended)
                row.update((k, v) for k, v in member.items() if v == v)
                history[p].append(row)
                if verbose:
                    print(' '.join(f'{k}={v:.4g}' for k, v in row.items()))
    return history


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512, help='envs per member')
    ap.add_argument('--size', type=int, default=9)
    ap.add_argument('--observation', default='partial_2')
    ap.add_argument('--steps', type=int, default=20000)
    ap.add_argument('--update-steps', type=int, default=5)
    ap.add_argument('--lrs', type=float, nargs='+', default=[3e-4, 1e-3, 3e-3], help='one member per learning rate')
    ap.add_argument('--gae-lambda', type=float, default=None, help='GAE with this lambda instead of n-step returns')
    args = ap.parse_args()
    run(args.num_envs, args.size, args.observation, args.steps, args.update_steps, lrs=args.lrs,
        gae_lambda=args.gae_lambda)
