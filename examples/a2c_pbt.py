#!/usr/bin/env python3
"""examples/a2c_population.py with POPULATION-BASED TRAINING: the P members start as a sweep over learning rates, and every
`--pbt-interval` windows the worst `--pbt-fraction` of them, by smoothed reward rate, take over the weights, the Adam state
and the hyper-parameters of members drawn from the best, with the copied lr and entropy_coef multiplied by 0.8 or 1.2
(`FusedA2CPopulation.exploit`: two launches).  The score is a column of `RolloutStats(env, population=P).smooth`, which is
already on the device, so nothing is read back to decide who copies whom; the only host copies are made per log line,
which prints every member's CURRENT lr / entropy_coef (`hyperparameters()`) beside its log columns.  `--save-video PATH`
records the first env of each of the first `--video-envs` members in every `--video-interval`-th window, side by side
(`env.record_start` / `env.record_frames`: a replay after the fact; without the option nothing of it runs).

    python examples/a2c_pbt.py --num-envs 512 --steps 20000 --lrs 1e-4 3e-4 1e-3 3e-3 --pbt-interval 50
    python examples/a2c_pbt.py --steps 20000 --save-video members.gif --video-interval 100
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402
from wurm_amd.recording import WindowRecorder  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, RolloutStats  # noqa: E402
from wurm_amd.rl.rollout_stats import COLUMNS  # noqa: E402


def run(num_envs=512, size=9, observation='partial_2', steps=20000, update_steps=5, gamma=0.99,
        lrs=(1e-4, 3e-4, 1e-3, 3e-3), entropy=0.01, pbt_interval=50, pbt_fraction=0.25, log_interval=2000, seed=0,
        device='cuda', verbose=True, gae_lambda=None, save_video=None, video_envs=None, video_interval=1):
    """num_envs: per member; pbt_interval: windows between two exploits.  Returns one list of log rows per member."""
    P = len(lrs)
    env = SingleSnake(num_envs=P * num_envs, size=size, observation_mode=observation, device=device, seed=seed)
    state = env.reset()
    models = []
    for p in range(P):
        torch.manual_seed(seed + p)
        models.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=state[0].numel()).to(device))
    pop = FusedA2CPopulation(models, lr=list(lrs), gamma=gamma, entropy_coef=entropy, max_grad_norm=0.5,
                             use_gae=gae_lambda is not None, gae_lambda=gae_lambda)
    stats = RolloutStats(env, population=P)
    score_column = COLUMNS.index('reward_rate')
    history, t0, replaced = [[] for _ in range(P)], time.perf_counter(), torch.zeros(P, dtype=torch.int32, device=device)
    # the first env of each member (of the first `video_envs` members): indices are the env object's, whatever the population
    watched = [p * num_envs for p in range(P if video_envs is None else min(video_envs, P))]
    video = WindowRecorder(env, save_video, watched, video_interval) if save_video else None
    for window, i_step in enumerate(range(update_steps, steps + 1, update_steps), start=1):
        rec = video.start(window - 1) if video else None
        out = env.policy_rollout(pop.params, state, update_steps, check=False, population=P)
        if rec is not None:
            video.finish(rec, out['actions'])
        res = pop.update(state, out)
        state = out['state']
        stats.update(out)
        if window % pbt_interval == 0:
            # the members' smoothed reward rates never leave the device (a view of the smoother's table is copied by
            # `exploit` into a contiguous vector); neither does who was replaced
            chosen = pop.exploit(stats.smooth[:, score_column], fraction=pbt_fraction, seed=seed)
            replaced += chosen['parent'] != torch.arange(P, dtype=torch.int32, device=device)
        if i_step % log_interval < update_steps or i_step + update_steps > steps:
            dt = time.perf_counter() - t0
            hyper, times = pop.hyperparameters(), replaced.cpu().tolist()                   # one copy each per log line
            # (the loss with each member's own, current entropy_coef)
            loss = (res['value_loss'] + res['policy_loss'] - pop.hyper[:, 2].float() * res['entropy']).cpu().tolist()
            for p, member in enumerate(stats.read()):
                row = dict(member=p, lr=hyper['lr'][p], entropy_coef=hyper['entropy_coef'][p], replaced=times[p],
                           step=i_step, env_steps_per_s=i_step * P * num_envs / dt, loss=loss[p])
                row.update((k, v) for k, v in member.items() if v == v)
                history[p].append(row)
                if verbose:
                    print(' '.join(f'{k}={v:.4g}' for k, v in row.items()))
    if video:
        video.close()
    return history


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512, help='envs per member')
    ap.add_argument('--size', type=int, default=9)
    ap.add_argument('--observation', default='partial_2')
    ap.add_argument('--steps', type=int, default=20000)
    ap.add_argument('--update-steps', type=int, default=5)
    ap.add_argument('--lrs', type=float, nargs='+', default=[1e-4, 3e-4, 1e-3, 3e-3], help='one member per learning rate')
    ap.add_argument('--entropy', type=float, default=0.01)
    ap.add_argument('--pbt-interval', type=int, default=50, help='windows between two exploit steps')
    ap.add_argument('--pbt-fraction', type=float, default=0.25, help='the share of members replaced per exploit step')
    ap.add_argument('--gae-lambda', type=float, default=None, help='GAE with this lambda instead of n-step returns')
    ap.add_argument('--save-video', default=None, metavar='PATH', help='record envs of the fused windows (.gif / .npy / .mp4)')
    ap.add_argument('--video-envs', type=int, default=None, metavar='K', help='the first env of each of the first K members (default: all)')
    ap.add_argument('--video-interval', type=int, default=1, help='every this many windows one is recorded')
    args = ap.parse_args()
    run(args.num_envs, args.size, args.observation, args.steps, args.update_steps, lrs=args.lrs, entropy=args.entropy,
        pbt_interval=args.pbt_interval, pbt_fraction=args.pbt_fraction, gae_lambda=args.gae_lambda,
        save_video=args.save_video, video_envs=args.video_envs, video_interval=args.video_interval)
