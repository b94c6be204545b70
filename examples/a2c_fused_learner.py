#!/usr/bin/env python3
"""The single-agent A2C experiment of the reference (experiments/main.py:194-247) with BOTH halves in HIP: the acting
half is `env.policy_rollout(learner.params, state, update_steps)` (policy -> sample -> step -> reset inside the env
kernel, as in examples/a2c_fused_actor.py), the learning half is `learner.update(state, out)`: forward, return scan, loss,
backward pass, clip_grad_norm_ and Adam in three launches (wurm_amd.rl.FusedA2CLearner).  Per update the host issues four
kernel launches and reads nothing back; the loss is copied to the host only for a log line.  `--gae-lambda` switches the
returns from n-step to generalised advantage estimation (the reference's `--gae-lambda`), still in the same launches.
The log line has the reference's columns (main.py:252-316: episodes, reward_rate, policy_entropy, edge_collisions,
self_collisions, avg_size and their smoothed `ewm_` versions) and the mean and maximum return, length and final snake
size of the episodes that ended since the last line: `wurm_amd.rl.RolloutStats` keeps them on the device, two more
launches per window, and is read once per line.  `--save-video PATH` records the first `--video-envs` envs of every
`--video-interval`-th window (a .gif or .npy, or an .mp4 where ffmpeg is installed): those windows are replayed for the
chosen envs after the fact (`env.record_start` / `env.record_frames`), the training launches are the same either way, and
without the option nothing of it runs.

    python examples/a2c_fused_learner.py --num-envs 512 --steps 20000
    python examples/a2c_fused_learner.py --num-envs 512 --steps 20000 --gae-lambda 0.95
    python examples/a2c_fused_learner.py --steps 20000 --save-video snake.gif --video-envs 4 --video-interval 100
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
from wurm_amd.rl import FusedA2CLearner, RolloutStats  # noqa: E402


def run(num_envs=512, size=9, observation='partial_2', steps=20000, update_steps=5, gamma=0.99, lr=1e-3, entropy=0.01,
        log_interval=2000, seed=0, device='cuda', verbose=True, gae_lambda=None, save_video=None, video_envs=4,
        video_interval=1):
    torch.manual_seed(seed)
    env = SingleSnake(num_envs=num_envs, size=size, observation_mode=observation, device=device, seed=seed)
    state = env.reset()                                                     # main.py:195
    model = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=state[0].numel()).to(device)
    learner = FusedA2CLearner(model, lr=lr, gamma=gamma, entropy_coef=entropy, max_grad_norm=0.5,
                              use_gae=gae_lambda is not None, gae_lambda=gae_lambda)        # multiagent.py:274-275
    stats = RolloutStats(env)                                               # :252-274, on the device
    video = WindowRecorder(env, save_video, range(min(video_envs, num_envs)), video_interval) if save_video else None
    history, t0 = [], time.perf_counter()
    for window, i_step in enumerate(range(update_steps, steps + 1, update_steps)):
        rec = video.start(window) if video else None                                            # :184-186, 201-202
        out = env.policy_rollout(learner.params, state, update_steps, check=False)              # :207-227, fused
        if rec is not None:
            video.finish(rec, out['actions'])
        res = learner.update(state, out)                                                         # :229-245, fused
        state = out['state']
        stats.update(out)
        if i_step % log_interval < update_steps or i_step + update_steps > steps:
            dt = time.perf_counter() - t0
            loss = res['value_loss'] + res['policy_loss'] - entropy * res['entropy']             # :239-242
            row = dict(step=i_step, env_steps_per_s=i_step * num_envs / dt, loss=float(loss))
            # since the last line (the episode columns are left out of a line before which no episode ended)
            row.update((k, v) for k, v in stats.read().items() if v == v)
            history.append(row)
            if verbose:
                print(' '.join(f'{k}={v:.4g}' for k, v in row.items()))
    if video:
        video.close()
    return history


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512)
    ap.add_argument('--size', type=int, default=9)
    ap.add_argument('--observation', default='partial_2')
    ap.add_argument('--steps', type=int, default=20000)
    ap.add_argument('--update-steps', type=int, default=5)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--gae-lambda', type=float, default=None, help='GAE with this lambda instead of n-step returns')
    ap.add_argument('--save-video', default=None, metavar='PATH', help='record envs of the fused windows (.gif / .npy / .mp4)')
    ap.add_argument('--video-envs', type=int, default=4, metavar='K', help='the first K envs are recorded')
    ap.add_argument('--video-interval', type=int, default=1, help='every this many windows one is recorded')
    args = ap.parse_args()
    run(args.num_envs, args.size, args.observation, args.steps, args.update_steps, lr=args.lr,
        gae_lambda=args.gae_lambda, save_video=args.save_video, video_envs=args.video_envs,
        video_interval=args.video_interval)
