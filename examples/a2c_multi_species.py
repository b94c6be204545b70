"""Multi-agent A2C with a feed-forward policy per species, on this project's HIP paths end to end: the acting loop of the
reference's experiments/multiagent.py:350-378 is `MultiSnake.policy_window` — ONE launch per window where the configuration
is fused ('partial_n' crops with n <= 3: `--observation partial_3`), else `MultiSnake.act_window`, which `--window act`
also selects (two launches per step: one `act` for every snake of every species, one `step` with the postponed reset; same
bits either way, so the two can be run side by side) —, the learners are one `FusedA2CPopulation` with a member per
species (three launches per window), the log columns of multiagent.py:486-505 are kept on the device by
`MultiRolloutStats` (two launches per window; copied to the host only when a line is printed).  `--save-video PATH` records
the first `--video-envs` envs of every `--video-interval`-th window (a .gif or .npy, or an .mp4 where ffmpeg is installed),
as multiagent.py's `--save-video` does: those windows are replayed for the chosen envs after the fact
(`MultiSnake.record_start` / `record_frames`, one launch more per recorded window); the others pay nothing.

    python examples/a2c_multi_species.py --num-envs 512 --n-agents 4 --n-species 2 --total-steps 200000
    python examples/a2c_multi_species.py --total-steps 200000 --save-video snakes.gif --video-envs 4 --video-interval 100
    python examples/a2c_multi_species.py --observation partial_3 --total-steps 200000               # the fused window
    python examples/a2c_multi_species.py --observation partial_3 --window act --total-steps 200000  # the same run, old loop
    python examples/a2c_multi_species.py --num-envs 8 --n-agents 2 --n-species 2 --size 12 --total-steps 640   # tiny

The policy has the four moves of `FeedforwardAgent`; the env runs with boost=False.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.recording import WindowRecorder  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, MultiRolloutStats  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512)
    ap.add_argument('--n-agents', type=int, default=4)
    ap.add_argument('--n-species', type=int, default=2)
    ap.add_argument('--size', type=int, default=25)
    ap.add_argument('--update-steps', type=int, default=20)
    ap.add_argument('--total-steps', type=int, default=200000, help='env steps summed over the batch')
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--gamma', type=float, default=0.99)
    ap.add_argument('--entropy', type=float, default=0.01)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--observation', default='partial_5', help="'partial_n': the crop every agent sees")
    ap.add_argument('--window', choices=('policy', 'act'), default='policy',
                    help='policy: MultiSnake.policy_window (one launch per window where fused); act: MultiSnake.act_window')
    ap.add_argument('--save-video', default=None, metavar='PATH', help='record envs of the windows (.gif / .npy / .mp4)')
    ap.add_argument('--video-envs', type=int, default=4, metavar='K', help='the first K envs are recorded')
    ap.add_argument('--video-interval', type=int, default=1, help='every this many windows one is recorded')
    args = ap.parse_args(argv)
    N, K, P, T = args.num_envs, args.n_agents, args.n_species, args.update_steps
    if K % P:
        raise SystemExit('--n-species must divide --n-agents: a FusedA2CPopulation member owns equally many envs')
    E = 3 * (2 * int(args.observation.split('_')[1]) + 1) ** 2
    torch.manual_seed(args.seed)
    env = MultiSnake(num_envs=N, num_snakes=K, size=args.size, observation_mode=args.observation, device=args.device,
                     boost=False, food_mode='random_rate', respawn_mode='any', seed=args.seed)
    agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(env.device) for _ in range(P)]
    learner = FusedA2CPopulation(agents, lr=args.lr, gamma=args.gamma, entropy_coef=args.entropy)
    stats = MultiRolloutStats(env)
    video = WindowRecorder(env, args.save_video, range(min(args.video_envs, N)), args.video_interval) \
        if args.save_video else None
    run_window = env.policy_window if args.window == 'policy' else env.act_window
    print(f'window: {args.window}' + (f' (fused: {env.policy_window_fused(P)})' if args.window == 'policy' else ''), flush=True)
    state = env.reset()
    steps, window = 0, 0
    while steps < args.total_steps:
        rec = video.start(window) if video else None
        out = run_window(learner.params, state, T, info=True)
        if rec is not None:
            video.finish(rec, out['actions'])
        x0 = torch.stack(list(state.values())).reshape(K * N, E)
        res = learner.update(x0, out)
        stats.update(out)
        state = out['state']
        steps += T * N
        window += 1
        if window % 10 == 1 or steps >= args.total_steps:
            # since the last line: agent 0's columns (smoothed, as the reference prints them) and each species' means
            species = stats.read(reset=False, num_species=P)
            a = stats.read()[0]
            vl = res['value_loss'].tolist()
            print(f'steps {steps:9d} episodes {a["episodes"]:6d} | agent 0: Reward {a["ewm_reward"]:+.2e} Food '
                  f'{a["ewm_food"]:.2e} Entropy {a["ewm_policy_entropy"]:.2e} Done {a["ewm_done"]:.2e} Edge '
                  f'{a["ewm_edge_collisions"]:.2e} Collision {a["ewm_snake_collisions"]:.2e} Size {a["ewm_size"]:.3f} '
                  f'Return {a["ewm_return"]:.3f} | ' + ' | '.join(
                      f'species {s}: reward {r["reward"]:+.4f} done {r["done"]:.4f} size {r["size"]:.3f} life '
                      f'{r["life_length_mean"]:.1f} value loss {vl[s]:.4f} entropy {r["policy_entropy"]:.3f}'
                      for s, r in enumerate(species)), flush=True)
    if video:
        video.close()
    return learner


if __name__ == '__main__':
    main()
