"""A league evaluation in ONE env object: the counterpart of the reference's experiments/eval.py, which draws `--n-rounds`
random matchups of `--n-agents` agents out of a folder of checkpoints and starts one `experiments.multiagent --train False`
process per matchup.  Here every env of a MultiSnake batch gets a line-up of its own — `--n-agents` of the `--n-policies`
policies, drawn at random, with or without replacement within an env — and all of them play at once:
`MultiSnake.league_plan` sorts the (snake, env) rows by policy once, `MultiSnake.league_window` acts for every row with the
policy its line-up names (one launch) and steps (one launch), and `wurm_amd.rl.LeagueTable` adds every policy's results on
the device (one launch per window; copied to the host once, at the end).  `--device-draw` draws and sorts the line-ups
on the device (`MultiSnake.league_draw`: no host read, other line-ups than the host draw's).  `--save-video PATH` replays
the first `--video-envs` envs of every `--video-interval`-th window after the fact (`record_start` / `record_frames`).

    python examples/league_eval.py --n-policies 16 --n-agents 4 --num-envs 512 --total-steps 200000
    python examples/league_eval.py --params population.pt --n-agents 2 --with-replacement
    python examples/league_eval.py --n-policies 5 --n-agents 2 --num-envs 8 --size 12 --total-steps 640 --save-video league.gif

`--params FILE` is a torch file holding an (A, num_params) tensor, or a dict with one under 'params' — what
`FusedA2CPopulation.state_dict()` gives; without it the policies are freshly initialised `FeedforwardAgent`s (a league of
equals: the table then shows the spread of the game, not of skill).  `--redraw K` draws new line-ups every K windows.
The policy has the four moves of `FeedforwardAgent`; the env runs with boost=False.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wurm_amd.agents import FeedforwardAgent, pack_policy_params  # noqa: E402
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.recording import WindowRecorder  # noqa: E402
from wurm_amd.rl import LeagueTable  # noqa: E402


def draw_lineup(num_policies, num_agents, num_envs, with_replacement, generator):
    """(num_agents, num_envs) int64 on the CPU: per env `num_agents` policies out of `num_policies`, uniformly at random"""
    if with_replacement:
        return torch.randint(num_policies, (num_agents, num_envs), generator=generator)
    if num_agents > num_policies:
        raise SystemExit(f'{num_agents} agents per env out of {num_policies} policies needs --with-replacement')
    keys = torch.rand((num_envs, num_policies), generator=generator)      # a random permutation per env: its first K
    return keys.argsort(dim=1)[:, :num_agents].t().contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512)
    ap.add_argument('--n-agents', type=int, default=4, help='snakes per env')
    ap.add_argument('--n-policies', type=int, default=16, help='fresh policies (ignored with --params)')
    ap.add_argument('--params', default=None, metavar='FILE', help="torch file: (A, num_params) tensor, or a dict with 'params'")
    ap.add_argument('--with-replacement', action='store_true', help='a policy may play several snakes of one env')
    ap.add_argument('--size', type=int, default=25)
    ap.add_argument('--window-steps', type=int, default=20)
    ap.add_argument('--total-steps', type=int, default=200000, help='env steps summed over the batch')
    ap.add_argument('--redraw', type=int, default=0, metavar='K', help='new line-ups every K windows (0: one draw)')
    ap.add_argument('--device-draw', action='store_true', help='draw and sort the line-ups on the device (league_draw)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--observation', default='partial_5', help="'partial_n': the crop every agent sees")
    ap.add_argument('--save-video', default=None, metavar='PATH', help='record envs of the windows (.gif / .npy / .mp4)')
    ap.add_argument('--video-envs', type=int, default=4, metavar='K', help='the first K envs are recorded')
    ap.add_argument('--video-interval', type=int, default=1, help='every this many windows one is recorded')
    args = ap.parse_args(argv)
    N, K, T = args.num_envs, args.n_agents, args.window_steps
    E = 3 * (2 * int(args.observation.split('_')[1]) + 1) ** 2
    torch.manual_seed(args.seed)
    env = MultiSnake(num_envs=N, num_snakes=K, size=args.size, observation_mode=args.observation, device=args.device,
                     boost=False, food_mode='random_rate', respawn_mode='any', seed=args.seed)
    if args.params:
        params = torch.load(args.params, map_location='cpu')
        params = (params['params'] if isinstance(params, dict) else params).to(env.device, torch.float32).contiguous()
    else:
        params = torch.stack([pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E))
                              for _ in range(args.n_policies)]).to(env.device)
    A = params.shape[0]
    table = LeagueTable(A, env.device)
    video = WindowRecorder(env, args.save_video, range(min(args.video_envs, N)), args.video_interval) \
        if args.save_video else None
    g = torch.Generator().manual_seed(args.seed)

    def draw():
        if args.device_draw:
            if not args.with_replacement and K > A:
                raise SystemExit(f'{K} agents per env out of {A} policies needs --with-replacement')
            return env.league_draw(A, replacement=args.with_replacement)
        return env.league_plan(draw_lineup(A, K, N, args.with_replacement, g).to(env.device), A)

    plan = draw()
    state = env.reset()
    steps, window = 0, 0
    while steps < args.total_steps:
        if args.redraw and window and window % args.redraw == 0:
            plan = draw()
        rec = video.start(window) if video else None
        out = env.league_window(params, state, T, plan, info=True)
        if rec is not None:
            video.finish(rec, out['actions'])
        table.update(plan, out)
        state = out['state']
        steps += T * N
        window += 1
    if video:
        video.close()
    rows = table.read()
    print(f'{A} policies, {K} per env, {N} envs, {steps} env steps in {window} windows'
          + (', with replacement' if args.with_replacement else ''))
    print('policy  row-steps   deaths  reward/step   food/step   size  life length  reward/life  edge/step  snake/step')
    for a in sorted(range(A), key=lambda a: -(rows[a]['reward_per_step'] if rows[a]['steps'] else float('-inf'))):
        r = rows[a]
        print(f'{a:6d} {int(r["steps"]):10d} {int(r["deaths"]):8d} {r["reward_per_step"]:+12.5f} {r["food_per_step"]:11.5f} '
              f'{r["size_mean"]:6.2f} {r["life_length_mean"]:12.1f} {r["reward_per_life"]:+12.3f} '
              f'{r["edge_collisions_per_step"]:10.5f} {r["snake_collisions_per_step"]:11.5f}')
    return rows


if __name__ == '__main__':
    main()
