"""Self-play in a league: A policies play each other in ONE MultiSnake batch, every env with a line-up of its own, and the
SAME object that plays them trains them — `FusedA2CPopulation.update(state, out, plan=plan)` gives every policy the
columns its line-up put it in, however many, in three launches (include/wurm_hip.h: wurm_a2c_ff_league_update).

    A policies = FusedA2CPopulation
    per window:  league_window -> pop.update(state, out, plan=plan, learn=...) -> LeagueTable.update

Every `--redraw` windows the line-ups are drawn again (`league_plan`: the only call of the loop that has to synchronise;
the progress line every 50 windows reads the losses back; with `--device-draw` the line-ups are drawn and sorted on the
device by `league_draw`, and the loop queues without a host read) and, with
`--exploit`, population-based training takes its step on the scores of the windows since the last draw,
`reward / steps` out of `LeagueTable.table` on the device: the worst policies become perturbed copies of the best.
`--learners L` trains only the first L policies; the others stay as they are, a pool of frozen checkpoints the learners
meet (they still play and are still scored).  `step` is shared by the policies.

    python examples/league_selfplay.py --n-policies 8 --n-agents 4 --num-envs 512 --total-steps 2000000
    python examples/league_selfplay.py --n-policies 16 --learners 4 --params pool.pt --redraw 50
    python examples/league_selfplay.py --n-policies 4 --n-agents 2 --num-envs 8 --size 12 --total-steps 1600 --exploit
    python examples/league_selfplay.py --n-policies 8 --device-draw --matchmaking prioritised --redraw 5
    python examples/league_selfplay.py --n-policies 16 --learners 4 --device-draw --pin-learners

`--device-draw` draws with `MultiSnake.league_draw`.  `--matchmaking prioritised` (with it) meets strong opponents more
often: at every redraw the policies are ranked by reward per row-step out of `LeagueTable.table`, with torch ops on the
device, and the policy of rank r (0 = best) holds A - r tickets; `uniform` gives every policy one.  `--pin-learners` (with
it) seats the first L policies as snake 0 in turn, one per draw, and draws the other seats from the pool.

`--params FILE` as for examples/league_eval.py; `--save FILE` writes `pop.state_dict()` at the end.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.league_eval import draw_lineup  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import MultiSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation, LeagueTable  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-envs', type=int, default=512)
    ap.add_argument('--n-agents', type=int, default=4, help='snakes per env')
    ap.add_argument('--n-policies', type=int, default=8)
    ap.add_argument('--learners', type=int, default=None, metavar='L',
                    help='only the first L policies learn; the rest are a frozen pool (default: all learn)')
    ap.add_argument('--params', default=None, metavar='FILE', help="torch file: (A, num_params) tensor, or a dict with 'params'")
    ap.add_argument('--with-replacement', action='store_true', help='a policy may play several snakes of one env')
    ap.add_argument('--size', type=int, default=25)
    ap.add_argument('--window-steps', type=int, default=20)
    ap.add_argument('--total-steps', type=int, default=2000000, help='env steps summed over the batch')
    ap.add_argument('--redraw', type=int, default=25, metavar='K', help='new line-ups every K windows')
    ap.add_argument('--device-draw', action='store_true', help='draw and sort the line-ups on the device (league_draw)')
    ap.add_argument('--matchmaking', choices=('uniform', 'prioritised'), default='uniform',
                    help='prioritised (needs --device-draw): tickets by rank of reward per step in the table')
    ap.add_argument('--pin-learners', action='store_true',
                    help='(needs --device-draw) the first L policies take seat 0 in turn, the rest are drawn')
    ap.add_argument('--exploit', action='store_true', help='a PBT step (FusedA2CPopulation.exploit) at every redraw')
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--gamma', type=float, default=0.99)
    ap.add_argument('--entropy', type=float, default=0.01)
    ap.add_argument('--gae-lambda', type=float, default=None, help='generalised advantage estimation with this lambda')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--observation', default='partial_5', help="'partial_n': the crop every agent sees")
    ap.add_argument('--save', default=None, metavar='FILE', help='write the population state_dict here at the end')
    args = ap.parse_args(argv)
    N, K, T, A = args.num_envs, args.n_agents, args.window_steps, args.n_policies
    E = 3 * (2 * int(args.observation.split('_')[1]) + 1) ** 2
    L = A if args.learners is None else args.learners
    if not 1 <= L <= A:
        raise SystemExit(f'--learners must lie in [1, {A}]')
    if args.exploit and L < A:
        raise SystemExit('--exploit replaces the worst policies, frozen ones included: use it without --learners')
    if (args.matchmaking != 'uniform' or args.pin_learners) and not args.device_draw:
        raise SystemExit('--matchmaking prioritised and --pin-learners draw on the device: add --device-draw')
    torch.manual_seed(args.seed)
    env = MultiSnake(num_envs=N, num_snakes=K, size=args.size, observation_mode=args.observation, device=args.device,
                     boost=False, food_mode='random_rate', respawn_mode='any', seed=args.seed)
    agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(env.device) for _ in range(A)]
    pop = FusedA2CPopulation(agents, lr=args.lr, gamma=args.gamma, entropy_coef=args.entropy,
                             use_gae=args.gae_lambda is not None, gae_lambda=args.gae_lambda)
    if args.params:
        params = torch.load(args.params, map_location='cpu')
        params = params['params'] if isinstance(params, dict) else params
        pop.params.copy_(params.to(env.device, torch.float32))
    learn = None if L == A else (torch.arange(A, device=env.device) < L)   # a device mask, made once
    table = LeagueTable(A, env.device)
    g = torch.Generator().manual_seed(args.seed)

    def tickets():
        """None (one ticket each), or A - rank by reward per row-step since the last draw: torch ops on the device, no
        host read.  A policy that did not play (0 / 0 = NaN) ranks last; before the first window all do, in index order."""
        if args.matchmaking == 'uniform':
            return None
        score = torch.nan_to_num(table.table[:, 1] / table.table[:, 0], nan=float('-inf'))
        best_first = torch.argsort(score, descending=True, stable=True)
        held = torch.empty(A, dtype=torch.int32, device=env.device)
        held[best_first] = torch.arange(A, 0, -1, dtype=torch.int32, device=env.device)
        return held

    def draw(held=None):
        if not args.device_draw:
            return env.league_plan(draw_lineup(A, K, N, args.with_replacement, g).to(env.device), A)
        pinned = [env.league_draws % L] + [-1] * (K - 1) if args.pin_learners else None
        return env.league_draw(A, tickets=held, replacement=args.with_replacement, pinned=pinned)

    plan = draw(tickets())
    state = env.reset()
    steps, window = 0, 0
    while steps < args.total_steps:
        if window and window % args.redraw == 0:
            held = tickets()   # (from the table as it stands, before --exploit clears it)
            if args.exploit:   # reward per row-step since the last draw; a policy that did not play (0 / 0 = NaN) is worst
                pop.exploit(table.table[:, 1] / table.table[:, 0], seed=args.seed)
                table.reset()
            plan = draw(held)
        out = env.league_window(pop.params, state, T, plan, info=True)
        res = pop.update(state, out, plan=plan, learn=learn)
        table.update(plan, out)
        state = out['state']
        steps += T * N
        window += 1
        if window % 50 == 0:
            loss = (res['value_loss'] + res['policy_loss']).tolist()
            print(f'window {window}, {steps} env steps: loss per policy ' + ' '.join(f'{x:+.3f}' for x in loss))
    rows = table.read()
    print(f'{A} policies ({L} learning), {K} per env, {N} envs, {steps} env steps in {window} windows, {pop.step} updates')
    print('policy  learns  row-steps  reward/step   food/step   size  life length')
    for a in sorted(range(A), key=lambda a: -(rows[a]['reward_per_step'] if rows[a]['steps'] else float('-inf'))):
        r = rows[a]
        print(f'{a:6d} {"yes" if a < L else "no":>7} {int(r["steps"]):10d} {r["reward_per_step"]:+12.5f} '
              f'{r["food_per_step"]:11.5f} {r["size_mean"]:6.2f} {r["life_length_mean"]:12.1f}')
    if args.save:
        torch.save(pop.state_dict(), args.save)
    return rows


if __name__ == '__main__':
    main()
