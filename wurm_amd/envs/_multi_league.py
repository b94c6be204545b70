"""MultiSnake.league_plan / act_league / league_window (wurm_amd/envs/multi_snake.py): a LEAGUE of policies in one batch, a
line-up per env — the counterpart of the reference's experiments/eval.py, which draws random matchups of agents out of a
folder of checkpoints and starts one `experiments.multiagent --train False` process per matchup (include/wurm_hip.h:
wurm_multi_act_league; kernel: wurm_amd/csrc/multi_league.hpp).

`act` binds a policy to a snake INDEX: snake k of every env plays row k * num_species // num_snakes of `params`.  Here
`lineup[k, i]` names the row of `params` that plays snake k of env i, so one env object plays N different matchups of K out
of A policies at once.  Everything else is `act`'s: a row is one (snake k, env i) pair, r = k * N + i; its draw comes from
the Philox stream (env_offset + i) * K + k at `env.policy_calls`; the outputs are laid out agent-major.  A row's probs,
value and action depend on its observation, its policy's row of `params`, the seed and the two counters — not on who plays
any other row, nor on how many policies there are.

The plan.  The kernel serves one policy per workgroup (that policy's first layer in LDS), so it wants each policy's rows
as a list: `league_plan` sorts the K N rows by policy once per draw of matchups (a stable sort: rows ascending within a
policy) into `order` (K N) int32 and `offsets` (A + 1) int64.  Both stay on the device and no later call reads them on the
host: the launch is sized from K, N and A alone.

Learning.  `FusedA2CPopulation.update(state, out, plan=plan, learn=None)` (wurm_amd/rl/fused_population.py;
include/wurm_hip.h: wurm_a2c_ff_league_*) takes a `league_window` and its plan: policy a learns from the columns
`order[offsets[a] : offsets[a + 1]]`, however many, in the three launches of one update, bit for bit as a
`FusedA2CLearner` would from copies of those columns.  `learn` masks policies out (a pool of frozen checkpoints); they and
policies without rows keep their weights and Adam state.

What is not here.  `policy_window` is not fused for line-ups (`league_window` makes two launches per step, like
`act_window`).  The learner's `step` is shared by the policies: one that sat windows out is stepped with the bias
corrections of the shared count.  Both the acting and the learning grid are sized by A, not by rows per policy, so a skewed
line-up leaves workgroups idle while the largest policy's work.
"""
import operator
from collections import namedtuple

import torch

from wurm_amd import _lib
from wurm_amd.envs import _multi_act

# lineup (K, N) as given; order (K N) int32, offsets (A + 1) int64 on lineup's device; num_policies A
LeaguePlan = namedtuple('LeaguePlan', ('lineup', 'order', 'offsets', 'num_policies'))

_INTS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def block_lineup(num_snakes: int, num_envs: int, num_species: int, device=None) -> torch.Tensor:
    """the line-up `act` plays: lineup[k, :] = k * num_species // num_snakes"""
    rows = torch.tensor([_multi_act.species_of(k, num_snakes, num_species) for k in range(num_snakes)], dtype=torch.long,
                        device=device)
    return rows.unsqueeze(1).expand(num_snakes, num_envs).contiguous()


def league_plan(env, lineup, num_policies) -> LeaguePlan:
    """MultiSnake.league_plan.  Needs of `env` only num_snakes and num_envs; works on CPU tensors as on device ones (the
    plan lives where `lineup` lives).  One host synchronisation: the range check."""
    K, N = int(env.num_snakes), int(env.num_envs)
    try:
        A = operator.index(num_policies)
    except TypeError:
        raise RuntimeError(f'MultiSnake.league_plan: num_policies must be an int, got {type(num_policies).__name__}')
    if not 1 <= A < 2 ** 31:
        raise RuntimeError(f'MultiSnake.league_plan: num_policies must lie in [1, 2^31), got {A}')
    if not isinstance(lineup, torch.Tensor):
        raise RuntimeError(f'MultiSnake.league_plan: lineup must be a tensor, got {type(lineup).__name__}')
    if lineup.dtype not in _INTS:
        raise RuntimeError(f'MultiSnake.league_plan: lineup must be an integer tensor, got {lineup.dtype}')
    if tuple(lineup.shape) != (K, N):
        raise RuntimeError(f'MultiSnake.league_plan: lineup has shape {tuple(lineup.shape)}, expected (num_snakes, num_envs) '
                           f'= ({K}, {N})')
    if K * N >= 2 ** 31:
        raise RuntimeError(f'MultiSnake.league_plan: {K} x {N} rows do not fit the int32 row list')
    flat = lineup.reshape(-1).to(torch.long)
    if K * N:
        lo, hi = torch.stack(torch.aminmax(flat)).tolist()  # (the one synchronisation)
        if lo < 0 or hi >= A:
            raise RuntimeError(f'MultiSnake.league_plan: lineup has entries in [{lo}, {hi}], outside [0, num_policies = {A})')
    order = torch.sort(flat, stable=True).indices.to(torch.int32)
    counts = torch.bincount(flat, minlength=A)
    offsets = torch.zeros(A + 1, dtype=torch.long, device=lineup.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    return LeaguePlan(lineup, order, offsets, A)


def _checked(env, plan, rows, N, what) -> int:
    """the plan against the env, a batch of N envs and params of `rows` rows: its number of policies"""
    if not isinstance(plan, LeaguePlan):
        raise RuntimeError(f'MultiSnake.{what}: plan must come from league_plan, got {type(plan).__name__}')
    K, A = env.num_snakes, plan.num_policies
    if tuple(plan.lineup.shape) != (K, N):
        raise RuntimeError(f'MultiSnake.{what}: the plan is for a line-up of shape {tuple(plan.lineup.shape)}, the '
                           f'observations for ({K}, {N})')
    if plan.order.device != env.device:
        raise RuntimeError(f'MultiSnake.{what}: the plan is on {plan.order.device}, the env on {env.device}')
    if A > rows:
        raise RuntimeError(f'MultiSnake.{what}: the plan names {A} policies but params has {rows} rows')
    return A


def act_league(env, params, observations, plan, out=None) -> dict:
    """MultiSnake.act_league.  out: as for `_multi_act.act`."""
    E = _multi_act._num_inputs(env)
    rows = _multi_act._param_rows(env, params, E)  # (as `act` checks them: type, dtype, shape, layout, device)
    obs, N = _multi_act._observations(env, observations, E)
    A = _checked(env, plan, rows, N, 'act_league')
    K, dev = env.num_snakes, env.device
    actions, probs, values = _multi_act._outputs(env, N, out)
    ptr = _lib.ptr
    rc = _lib.call(dev.index, _lib.lib().wurm_multi_act_league, ptr(params), ptr(obs), ptr(plan.order), ptr(plan.offsets),
                   ptr(actions), ptr(probs), ptr(values), _lib.i64(N), K, A, E, _lib.u64(env.seed),
                   _lib.u64(env.policy_calls), _lib.i64(env.env_offset), _lib.stream_ptr(dev.index))
    _lib.check(rc, 'MultiSnake.act_league')
    return _multi_act._acted(env, actions, probs, values)


def league_window(env, params, state, num_steps, plan, info=False) -> dict:
    """MultiSnake.league_window: `_multi_act.act_window` with `act_league` as its acting call"""
    if int(num_steps) == 0:  # (no acting call will look at them)
        rows = _multi_act._param_rows(env, params, _multi_act._num_inputs(env))
        _checked(env, plan, rows, env.num_envs, 'league_window')
    return _multi_act.act_window(env, params, state, num_steps, info=info,
                                 acting=lambda state, out: act_league(env, params, state, plan, out))
