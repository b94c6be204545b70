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

Matchmaking on the device.  `league_plan` in its default form reads the range of the line-up back, and a line-up drawn on
the host cannot depend on `LeagueTable.table` without reading that.  `league_draw(env, A, tickets, replacement, pinned)`
draws a line-up per env from integer tickets held on the device (include/wurm_hip.h: wurm_multi_league_draw; kernel:
wurm_amd/csrc/multi_matchmaking.hpp; the rule restated in tests/league_draw_ref.py) and `league_plan(..., sync=False)`
builds `order` / `offsets` with HIP kernels (wurm_multi_league_plan: a stable counting sort, the torch path's bits): both on
the current stream, neither reads anything on the host.  The draw is keyed by `env.league_draws`, a counter of its own that
a call advances by one; the env's RNG counter and `policy_calls` are not consumed.  An entry outside [0, A) cannot be
refused without a read: its row is in no list, `env.league_dropped` (a device int32 scalar) counts such rows, and `order`
holds -1 behind `offsets[A]`, where no consumer reads.

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
import ctypes
import operator
from collections import namedtuple

import torch

from wurm_amd import _lib
from wurm_amd.envs import _multi_act

# lineup (K, N) as given; order (K N) int32, offsets (A + 1) int64 on lineup's device; num_policies A
LeaguePlan = namedtuple('LeaguePlan', ('lineup', 'order', 'offsets', 'num_policies'))

_INTS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)
_MAX_SEATS = 64  # draw::MAX_SEATS of wurm_amd/csrc/multi_matchmaking.hpp


def block_lineup(num_snakes: int, num_envs: int, num_species: int, device=None) -> torch.Tensor:
    """the line-up `act` plays: lineup[k, :] = k * num_species // num_snakes"""
    rows = torch.tensor([_multi_act.species_of(k, num_snakes, num_species) for k in range(num_snakes)], dtype=torch.long,
                        device=device)
    return rows.unsqueeze(1).expand(num_snakes, num_envs).contiguous()


def _num_policies(num_policies, what) -> int:
    try:
        A = operator.index(num_policies)
    except TypeError:
        raise RuntimeError(f'MultiSnake.{what}: num_policies must be an int, got {type(num_policies).__name__}')
    if not 1 <= A < 2 ** 31:
        raise RuntimeError(f'MultiSnake.{what}: num_policies must lie in [1, 2^31), got {A}')
    return A


def league_plan(env, lineup, num_policies, sync=True) -> LeaguePlan:
    """MultiSnake.league_plan.  sync=True needs of `env` only num_snakes and num_envs; works on CPU tensors as on device
    ones (the plan lives where `lineup` lives).  One host synchronisation: the range check.  sync=False: `_device_plan`."""
    K, N = int(env.num_snakes), int(env.num_envs)
    A = _num_policies(num_policies, 'league_plan')
    if not isinstance(lineup, torch.Tensor):
        raise RuntimeError(f'MultiSnake.league_plan: lineup must be a tensor, got {type(lineup).__name__}')
    if lineup.dtype not in _INTS:
        raise RuntimeError(f'MultiSnake.league_plan: lineup must be an integer tensor, got {lineup.dtype}')
    if tuple(lineup.shape) != (K, N):
        raise RuntimeError(f'MultiSnake.league_plan: lineup has shape {tuple(lineup.shape)}, expected (num_snakes, num_envs) '
                           f'= ({K}, {N})')
    if K * N >= 2 ** 31:
        raise RuntimeError(f'MultiSnake.league_plan: {K} x {N} rows do not fit the int32 row list')
    if not sync:
        return _device_plan(env, lineup, A, 'league_plan')
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


_LINEUP_DTYPES = {torch.int64: _lib.LINEUP_I64, torch.int32: _lib.LINEUP_I32, torch.int16: _lib.LINEUP_I16,
                  torch.int8: _lib.LINEUP_I8, torch.uint8: _lib.LINEUP_U8}


def _on_env_device(env, t, what, name):
    if env.device.type != 'cuda':
        raise RuntimeError(f'MultiSnake.{what}: the env is on {env.device}; the device forms need a HIP device')
    if t is not None and t.device != env.device:
        raise RuntimeError(f'MultiSnake.{what}: {name} is on {t.device}, the env on {env.device}')


def _device_plan(env, lineup, A, what) -> LeaguePlan:
    """`order` / `offsets` of a checked (K, N) line-up by wurm_multi_league_plan: WURM_LEAGUE_PLAN_LAUNCHES launches on
    the current stream and no host read.  An entry outside [0, A) cannot be refused here: its row is left out of every
    list and counted in `env.league_dropped`, a device int32 scalar this call rewrites; `order` keeps its K N entries,
    those behind offsets[A] are -1."""
    _on_env_device(env, lineup, what, 'lineup')
    if not lineup.is_contiguous():
        raise RuntimeError(f'MultiSnake.{what}: lineup must be contiguous')
    dev, rows = env.device, lineup.numel()
    order = torch.empty(rows, dtype=torch.int32, device=dev)
    if getattr(env, 'league_dropped', None) is None:
        env.league_dropped = torch.zeros((), dtype=torch.int32, device=dev)
    if rows == 0:
        env.league_dropped.zero_()
        return LeaguePlan(lineup, order, torch.zeros(A + 1, dtype=torch.long, device=dev), A)
    offsets = torch.empty(A + 1, dtype=torch.long, device=dev)
    nbytes = _lib.lib().wurm_multi_league_plan_workspace_bytes(rows, A)
    # (the caching allocator hands out and takes back a block in the order of the stream it was made on: no synchronisation)
    workspace = torch.empty(nbytes // 8, dtype=torch.long, device=dev)
    c = _lib.LeaguePlanCall(_lib.ptr(lineup), _lib.ptr(order), _lib.ptr(offsets), _lib.ptr(env.league_dropped),
                            _lib.ptr(workspace), nbytes, rows, A, _LINEUP_DTYPES[lineup.dtype], _lib.stream_ptr(dev.index))
    _lib.check(_lib.call(dev.index, _lib.lib().wurm_multi_league_plan, ctypes.addressof(c)), f'MultiSnake.{what}')
    return LeaguePlan(lineup, order, offsets, A)


def _pinned(pinned, K, A, replacement):
    """`pinned` as K ints (None: all -1), checked on the host"""
    if pinned is None:
        return [-1] * K
    try:
        pins = [operator.index(p) for p in pinned]
    except TypeError:
        raise RuntimeError(f'MultiSnake.league_draw: pinned must be a sequence of ints or None, got {pinned!r}')
    if len(pins) != K:
        raise RuntimeError(f'MultiSnake.league_draw: pinned has {len(pins)} entries, expected num_snakes = {K}')
    bad = [p for p in pins if not -1 <= p < A]
    if bad:
        raise RuntimeError(f'MultiSnake.league_draw: pinned entries {bad} lie outside [-1, num_policies = {A})')
    seated = [p for p in pins if p >= 0]
    if not replacement and len(set(seated)) != len(seated):
        raise RuntimeError(f'MultiSnake.league_draw: without replacement no policy may be pinned twice, got {pins}')
    return pins


def league_draw(env, num_policies, tickets=None, replacement=False, pinned=None) -> LeaguePlan:
    """MultiSnake.league_draw: the line-up of every env drawn on the device (wurm_multi_league_draw, one launch) and its
    plan built there (`_device_plan`), on the current stream, without a host read.  Advances `env.league_draws` by one and
    consumes neither the env's RNG counter nor `policy_calls`."""
    K, N = int(env.num_snakes), int(env.num_envs)
    A = _num_policies(num_policies, 'league_draw')
    replacement = bool(replacement)
    if tickets is not None:
        if not isinstance(tickets, torch.Tensor):
            raise RuntimeError(f'MultiSnake.league_draw: tickets must be a tensor or None, got {type(tickets).__name__}')
        if tickets.dtype != torch.int32:
            raise RuntimeError(f'MultiSnake.league_draw: tickets must be int32, got {tickets.dtype}')
        if tuple(tickets.shape) != (A,) or not tickets.is_contiguous():
            raise RuntimeError(f'MultiSnake.league_draw: tickets has shape {tuple(tickets.shape)}, expected a contiguous '
                               f'(num_policies,) = ({A},)')
    pins = _pinned(pinned, K, A, replacement)
    if not replacement and A < K:
        raise RuntimeError(f'MultiSnake.league_draw: without replacement {K} seats need at least as many policies, got {A}')
    if K > _MAX_SEATS:
        raise NotImplementedError(f'MultiSnake.league_draw: at most {_MAX_SEATS} snakes per env, got {K}')
    if K * N >= 2 ** 31:
        raise RuntimeError(f'MultiSnake.league_draw: {K} x {N} rows do not fit the int32 row list')
    _on_env_device(env, tickets, 'league_draw', 'tickets')
    dev = env.device
    lineup = torch.empty((K, N), dtype=torch.long, device=dev)
    host_pins = (ctypes.c_int32 * K)(*pins)
    c = _lib.LeagueDraw(_lib.ptr(tickets), _lib.ptr(lineup), ctypes.addressof(host_pins), N, int(env.env_offset),
                        _lib.u64(env.seed), _lib.u64(env.league_draws), K, A, int(replacement), _lib.stream_ptr(dev.index))
    _lib.check(_lib.call(dev.index, _lib.lib().wurm_multi_league_draw, ctypes.addressof(c)), 'MultiSnake.league_draw')
    env.league_draws += 1
    return _device_plan(env, lineup, A, 'league_draw')


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
