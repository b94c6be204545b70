"""MultiSnake.act / MultiSnake.act_window (wurm_amd/envs/multi_snake.py): the acting half of the reference's multi-agent loop
(experiments/multiagent.py:350-378) — per agent a torch forward, a `Categorical`, a sample and a few clones — as ONE launch
for every snake and every species (include/wurm_hip.h: wurm_multi_act; kernel: wurm_amd/csrc/multi_act.hpp).

Layout.  A row is one (snake k, env i) pair.  Agent-major, as `step` lays its outputs out: row / column k * N + i.  Snake k
belongs to species `species_of(k, K, P)` = k * P // K (multiagent.py:356), so a species owns consecutive snakes and, in the
(T, K N, ...) tensors of `act_window`, a consecutive block of columns; when P divides K the blocks are equal and the window
is the member layout `FusedA2CPopulation.update` expects, one member per species.  The sampling uniform of a row comes
from the Philox stream of `env_id_of(i, k, K, env_offset)` = (env_offset + i) * K + k at the env's POLICY call counter
(`env.policy_calls`), which `act` advances by one; the env's own RNG counter is not touched, so a reset postponed behind a
step stays postponed across an `act` and the env's trajectory for given actions does not depend on who chose them.

What is not here: the 8-action boost head (the shared policy spec and `FeedforwardAgent` have 4 actions: with `boost=True`
the policy never boosts) and the reference's ConvAgent / GRUAgent.  The window fused into ONE launch with the env kernel is
`MultiSnake.policy_window` (wurm_amd/envs/_multi_policy_window.py), which returns what `act_window` returns, bit for bit;
`act_window` is its yardstick and what it runs for the configurations it does not fuse.
"""
import torch

from wurm_amd import _lib

MAX_OBS_N = 6  # 'partial_n' crops the kernel serves: E = 3 (2n+1)^2 <= 507


def species_of(k: int, num_snakes: int, num_species: int) -> int:
    """the species of snake k (experiments/multiagent.py:356: integer division)"""
    return k * num_species // num_snakes


def env_id_of(i: int, k: int, num_snakes: int, env_offset: int = 0) -> int:
    """the Philox stream of snake k of env i: every agent of every env of a sharded batch has its own"""
    return (env_offset + i) * num_snakes + k


def column_of(k: int, i: int, num_envs: int) -> int:
    """the column of snake k of env i in the (T, K N, ...) tensors of act_window, and the row of the kernel"""
    return k * num_envs + i


def species_columns(s: int, num_snakes: int, num_envs: int, num_species: int) -> range:
    """the consecutive block of columns species s owns"""
    first = -(-s * num_snakes // num_species)
    end = -(-(s + 1) * num_snakes // num_species)
    return range(first * num_envs, end * num_envs)


def num_policy_params(num_inputs: int) -> int:
    """elements of one `pack_policy_params` row"""
    return 64 * num_inputs + 64 + 4096 + 64 + 256 + 4 + 64 + 1


def _num_inputs(env) -> int:
    """E of the env's observations; the refusals that need no tensor"""
    mode = env.observation_mode
    n = -1
    if isinstance(mode, str) and mode.startswith('partial_'):
        try:
            n = int(mode.split('_')[1])
        except ValueError:
            n = -1
    if not 0 <= n <= MAX_OBS_N:
        raise NotImplementedError(f"MultiSnake.act: observation_mode {mode!r} is not served: the feed-forward policy takes "
                                  f"'partial_n' observations with n <= {MAX_OBS_N}")
    if env.dtype != torch.float:
        raise NotImplementedError(f'MultiSnake.act: dtype {env.dtype} is not served: the policy reads fp32 observations '
                                  f'(dtype=torch.float)')
    return 3 * (2 * n + 1) ** 2


def _param_rows(env, params, E) -> int:
    """`params` checked but for how many rows it needs (`_params`, `_multi_league`): the rows it has"""
    if not isinstance(params, torch.Tensor):
        raise RuntimeError(f'MultiSnake.act: params must be a tensor, got {type(params).__name__}')
    if params.dtype != torch.float32:
        raise RuntimeError(f'MultiSnake.act: params must be fp32, got {params.dtype}')
    P = num_policy_params(E)
    if params.dim() not in (1, 2) or params.shape[-1] != P:
        raise RuntimeError(f'MultiSnake.act: params has shape {tuple(params.shape)}, expected (num_species, {P}) or ({P},) '
                           f'for {E} inputs')
    if not params.is_contiguous():
        raise RuntimeError(f'MultiSnake.act: params must be contiguous, got strides {params.stride()}')
    if params.device.type != 'cuda':
        raise _lib.WurmHipError(f'MultiSnake.act runs on the GPU: params is on {params.device}. There is no CPU fallback.')
    if params.device != env.device:
        raise RuntimeError(f'MultiSnake.act: params is on {params.device}, the env on {env.device}')
    return params.shape[0] if params.dim() == 2 else 1


def _params(env, params, num_species, E):
    """(params, num_species) checked"""
    rows = _param_rows(env, params, E)
    if num_species is None:
        num_species = rows
    num_species = int(num_species)
    if not 1 <= num_species <= env.num_snakes:
        raise RuntimeError(f'MultiSnake.act: num_species {num_species} must lie in [1, num_snakes = {env.num_snakes}]')
    if num_species > rows:
        raise RuntimeError(f'MultiSnake.act: num_species {num_species} but params has {rows} rows')
    return params, num_species


def _observations(env, observations, E):
    """(tensor whose storage holds the (K, N, E) block at its data_ptr, N).  A dict whose tensors are consecutive views of
    one buffer (what `step` and `reset` return) is used in place; anything else is stacked once."""
    K, dev = env.num_snakes, env.device
    if isinstance(observations, dict):
        vals = list(observations.values())
        if len(vals) != K:
            raise RuntimeError(f'MultiSnake.act: {len(vals)} observations for {K} snakes')
    elif isinstance(observations, torch.Tensor):
        vals = [observations]
    else:
        raise RuntimeError(f'MultiSnake.act: observations must be a dict or a tensor, got {type(observations).__name__}')
    for v in vals:
        if v.device.type != 'cuda':
            raise _lib.WurmHipError(f'MultiSnake.act runs on the GPU: an observation is on {v.device}. There is no CPU '
                                    f'fallback.')
        if v.device != dev:
            raise RuntimeError(f'MultiSnake.act: an observation is on {v.device}, the env on {dev}')
        if v.dtype != torch.float32:
            raise RuntimeError(f'MultiSnake.act: observations must be fp32, got {v.dtype}')
    if isinstance(observations, torch.Tensor):
        t = observations
        if t.dim() < 3 or t.shape[0] != K or int(torch.Size(t.shape[2:]).numel()) != E:
            raise RuntimeError(f'MultiSnake.act: observations have shape {tuple(t.shape)}, expected ({K}, N, {E}) or '
                               f'({K}, N, 3, w, w)')
        return t.contiguous(), t.shape[1]
    v0 = vals[0]
    N = v0.shape[0] if v0.dim() > 0 else -1
    for v in vals:
        if v.dim() < 2 or v.shape[0] != N or int(torch.Size(v.shape[1:]).numel()) != E:
            raise RuntimeError(f'MultiSnake.act: an observation has shape {tuple(v.shape)}, expected (N, {E}) or '
                               f'(N, 3, w, w)')
    base, row = v0.data_ptr(), 4 * N * E
    if all(v.is_contiguous() and v.data_ptr() == base + j * row for j, v in enumerate(vals)):
        return v0, N  # (alive through the caller's dict until the launch has been queued)
    return torch.stack([v.reshape(N, E) for v in vals]), N


def _outputs(env, N, out):
    """(actions (K, N) int64, probs (K, N, 4), values (K, N)) for the kernel to write: `out` (a window's rows) or fresh"""
    K, dev = env.num_snakes, env.device
    if out is None:
        return (torch.empty((K, N), dtype=torch.long, device=dev), torch.empty((K, N, 4), dtype=torch.float32, device=dev),
                torch.empty((K, N), dtype=torch.float32, device=dev))
    if out[0].shape != (K, N):  # (the window's rows are sized for the env's own batch)
        raise RuntimeError(f'MultiSnake.act_window: observations of {N} envs for an env object of {out[0].shape[1]}')
    return out


def _acted(env, actions, probs, values) -> dict:
    """what `act` returns, behind its launch"""
    env.policy_calls += 1
    # (a plain dict of the K rows of one (K, N) int64 block: what the step machine launches on without stacking)
    return {'actions': {f'agent_{k}': a for k, a in enumerate(actions.unbind(0))}, 'actions_t': actions, 'probs': probs,
            'values': values}


def act(env, params, observations, num_species=None, out=None) -> dict:
    """MultiSnake.act.  out: (actions (K, N) int64, probs (K, N, 4), values (K, N)) to write into (act_window's rows)."""
    E = _num_inputs(env)
    params, P = _params(env, params, num_species, E)
    obs, N = _observations(env, observations, E)
    K, dev = env.num_snakes, env.device
    actions, probs, values = _outputs(env, N, out)
    ptr = _lib.ptr
    rc = _lib.call(dev.index, _lib.lib().wurm_multi_act, ptr(params), ptr(obs), ptr(actions), ptr(probs), ptr(values),
                   _lib.i64(N), K, P, E, _lib.u64(env.seed), _lib.u64(env.policy_calls), _lib.i64(env.env_offset),
                   _lib.stream_ptr(dev.index))
    _lib.check(rc, 'MultiSnake.act')
    return _acted(env, actions, probs, values)


# the keys `act_window(..., info=True)` adds: (name, prefix of the step's info key, dtype)
INFO_KEYS = (('food', 'food_', torch.float32), ('size', 'size_', torch.float32), ('boost', 'boost_', torch.bool),
             ('snake_collision', 'snake_collision_', torch.bool), ('edge_collision', 'edge_collision_', torch.bool))


def act_window(env, params, state, num_steps, num_species=None, info=False, acting=None) -> dict:
    """MultiSnake.act_window.  acting: `acting(state, out)` in place of `act(env, params, state, num_species, out)` — the
    acting call of another binding of policies to rows (`_multi_league.league_window`), which has checked its own
    arguments; stepping, resetting and gathering are the same."""
    T, K, N, dev = int(num_steps), env.num_snakes, env.num_envs, env.device
    if T < 0:
        raise RuntimeError(f'MultiSnake.act_window: num_steps must not be negative, got {T}')
    E = _num_inputs(env)
    if acting is None:
        acting = lambda state, out: act(env, params, state, num_species, out)
        if T == 0:
            _params(env, params, num_species, E)
    actions = torch.empty((T, K * N), dtype=torch.long, device=dev)
    probs = torch.empty((T, K * N, 4), dtype=torch.float32, device=dev)
    values = torch.empty((T, K * N), dtype=torch.float32, device=dev)
    keys = [f'agent_{k}' for k in range(K)]
    obs_rows, reward_rows, done_rows, all_rows, infos = [], [], [], [], []
    for t in range(T):
        a = acting(state, (actions[t].view(K, N), probs[t].view(K, N, 4), values[t].view(K, N)))
        obs, rewards, dones, step_info = env.step(a['actions'])
        env.reset(dones['__all__'], return_observations=False)
        if info:
            infos.append(step_info)  # (a dict over the step's output slab that carves its rows when it is read, below)
        # (views of the step's own output slab: gathered once, behind the loop)
        obs_rows.extend(obs[k] for k in keys)
        reward_rows.extend(rewards[k] for k in keys)
        done_rows.extend(dones[k] for k in keys)
        all_rows.append(dones['__all__'])
        state = obs
    if T == 0:
        observations = torch.empty((0, K * N, E), dtype=torch.float32, device=dev)
        rewards_t = torch.empty((0, K * N), dtype=torch.float32, device=dev)
        dones_t = torch.empty((0, K * N), dtype=torch.bool, device=dev)
        all_done = torch.empty((0, N), dtype=torch.bool, device=dev)
    else:
        observations = torch.stack(obs_rows).view(T, K * N, E)
        rewards_t = torch.stack(reward_rows).view(T, K * N)
        dones_t = torch.stack(done_rows).view(T, K * N)
        all_done = torch.stack(all_rows)
    out = {'observations': observations, 'actions': actions, 'probs': probs, 'values': values, 'rewards': rewards_t,
           'dones': dones_t, 'all_done': all_done, 'state': state}
    if info:  # what `step` logged per agent (reference :707-729), gathered like rewards and dones: one stack per key
        for name, prefix, dtype in INFO_KEYS:
            if T == 0:
                out[name] = torch.empty((0, K * N), dtype=dtype, device=dev)
            else:
                out[name] = torch.stack([i[f'{prefix}{k}'] for i in infos for k in range(K)]).view(T, K * N)
    return out
