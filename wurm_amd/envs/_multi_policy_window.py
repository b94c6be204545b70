"""MultiSnake.policy_window / MultiSnake.policy_window_fused (wurm_amd/envs/multi_snake.py): `act_window` — T iterations of
act / step / reset(dones['__all__']), two launches per step — as ONE launch with the envs on chip (include/wurm_hip.h:
wurm_multi_policy_window; kernel: wurm_amd/csrc/multi_policy_window.hpp).  Same arguments, same dict, same bits: the kernel
is assembled from the step, reset, crop and policy code the per-call launches run, and draws from the same counters
(step t at c + 2 t, its reset at c + 2 t + 1, the policy at policy_calls + t).

Host protocol: that of `MultiSnake.rollout` on the fp32 tensors — except that a reset(done) postponed in front of the window
is not flushed but handed to the launch (`pre_done` / `pre_call`, as `step` hands it over), and that the reset of the last
step, which `act_window` leaves postponed, is applied inside the launch: its counter is spent either way, and whatever looks
at the state applies a postponed reset first, so no caller can tell.  A resident mirror (large batches) is written out and
marked stale, as `rollout` on the tensors does.

What falls back to `act_window` (`policy_window_fused` says which): 'partial_n' with n > 3, `dtype=torch.half`, an env
whose `env_lifetimes` somebody has asked for, a grid the fused rollouts do not serve (size < 5), and whatever
wurm_multi_policy_window_plan refuses.
"""
import ctypes
from collections import OrderedDict

import torch

from wurm_amd import _lib
from wurm_amd.envs import _multi_act

MAX_FUSED_OBS_N = 3  # E = 3 (2n+1)^2 <= 147


def plan(env, num_species) -> int:
    """0: `policy_window` runs `act_window`; 1: fused, the species' weights resident on chip; 2: fused, weights reloaded per
    species (more than 4 species, or 4 at 'partial_3')"""
    mode = env.observation_mode
    if not (isinstance(mode, str) and mode.startswith('partial_')):
        return 0
    try:
        n = int(mode.split('_')[1])
    except ValueError:
        return 0
    if not 0 <= n <= MAX_FUSED_OBS_N or env.dtype != torch.float or env._lifetimes_touched or env._force_act_window:
        return 0
    return int(_lib.lib().wurm_multi_policy_window_plan(env.num_snakes, env.size, n, int(num_species), _lib.i64(env.num_envs)))


def policy_window(env, params, state, num_steps, num_species=None, info=False) -> dict:
    """MultiSnake.policy_window"""
    T, K, N, dev = int(num_steps), env.num_snakes, env.num_envs, env.device
    if T < 0:
        raise RuntimeError(f'MultiSnake.act_window: num_steps must not be negative, got {T}')
    E = _multi_act._num_inputs(env)
    params, P = _multi_act._params(env, params, num_species, E)
    if T == 0 or N == 0 or not plan(env, P):
        return _multi_act.act_window(env, params, state, T, P, info)
    obs0, n0 = _multi_act._observations(env, state, E)
    if n0 != N:
        raise RuntimeError(f'MultiSnake.act_window: observations of {n0} envs for an env object of {N}')
    fs = env._fs
    ro = env._reset_obs
    if ro.probe is not None or ro.ref is not None:
        env._reset_obs_bookkeeping()
    # the state tensors, normalised, with the postponed reset still owed: it belongs in front of THIS launch
    pend, fs.pending = fs.pending, False
    try:
        foods, heads, bodies, dones, orientations, colours, boost = env._state()
    finally:
        fs.pending = pend
    KN = K * N
    f32, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.bool, device=dev)
    out = {'observations': torch.empty((T, KN, E), **f32), 'actions': torch.empty((T, KN), dtype=torch.long, device=dev),
           'probs': torch.empty((T, KN, 4), **f32), 'values': torch.empty((T, KN), **f32),
           'rewards': torch.empty((T, KN), **f32), 'dones': torch.empty((T, KN), **u8),
           'all_done': torch.empty((T, N), **u8)}
    extra = {name: torch.empty((T, KN), dtype=dtype, device=dev) for name, _, dtype in _multi_act.INFO_KEYS}
    c, ptr = _lib.MultiPolicyWindowCall(), _lib.ptr
    c.foods, c.heads, c.bodies, c.dones = ptr(foods), ptr(heads), ptr(bodies), ptr(dones)
    c.orientations, c.colours, c.boost_this_step = ptr(orientations), ptr(colours), ptr(boost)
    c.pre_done = ptr(env._pend) if pend else None
    c.params, c.obs0 = ptr(params), ptr(obs0)
    c.actions, c.probs, c.values, c.observations = (ptr(out[k]) for k in ('actions', 'probs', 'values', 'observations'))
    c.rewards, c.dones_out, c.all_done = ptr(out['rewards']), ptr(out['dones']), ptr(out['all_done'])
    c.food, c.sizes, c.boost = ptr(extra['food']), ptr(extra['size']), ptr(extra['boost'])
    c.snake_collision, c.edge_collision = ptr(extra['snake_collision']), ptr(extra['edge_collision'])
    c.num_envs, c.num_steps, c.env_offset, c.num_params = N, T, env.env_offset, params.shape[-1]
    c.seed, c.call0, c.pre_call, c.policy_call0 = _lib.u64(env.seed), _lib.u64(fs.call), _lib.u64(fs.pend_call if pend else 0), \
        _lib.u64(env.policy_calls)
    c.num_snakes, c.size, c.obs_n, c.num_species = K, env.size, int(env.observation_mode.split('_')[1]), P
    c.waves_per_group = int(env._policy_window_wpb)
    c.cfg = env._cfg()
    rc = _lib.call(dev.index, _lib.lib().wurm_multi_policy_window, ctypes.byref(c), _lib.stream_ptr(dev.index))
    _lib.check(rc, 'MultiSnake.policy_window')
    # (only now: if anything above raised, the postponed reset and the counters are still owed)
    fs.pending = False
    env._next_call(2 * T)
    env.policy_calls += T
    env._info = None
    env._out.rewards_src, env._out.rewards_t, env._out.rewards_at = out['rewards'][-1].view(K, N), None, fs.steps
    w = 2 * c.obs_n + 1
    out['state'] = OrderedDict((f'agent_{k}', o) for k, o in enumerate(out['observations'][-1].view(K, N, 3, w, w).unbind(0)))
    if info:
        out.update(extra)
    return out
