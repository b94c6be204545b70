"""MultiSnake.record_start / MultiSnake.record_frames (wurm_amd/envs/multi_snake.py): the frames of a fused multi-agent
window — `act_window`, `rollout` — for a few chosen envs, by replaying them after the fact in one launch
(include/wurm_hip.h: wurm_multi_rollout_frames; kernel: wurm_amd/csrc/multi_frames.hpp).  The multi-agent twin of the pair in
wurm_amd/envs/_fast_step.py; the windows themselves are not touched and pay nothing."""
import ctypes
import weakref

import torch

from wurm_amd import _lib

# the seven tensors that are the state of an env, in the order of the entry point's arguments and of `final`
STATE_NAMES = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours', 'boost_this_step')


class MultiFrameRecord(object):
    """What `record_start` keeps of the moment before a window: the selected envs' state and what keys their random draws."""

    def __init__(self, env, select, start, call):
        self.owner = weakref.ref(env)
        self.select, self.start, self.call = select, tuple(start), int(call)
        self.seed, self.env_offset, self.size, self.num_snakes = int(env.seed), int(env.env_offset), int(env.size), \
            int(env.num_snakes)
        self.cfg = _lib.MultiConfig.from_buffer_copy(env._cfg())  # a copy: the env's cached block may be replaced


def _agents(idx: torch.Tensor, K: int) -> torch.Tensor:
    """the rows of the per-agent tensors that belong to the envs `idx` (agent = env * num_snakes + i)"""
    return (idx[:, None] * K + torch.arange(K, device=idx.device)).reshape(-1)


def record_start(env, select) -> MultiFrameRecord:
    """MultiSnake.record_start"""
    sel = torch.as_tensor(select, dtype=torch.long).to(env.device).reshape(-1).contiguous()
    if sel.numel() == 0:
        raise RuntimeError('record_start: select is empty')
    # (a postponed reset applied with its own counter, a lazy mirror written out: the tensors are the state, read only)
    foods, heads, bodies, dones, orientations, colours, boost = env._state(write=False)
    # (the gather itself must stay inside the tensors: what is out of range is the replay kernel's to report)
    idx = sel.clamp(0, env.num_envs - 1)
    aidx = _agents(idx, env.num_snakes)
    start = (foods.index_select(0, idx),) + tuple(t.index_select(0, aidx) for t in (heads, bodies, dones, orientations,
                                                                                    colours, boost))
    return MultiFrameRecord(env, sel, start, env._fs.call)


def record_frames(env, rec, actions) -> dict:
    """MultiSnake.record_frames"""
    if not isinstance(rec, MultiFrameRecord) or rec.owner() is not env:
        raise RuntimeError('record_frames: this record was started on another env object')
    N, K, S, dev = env.num_envs, env.num_snakes, env.size, env.device
    ok = isinstance(actions, torch.Tensor) and actions.dtype == torch.long and actions.device == dev and \
        actions.is_contiguous() and ((actions.dim() == 2 and actions.shape[1] == K * N) or
                                     (actions.dim() == 3 and tuple(actions.shape[1:]) == (K, N)))
    if not ok:
        raise RuntimeError(f'record_frames: actions must be the contiguous int64 device tensor of the window: (T, {K * N}) '
                           f"as act_window returns it or (T, {K}, {N}) as rollout takes it")
    T = int(actions.shape[0])
    if (rec.seed, rec.env_offset, rec.size, rec.num_snakes) != (int(env.seed), int(env.env_offset), int(S), int(K)):
        raise RuntimeError('record_frames: stale record — seed, env_offset, size or num_snakes changed since record_start')
    if bytes(rec.cfg) != bytes(env._cfg()):
        raise RuntimeError('record_frames: stale record — the dynamics (boost, food_mode, food_rate, food_on_death_prob, '
                           'boost_cost_prob, max_food, reward_on_death, respawn_mode, colour_mode) changed since '
                           'record_start; a window must run under one configuration to be replayed')
    if int(env._fs.call) != rec.call + 2 * T:
        raise RuntimeError(f'record_frames: stale record — it was started at call counter {rec.call} and a window of '
                           f'{T} steps ends at {rec.call + 2 * T}, but the counter is {int(env._fs.call)}: another '
                           f'call that draws random numbers ran since record_start besides the window')
    k = rec.select.numel()
    frames = torch.empty((T + 1, k, 3, S, S), dtype=torch.short, device=dev)
    final = tuple(torch.empty_like(t) for t in rec.start)
    status = torch.empty(k, dtype=torch.uint8, device=dev)
    ptr = _lib.ptr
    rc = _lib.call(dev.index, _lib.lib().wurm_multi_rollout_frames, *[ptr(t) for t in rec.start], ptr(rec.select),
                   ptr(actions) if T > 0 else None, ptr(frames), *[ptr(t) for t in final], ptr(status), _lib.i64(k),
                   _lib.i64(N), K, S, _lib.i64(T), ctypes.byref(rec.cfg), _lib.u64(rec.seed), _lib.u64(rec.call),
                   _lib.i64(rec.env_offset), _lib.stream_ptr(dev.index))
    _lib.check(rc, 'MultiSnake.record_frames')
    return dict(frames=frames, final=dict(zip(STATE_NAMES, final)), status=status)
