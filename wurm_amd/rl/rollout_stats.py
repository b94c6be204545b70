"""The log columns of the reference's experiment (experiments/main.py:252-316: episodes, reward_rate, policy_entropy,
edge_collisions, self_collisions, avg_size and their exponentially smoothed versions) for the fused training loop, plus
per-episode return, length and final snake size: `RolloutStats.update(out)` takes what `env.policy_rollout` returned and
enqueues two launches (include/wurm_hip.h: wurm_rollout_stats; wurm_amd/csrc/rollout_stats.hpp), `read()` is the one
host copy, made when a log line is due.

`avg_size` is the reference's headline metric and is read there from `env.envs` after every step's reset; a fused
window only has the state after its last step.  The length of a snake is therefore CARRIED per env: 3 after a reset,
one more exactly when the step's reward is 1.  So are the return and the length of the running episode, across windows.
"""
import ctypes
import math

import torch

from wurm_amd import _lib
from wurm_amd.constants import BODY_CHANNEL

# per-step columns in the order of the table, the smoother and accum[1:7] (wurm_hip.h), under the names of the log
COLUMNS = ('done_rate', 'reward_rate', 'edge_collisions', 'self_collisions', 'avg_size', 'policy_entropy')
ACC = 12


class RolloutStats(object):
    """Training statistics of chained `policy_rollout` windows, kept on the device.

    Args:
        env: the SingleSnake or SimpleGridworld the windows come from (its num_envs, device and, for SingleSnake, the
            current length of every snake: build this after `env.reset()` and before the first window, or at any
            window boundary).  SimpleGridworld has no size and no self-collision column: they stay 0.
        population: None, or P: member p owns the envs [p N / P, (p + 1) N / P) as in `policy_rollout(..., population=P)`
            and every result gains a leading member dimension; member p's numbers are bit for bit those of a
            stand-alone RolloutStats on its columns.
        alpha: the reference's ExponentialMovingAverageTracker(alpha), applied to the per-step batch means.
    """

    def __init__(self, env, population: int = None, alpha: float = 0.025):
        N = int(env.num_envs)
        P = 1 if population is None else int(population)
        if P <= 0 or N <= 0 or N % P != 0:
            raise RuntimeError(f'population must be a positive divisor of num_envs ({N}), got {population}')
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise RuntimeError(f'alpha must lie in [0, 1], got {alpha}')
        self.num_envs, self.num_members, self.population, self.alpha = N, P, population, alpha
        self.device = dev = torch.device(env.device)
        self.snake = hasattr(env, 'initial_snake_length')
        self.initial_size = int(env.initial_snake_length) if self.snake else 0
        # (3, N) words: episode return (fp32 bits), episode length, snake size (wurm_hip.h)
        self.carry = torch.zeros((3, N), dtype=torch.int32, device=dev)
        if self.snake:
            self.carry[2] = env.envs[:, BODY_CHANNEL].flatten(1).amax(1).to(torch.int32)  # main.py:273
        self.accum = self._fresh_accum()
        self.smooth = torch.full((P, len(COLUMNS)), math.nan, dtype=torch.float64, device=dev)
        self._workspace = {}

    def _fresh_accum(self):
        accum = torch.zeros((self.num_members, ACC), dtype=torch.float64, device=self.device)
        accum[:, 10:] = -math.inf  # the two maxima: no episode yet
        return accum

    # the carry's rows under their types
    @property
    def episode_return(self) -> torch.Tensor:
        return self.carry[0].view(torch.float32)

    @property
    def episode_length(self) -> torch.Tensor:
        return self.carry[1]

    @property
    def size(self) -> torch.Tensor:
        return self.carry[2]

    def _inputs(self, out):
        dev, N = self.device, self.num_envs
        rewards, dones, edge = out['rewards'], out['dones'], out['edge_collision']
        selfc, probs = out.get('self_collision') if self.snake else None, out.get('probs')
        if rewards.dim() != 2 or rewards.numel() == 0:
            raise RuntimeError('rewards must be a non-empty (num_steps, num_envs) tensor')
        T = rewards.shape[0]
        if rewards.shape[1] != N:
            raise RuntimeError(f'rewards has {rewards.shape[1]} envs, the statistics were built for {N}')
        if rewards.dtype != torch.float32:
            raise RuntimeError('rewards must be fp32')
        flags = [('dones', dones), ('edge_collision', edge)] + ([('self_collision', selfc)] if selfc is not None else [])
        for name, t in flags:
            if t.shape != (T, N) or t.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError(f'{name} must be a (num_steps, num_envs) bool tensor')
        if probs is not None and (probs.shape != (T, N, 4) or probs.dtype != torch.float32):
            raise RuntimeError('probs must be a (num_steps, num_envs, 4) fp32 tensor')
        for name, t in [('rewards', rewards), ('probs', probs)] + flags:
            if t is not None and t.device != dev:
                raise RuntimeError(f'{name} must be on the device of the env ({dev})')
        if dev.type != 'cuda':
            raise _lib.WurmHipError('RolloutStats.update runs on the GPU: the env and its rollouts live on the device')
        ws = self._workspace.get(T)
        if ws is None:
            nbytes = _lib.lib().wurm_rollout_stats_workspace_bytes(N, T, self.num_members)
            ws = self._workspace[T] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
        cont = lambda t: None if t is None else t.contiguous()
        return cont(rewards), cont(dones), cont(edge), cont(selfc), cont(probs), ws, T

    def update(self, out: dict, per_step: bool = False):
        """Adds one window — the dict `policy_rollout` returned (`rewards`, `dones`, `edge_collision`, and where present
        `self_collision` and `probs`) — in two launches; nothing is copied to the host.  per_step=True returns the
        window's (T, 6) device table (population: (P, T, 6)) of float64 batch SUMS per step, columns `COLUMNS`."""
        rewards, dones, edge, selfc, probs, (ws, nbytes), T = self._inputs(out)
        dev, P = self.device, self.num_members
        table = torch.empty((P, T, len(COLUMNS)), dtype=torch.float64, device=dev) if per_step else None
        rc = _lib.call(dev.index, _lib.lib().wurm_rollout_stats, _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(edge),
                       _lib.ptr(selfc), _lib.ptr(probs), _lib.ptr(self.carry), _lib.ptr(self.accum),
                       _lib.ptr(self.smooth), _lib.ptr(table), _lib.ptr(ws), _lib.i64(nbytes), _lib.i64(self.num_envs),
                       _lib.i64(T), _lib.i64(P), self.initial_size, ctypes.c_double(self.alpha),
                       _lib.stream_ptr(dev.index))
        _lib.check(rc, 'RolloutStats.update')
        if per_step:
            return table if self.population is not None else table[0]

    def read(self, reset: bool = True):
        """The one host copy: a dict (population: a list of P dicts) of the statistics since the last `read(reset=True)`:
        `steps` (env steps), `episodes`, the means per env step `done_rate`, `reward_rate`, `policy_entropy`,
        `edge_collisions`, `self_collisions`, `avg_size`, over the finished episodes `episode_return_mean`,
        `episode_length_mean`, `episode_size_mean`, `episode_return_max`, `episode_size_max` (nan without an episode),
        and `ewm_<column>` for the six per-step columns.  reset=True clears the sums; the carry and the smoother go on."""
        both = torch.cat([self.accum, self.smooth], dim=1).cpu().tolist()
        if reset:
            self.accum.copy_(self._fresh_accum())
        rows = []
        for r in both:
            steps, episodes = r[0], r[1]
            per_step = lambda x: x / steps if steps else math.nan
            per_episode = lambda x: x / episodes if episodes else math.nan
            row = dict(steps=int(steps), episodes=int(episodes))
            row.update((name, per_step(r[1 + k])) for k, name in enumerate(COLUMNS))
            row.update(episode_return_mean=per_episode(r[7]), episode_length_mean=per_episode(r[8]),
                       episode_size_mean=per_episode(r[9]), episode_return_max=r[10] if episodes else math.nan,
                       episode_size_max=r[11] if episodes else math.nan)
            row.update(('ewm_' + name, r[ACC + k]) for k, name in enumerate(COLUMNS))
            rows.append(row)
        return rows if self.population is not None else rows[0]

    def state_dict(self) -> dict:
        return {'carry': self.carry.clone(), 'accum': self.accum.clone(), 'smooth': self.smooth.clone()}

    def load_state_dict(self, state: dict):
        for name in ('carry', 'accum', 'smooth'):
            mine, theirs = getattr(self, name), state[name]
            if theirs.shape != mine.shape or theirs.dtype != mine.dtype:
                raise RuntimeError(f'{name}: expected {tuple(mine.shape)} {mine.dtype}, got {tuple(theirs.shape)} '
                                   f'{theirs.dtype}')
        for name in ('carry', 'accum', 'smooth'):
            getattr(self, name).copy_(state[name])
