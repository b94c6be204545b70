"""The per-agent log columns of the reference's multi-agent experiment (experiments/multiagent.py:486-505: `reward_i`,
`policy_entropy_i`, `food_i`, `edge_collisions_i`, `snake_collisions_i`, `boost_i`, `size_i`, `done_i`, `return_i`, their
exponentially smoothed versions and `episodes`) for the fused multi-agent loop, plus the return and length of every life:
`MultiRolloutStats.update(out)` takes what `MultiSnake.act_window(..., info=True)` (or `MultiSnake.rollout`) returned and
enqueues two launches (include/wurm_hip.h: wurm_multi_rollout_stats; wurm_amd/csrc/multi_rollout_stats.hpp), `read()` is
the one host copy, made when a log line is due.

Seven of the nine columns are means over a per-agent mask (`~done_i`, or `done_i` for `return_i`).  ONE DEVIATION from the
reference: a step whose mask is empty gives it a NaN mean, and that NaN poisons its tracker for good (`return_i` does so
on the first step without a death); here such a step leaves the column's smoothed value as it was.
"""
import ctypes
import math

import torch

from wurm_amd import _lib
from wurm_amd.envs._multi_act import species_of

# the smoother's columns in the reference's order (multiagent.py:493-502), each as (numerator, mask) among the ten per-step
# sums of the table and accum[1:11] (wurm_hip.h); mask None: all N envs
SUMS = ('alive', 'done', 'reward', 'policy_entropy', 'food', 'boost', 'size', 'edge_collisions', 'snake_collisions',
        'size_at_death')
COLUMNS = ('reward', 'policy_entropy', 'food', 'edge_collisions', 'snake_collisions', 'boost', 'size', 'done', 'return')
RATIOS = ((2, 0), (3, 0), (4, 0), (7, None), (8, None), (5, 0), (6, 0), (1, None), (9, 1))
ACC = 16
_FLOATS = ('rewards', 'food', 'size')
_FLAGS = ('dones', 'boost', 'snake_collision', 'edge_collision')
_INFO = ('food', 'size', 'boost', 'snake_collision', 'edge_collision')


def _row(r, smooth=None):
    """one dict of `read()` from an accumulator row (a list of 16 floats)"""
    steps, deaths = r[0], r[2]
    ratio = lambda num, den: num / den if den else math.nan
    row = dict(steps=int(steps), episodes=int(r[15]))
    for name, (num, den) in zip(COLUMNS, RATIOS):
        row[name] = ratio(r[1 + num], steps if den is None else r[1 + den])
    row.update(life_return_mean=ratio(r[11], deaths), life_length_mean=ratio(r[12], deaths),
               size_at_death_max=r[13] if deaths else math.nan, life_return_max=r[14] if deaths else math.nan)
    if smooth is not None:
        row.update(('ewm_' + name, s) for name, s in zip(COLUMNS, smooth))
    return row


class MultiRolloutStats(object):
    """Training statistics of chained MultiSnake windows, per agent, kept on the device.

    Args:
        env: the MultiSnake the windows come from (its num_envs, num_snakes and device).
        alpha: the reference's ExponentialMovingAverageTracker(alpha), applied to the per-step masked means.
    """

    def __init__(self, env, alpha: float = 0.025):
        N, K = int(env.num_envs), int(env.num_snakes)
        if N <= 0 or K <= 0:
            raise RuntimeError(f'num_envs and num_snakes must be positive, got {N} and {K}')
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise RuntimeError(f'alpha must lie in [0, 1], got {alpha}')
        self.num_envs, self.num_snakes, self.alpha = N, K, alpha
        self.device = dev = torch.device(env.device)
        # (2, K N) words: the life's return (fp32 bits) and length of every (snake, env) pair (wurm_hip.h)
        self.carry = torch.zeros((2, K * N), dtype=torch.int32, device=dev)
        self.accum = self._fresh_accum()
        self.smooth = torch.full((K, len(COLUMNS)), math.nan, dtype=torch.float64, device=dev)
        self._workspace = {}

    def _fresh_accum(self):
        accum = torch.zeros((self.num_snakes, ACC), dtype=torch.float64, device=self.device)
        accum[:, 13:15] = -math.inf  # the two maxima: no death yet
        return accum

    # the carry's rows under their types
    @property
    def life_return(self) -> torch.Tensor:
        return self.carry[0].view(torch.float32)

    @property
    def life_length(self) -> torch.Tensor:
        return self.carry[1]

    def _inputs(self, out):
        dev, N, K = self.device, self.num_envs, self.num_snakes
        for name in _FLOATS + _FLAGS:
            if out.get(name) is None:
                hint = ': pass info=True to MultiSnake.act_window' if name in _INFO else ''
                raise RuntimeError(f'MultiRolloutStats.update: the window has no {name!r}{hint}')
        rewards = out['rewards']
        if rewards.dim() not in (2, 3) or rewards.numel() == 0 or \
                tuple(rewards.shape[1:]) not in ((K * N,), (K, N)):
            raise RuntimeError(f'MultiRolloutStats.update: rewards has shape {tuple(rewards.shape)}, expected a non-empty '
                               f'(num_steps, {K * N}) or (num_steps, {K}, {N})')
        T, shape = rewards.shape[0], tuple(rewards.shape)
        probs, all_done = out.get('probs'), out.get('all_done')
        named = [(n, out[n], shape, (torch.float32,)) for n in _FLOATS]
        named += [(n, out[n], shape, (torch.bool, torch.uint8)) for n in _FLAGS]
        if probs is not None:
            named.append(('probs', probs, shape + (4,), (torch.float32,)))
        if all_done is not None:
            named.append(('all_done', all_done, (T, N), (torch.bool, torch.uint8)))
        for name, t, want, dtypes in named:
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f'MultiRolloutStats.update: {name} must be a tensor, got {type(t).__name__}')
            if tuple(t.shape) != want:
                raise RuntimeError(f'MultiRolloutStats.update: {name} has shape {tuple(t.shape)}, expected {want}')
            if t.dtype not in dtypes:
                raise RuntimeError(f'MultiRolloutStats.update: {name} must be {" or ".join(map(str, dtypes))}, got '
                                   f'{t.dtype}')
            if t.device != dev:
                raise RuntimeError(f'MultiRolloutStats.update: {name} is on {t.device}, the env on {dev}')
        if dev.type != 'cuda':
            raise _lib.WurmHipError('MultiRolloutStats.update runs on the GPU: the env and its windows live on the device')
        ws = self._workspace.get(T)
        if ws is None:
            nbytes = _lib.lib().wurm_multi_rollout_stats_workspace_bytes(N, K, T)
            ws = self._workspace[T] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
        # ((T, K, N) views of `rollout`'s blocks: made contiguous; (T, K N) and (T, K, N) are the same memory then)
        tensors = [t.contiguous() for _, t, _, _ in named[:7]]
        return tensors, (probs.contiguous() if probs is not None else None), \
            (all_done.contiguous() if all_done is not None else None), ws, T

    def update(self, out: dict, per_step: bool = False):
        """Adds one window — the dict `act_window(..., info=True)` returned (`rewards`, `food`, `size`, `dones`, `boost`,
        `snake_collision`, `edge_collision` as (T, K N), `probs`, `all_done`), or that of `MultiSnake.rollout` (the same keys
        as (T, K, N), no `probs`: the entropy column stays 0) — in two launches; nothing is copied to the host.
        per_step=True returns the window's (K, T, 10) device table of float64 batch SUMS per step, columns `SUMS`."""
        tensors, probs, all_done, (ws, nbytes), T = self._inputs(out)
        dev, K = self.device, self.num_snakes
        table = torch.empty((K, T, len(SUMS)), dtype=torch.float64, device=dev) if per_step else None
        ptr = _lib.ptr
        rc = _lib.call(dev.index, _lib.lib().wurm_multi_rollout_stats, *[ptr(t) for t in tensors], ptr(probs),
                       ptr(all_done), ptr(self.carry), ptr(self.accum), ptr(self.smooth), ptr(table), ptr(ws),
                       _lib.i64(nbytes), _lib.i64(self.num_envs), _lib.i64(K), _lib.i64(T), ctypes.c_double(self.alpha),
                       _lib.stream_ptr(dev.index))
        _lib.check(rc, 'MultiRolloutStats.update')
        return table

    def read(self, reset: bool = True, num_species: int = None):
        """The one host copy: a list of K dicts (one per agent) of the statistics since the last `read(reset=True)`:
        `steps` (env steps), `episodes` (envs whose snakes were all dead), the nine columns `reward`, `policy_entropy`,
        `food`, `boost`, `size` (means over the steps the agent was alive), `edge_collisions`, `snake_collisions`, `done`
        (means over all steps), `return` (the mean size at death), each the window-long sum over the window-long mask (nan
        where the mask never held); over the deaths `life_return_mean`, `life_length_mean`, `size_at_death_max`,
        `life_return_max` (nan without one); and `ewm_<column>` for the nine columns.
        num_species=P: P dicts instead, one per species (`species_of`): the sums of a species' snakes are added on the host
        before dividing (maxima folded, `episodes` counts envs and is not added), and there are no smoothed values.
        reset=True clears the sums; the carry and the smoother go on."""
        K = self.num_snakes
        if num_species is not None and not 1 <= int(num_species) <= K:
            raise RuntimeError(f'num_species {num_species} must lie in [1, num_snakes = {K}]')
        both = torch.cat([self.accum, self.smooth], dim=1).cpu().tolist()
        if reset:
            self.accum.copy_(self._fresh_accum())
        if num_species is None:
            return [_row(r[:ACC], r[ACC:]) for r in both]
        P = int(num_species)
        rows = [[0.0] * 13 + [-math.inf] * 2 + [0.0] for _ in range(P)]
        for k, r in enumerate(both):
            s = rows[species_of(k, K, P)]
            for j in range(13):
                s[j] += r[j]
            s[13], s[14], s[15] = max(s[13], r[13]), max(s[14], r[14]), r[15]
        return [_row(s) for s in rows]

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
