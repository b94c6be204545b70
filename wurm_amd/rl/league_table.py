"""The results of a league per POLICY (wurm_amd/envs/_multi_league.py: a line-up per env): `LeagueTable.update(plan, out)`
takes the plan a window was played under and what `MultiSnake.league_window` returned, and adds every policy's sums over
its (snake, env) rows and the window's steps to a (num_policies, 8) float64 table on the device, in one launch
(include/wurm_hip.h: wurm_multi_league_scores; wurm_amd/csrc/multi_league.hpp: league_scores_kernel).  `read()` is the one
host copy.  The per-agent columns of a fixed pairing, with the reference's masks and smoothers, are `MultiRolloutStats`.

The sums are plain: `steps` counts row-steps (T per row a policy plays, alive or not), `deaths` the steps with `dones` set
(a snake that stays dead for several steps counts on each, as `MultiRolloutStats` has it), the rest add the window's
tensors as they are.  Counts, sizes and rewards from {-1, 0, 1} are integers: exact in double, in any order.
"""
import math

import torch

from wurm_amd import _lib
from wurm_amd.envs._multi_league import LeaguePlan

COLUMNS = ('steps', 'reward', 'deaths', 'food', 'snake_collisions', 'edge_collisions', 'boost', 'size_sum')
# the `info=True` keys of a window -> their columns; all of them or none
_INFO = ('food', 'size', 'boost', 'snake_collision', 'edge_collision')


def row_dict(r) -> dict:
    """one dict of `read()` from a table row (eight floats): the sums, and the means that follow from them"""
    row = dict(zip(COLUMNS, r))
    steps, deaths = row['steps'], row['deaths']
    ratio = lambda num, den: num / den if den else math.nan
    for name in ('reward', 'food', 'snake_collisions', 'edge_collisions', 'boost', 'deaths'):
        row[name + '_per_step'] = ratio(row[name], steps)
    row['size_mean'] = ratio(row['size_sum'], steps)
    row['reward_per_life'] = ratio(row['reward'], deaths)
    row['food_per_life'] = ratio(row['food'], deaths)
    row['life_length_mean'] = ratio(steps, deaths)
    return row


class LeagueTable(object):
    """Per-policy sums of chained league windows, kept on the device.

    Args:
        num_policies: A, the rows of `params` the plans name.
        device: where the windows live.
    """

    def __init__(self, num_policies: int, device):
        A = int(num_policies)
        if A < 1:
            raise RuntimeError(f'num_policies must be positive, got {A}')
        self.num_policies, self.device = A, torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.table = torch.zeros((A, len(COLUMNS)), dtype=torch.float64, device=self.device)

    def _inputs(self, plan, out):
        dev, A = self.device, self.num_policies
        if not isinstance(plan, LeaguePlan):
            raise RuntimeError(f'LeagueTable.update: plan must come from league_plan, got {type(plan).__name__}')
        if plan.num_policies != A:
            raise RuntimeError(f'LeagueTable.update: the plan names {plan.num_policies} policies, the table has {A}')
        R = plan.order.numel()
        for name in ('rewards', 'dones'):
            if out.get(name) is None:
                raise RuntimeError(f'LeagueTable.update: the window has no {name!r}')
        have = [name for name in _INFO if out.get(name) is not None]
        if have and len(have) != len(_INFO):
            raise RuntimeError(f'LeagueTable.update: the window has {have} but not the other info=True keys of {_INFO}')
        rewards = out['rewards']
        if not isinstance(rewards, torch.Tensor) or rewards.dim() != 2 or rewards.shape[1] != R:
            shape = tuple(rewards.shape) if isinstance(rewards, torch.Tensor) else type(rewards).__name__
            raise RuntimeError(f'LeagueTable.update: rewards has shape {shape}, expected (num_steps, {R}) for this plan')
        shape = tuple(rewards.shape)
        floats, flags = (torch.float32,), (torch.bool, torch.uint8)
        named = [('rewards', floats), ('dones', flags)]
        if have:
            named += [('food', floats), ('size', floats), ('boost', flags), ('snake_collision', flags),
                      ('edge_collision', flags)]
        tensors = []
        for name, dtypes in named:
            t = out[name]
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f'LeagueTable.update: {name} must be a tensor, got {type(t).__name__}')
            if tuple(t.shape) != shape:
                raise RuntimeError(f'LeagueTable.update: {name} has shape {tuple(t.shape)}, expected {shape}')
            if t.dtype not in dtypes:
                raise RuntimeError(f'LeagueTable.update: {name} must be {" or ".join(map(str, dtypes))}, got {t.dtype}')
            if t.device != dev:
                raise RuntimeError(f'LeagueTable.update: {name} is on {t.device}, the table on {dev}')
            tensors.append(t.contiguous())
        if plan.order.device != dev:
            raise RuntimeError(f'LeagueTable.update: the plan is on {plan.order.device}, the table on {dev}')
        if dev.type != 'cuda':
            raise _lib.WurmHipError('LeagueTable.update runs on the GPU: the windows live on the device')
        tensors += [None] * (7 - len(tensors))
        return tensors, R, shape[0]

    def update(self, plan, out: dict) -> None:
        """Adds one window — the dict `league_window(params, state, T, plan)` returned (`rewards`, `dones` (T, K N); with
        info=True also `food`, `size`, `boost`, `snake_collision`, `edge_collision`, else those columns get nothing) —
        under the plan it was played with, in one launch; nothing is copied to the host."""
        tensors, R, T = self._inputs(plan, out)
        dev, ptr = self.device, _lib.ptr
        rc = _lib.call(dev.index, _lib.lib().wurm_multi_league_scores, *[ptr(t) for t in tensors], ptr(plan.order),
                       ptr(plan.offsets), ptr(self.table), _lib.i64(R), _lib.i64(T), self.num_policies,
                       _lib.stream_ptr(dev.index))
        _lib.check(rc, 'LeagueTable.update')

    def read(self) -> list:
        """The one host copy: a list of num_policies dicts — the eight sums `COLUMNS`, the means per row-step
        `reward_per_step`, `food_per_step`, `snake_collisions_per_step`, `edge_collisions_per_step`, `boost_per_step`,
        `deaths_per_step`, `size_mean`, and per life (per death) `reward_per_life`, `food_per_life`, `life_length_mean`
        (nan where the denominator is 0: a policy that never played, or never died)."""
        return [row_dict(r) for r in self.table.cpu().tolist()]

    def reset(self) -> None:
        self.table.zero_()
