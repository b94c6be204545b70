"""P independent A2C learners in the three launches of one (include/wurm_hip.h: wurm_a2c_ff_pop_*): the sweep over
seeds and hyper-parameters that experiments/main.py is run for (`--r`, `--lr`, `--gamma`, `--entropy`), as one env
object, one `policy_rollout(..., population=P)` and one `FusedA2CPopulation.update` per window.

Member p owns the envs [p M, (p + 1) M) of the N = P M envs, row p of the (P, num_params) buffers `params`, `exp_avg`
and `exp_avg_sq`, and its own lr, gamma, entropy_coef and gae_lambda.  Every result of member p is bit for bit what a
`FusedA2CLearner` of its own computes from contiguous copies of its columns: its part of the grid is the grid of that
stand-alone update.  The per-member hyper-parameters live in a small device table built once, here; an update copies
nothing to the device and reads nothing back.

`exploit(scores)` is the step of population-based training: the worst members take over the weights, Adam state and
hyper-parameters of good ones and perturb the copied lr and entropy_coef, on the device, in two launches
(wurm_amd/csrc/a2c_pbt.hpp).  From then on the table, not the constructor's arguments, says what the members train with:
`hyperparameters()` reads it.
"""
import ctypes
import math

import numpy as np
import torch

from wurm_amd import _lib
from wurm_amd.rl.fused_learner import _FusedA2C, _Kind, _parts


def _per_member(name, value, P):
    """a scalar or a sequence of P numbers as a list of P floats"""
    if isinstance(value, (int, float, np.floating, np.integer)):
        return [float(value)] * P
    values = [float(v) for v in value]
    if len(values) != P:
        raise ValueError(f'{name}: {len(values)} values for {P} agents (a scalar, or one value per agent)')
    return values


class FusedA2CPopulation(_FusedA2C):
    """`FusedA2CLearner` for a list of agents that learn side by side, each from its own envs.

    Args:
        agents: P `FeedforwardAgent`s that `pack_policy_params` accepts, all with the same number of inputs
        lr, gamma, entropy_coef, gae_lambda: a scalar, or a sequence of P (one per agent)
        max_grad_norm, betas, eps, value_loss, use_gae: shared, as FusedA2CLearner's
    Return normalisation is not offered (FusedA2CLearner explains why).
    `lr`, `gamma`, `entropy_coef` and `gae_lambda` remain the values the population was built with; `hyperparameters()`
    gives the current ones, which `exploit` changes.
    `grad`, `apply` and `update` take and return what FusedA2CLearner's do with a leading member dimension: `grad`
    (P, num_params), the losses and `grad_norm` (P,); state and out are what a `policy_rollout(..., population=P)` started
    from and returned, (N, ...) and (T, N, ...).
    """
    _WHOSE, _LOSS_INDEX = 'agents', tuple((slice(None), i) for i in range(3))
    _STATE_TENSORS, _STATE_NUMBERS = _FusedA2C._STATE_TENSORS + ('hyper',), _FusedA2C._STATE_NUMBERS + ('generation',)

    def __init__(self, agents, lr=1e-3, gamma=0.99, entropy_coef=0.0, max_grad_norm: float = 0.5, betas=(0.9, 0.999),
                 eps: float = 1e-8, value_loss: str = 'smooth_l1', use_gae: bool = False, gae_lambda=None):
        agents = list(agents)
        P = len(agents)
        if P == 0:
            raise ValueError('FusedA2CPopulation needs at least one agent')
        super().__init__(agents, lr, gamma, entropy_coef, max_grad_norm, betas, eps, value_loss, use_gae, gae_lambda)
        self.agents = agents
        self.num_members = P
        self._losses_shape, self._norm_shape = (P, 3), (P,)
        # gamma * lambda is one Python float per member, rounded once (FusedA2CLearner.gamma_lambda)
        self.gamma_lambda = [float(np.float32(g * l)) for g, l in zip(self.gamma, self.gae_lambda)] if use_gae else None
        # the hyper-parameter table (P, 4) of doubles: filled by the library on the host, copied to the device ONCE
        f32 = lambda values: (ctypes.c_float * P)(*values)
        table = np.zeros((P, 4), dtype=np.float64)
        values = {'lr': f32(self.lr), 'gamma': f32(self.gamma), 'entropy_coef': f32(self.entropy_coef),
                  'gamma_lambda': f32(self.gamma_lambda) if use_gae else None, 'num_members': P, 'table': table.ctypes.data}
        _lib.check(_lib.call_named(None, _lib.lib().wurm_a2c_ff_pop_hyper, values), 'FusedA2CPopulation: lr / gae_lambda')
        self.hyper = torch.from_numpy(table).to(self.params.device)
        self.generation = 0  # the number of `exploit` calls so far: the counter of their random draws

    _own = staticmethod(_per_member)

    @staticmethod
    def _buffer(rows):
        if any(r.numel() != rows[0].numel() for r in rows):
            raise RuntimeError('the agents of a population must all have the same num_inputs')
        if any(r.device != rows[0].device for r in rows):
            raise RuntimeError('the agents of a population must all be on the same device')
        return torch.stack(rows).contiguous()  # (P, num_params)

    def _check_envs(self, N):
        if N % self.num_members != 0:
            raise RuntimeError(f'{N} envs do not divide into {self.num_members} members')

    # ------------------------------------------------------------------ learning from a league window

    def _kind(self, plan, learn, what):
        """The kind of a call: the population's without a plan, else the league's with the checked plan and `learn` (as
        bytes).  Both read a member's lr, gamma, entropy_coef and gamma_lambda from its row of the table."""
        name = f'{type(self).__name__}.{what}'
        names = {'hyper': self.hyper.data_ptr(), 'num_members': self.num_members}
        if plan is None:
            if learn is not None:
                raise RuntimeError(f'{name}: learn goes with a plan (without one every member learns)')
            return _Kind('wurm_a2c_ff_pop_', self._check_envs, torch.empty, names, None)
        from wurm_amd.envs._multi_league import LeaguePlan
        if not isinstance(plan, LeaguePlan):
            raise RuntimeError(f'{name}: plan must come from league_plan, got {type(plan).__name__}')
        P, dev = self.num_members, self.params.device
        if plan.num_policies != P:
            raise RuntimeError(f'{name}: the plan names {plan.num_policies} policies but the population has {P} members')
        if learn is not None:
            if not isinstance(learn, torch.Tensor) or tuple(learn.shape) != (P,) or \
                    learn.dtype not in (torch.bool, torch.uint8):
                got = f'{tuple(learn.shape)} {learn.dtype}' if isinstance(learn, torch.Tensor) else type(learn).__name__
                raise RuntimeError(f'{name}: learn must be a ({P},) bool or uint8 tensor, got {got}')
        if dev.type != 'cuda':
            raise _lib.WurmHipError(f'{name} runs on the GPU: move the agents to the device first')
        if plan.order.device != dev:
            raise RuntimeError(f'{name}: the plan is on {plan.order.device}, the agents on {dev}')
        if learn is not None:
            if learn.device != dev:
                raise RuntimeError(f'{name}: learn is on {learn.device}, the agents on {dev}')
            learn = learn.contiguous().view(torch.uint8)
        rows = plan.order.numel()
        names.update(order=plan.order.data_ptr(), offsets=plan.offsets.data_ptr(), learn=_lib.ptr(learn), num_rows=rows)

        def check(N):
            if rows != N:
                raise RuntimeError(f'the window has {N} columns, the plan {rows} rows (num_snakes x num_envs)')
        # (a league writes only the columns of the members that learn: the rest stay zeros)
        return _Kind('wurm_a2c_ff_league_', check, torch.zeros, names, learn)

    def grad(self, state: torch.Tensor, out: dict, plan=None, learn=None):
        """FusedA2CLearner.grad for every member.  With `plan`, a `LeaguePlan` of `num_members` policies (MultiSnake.
        league_plan), the window is a league's: `out` what `league_window` returned, (T, K N, ...) tensors whose column
        k N + i is snake k of env i, and `state` the observations it started from, the dict of K (N, ...) tensors that
        `reset`, `step` and the window's 'state' are, or a (K, N, ...) tensor.  Member
        a learns from the columns the plan gives policy a, however many (include/wurm_hip.h: wurm_a2c_ff_league_*): its
        results are bit for bit those of a FusedA2CLearner on copies of these columns in the plan's order.
        learn: (P,) bool / uint8 device tensor or None; a member with learn[a] == 0, like one without columns, gets
        zeros for its `grad`, losses and `grad_norm`, and `update` / `apply` leave its weights and Adam state alone.
        `values` / `returns` are (T, K N), zeros in the columns of such members."""
        state = self._rows(state, plan)
        return self._grad(self._kind(plan, learn, 'grad'), state, out)

    def update(self, state: torch.Tensor, out: dict, plan=None, learn=None) -> dict:
        """FusedA2CLearner.update for every member, in three launches; `plan` and `learn` as for `grad`.  `step` is
        shared: it advances for every member, also for one that sits this window out, whose next Adam step then has the
        bias corrections of the shared count."""
        state = self._rows(state, plan)
        return self._update(self._kind(plan, learn, 'update'), state, out)

    def apply(self, grad: torch.Tensor, plan=None, learn=None) -> torch.Tensor:
        """FusedA2CLearner.apply for every member; with `plan` (and `learn`) only the members that `grad` let learn step"""
        return self._apply(self._kind(plan, learn, 'apply'), grad)

    @staticmethod
    def _rows(state, plan):
        """the observations a league window started from as ONE tensor whose rows are the columns k N + i: a (K, N, ...)
        tensor as it is; the dict `reset` / `step` / `league_window` return (agent_0 .. agent_{K-1}, (N, ...) each) in
        place when its tensors are consecutive views of one buffer (they are), else stacked once"""
        if plan is None or not isinstance(state, dict):
            return state
        vals = list(state.values())
        v0, rest = vals[0], vals[0][0].numel() if len(vals[0]) else 0
        step = 4 * v0.shape[0] * rest
        if all(v.is_contiguous() and v.dtype == torch.float32 and v.shape == v0.shape and
               v.data_ptr() == v0.data_ptr() + j * step for j, v in enumerate(vals)):
            return v0.as_strided((len(vals) * v0.shape[0], rest), (rest, 1))
        return torch.stack([v.reshape(v.shape[0], -1) for v in vals])

    def _moved(self):
        return any(_parts(a)[0].data_ptr() != row.data_ptr() for a, row in zip(self.agents, self.params))

    def _fits(self, grad):
        return grad.shape == self.params.shape

    @staticmethod
    def _per_agent(norm):
        return norm

    # ------------------------------------------------------------------ population-based training

    def exploit(self, scores: torch.Tensor, num_replace: int = None, fraction: float = 0.25, lr_factors=(0.8, 1.2),
                entropy_factors=(0.8, 1.2), lr_bounds=(0.0, math.inf), entropy_bounds=(0.0, math.inf),
                seed: int = 0) -> dict:
        """The exploit / explore step of population-based training, in two launches with nothing read back
        (include/wurm_hip.h: wurm_a2c_ff_pop_exploit): each of the worst `num_replace` members by `scores` takes the
        weights, the Adam state and the hyper-parameters of a member drawn from the best `num_replace`; its copied lr and
        entropy_coef are each multiplied by one of the two factors (a coin each) and clamped to the bounds.  Everyone
        else keeps everything.  The agents' modules are views of the rows and show the copied weights; `step` is shared
        and unchanged.

        scores: (P,) device tensor, higher is better, a NaN is worst — `stats.smooth[:, k]` of a
            `RolloutStats(env, population=P)`, say.  float64 is used as it is, float32 is converted on the device.
        num_replace: k, at most P // 2; default int(fraction * P).
        seed: of the draws, together with `self.generation`, which counts the calls (it starts at 0).
        Returns {'order': (P,) int32, the members best to worst, 'parent': (P,) int32, whose weights member p now has
        (p itself unless it was replaced)}, both on the device."""
        P = self.num_members
        k = int(fraction * P) if num_replace is None else int(num_replace)
        if k < 0 or 2 * k > P:
            raise ValueError(f'num_replace must lie in [0, {P // 2}] for {P} members, got {k}')
        if scores.shape != (P,) or scores.dtype not in (torch.float64, torch.float32):
            raise RuntimeError(f'scores must be a ({P},) float64 or float32 tensor, got {tuple(scores.shape)} '
                               f'{scores.dtype}')
        dev = self.params.device
        if dev.type != 'cuda':
            raise _lib.WurmHipError('FusedA2CPopulation.exploit runs on the GPU: move the agents to the device first')
        if scores.device != dev:
            raise RuntimeError(f'scores must be on the device of the agents ({dev})')
        # (no `_moved()` here: it walks the P agents on the host, which at P = 256 costs a hundred times the two kernels;
        # the next `update` makes that check and raises)
        scores = scores.to(torch.float64).contiguous()
        order = torch.empty(P, dtype=torch.int32, device=dev)
        parent = torch.empty(P, dtype=torch.int32, device=dev)
        perturb = (ctypes.c_double * 8)(lr_factors[0], lr_factors[1], lr_bounds[0], lr_bounds[1], entropy_factors[0],
                                        entropy_factors[1], entropy_bounds[0], entropy_bounds[1])
        rc = _lib.call(dev.index, _lib.lib().wurm_a2c_ff_pop_exploit, _lib.ptr(self.params), _lib.ptr(self.exp_avg),
                       _lib.ptr(self.exp_avg_sq), _lib.ptr(self.hyper), _lib.ptr(scores), _lib.ptr(order),
                       _lib.ptr(parent), _lib.i64(self.params.shape[1]), _lib.i64(P), _lib.i64(k),
                       ctypes.addressof(perturb), _lib.u64(seed), _lib.i64(self.generation), _lib.stream_ptr(dev.index))
        _lib.check(rc, 'FusedA2CPopulation.exploit: lr_factors / entropy_factors / lr_bounds / entropy_bounds')
        self.generation += 1
        return {'order': order, 'parent': parent}

    def hyperparameters(self) -> dict:
        """The members' CURRENT hyper-parameters, the one host copy of the table: {'lr', 'gamma', 'entropy_coef'} and,
        with GAE, 'gae_lambda', each a list of P floats.  The table holds gamma * gae_lambda rounded to float, so
        'gae_lambda' is that column divided by gamma (0 where gamma is 0): the constructor's value to float rounding.
        The attributes `lr`, `gamma`, `entropy_coef` and `gae_lambda` stay what the population was BUILT with; after an
        `exploit` they no longer describe the members, and this does."""
        lr, gamma, entropy_coef, gamma_lambda = self.hyper.t().cpu().tolist()
        res = {'lr': lr, 'gamma': gamma, 'entropy_coef': entropy_coef}
        if self.use_gae:
            res['gae_lambda'] = [gl / g if g else 0.0 for gl, g in zip(gamma_lambda, gamma)]
        return res
