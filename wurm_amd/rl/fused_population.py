"""P independent A2C learners in the three launches of one (include/wurm_hip.h: wurm_a2c_ff_pop_*): the sweep over
seeds and hyper-parameters that experiments/main.py is run for (`--r`, `--lr`, `--gamma`, `--entropy`), as one env
object, one `policy_rollout(..., population=P)` and one `FusedA2CPopulation.update` per window.

Member p owns the envs [p M, (p + 1) M) of the N = P M envs, row p of the (P, num_params) buffers `params`, `exp_avg`
and `exp_avg_sq`, and its own lr, gamma, entropy_coef and gae_lambda.  Every result of member p is bit for bit what a
`FusedA2CLearner` of its own computes from contiguous copies of its columns: its part of the grid is the grid of that
stand-alone update.  The per-member hyper-parameters live in a small device table built once, here; an update copies
nothing to the device and reads nothing back.
"""
import ctypes

import numpy as np
import torch

from wurm_amd import _lib
from wurm_amd.rl.fused_learner import _FusedA2C, _parts


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
    `grad`, `apply` and `update` take and return what FusedA2CLearner's do with a leading member dimension: `grad`
    (P, num_params), the losses and `grad_norm` (P,); state and out are what a `policy_rollout(..., population=P)` started
    from and returned, (N, ...) and (T, N, ...).
    """
    _ENTRY, _WHOSE, _LOSS_INDEX = 'wurm_a2c_ff_pop_', 'agents', tuple((slice(None), i) for i in range(3))

    def __init__(self, agents, lr=1e-3, gamma=0.99, entropy_coef=0.0, max_grad_norm: float = 0.5, betas=(0.9, 0.999),
                 eps: float = 1e-8, value_loss: str = 'smooth_l1', use_gae: bool = False, gae_lambda=None):
        agents = list(agents)
        P = len(agents)
        if P == 0:
            raise ValueError('FusedA2CPopulation needs at least one agent')
        super().__init__(agents, lr, gamma, entropy_coef, max_grad_norm, betas, eps, value_loss, use_gae, gae_lambda)
        self.agents = agents
        self.num_members = P
        self._members, self._losses_shape, self._norm_shape = (P,), (P, 3), (P,)
        # gamma * lambda is one Python float per member, rounded once (FusedA2CLearner.gamma_lambda)
        self.gamma_lambda = [float(np.float32(g * l)) for g, l in zip(self.gamma, self.gae_lambda)] if use_gae else None
        # the hyper-parameter table (P, 4) of doubles: filled by the library on the host, copied to the device ONCE
        f32 = lambda values: (ctypes.c_float * P)(*values)
        table = np.zeros((P, 4), dtype=np.float64)
        columns = [f32(self.lr), f32(self.gamma), f32(self.entropy_coef), f32(self.gamma_lambda) if use_gae else None]
        rc = _lib.lib().wurm_a2c_ff_pop_hyper(*[ctypes.addressof(c) if c is not None else None for c in columns],
                                              _lib.i64(P), table.ctypes.data)
        _lib.check(rc, 'FusedA2CPopulation: lr / gae_lambda')
        self.hyper = torch.from_numpy(table).to(self.params.device)

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

    def _moved(self):
        return any(_parts(a)[0].data_ptr() != row.data_ptr() for a, row in zip(self.agents, self.params))

    def _workspace_bytes(self, N, T, E):
        return _lib.lib().wurm_a2c_ff_pop_workspace_bytes(N, T, E, self.num_members)

    def _fits(self, grad):
        return grad.shape == self.params.shape

    @staticmethod
    def _per_agent(norm):
        return norm

    # the population entry points read a member's lr, gamma, entropy_coef and gamma_lambda from its row of the table
    def _loss_args(self):
        return (_lib.ptr(self.hyper),)

    def _step_args(self, apply):
        return (_lib.ptr(self.hyper), self.step + 1) if apply else (self.step + 1,)

    def _gae_args(self, returns):
        return (_lib.ptr(returns),) if self.use_gae else ()
