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
from wurm_amd.agents import pack_policy_params
from wurm_amd.rl.fused_learner import VALUE_LOSSES, _parts


def _per_member(name, value, P):
    """a scalar or a sequence of P numbers as a list of P floats"""
    if isinstance(value, (int, float, np.floating, np.integer)):
        return [float(value)] * P
    values = [float(v) for v in value]
    if len(values) != P:
        raise ValueError(f'{name}: {len(values)} values for {P} agents (a scalar, or one value per agent)')
    return values


class FusedA2CPopulation(object):
    """`FusedA2CLearner` for a list of agents that learn side by side, each from its own envs.

    Args:
        agents: P `FeedforwardAgent`s that `pack_policy_params` accepts, all with the same number of inputs
        lr, gamma, entropy_coef, gae_lambda: a scalar, or a sequence of P (one per agent)
        max_grad_norm, betas, eps, value_loss, use_gae: shared, as FusedA2CLearner's
    Return normalisation is not offered (FusedA2CLearner explains why).
    """

    def __init__(self, agents, lr=1e-3, gamma=0.99, entropy_coef=0.0, max_grad_norm: float = 0.5, betas=(0.9, 0.999),
                 eps: float = 1e-8, value_loss: str = 'smooth_l1', use_gae: bool = False, gae_lambda=None):
        agents = list(agents)
        P = len(agents)
        if P == 0:
            raise ValueError('FusedA2CPopulation needs at least one agent')
        if use_gae and gae_lambda is None:
            raise NotImplementedError('use_gae=True needs gae_lambda: pass FusedA2CPopulation(..., gae_lambda=0.95)')
        if value_loss not in VALUE_LOSSES:
            raise NotImplementedError(f"value_loss {value_loss!r}: the fused learner has 'smooth_l1' and 'mse'")
        self.lr = _per_member('lr', lr, P)
        self.gamma = _per_member('gamma', gamma, P)
        self.entropy_coef = _per_member('entropy_coef', entropy_coef, P)
        self.gae_lambda = _per_member('gae_lambda', gae_lambda, P) if use_gae else None
        rows = [pack_policy_params(a) for a in agents]  # raises NotImplementedError for any other architecture
        if any(r.numel() != rows[0].numel() for r in rows):
            raise RuntimeError('the agents of a population must all have the same num_inputs')
        if any(r.device != rows[0].device for r in rows):
            raise RuntimeError('the agents of a population must all be on the same device')
        self.agents = agents
        self.num_members = P
        self.params = torch.stack(rows).contiguous()  # (P, num_params)
        for row, agent in zip(self.params, agents):   # every module's parameters become views of its row
            offset = 0
            for p in _parts(agent):
                n = p.numel()
                p.data = row[offset:offset + n].view(p.shape)
                offset += n
        self.num_inputs = agents[0].feedforward[0][0].in_features
        self.max_grad_norm = float(max_grad_norm)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.value_loss = VALUE_LOSSES[value_loss]
        self.use_gae = bool(use_gae)
        # gamma * lambda is one Python float per member, rounded once (FusedA2CLearner.gamma_lambda)
        self.gamma_lambda = [float(np.float32(g * l)) for g, l in zip(self.gamma, self.gae_lambda)] if use_gae else None
        self.step = 0
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self._workspace = {}
        # the hyper-parameter table (P, 4) of doubles: filled by the library on the host, copied to the device ONCE
        f32 = lambda values: (ctypes.c_float * P)(*values)
        table = np.zeros((P, 4), dtype=np.float64)
        columns = [f32(self.lr), f32(self.gamma), f32(self.entropy_coef), f32(self.gamma_lambda) if use_gae else None]
        rc = _lib.lib().wurm_a2c_ff_pop_hyper(*[ctypes.addressof(c) if c is not None else None for c in columns],
                                              _lib.i64(P), table.ctypes.data)
        _lib.check(rc, 'FusedA2CPopulation: lr / gae_lambda')
        self.hyper = torch.from_numpy(table).to(self.params.device)

    # ------------------------------------------------------------------ plumbing

    def _inputs(self, state, out):
        dev, E, P = self.params.device, self.num_inputs, self.num_members
        if dev.type != 'cuda':
            raise _lib.WurmHipError('FusedA2CPopulation.grad / update run on the GPU: move the agents to the device first')
        obs, actions, rewards, dones = out['observations'], out['actions'], out['rewards'], out['dones']
        if rewards.dim() != 2 or rewards.numel() == 0:
            raise RuntimeError('rewards must be a non-empty (num_steps, num_envs) tensor')
        T, N = rewards.shape
        if N % P != 0:
            raise RuntimeError(f'{N} envs do not divide into {P} members')
        for name, t in (('state', state), ('observations', obs), ('actions', actions), ('rewards', rewards),
                        ('dones', dones)):
            if t.device != dev:
                raise RuntimeError(f'{name} must be on the device of the agents ({dev})')
        if state.numel() != N * E or obs.numel() != T * N * E or state.dtype != torch.float32 or \
                obs.dtype != torch.float32:
            raise RuntimeError(f'state / observations must be fp32 with {E} inputs per env ({N} envs, {T} steps)')
        if actions.shape != (T, N) or actions.dtype != torch.long:
            raise RuntimeError('actions must be a (num_steps, num_envs) int64 tensor')
        if rewards.dtype != torch.float32:
            raise RuntimeError('rewards must be fp32')
        if dones.shape != (T, N) or dones.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('dones must be a (num_steps, num_envs) bool tensor')
        if any(_parts(a)[0].data_ptr() != row.data_ptr() for a, row in zip(self.agents, self.params)):
            raise RuntimeError('an agent was moved after the population was built: its parameters left the buffer')
        key = (N, T, E)
        ws = self._workspace.get(key)
        if ws is None:
            nbytes = _lib.lib().wurm_a2c_ff_pop_workspace_bytes(N, T, E, P)
            ws = self._workspace[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
        return (state.contiguous(), obs.contiguous(), actions.contiguous(), rewards.contiguous(), dones.contiguous(),
                ws, N, T)

    def _outputs(self, N, T):
        dev, P = self.params.device, self.num_members
        return (torch.empty_like(self.params), torch.empty((P, 3), dtype=torch.float32, device=dev),
                torch.empty((T, N), dtype=torch.float32, device=dev),
                torch.empty((T, N), dtype=torch.float32, device=dev) if self.use_gae else None)

    @staticmethod
    def _losses(losses, values, returns):
        res = {'value_loss': losses[:, 0], 'policy_loss': losses[:, 1], 'entropy': losses[:, 2], 'values': values}
        if returns is not None:
            res['returns'] = returns
        return res

    def _grad_args(self, x0, obs, actions, rewards, dones, grad, losses, values, ws, nbytes, N, T):
        return (_lib.ptr(self.params), _lib.ptr(x0), _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones),
                _lib.ptr(self.hyper), self.value_loss, _lib.ptr(grad), _lib.ptr(losses), _lib.ptr(values), _lib.ptr(ws),
                _lib.i64(nbytes), _lib.i64(N), _lib.i64(T), self.num_inputs, _lib.i64(self.num_members))

    def _apply_args(self, norm):
        return (_lib.ptr(norm), _lib.i64(self.step + 1), ctypes.c_float(self.betas[0]), ctypes.c_float(self.betas[1]),
                ctypes.c_float(self.eps), ctypes.c_float(self.max_grad_norm))

    # ------------------------------------------------------------------ the calls

    def grad(self, state: torch.Tensor, out: dict):
        """(grad, losses): the unclipped gradients (P, num_params), rows in `pack_policy_params` order, and a dict of
        (P,) device tensors `value_loss`, `policy_loss`, `entropy` (+ `values` (T, N); with GAE also `returns` (T, N)).
        state, out: what a `policy_rollout(..., population=P)` started from and returned — (N, ...) and (T, N, ...)."""
        x0, obs, actions, rewards, dones, (ws, nbytes), N, T = self._inputs(state, out)
        grad, losses, values, returns = self._outputs(N, T)
        dev = self.params.device
        fn = _lib.lib().wurm_a2c_ff_pop_grad_gae if self.use_gae else _lib.lib().wurm_a2c_ff_pop_grad
        rc = _lib.call(dev.index, fn, *self._grad_args(x0, obs, actions, rewards, dones, grad, losses, values, ws,
                                                       nbytes, N, T),
                       _lib.stream_ptr(dev.index), *((_lib.ptr(returns),) if self.use_gae else ()))
        _lib.check(rc, 'FusedA2CPopulation.grad')
        return grad, self._losses(losses, values, returns)

    def apply(self, grad: torch.Tensor) -> torch.Tensor:
        """clip_grad_norm_ + one Adam step of every member on its row of `grad` (P, num_params; not modified); returns
        the P norms (device tensor)."""
        dev = self.params.device
        if dev.type != 'cuda':
            raise _lib.WurmHipError('FusedA2CPopulation.apply runs on the GPU')
        if grad.device != dev or grad.dtype != torch.float32 or grad.shape != self.params.shape or \
                not grad.is_contiguous():
            raise RuntimeError('grad must be a contiguous fp32 (num_members, num_params) device tensor')
        norm = torch.empty(self.num_members, dtype=torch.float32, device=dev)
        args = self._apply_args(norm)
        rc = _lib.call(dev.index, _lib.lib().wurm_a2c_ff_pop_apply, _lib.ptr(self.params), _lib.ptr(grad),
                       _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), args[0], _lib.ptr(self.hyper), *args[1:],
                       _lib.i64(self.params.shape[1]), _lib.i64(self.num_members), _lib.stream_ptr(dev.index))
        _lib.check(rc, 'FusedA2CPopulation.apply')
        self.step += 1
        return norm

    def update(self, state: torch.Tensor, out: dict) -> dict:
        """One optimiser step of every member from one population rollout window, in three launches: the losses of
        `grad` plus `grad_norm` (P,) (before clipping) and `grad` (P, num_params) (unclipped), all device tensors."""
        x0, obs, actions, rewards, dones, (ws, nbytes), N, T = self._inputs(state, out)
        grad, losses, values, returns = self._outputs(N, T)
        dev = self.params.device
        norm = torch.empty(self.num_members, dtype=torch.float32, device=dev)
        fn = _lib.lib().wurm_a2c_ff_pop_update_gae if self.use_gae else _lib.lib().wurm_a2c_ff_pop_update
        rc = _lib.call(dev.index, fn, *self._grad_args(x0, obs, actions, rewards, dones, grad, losses, values, ws,
                                                       nbytes, N, T),
                       _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), *self._apply_args(norm),
                       _lib.stream_ptr(dev.index), *((_lib.ptr(returns),) if self.use_gae else ()))
        _lib.check(rc, 'FusedA2CPopulation.update')
        self.step += 1
        res = self._losses(losses, values, returns)
        res['grad_norm'] = norm
        res['grad'] = grad
        return res
