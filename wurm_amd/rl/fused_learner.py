"""The learning half of the single-agent A2C experiment (experiments/main.py:207-245 with A2C(gamma) defaults) as three
kernel launches: `FusedA2CLearner.update(state, out)` takes what `env.policy_rollout` returned and leaves updated
weights, with no host synchronisation (include/wurm_hip.h: wurm_a2c_ff_update; wurm_amd/csrc/a2c_learner.hpp).

The agent's eight parameters are moved into ONE contiguous fp32 buffer in `pack_policy_params` order and become views
of it, so `learner.params` is directly the `params` argument of `policy_rollout` and the module always shows the
current weights.

Returns are the n-step ones of A2C(gamma) or, with `use_gae=True, gae_lambda=...`, generalised advantage estimates
(wurm/rl/a2c.py:50-59) with the gradient that flows through them into the value head, as the reference's undetached
`returns` have it (wurm_a2c_ff_grad_gae / wurm_a2c_ff_update_gae: the same three launches).  Return normalisation and a
custom value loss are not part of the fused path (NotImplementedError: keep wurm_amd.rl.A2C and torch for those):
normalised returns need the mean and the standard deviation of all N T returns between the scan and the backward pass,
which one workgroup per block of envs cannot know.
"""
import ctypes

import numpy as np
import torch

from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params

VALUE_LOSSES = {'smooth_l1': 0, 'mse': 1}


def _parts(agent):
    l1, l2 = agent.feedforward[0][0], agent.feedforward[1][0]
    return [l1.weight, l1.bias, l2.weight, l2.bias, agent.action_head.weight, agent.action_head.bias,
            agent.value_head.weight, agent.value_head.bias]


class FusedA2CLearner(object):
    """A2C loss, backward pass, clip_grad_norm_ and Adam of the 2 x 64 feed-forward actor-critic in HIP.

    Args:
        agent: a `FeedforwardAgent` that `pack_policy_params` accepts (2 layers, 64 units, 4 actions)
        lr, betas, eps: torch.optim.Adam's (no weight decay, no amsgrad)
        gamma: discount;  entropy_coef: weight of the mean entropy;  max_grad_norm: clip_grad_norm_'s (<= 0: none)
        value_loss: 'smooth_l1' (F.smooth_l1_loss, the reference's default) or 'mse'
        use_gae, gae_lambda: A2C's; `gae_lambda` is required with `use_gae` and ignored without it
    """

    def __init__(self, agent: FeedforwardAgent, lr: float = 1e-3, gamma: float = 0.99, entropy_coef: float = 0.0,
                 max_grad_norm: float = 0.5, betas=(0.9, 0.999), eps: float = 1e-8, value_loss: str = 'smooth_l1',
                 use_gae: bool = False, normalise_returns: bool = False, gae_lambda: float = None):
        if normalise_returns:
            raise NotImplementedError('the fused learner does not normalise returns: use wurm_amd.rl.A2C for that')
        if use_gae and gae_lambda is None:
            raise NotImplementedError('use_gae=True needs gae_lambda: pass FusedA2CLearner(..., gae_lambda=0.95)')
        if value_loss not in VALUE_LOSSES:
            raise NotImplementedError(f"value_loss {value_loss!r}: the fused learner has 'smooth_l1' and 'mse'")
        flat = pack_policy_params(agent)  # raises NotImplementedError for any other architecture
        self.agent = agent
        self.params = flat
        offset = 0
        for p in _parts(agent):  # the module's parameters become views of the one buffer
            n = p.numel()
            p.data = flat[offset:offset + n].view(p.shape)
            offset += n
        self.num_inputs = agent.feedforward[0][0].in_features
        self.lr, self.gamma, self.entropy_coef, self.max_grad_norm = float(lr), float(gamma), float(entropy_coef), float(max_grad_norm)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.value_loss = VALUE_LOSSES[value_loss]
        self.use_gae = bool(use_gae)
        self.gae_lambda = float(gae_lambda) if use_gae else None
        # gamma * lambda is one Python float in the reference (a2c.py:56), rounded once: as wurm_amd.rl.a2c_returns does
        self.gamma_lambda = float(np.float32(self.gamma * self.gae_lambda)) if use_gae else 0.0
        self.step = 0
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self._workspace = {}

    # ------------------------------------------------------------------ plumbing

    def _inputs(self, state, out):
        dev, E = self.params.device, self.num_inputs
        if dev.type != 'cuda':
            raise _lib.WurmHipError('FusedA2CLearner.grad / update run on the GPU: move the agent to the device first')
        obs, actions, rewards, dones = out['observations'], out['actions'], out['rewards'], out['dones']
        if rewards.dim() != 2 or rewards.numel() == 0:
            raise RuntimeError('rewards must be a non-empty (num_steps, num_envs) tensor')
        T, N = rewards.shape
        for name, t in (('state', state), ('observations', obs), ('actions', actions), ('rewards', rewards),
                        ('dones', dones)):
            if t.device != dev:
                raise RuntimeError(f'{name} must be on the device of the agent ({dev})')
        if state.numel() != N * E or obs.numel() != T * N * E or state.dtype != torch.float32 or \
                obs.dtype != torch.float32:
            raise RuntimeError(f'state / observations must be fp32 with {E} inputs per env ({N} envs, {T} steps)')
        if actions.shape != (T, N) or actions.dtype != torch.long:
            raise RuntimeError('actions must be a (num_steps, num_envs) int64 tensor')
        if rewards.dtype != torch.float32:
            raise RuntimeError('rewards must be fp32')
        if dones.shape != (T, N) or dones.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('dones must be a (num_steps, num_envs) bool tensor')
        if _parts(self.agent)[0].data_ptr() != self.params.data_ptr():
            raise RuntimeError('the agent was moved after the learner was built: its parameters left the buffer')
        key = (N, T, E)
        ws = self._workspace.get(key)
        if ws is None:
            nbytes = _lib.lib().wurm_a2c_ff_workspace_bytes(N, T, E)
            ws = self._workspace[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
        return (state.contiguous(), obs.contiguous(), actions.contiguous(), rewards.contiguous(), dones.contiguous(),
                ws, N, T)

    def _outputs(self, N, T):
        dev = self.params.device
        return (torch.empty_like(self.params), torch.empty(3, dtype=torch.float32, device=dev),
                torch.empty((T, N), dtype=torch.float32, device=dev),
                torch.empty((T, N), dtype=torch.float32, device=dev) if self.use_gae else None)

    @staticmethod
    def _losses(losses, values, returns):
        res = {'value_loss': losses[0], 'policy_loss': losses[1], 'entropy': losses[2], 'values': values}
        if returns is not None:
            res['returns'] = returns
        return res

    def _gae_args(self, returns):
        return (ctypes.c_float(self.gamma_lambda), _lib.ptr(returns)) if self.use_gae else ()

    # ------------------------------------------------------------------ the two calls

    def grad(self, state: torch.Tensor, out: dict):
        """(flat_grad, losses): the unclipped gradient of the loss in `pack_policy_params` order and a dict of 0-dim
        device tensors `value_loss`, `policy_loss`, `entropy` (+ `values`, (T, N): the value of every policy input; with
        GAE also `returns`, (T, N)).
        state: the observation the rollout started from; out: what `policy_rollout` returned (or any dict with
        `observations` (T,N,...), `actions`, `rewards`, `dones` (T,N))."""
        x0, obs, actions, rewards, dones, (ws, nbytes), N, T = self._inputs(state, out)
        grad, losses, values, returns = self._outputs(N, T)
        dev = self.params.device
        fn = _lib.lib().wurm_a2c_ff_grad_gae if self.use_gae else _lib.lib().wurm_a2c_ff_grad
        rc = _lib.call(dev.index, fn, _lib.ptr(self.params), _lib.ptr(x0), _lib.ptr(obs),
                       _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), ctypes.c_float(self.gamma),
                       ctypes.c_float(self.entropy_coef), self.value_loss, _lib.ptr(grad), _lib.ptr(losses),
                       _lib.ptr(values), _lib.ptr(ws), _lib.i64(nbytes), _lib.i64(N), _lib.i64(T), self.num_inputs,
                       _lib.stream_ptr(dev.index), *self._gae_args(returns))
        _lib.check(rc, 'FusedA2CLearner.grad')
        return grad, self._losses(losses, values, returns)

    def apply(self, grad: torch.Tensor) -> torch.Tensor:
        """clip_grad_norm_ + one Adam step on a flat gradient (not modified); returns its norm (0-dim device tensor)."""
        dev = self.params.device
        if dev.type != 'cuda':
            raise _lib.WurmHipError('FusedA2CLearner.apply runs on the GPU')
        if grad.device != dev or grad.dtype != torch.float32 or grad.numel() != self.params.numel() or \
                not grad.is_contiguous():
            raise RuntimeError('grad must be a contiguous fp32 device tensor with one element per parameter')
        norm = torch.empty(1, dtype=torch.float32, device=dev)
        rc = _lib.call(dev.index, _lib.lib().wurm_a2c_ff_apply, _lib.ptr(self.params), _lib.ptr(grad),
                       _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(norm), _lib.i64(self.step + 1),
                       ctypes.c_float(self.lr), ctypes.c_float(self.betas[0]), ctypes.c_float(self.betas[1]),
                       ctypes.c_float(self.eps), ctypes.c_float(self.max_grad_norm), _lib.i64(self.params.numel()),
                       _lib.stream_ptr(dev.index))
        _lib.check(rc, 'FusedA2CLearner.apply')
        self.step += 1
        return norm[0]

    def update(self, state: torch.Tensor, out: dict) -> dict:
        """One optimiser step from one rollout window: the losses of `grad` plus `grad_norm` (before clipping) and
        `grad` (unclipped), all device tensors — nothing is copied to the host."""
        x0, obs, actions, rewards, dones, (ws, nbytes), N, T = self._inputs(state, out)
        grad, losses, values, returns = self._outputs(N, T)
        dev = self.params.device
        norm = torch.empty(1, dtype=torch.float32, device=dev)
        fn = _lib.lib().wurm_a2c_ff_update_gae if self.use_gae else _lib.lib().wurm_a2c_ff_update
        rc = _lib.call(dev.index, fn, _lib.ptr(self.params), _lib.ptr(x0), _lib.ptr(obs),
                       _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), ctypes.c_float(self.gamma),
                       ctypes.c_float(self.entropy_coef), self.value_loss, _lib.ptr(grad), _lib.ptr(losses),
                       _lib.ptr(values), _lib.ptr(ws), _lib.i64(nbytes), _lib.i64(N), _lib.i64(T), self.num_inputs,
                       _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(norm), _lib.i64(self.step + 1),
                       ctypes.c_float(self.lr), ctypes.c_float(self.betas[0]), ctypes.c_float(self.betas[1]),
                       ctypes.c_float(self.eps), ctypes.c_float(self.max_grad_norm), _lib.stream_ptr(dev.index),
                       *self._gae_args(returns))
        _lib.check(rc, 'FusedA2CLearner.update')
        self.step += 1
        res = self._losses(losses, values, returns)
        res['grad_norm'] = norm[0]
        res['grad'] = grad
        return res
