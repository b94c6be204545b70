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
import collections

import numpy as np
import torch

from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params

VALUE_LOSSES = {'smooth_l1': 0, 'mse': 1}


def _parts(agent):
    l1, l2 = agent.feedforward[0][0], agent.feedforward[1][0]
    return [l1.weight, l1.bias, l2.weight, l2.bias, agent.action_head.weight, agent.action_head.bias,
            agent.value_head.weight, agent.value_head.bias]


# One of the three kinds of entry points, as a call sees it.  entry: the prefix of their names ('wurm_a2c_ff_', '..._pop_',
# '..._league_');  check(N): raises unless the kind takes a window of N columns;  new: torch.empty, or torch.zeros where
# the kernels leave columns of `values` / `returns` unwritten;  names: the values the kind adds under the header's
# parameter names;  keep: tensors made for this call whose addresses are among them
_Kind = collections.namedtuple('_Kind', 'entry check new names keep')
_any_envs = lambda N: None


class _FusedA2C(object):
    """What FusedA2CLearner and FusedA2CPopulation (fused_population.py) share: the constructor's refusals, the packing of
    the agents into one buffer, the checks of a rollout window, the output tensors and the marshalling of the three calls.
    A subclass says how its hyper-parameters are kept (`_own`), what one agent's part of `losses` and `grad_norm` is, and,
    at the top of `grad`, `apply` and `update`, which kind of entry points the call goes to (`_kind`: a `_Kind`).
    Every call hands the library ONE dict of values under the parameter names of include/wurm_hip.h (`_lib.call_named`):
    the header alone says in which order an entry point takes them."""
    _WHOSE = None       # 'agent' / 'agents', for the messages
    _LOSS_INDEX = None  # the three indices into `losses` that give value_loss, policy_loss and entropy

    def __init__(self, agents, lr, gamma, entropy_coef, max_grad_norm, betas, eps, value_loss, use_gae, gae_lambda):
        name, P = type(self).__name__, len(agents)
        if use_gae and gae_lambda is None:
            raise NotImplementedError(f'use_gae=True needs gae_lambda: pass {name}(..., gae_lambda=0.95)')
        if value_loss not in VALUE_LOSSES:
            raise NotImplementedError(f"value_loss {value_loss!r}: the fused learner has 'smooth_l1' and 'mse'")
        self.lr, self.gamma = self._own('lr', lr, P), self._own('gamma', gamma, P)
        self.entropy_coef = self._own('entropy_coef', entropy_coef, P)
        self.gae_lambda = self._own('gae_lambda', gae_lambda, P) if use_gae else None
        rows = [pack_policy_params(a) for a in agents]  # raises NotImplementedError for any other architecture
        self.params = self._buffer(rows)                # (num_params,) or (P, num_params)
        for row, agent in zip(self.params.view(P, -1), agents):  # every module's parameters become views of its row
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
        self.step = 0
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self._workspace = {}

    # ------------------------------------------------------------------ plumbing

    def _values(self, kind):
        """what an entry point of `kind` may ask for by name, the window and the outputs aside"""
        values = {'params': self.params.data_ptr(), 'exp_avg': self.exp_avg.data_ptr(),
                  'exp_avg_sq': self.exp_avg_sq.data_ptr(), 'step': self.step + 1, 'beta1': self.betas[0],
                  'beta2': self.betas[1], 'eps': self.eps, 'max_grad_norm': self.max_grad_norm,
                  'num_params': self.params.shape[-1], 'value_loss_kind': self.value_loss, 'num_inputs': self.num_inputs,
                  'stream': _lib.stream_ptr(self.params.device.index)}
        values.update(kind.names)
        return values

    def _window(self, kind, state, out):
        """(values, tensors): the checked rollout window, fresh outputs and the workspace on top of `_values`, and the
        tensors behind the addresses among them, by parameter name"""
        dev, E = self.params.device, self.num_inputs
        if dev.type != 'cuda':
            raise _lib.WurmHipError(f'{type(self).__name__}.grad / update run on the GPU: move the {self._WHOSE} to the '
                                    f'device first')
        obs, actions, rewards, dones = out['observations'], out['actions'], out['rewards'], out['dones']
        if rewards.dim() != 2 or rewards.numel() == 0:
            raise RuntimeError('rewards must be a non-empty (num_steps, num_envs) tensor')
        T, N = rewards.shape
        kind.check(N)
        for name, t in (('state', state), ('observations', obs), ('actions', actions), ('rewards', rewards),
                        ('dones', dones)):
            if t.device != dev:
                raise RuntimeError(f'{name} must be on the device of the {self._WHOSE} ({dev})')
        if state.numel() != N * E or obs.numel() != T * N * E or state.dtype != torch.float32 or \
                obs.dtype != torch.float32:
            raise RuntimeError(f'state / observations must be fp32 with {E} inputs per env ({N} envs, {T} steps)')
        if actions.shape != (T, N) or actions.dtype != torch.long:
            raise RuntimeError('actions must be a (num_steps, num_envs) int64 tensor')
        if rewards.dtype != torch.float32:
            raise RuntimeError('rewards must be fp32')
        if dones.shape != (T, N) or dones.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError('dones must be a (num_steps, num_envs) bool tensor')
        if self._moved():
            raise RuntimeError(f'an agent was moved after the {type(self).__name__} was built: its parameters left the '
                               f'buffer')
        values = self._values(kind)
        values['num_envs'], values['num_steps'] = N, T
        ws = self._workspace.get((kind.entry, N, T, E))
        if ws is None:
            nbytes = _lib.call_named(None, getattr(_lib.lib(), kind.entry + 'workspace_bytes'), values)
            ws = self._workspace[kind.entry, N, T, E] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
        new, f32 = kind.new, torch.float32
        tensors = {'obs0': state.contiguous(), 'obs': obs.contiguous(), 'actions': actions.contiguous(),
                   'rewards': rewards.contiguous(), 'dones': dones.contiguous(), 'workspace': ws[0],
                   'grad': torch.empty_like(self.params),
                   'losses': torch.empty(self._losses_shape, dtype=f32, device=dev),
                   'values_out': new((T, N), dtype=f32, device=dev),
                   'returns_out': new((T, N), dtype=f32, device=dev) if self.use_gae else None}
        values.update({name: _lib.ptr(t) for name, t in tensors.items()}, workspace_bytes=ws[1])
        return values, tensors

    def _call(self, kind, what, values):
        """the entry point `what` ('grad', 'apply', 'update') of `kind`, or its GAE form"""
        gae = '_gae' if self.use_gae and what != 'apply' else ''
        fn = getattr(_lib.lib(), kind.entry + what + gae)
        _lib.check(_lib.call_named(self.params.device.index, fn, values), f'{type(self).__name__}.{what}')

    def _losses(self, tensors):
        i, losses = self._LOSS_INDEX, tensors['losses']
        res = {'value_loss': losses[i[0]], 'policy_loss': losses[i[1]], 'entropy': losses[i[2]],
               'values': tensors['values_out']}
        if tensors['returns_out'] is not None:
            res['returns'] = tensors['returns_out']
        return res

    # ------------------------------------------------------------------ the calls

    def grad(self, state: torch.Tensor, out: dict):
        """(grad, losses): the unclipped gradient(s) of the loss, of the shape of `params` in `pack_policy_params` order,
        and a dict of device tensors `value_loss`, `policy_loss`, `entropy` — 0-dim for FusedA2CLearner, (P,) for
        FusedA2CPopulation — plus `values`, (T, N): the value of every policy input, and with GAE `returns`, (T, N).
        state: the observation the rollout started from, (N, ...); out: what `policy_rollout` returned (or any dict
        with `observations` (T, N, ...), `actions`, `rewards`, `dones` (T, N))."""
        return self._grad(self._kind(), state, out)

    def _grad(self, kind, state, out):
        values, tensors = self._window(kind, state, out)
        self._call(kind, 'grad', values)
        return tensors['grad'], self._losses(tensors)

    def apply(self, grad: torch.Tensor) -> torch.Tensor:
        """clip_grad_norm_ + one Adam step of every agent on a gradient of the shape of `params` (not modified); returns
        its norm (device tensor: 0-dim for FusedA2CLearner, (P,) for FusedA2CPopulation)."""
        return self._apply(self._kind(), grad)

    def _apply(self, kind, grad):
        dev = self.params.device
        if dev.type != 'cuda':
            raise _lib.WurmHipError(f'{type(self).__name__}.apply runs on the GPU')
        if grad.device != dev or grad.dtype != torch.float32 or not self._fits(grad) or not grad.is_contiguous():
            raise RuntimeError(f'grad must be a contiguous fp32 device tensor that matches params '
                               f'{tuple(self.params.shape)}')
        norm = torch.empty(self._norm_shape, dtype=torch.float32, device=dev)
        values = self._values(kind)
        values['grad'], values['grad_norm'] = grad.data_ptr(), norm.data_ptr()
        self._call(kind, 'apply', values)
        self.step += 1
        return self._per_agent(norm)

    def update(self, state: torch.Tensor, out: dict) -> dict:
        """One optimiser step of every agent from one rollout window, in three launches: the losses of `grad` plus
        `grad_norm` (before clipping) and `grad` (unclipped), all device tensors — nothing is copied to the host."""
        return self._update(self._kind(), state, out)

    def _update(self, kind, state, out):
        values, tensors = self._window(kind, state, out)
        norm = torch.empty(self._norm_shape, dtype=torch.float32, device=self.params.device)
        values['grad_norm'] = norm.data_ptr()
        self._call(kind, 'update', values)
        self.step += 1
        res = self._losses(tensors)
        res['grad_norm'] = self._per_agent(norm)
        res['grad'] = tensors['grad']
        return res

    # ------------------------------------------------------------------ checkpoints

    _STATE_TENSORS = ('params', 'exp_avg', 'exp_avg_sq')  # (the population adds its hyper-parameter table)
    _STATE_NUMBERS = ('step',)                            # (and its generation)

    def state_dict(self) -> dict:
        """Clones of the weights and the Adam state, plus `step` (FusedA2CPopulation: also the hyper-parameter table
        `hyper` and `generation`): what `load_state_dict` of a learner built the same way needs to go on bit for bit.
        The constructor's arguments are not part of it.  Works on CPU tensors too: no kernel is involved."""
        state = {name: getattr(self, name).clone() for name in self._STATE_TENSORS}
        state.update((name, getattr(self, name)) for name in self._STATE_NUMBERS)
        return state

    def load_state_dict(self, state: dict):
        """Copies a `state_dict()` IN PLACE: the modules' parameters stay views of `params` and show the loaded weights.
        Every shape and dtype is checked before anything is copied (RuntimeError, nothing changed)."""
        for name in self._STATE_TENSORS:
            mine, theirs = getattr(self, name), state[name]
            if theirs.shape != mine.shape or theirs.dtype != mine.dtype:
                raise RuntimeError(f'{name}: expected {tuple(mine.shape)} {mine.dtype}, got {tuple(theirs.shape)} '
                                   f'{theirs.dtype}')
        numbers = {name: int(state[name]) for name in self._STATE_NUMBERS}
        if any(v < 0 for v in numbers.values()):
            raise RuntimeError(f'{self._STATE_NUMBERS} must not be negative, got {numbers}')
        for name in self._STATE_TENSORS:
            getattr(self, name).copy_(state[name])
        for name, value in numbers.items():
            setattr(self, name, value)


class FusedA2CLearner(_FusedA2C):
    """A2C loss, backward pass, clip_grad_norm_ and Adam of the 2 x 64 feed-forward actor-critic in HIP.

    Args:
        agent: a `FeedforwardAgent` that `pack_policy_params` accepts (2 layers, 64 units, 4 actions)
        lr, betas, eps: torch.optim.Adam's (no weight decay, no amsgrad)
        gamma: discount;  entropy_coef: weight of the mean entropy;  max_grad_norm: clip_grad_norm_'s (<= 0: none)
        value_loss: 'smooth_l1' (F.smooth_l1_loss, the reference's default) or 'mse'
        use_gae, gae_lambda: A2C's; `gae_lambda` is required with `use_gae` and ignored without it
    """
    _WHOSE, _LOSS_INDEX, _losses_shape, _norm_shape = 'agent', (0, 1, 2), (3,), (1,)

    def __init__(self, agent: FeedforwardAgent, lr: float = 1e-3, gamma: float = 0.99, entropy_coef: float = 0.0,
                 max_grad_norm: float = 0.5, betas=(0.9, 0.999), eps: float = 1e-8, value_loss: str = 'smooth_l1',
                 use_gae: bool = False, normalise_returns: bool = False, gae_lambda: float = None):
        if normalise_returns:
            raise NotImplementedError('the fused learner does not normalise returns: use wurm_amd.rl.A2C for that')
        super().__init__([agent], lr, gamma, entropy_coef, max_grad_norm, betas, eps, value_loss, use_gae, gae_lambda)
        self.agent = agent
        # gamma * lambda is one Python float in the reference (a2c.py:56), rounded once: as wurm_amd.rl.a2c_returns does
        self.gamma_lambda = float(np.float32(self.gamma * self.gae_lambda)) if use_gae else 0.0

    @staticmethod
    def _own(name, value, P):
        return float(value)

    @staticmethod
    def _buffer(rows):
        return rows[0]

    def _moved(self):
        return _parts(self.agent)[0].data_ptr() != self.params.data_ptr()

    def _fits(self, grad):
        return grad.numel() == self.params.numel()

    @staticmethod
    def _per_agent(norm):
        return norm[0]

    def _kind(self):
        # the stand-alone entry points take any number of envs, and the hyper-parameters by value as they are at this call
        return _Kind('wurm_a2c_ff_', _any_envs, torch.empty, {'gamma': self.gamma, 'entropy_coef': self.entropy_coef,
                                                              'lr': self.lr, 'gamma_lambda': self.gamma_lambda}, None)
