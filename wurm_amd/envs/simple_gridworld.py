"""SimpleGridworld — drop-in for the reference's wurm.envs.SimpleGridworld (wurm/envs/simple_gridworld.py:15-271)
on the gfx950 kernels of include/wurm_hip.h.  State `envs` is (num_envs, 2, size, size) fp32 = [food, agent].
Deviations are the ones listed in wurm_amd/envs/single_snake.py.  Per-call path: one launch per `step(a); reset(done)`
iteration, see wurm_amd/envs/_fast_step.py."""
from collections import namedtuple
from typing import Tuple

import torch

from wurm_amd import _lib
from wurm_amd.constants import DEFAULT_DEVICE
from wurm_amd.envs._fast_step import FastStepMixin
from wurm_amd.envs.single_snake import _draw_seed

Spec = namedtuple('Spec', ['reward_threshold'])


class SimpleGridworld(FastStepMixin):
    """Batched gridworld: the agent moves in the 4 cardinal directions, +1 reward on a food square (which then
    respawns), moving on to the border ring ends the episode (reference simple_gridworld.py:16-42)."""

    _CHANNELS = 2
    _NAME = 'SimpleGridworld'
    _STEP_SLOT = 'wurm_grid_step_slot'
    _ROLLOUT_FNS = ('wurm_grid_rollout', 'wurm_grid_rollout_resident')
    _POLICY_FN = 'wurm_grid_policy_rollout'
    _POLICY_POP_FN = 'wurm_grid_policy_rollout_pop'
    _FRAMES_FN = 'wurm_grid_rollout_frames'
    _FLAG_KEYS = ('dones', 'edge_collision')
    _BAD_STATUS = 'some envs do not hold exactly one agent and one food'
    _RESIDENT_FNS = ('wurm_grid_resident_bytes', 'wurm_grid_resident_size', 'wurm_grid_resident_flush')

    spec = Spec(float('inf'))

    def __init__(self,
                 num_envs: int,
                 size: int,
                 on_death: str = 'restart',
                 observation_mode: str = 'default',
                 device: str = DEFAULT_DEVICE,
                 start_location: Tuple[int, int] = None,
                 manual_setup: bool = False,
                 verbose: int = 0,
                 seed: int = None,
                 env_offset: int = 0,
                 lazy_reset: bool = True,
                 resident_mirror=None):
        # (`resident_mirror`: as SingleSnake's — large batches step on a mirror of one 32-bit record per env,
        # wurm_grid_resident_bytes, include/wurm_hip.h; `env.mirror_state()` tells what is in effect)
        self._resident_policy = resident_mirror
        self.num_envs = num_envs
        self.size = size
        self.on_death = on_death
        self.observation_mode = observation_mode
        self.start_location = start_location
        self.device = _lib.require_device(device)
        self.verbose = verbose
        self.seed = _draw_seed() if seed is None else int(seed)
        self.env_offset = int(env_offset)
        self.lazy_reset = bool(lazy_reset)
        self._mode_cache = {}
        self._fast_init()

        self.t = 0

        if not manual_setup:
            self._reset(torch.ones(num_envs, dtype=torch.bool, device=self.device), observe=False)

        self.viewer = None

        self.head_colour = torch.tensor((0, 255, 0), dtype=torch.short, device=self.device)
        self.food_colour = torch.tensor((255, 0, 0), dtype=torch.short, device=self.device)
        self.edge_colour = torch.tensor((0, 0, 0), dtype=torch.short, device=self.device)

    @property
    def start_location(self):
        return self._start_location

    @start_location.setter
    def start_location(self, value):
        """reference :254-262 reads it at reset time: a reset(done) that was postponed is applied with the start location
        of the moment it was called (the old one), and the observation the last step's launch pre-computed for
        `reset(done)` assumed the old one as well"""
        fs = getattr(self, '_fs', None)
        if fs is not None:
            if fs.pending:
                self._flush()
            fs.obs_after = None
            fs.ok = False       # the next step goes through _slow_step, which hands the call block the new location
        self._start_location = value
        if fs is not None:
            fs.lazy_ok = self._lazy_reset and self._lazy_supported()

    def _lazy_supported(self) -> bool:
        return self.size > 4 and self.start_location is not None

    def _configure_call(self, c):
        sy, sx = self.start_location if self.start_location is not None else (-1, -1)
        c.start_y, c.start_x = int(sy), int(sx)

    def _start_args(self):
        if self.start_location is None:
            raise NotImplementedError("Haven't implemented random starting locations")
        return int(self.start_location[0]), int(self.start_location[1])

    def _cannot_reset(self):
        if self.size <= 4:  # reference :249-260
            return NotImplementedError('Environemnts smaller than this don\'t make sense.')
        if self.start_location is None:
            return NotImplementedError("Haven't implemented random starting locations")

    def _launch_reset(self, envs, done, obs, m, n, call):
        rc = _lib.call(self.device.index, _lib.lib().wurm_grid_reset, _lib.ptr(envs), _lib.ptr(done), _lib.ptr(obs), m, n,
                       _lib.i64(self.num_envs), self.size, int(self.start_location[0]), int(self.start_location[1]),
                       _lib.u64(self.seed), _lib.u64(call), _lib.i64(self.env_offset), None,
                       _lib.stream_ptr(self.device.index))
        _lib.check(rc, 'SimpleGridworld.reset')

    def _parse_mode(self, observation_mode: str):
        self._obs_shape(observation_mode)  # (what is no mode of this class raises here: reference :132-133)
        return _lib.parse_obs_mode(observation_mode)

    def _out_mode(self):
        # (reset and rollout parse the string first: one that is no mode of any class is a ValueError there)
        m, n = _lib.parse_obs_mode(self.observation_mode)
        return m, n, self._obs_shape(self.observation_mode)

    def _obs_shape(self, mode: str):
        N, S = self.num_envs, self.size
        if mode == 'default':
            return (N, 3, S, S)
        if mode == 'raw':
            return (N, 2, S, S)
        if mode == 'positions':
            return (N, 4)
        raise Exception  # reference :132-133

    def _observe(self, observation_mode: str = 'default') -> torch.Tensor:
        """reference :111-133 ('positions' is generalised from num_envs == 1 to (N, 4))"""
        shape = self._obs_shape(observation_mode)
        m, n = _lib.parse_obs_mode(observation_mode)
        obs = torch.empty(shape, dtype=torch.float32, device=self.device)
        rc = _lib.call(self.device.index, _lib.lib().wurm_grid_observe, _lib.ptr(self._state()), _lib.ptr(obs), m, n, _lib.i64(self.num_envs),
                                          self.size, _lib.stream_ptr(self.device.index))
        _lib.check(rc, 'SimpleGridworld._observe')
        return obs

    def step(self, actions: torch.Tensor) -> (torch.Tensor, torch.Tensor, torch.Tensor, dict):
        """reference :135-202 (actions are not modified).  One launch; a reset(done) postponed by the previous iteration
        (wurm_amd/envs/_fast_step.py) is applied in front of the transition."""
        return self._fast_step(actions, 'SimpleGridworld.step')

    def _make_out(self, i: int):
        return self._v_obs[i], self._v_reward[i], self._v_done2[i], {'edge_collision': self._v_edgec[i]}

    def policy_rollout(self, params: torch.Tensor, state: torch.Tensor, num_steps: int, check: bool = True,
                       population: int = None) -> dict:
        """T iterations of `probs, value = model(state); action = Categorical(probs).sample(); state, reward, done, info =
        env.step(action); env.reset(done)` in one kernel launch (see SingleSnake.policy_rollout).  The env must be in
        'positions' mode (the reference's feed-forward agent takes a flat observation; experiments/main.py:129-137) with a
        start location.  params: `pack_policy_params` of an agent with 4 inputs; state: (num_envs, 4).  Returns (T, N, ...)
        tensors `actions`, `probs`, `values`, `rewards`, `dones`, `edge_collision`, `observations`, and `state`, `status`.
        `check=True` synchronises once and raises if any env did not hold exactly one agent and one food.
        population=P: P policies, `params` (P, num_params), member p in the envs [p N / P, (p + 1) N / P) (see SingleSnake)."""
        if self.observation_mode != 'positions':
            raise NotImplementedError(f'policy_rollout: observation mode {self.observation_mode!r} is an image; the '
                                      f"feed-forward agent takes 'positions' observations")
        if self.start_location is None:
            raise NotImplementedError("Haven't implemented random starting locations")
        if self.size <= 4 or self.size > 64:
            raise NotImplementedError(f'policy_rollout: grid size {self.size}; the fused actor serves sizes 5 to 64')
        return self._policy_rollout(params, state, num_steps, check, (), population)

    def _consistent(self):
        pass
