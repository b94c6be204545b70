"""SingleSnake — drop-in for the reference's wurm.envs.SingleSnake (wurm/envs/single_snake.py:17-428) whose
step / reset / _observe run as fused gfx950 kernels behind the C ABI of include/wurm_hip.h.

Same constructor keywords, public attributes (`envs`, `done`, `num_envs`, `size`, ...), return conventions and
error types as the reference.  Intentional deviations:
  * `done` and `info[...]` are torch.bool (the faithful translation of torch-1.1 uint8 masks: `~done` is a
    logical not, as experiments/main.py:215 needs);
  * randomness comes from a counter-based Philox generator (`seed`, `env_offset` keywords) instead of torch's
    global RNG stream, so trajectories do not depend on how the batch is sharded over GPUs;
  * `partial_n` observations of an env whose head left the grid are zeros (the reference raises at :191);
  * there is no CPU path: `device` must be a HIP GPU.

Per-call path: one launch per `step(a); reset(done)` iteration, see wurm_amd/envs/_fast_step.py.
"""
from collections import namedtuple

import torch

from wurm_amd import _lib
from wurm_amd.constants import DEFAULT_DEVICE
from wurm_amd.envs._fast_step import FastStepMixin

Spec = namedtuple('Spec', ['reward_threshold'])

_INT_TYPES = (torch.short, torch.int, torch.long)


def _draw_seed() -> int:
    # one draw from torch's global generator: `torch.manual_seed(k)` before construction pins the trajectories
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class SingleSnake(FastStepMixin):
    """Batched snake environment: state `envs` is (num_envs, 3, size, size) fp32 = [food, head, body]
    (reference single_snake.py:22-47)."""

    _CHANNELS = 3
    _NAME = 'SingleSnake'
    _STEP_SLOT = 'wurm_single_step_slot'
    _ROLLOUT_FNS = ('wurm_single_rollout', 'wurm_single_rollout_resident')
    _POLICY_FN = 'wurm_single_policy_rollout_mode'
    _POLICY_POP_FN = 'wurm_single_policy_rollout_pop'
    _FRAMES_FN = 'wurm_single_rollout_frames'
    _FLAG_KEYS = ('dones', 'self_collision', 'edge_collision')
    _BAD_STATUS = 'some envs are not well-formed snakes'
    _EMPTY_ROLLOUT_SKIPS_MIRROR = True   # rollout(): no steps, no look at the mirror (9 x 9's is not the rollout's anyway)

    spec = Spec(float('inf'))
    metadata = {
        'render.modes': ['rgb_array'],
        'video.frames_per_second': 12
    }

    def __init__(self,
                 num_envs: int,
                 size: int,
                 max_timesteps: int = None,
                 initial_snake_length: int = 3,
                 on_death: str = 'restart',
                 observation_mode: str = 'one_channel',
                 device: str = DEFAULT_DEVICE,
                 manual_setup: bool = False,
                 verbose: int = 0,
                 render_args: dict = None,
                 seed: int = None,
                 env_offset: int = 0,
                 lazy_reset: bool = True,
                 resident_mirror=None):
        """Reference keywords (single_snake.py:55-65) plus this build's: `seed`, `env_offset` (module docstring),
        `lazy_reset` (envs/_fast_step.py) and `resident_mirror` — None: large batches step on a compact mirror of the state
         chosen by batch size with adaptive rules; False: never; True / 'lazy' / 'eager': whenever the
        shape is served, without the adaptive rules (`env.mirror_state()` tells what is in effect and why)."""
        self._resident_policy = resident_mirror
        self.num_envs = num_envs
        self.size = size
        self.max_timesteps = max_timesteps
        self.initial_snake_length = initial_snake_length
        self.on_death = on_death
        self.observation_mode = observation_mode
        self.device = _lib.require_device(device)
        self.verbose = verbose
        self.seed = _draw_seed() if seed is None else int(seed)
        self.env_offset = int(env_offset)
        self._mode_cache = {}
        self.lazy_reset = bool(lazy_reset)
        self._fast_init()

        if render_args is None:
            self.render_args = {'num_rows': 1, 'num_cols': 1, 'size': 256}
        else:
            self.render_args = render_args

        self.t = 0

        if not manual_setup:
            # reference :90-93 _create_envs(num_envs): every env is built by the reset kernel
            self._reset(torch.ones(num_envs, dtype=torch.bool, device=self.device), observe=False)

        self.viewer = None

        self.body_colour = torch.tensor((0, 127, 0), dtype=torch.short, device=self.device)
        self.head_colour = torch.tensor((0, 255, 0), dtype=torch.short, device=self.device)
        self.food_colour = torch.tensor((255, 0, 0), dtype=torch.short, device=self.device)
        self.edge_colour = torch.tensor((0, 0, 0), dtype=torch.short, device=self.device)

    # ------------------------------------------------------------------ helpers

    def _lazy_supported(self) -> bool:
        return self.size > 8 and self.initial_snake_length == 3

    def _configure_call(self, c):
        pass

    def _start_args(self):
        return ()

    def _cannot_reset(self):
        # (a snake length this build does not make is refused at once, whether or not an env has to be created — the size
        # only when one has to be, reference :346-347: that one is handed back for `_reset` to raise)
        if self.initial_snake_length != 3:
            raise NotImplementedError('Only initial snake length = 3 has been implemented.')
        if self.size <= 8:  # reference :346-347
            return NotImplementedError('Cannot make an env this small without making this code more clever')

    def _launch_reset(self, envs, done, obs, m, n, call):
        rc = _lib.call(self.device.index, _lib.lib().wurm_single_reset, _lib.ptr(envs), _lib.ptr(done), _lib.ptr(obs),
                       m, n, _lib.i64(self.num_envs), self.size, _lib.u64(self.seed), _lib.u64(call),
                       _lib.i64(self.env_offset), None, _lib.stream_ptr(self.device.index))
        _lib.check(rc, 'SingleSnake.reset')

    def _obs_shape(self, mode: str):
        m, n = _lib.parse_obs_mode(mode)
        N, S = self.num_envs, self.size
        if m in (_lib.OBS_DEFAULT, _lib.OBS_RAW):
            return (N, 3, S, S)
        if m == _lib.OBS_ONE_CHANNEL:
            return (N, 1, S, S)
        if m == _lib.OBS_POSITIONS:
            return (N, 4)
        if m == _lib.OBS_PARTIAL:
            return (N, 3 * (2 * n + 1) ** 2)
        raise Exception  # reference :194-195

    def _parse_mode(self, observation_mode: str):
        if observation_mode in ('default', 'raw', 'one_channel', 'positions'):
            return _lib.parse_obs_mode(observation_mode)
        if isinstance(observation_mode, str) and observation_mode.startswith('partial_'):
            # reference :167 reads the window size from self.observation_mode
            src = self.observation_mode if self.observation_mode.startswith('partial_') else observation_mode
            return _lib.OBS_PARTIAL, int(src.split('_')[-1])
        raise Exception  # reference :194-195

    # ------------------------------------------------------------------ observations

    def _observe(self, observation_mode: str = 'default') -> torch.Tensor:
        """reference :130-195"""
        m, n, shape = self._mode_info(observation_mode)
        envs = self._state(write=False)
        obs = torch.empty(shape, dtype=torch.float32, device=self.device)
        rc = _lib.call(self.device.index, _lib.lib().wurm_single_observe, _lib.ptr(envs), _lib.ptr(obs), m, n, _lib.i64(self.num_envs),
                                            self.size, _lib.stream_ptr(self.device.index))
        _lib.check(rc, 'SingleSnake._observe')
        return obs

    # ------------------------------------------------------------------ step

    def step(self, actions: torch.Tensor) -> (torch.Tensor, torch.Tensor, torch.Tensor, dict):
        """reference :197-304.  `actions` is sanitised in place (reverse moves become forward moves).  One launch:
        a reset(done) postponed by the previous iteration (wurm_amd/envs/_fast_step.py) is applied in front of the
        transition."""
        return self._fast_step(actions, 'SingleSnake.step')

    def _make_out(self, i: int):
        """what `step` returns for slot i of the current output slab (built once per slab)"""
        return (self._v_obs[i], self._v_reward[i], self._v_done2[i],
                {'self_collision': self._v_selfc[i], 'edge_collision': self._v_edgec[i]})

    # ------------------------------------------------------------------ reset

    def _create_envs(self, num_envs: int) -> torch.Tensor:
        """reference :344-387 — a fresh batch of `num_envs` environments (does not touch self.envs)."""
        if self.size <= 8:
            raise NotImplementedError('Cannot make an env this small without making this code more clever')
        if self.initial_snake_length != 3:
            raise NotImplementedError('Only initial snake length = 3 has been implemented.')
        envs = torch.zeros((num_envs, 3, self.size, self.size), device=self.device)
        done = torch.ones(num_envs, dtype=torch.bool, device=self.device)
        rc = _lib.call(self.device.index, _lib.lib().wurm_single_reset, 
            _lib.ptr(envs), _lib.ptr(done), None, _lib.OBS_NONE, 0, _lib.i64(num_envs), self.size,
            _lib.u64(self.seed), _lib.u64(self._next_call()), _lib.i64(self.env_offset), None, _lib.stream_ptr(self.device.index))
        _lib.check(rc, 'SingleSnake._create_envs')
        return envs

    # ------------------------------------------------------------------ fused acting loop (extension; `rollout`: _fast_step.py)

    def policy_rollout(self, params: torch.Tensor, state: torch.Tensor, num_steps: int, check: bool = True,
                       population: int = None) -> dict:
        """T iterations of the acting half of experiments/main.py:207-227 in one kernel launch:

            probs, value = model(state); action = Categorical(probs).sample()
            state, reward, done, info = env.step(action); env.reset(done)

        params: `wurm_amd.agents.pack_policy_params(agent)` (inputs -> 64 -> 64 -> {4, 1}); state: the observation the
        policy acts on first, (num_envs, 3, 2n+1, 2n+1) for `partial_n` (n <= 6) or (num_envs, 4) for `positions`, as
        returned by reset / step — the two modes the reference's feed-forward agent takes (experiments/main.py:129-137).
        Returns (T, N, ...) tensors: `actions` (sanitised, int64),
        `probs`, `values` (no grad — the learner recomputes them from `observations`), `rewards`, `dones`,
        `self_collision`, `edge_collision`, `observations` (what step t returned, i.e. the policy input of step t+1)
        and `state` = observations[-1].  `check=True` synchronises once and raises if any env was outside the
        kernel's domain (not a well-formed snake — only possible if `env.envs` was edited by hand).

        population=P (extension): P independent policies in the same launch.  The envs are P members of num_envs / P
        consecutive envs each; member p acts with `params[p]` of a contiguous fp32 (P, num_params) tensor (RuntimeError
        otherwise, or if P does not divide num_envs).  Same keys and shapes; member p's columns are bit for bit what a
        stand-alone env of its envs (`env_offset` + p num_envs / P, the same seed and call count) returns."""
        m, n, shape = self._mode_info(self.observation_mode)
        if m not in (_lib.OBS_PARTIAL, _lib.OBS_POSITIONS):
            raise NotImplementedError(f'policy_rollout: observation mode {self.observation_mode!r} is an image; the '
                                      f"feed-forward agent takes 'partial_n' or 'positions' observations")
        if m == _lib.OBS_PARTIAL and n > 6:
            raise NotImplementedError(f'policy_rollout: partial_{n} crop; the fused actor serves n <= 6')
        if self.size > 64:
            raise NotImplementedError(f'policy_rollout: grid size {self.size}; the fused actor serves sizes up to 64')
        return self._policy_rollout(params, state, num_steps, check, (m, n), population)

    # ------------------------------------------------------------------ invariants

    def check_consistency(self, mask: torch.Tensor = None):
        """wurm.utils.env_consistency on self.envs (reference wurm/utils.py:167-178).

        mask (extension): a (num_envs,) bool tensor — only the envs it selects are checked, on the device and without
        gathering them: `env.check_consistency(~done.squeeze(-1))` is what experiments/main.py:214-215 asks with
        `env_consistency(env.envs[~done.squeeze(-1)])`, at the cost of one checker launch and one `any()`."""
        from wurm_amd.utils import consistency_mask, _or_reduce, _raise_for
        sel = None
        if mask is not None:
            sel = mask.view(self.num_envs)
            sel = sel if sel.dtype == torch.bool else sel != 0
        err = self._step_check_mask()  # from inside the last step's launch, where it computed them (resident mirror)
        if err is not None:
            if sel is not None:
                err = err * sel.to(err.dtype)
            if not bool(err.any()):
                return
            if bool((err == -1).any()):  # an env the launch could not vouch for (or a finished one that was asked about)
                err = None
        if err is None:
            err = consistency_mask(self._state(write=False))
            if sel is not None:
                err = err * sel.to(err.dtype)
        _raise_for(_or_reduce(err), one_food=True)

    # ------------------------------------------------------------------ rendering (host side)

    def render(self, mode: str = 'human'):
        """reference :389-428.  Only 'rgb_array' is provided (the 'human' viewer needs gym/pyglet)."""
        if mode == 'human':
            raise NotImplementedError("render('human') needs gym's SimpleImageViewer; use mode='rgb_array'")
        if mode != 'rgb_array':
            raise ValueError('Render mode not recognised.')
        from wurm_amd._render import frame
        return frame(self._get_rgb().cpu().numpy(), self.num_envs, self.render_args)
