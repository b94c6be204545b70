"""`MultiSnake.policy_window` without a device: the refusals of wurm_multi_policy_window (made before any HIP call), the plan
query behind `policy_window_fused`, and the Python refusals, which are `act_window`'s."""
import ctypes

import pytest
import torch

from wurm_amd import _lib
from wurm_amd.envs import MultiSnake, _multi_act, _multi_policy_window

INV, UNS, OK = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.OK
REQUIRED = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'colours', 'boost_this_step', 'params', 'obs0')
OUTPUTS = ('actions', 'probs', 'values', 'observations', 'rewards', 'dones_out', 'all_done', 'food', 'sizes', 'boost',
           'snake_collision', 'edge_collision')


def _block(p, **kw):
    """a call on which every check passes (host memory standing in for device pointers), with the fields `kw` replaced"""
    c = _lib.MultiPolicyWindowCall()
    for name in REQUIRED + OUTPUTS:
        setattr(c, name, p)
    c.num_envs, c.num_steps, c.num_snakes, c.size, c.obs_n, c.num_species = 4, 3, 2, 12, 2, 2
    c.num_params = _multi_act.num_policy_params(75)
    c.cfg = _lib.multi_config(2, True, 0.5, 0.5, 'only_one', 5e-4, -1, 'all', 'random')
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)  # non-null and 8-byte aligned: every call below is refused before anything is read or launched
    call = lambda **kw: lib.wurm_multi_policy_window(ctypes.byref(_block(p, **kw)), None)
    assert lib.wurm_multi_policy_window(None, None) == INV
    for name in REQUIRED + OUTPUTS:
        assert call(**{name: None}) == INV, name
    assert call(num_envs=-1) == INV and call(num_steps=-1) == INV
    assert call(num_snakes=0) == INV and call(num_snakes=-2) == INV and call(size=2) == INV
    assert call(num_species=0) == INV and call(num_species=3) == INV and call(num_species=-1) == INV
    assert call(waves_per_group=-1) == INV and call(waves_per_group=5) == INV
    # a params row that is not the row of E = 75 inputs (partial_3's, one element short, none)
    for n in (_multi_act.num_policy_params(147), _multi_act.num_policy_params(75) - 1, 0):
        assert call(num_params=n) == INV, n
    # a pointer that is not aligned to its element
    for name in ('foods', 'heads', 'bodies', 'params', 'obs0', 'probs', 'values', 'observations', 'rewards', 'food', 'sizes'):
        assert call(**{name: p + 2}) == INV, name
    for name in ('orientations', 'actions'):
        assert call(**{name: p + 4}) == INV, name
    assert call(colours=p + 1) == INV
    # outside what the kernel serves
    assert call(num_snakes=65, num_species=1) == UNS and call(size=65) == UNS and call(size=4) == UNS
    for n in (-1, 4, 5, 6, 7):  # (the refusal comes before num_params is compared with that n's row)
        assert call(obs_n=n) == UNS, n
    assert call(num_snakes=64, num_species=1, size=64) == UNS   # 2 K S^2 bytes of body grids alone: 512 KB of LDS
    # nothing to do: accepted without a launch (there is no device here to launch on), outputs not needed
    assert call(num_envs=0) == OK and call(num_steps=0) == OK
    assert call(num_steps=0, **{name: None for name in OUTPUTS}) == OK


def test_plan():
    plan = _lib.lib().wurm_multi_policy_window_plan
    # resident: the species' first layers fit LDS together, at most 4 heads in registers
    for K, S, n, P in ((1, 8, 0, 1), (2, 12, 2, 2), (4, 25, 3, 2), (4, 12, 2, 4), (3, 9, 3, 3), (10, 36, 3, 1)):
        assert plan(K, S, n, P, 512) == 1, (K, S, n, P)
    # reloaded: more than 4 species, or 4 x 40 KB of first layers
    for K, S, n, P in ((4, 12, 3, 4), (6, 12, 1, 5), (6, 12, 2, 6)):
        assert plan(K, S, n, P, 512) == 2, (K, S, n, P)
    # not served: crops beyond partial_3, shapes the fused rollouts refuse, species the env does not have
    for K, S, n, P in ((2, 12, 4, 1), (2, 12, 6, 2), (2, 4, 1, 1), (2, 65, 1, 1), (65, 12, 1, 1), (2, 12, 2, 3), (2, 12, 2, 0),
                       (64, 64, 1, 1)):
        assert plan(K, S, n, P, 512) == 0, (K, S, n, P)
    assert plan(2, 12, 2, 2, -1) == 0 and plan(2, 12, 2, 2, 0) == 1


class _Env(object):
    """what policy_window reads of a MultiSnake before it touches a tensor"""
    num_snakes, num_envs, size, seed, env_offset, policy_calls = 2, 3, 12, 0, 0, 0
    device = torch.device('cuda', 0)
    _lifetimes_touched = _force_act_window = False

    def __init__(self, mode='partial_2', dtype=torch.float):
        self.observation_mode, self.dtype = mode, dtype


def test_policy_window_fused():
    fused = lambda env, P=1: _multi_policy_window.plan(env, P) != 0
    assert fused(_Env()) and fused(_Env(), 2) and fused(_Env('partial_0')) and fused(_Env('partial_3'), 2)
    assert not fused(_Env('partial_4')) and not fused(_Env('partial_6')) and not fused(_Env('full'))
    assert not fused(_Env('partial_x')) and not fused(_Env(dtype=torch.half)) and not fused(_Env(), 3)
    env = _Env()
    env._lifetimes_touched = True
    assert not fused(env)
    env = _Env()
    env._force_act_window = True
    assert not fused(env)
    assert _multi_policy_window.plan(_Env('partial_3'), 2) == 1
    assert callable(MultiSnake.policy_window) and callable(MultiSnake.policy_window_fused)
    assert MultiSnake._force_act_window is False and MultiSnake._policy_window_wpb == 0


def test_python_refusals():
    """what act_window raises, policy_window raises — before any launch"""
    E = 75
    n = _multi_act.num_policy_params(E)
    params, obs = torch.zeros((2, n)), torch.zeros((2, 3, E))
    pw = _multi_policy_window.policy_window
    with pytest.raises(RuntimeError, match='negative'):
        pw(_Env(), params, obs, -1)
    for mode in ('full', 'partial_7', 'positions'):
        with pytest.raises(NotImplementedError, match=mode):
            pw(_Env(mode), params, obs, 2)
    with pytest.raises(NotImplementedError, match='float16'):
        pw(_Env(dtype=torch.half), params, obs, 2)
    with pytest.raises(RuntimeError, match='list'):
        pw(_Env(), [1.0], obs, 2)
    with pytest.raises(RuntimeError, match='float64'):
        pw(_Env(), params.double(), obs, 2)
    with pytest.raises(RuntimeError, match=str(n - 1)):
        pw(_Env(), params[:, :-1].contiguous(), obs, 2)
    with pytest.raises(_lib.WurmHipError, match='cpu'):
        pw(_Env(), params, obs, 2)


def test_symbols_are_declared():
    assert {'wurm_multi_policy_window', 'wurm_multi_policy_window_plan'} <= set(_lib.SYMBOLS)
    assert len(_lib.lib().wurm_multi_policy_window.argtypes) == 2
    assert len(_lib.lib().wurm_multi_policy_window_plan.argtypes) == 5
