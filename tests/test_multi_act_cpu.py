"""`MultiSnake.act` without a device: the refusals of wurm_multi_act (made before any HIP call), the Python refusals, and the
species / env_id / column formulas against a brute-force restatement."""
import ctypes

import numpy as np
import pytest
import torch

from tests import multi_act_ref as ref
from wurm_amd import _lib
from wurm_amd.envs import _multi_act

E2 = 75


def _call(params=1, obs=1, actions=1, probs=None, values=None, N=4, K=2, P=1, E=E2):
    """wurm_multi_act with host buffers standing in for device pointers: every case here must return before any HIP call"""
    keep = [np.zeros(8, np.float32) if x == 1 else None for x in (params, obs, actions)]
    ptrs = [k.ctypes.data if k is not None else None for k in keep]
    return _lib.lib().wurm_multi_act(ptrs[0], ptrs[1], ptrs[2], probs, values, N, K, P, E, 1, 0, 0, None)


def test_abi_refusals_need_no_device():
    assert _call(N=-1) == _lib.ERR_INVALID_ARG
    assert _call(K=-1) == _lib.ERR_INVALID_ARG
    assert _call(E=-75) == _lib.ERR_INVALID_ARG
    assert _call(P=0) == _lib.ERR_INVALID_ARG
    assert _call(P=3, K=2) == _lib.ERR_INVALID_ARG
    assert _call(K=0, P=1) == _lib.ERR_INVALID_ARG       # (no species fits into no snakes)
    for missing in ('params', 'obs', 'actions'):
        assert _call(**{missing: None}) == _lib.ERR_INVALID_ARG, missing
    for E in (0, 4, 74, 76, 3 * 15 * 15, 508):            # n = 7 is 3 * 15^2
        assert _call(E=E) == _lib.ERR_UNSUPPORTED, E
    # no envs: a successful no-op that launches nothing, null pointers included
    before = _lib.lib().wurm_launch_count()
    for E in ref.OBS_N:
        assert _call(params=None, obs=None, actions=None, N=0, E=E) == _lib.OK
    assert _lib.lib().wurm_launch_count() == before


@pytest.mark.parametrize('K,P', [(1, 1), (2, 1), (2, 2), (3, 2), (4, 2), (5, 1), (5, 2), (5, 5), (7, 3), (12, 5), (25, 4)])
def test_species_env_id_and_columns(K, P):
    N, off = 6, 1000
    species = ref.species_by_counting(K, P)
    assert [_multi_act.species_of(k, K, P) for k in range(K)] == species
    assert sorted(set(species)) == list(range(P))      # every species has a snake, in order
    assert species == sorted(species)
    ids = set()
    for k in range(K):
        for i in range(N):
            col = _multi_act.column_of(k, i, N)
            assert col == sum(1 for kk in range(K) for ii in range(N) if (kk, ii) < (k, i))   # agent-major
            assert col in _multi_act.species_columns(species[k], K, N, P)
            ids.add(_multi_act.env_id_of(i, k, K, off))
            assert _multi_act.env_id_of(i, k, K, off) == off * K + i * K + k
    assert len(ids) == K * N                             # one stream per agent
    # the blocks tile the columns, and are equal when P divides K (the member layout of FusedA2CPopulation)
    blocks = [_multi_act.species_columns(s, K, N, P) for s in range(P)]
    assert [c for b in blocks for c in b] == list(range(K * N))
    if K % P == 0:
        assert {len(b) for b in blocks} == {K // P * N}
    assert _multi_act.num_policy_params(E2) == 64 * E2 + 64 + 64 * 64 + 64 + 4 * 64 + 4 + 64 + 1


class _Env(object):
    """what the refusals that need no launch read of a MultiSnake"""
    num_snakes, num_envs, seed, env_offset, policy_calls = 2, 3, 0, 0, 0
    dtype = torch.float
    device = torch.device('cuda', 0)

    def __init__(self, mode='partial_2', dtype=torch.float):
        self.observation_mode, self.dtype = mode, dtype


def test_python_refusals():
    P = _multi_act.num_policy_params(E2)
    params, obs = torch.zeros((2, P)), torch.zeros((2, 3, E2))
    for mode in ('full', 'partial_7', 'positions', 'partial_x'):
        with pytest.raises(NotImplementedError, match=mode):
            _multi_act.act(_Env(mode), params, obs)
    with pytest.raises(NotImplementedError, match='float16'):
        _multi_act.act(_Env(dtype=torch.half), params, obs)
    # CPU tensors: there is no CPU path
    with pytest.raises(_lib.WurmHipError, match='cpu'):
        _multi_act.act(_Env(), params, obs)
    with pytest.raises(_lib.WurmHipError):
        _multi_act._observations(_Env(), obs, E2)
    with pytest.raises(_lib.WurmHipError):
        _multi_act._observations(_Env(), {'agent_0': obs[0], 'agent_1': obs[1]}, E2)
    # params: type, dtype, shape and layout are checked before the device
    with pytest.raises(RuntimeError, match='list'):
        _multi_act.act(_Env(), [1.0], obs)
    with pytest.raises(RuntimeError, match='float64'):
        _multi_act.act(_Env(), params.double(), obs)
    with pytest.raises(RuntimeError, match=str(P - 1)):
        _multi_act.act(_Env(), params[:, :-1].contiguous(), obs)
    with pytest.raises(RuntimeError, match='contiguous'):
        _multi_act.act(_Env(), torch.zeros((P, 2)).t(), obs)


def test_no_env_without_a_device():
    """the methods exist on the class; constructing the env needs a device (as tests/test_abi.py::test_no_cpu_fallback)"""
    from wurm_amd.envs import MultiSnake
    assert callable(MultiSnake.act) and callable(MultiSnake.act_window)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.WurmHipError):
            MultiSnake(num_envs=2, num_snakes=2, size=12, observation_mode='partial_2')


def test_symbol_is_declared_and_exported():
    assert 'wurm_multi_act' in _lib.SYMBOLS
    fn = _lib.lib().wurm_multi_act
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
