"""The league (`MultiSnake.league_plan` / `act_league` / `league_window`, `wurm_amd.rl.LeagueTable`) without a device:
`league_plan` on CPU tensors against the plan by brute force, every Python refusal, the refusals of wurm_multi_act_league
and wurm_multi_league_scores (made before any HIP call), and the symbols."""
import ctypes

import numpy as np
import pytest
import torch

from tests import multi_league_ref as ref
from wurm_amd import _lib
from wurm_amd.envs import _multi_act, _multi_league
from wurm_amd.rl import LeagueTable, league_table

E2 = 75


class _Env(object):
    """what `league_plan` and the refusals that need no launch read of a MultiSnake"""
    seed, env_offset, policy_calls = 0, 0, 0
    device = torch.device('cuda', 0)

    def __init__(self, K=2, N=3, mode='partial_2', dtype=torch.float):
        self.num_snakes, self.num_envs, self.observation_mode, self.dtype = K, N, mode, dtype


def _lineup(K, N, A, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'random':
        return torch.randint(A, (K, N), generator=g)
    if kind == 'one':             # all rows on one policy, the last: every other policy is without rows
        return torch.full((K, N), A - 1, dtype=torch.long)
    if kind == 'sparse':          # at most two distinct policies whatever A: policies without rows in between
        return torch.randint(2, (K, N), generator=g) * (A - 1)
    raise ValueError(kind)


@pytest.mark.parametrize('kind', ['random', 'one', 'sparse'])
@pytest.mark.parametrize('A', [1, 2, 7, 300])
@pytest.mark.parametrize('N', [1, 7, 64])
@pytest.mark.parametrize('K', [1, 3, 5])
def test_plan_is_the_brute_force_plan(K, N, A, kind):
    lineup = _lineup(K, N, A, kind, seed=K * 1000 + N * 10 + A)
    plan = _multi_league.league_plan(_Env(K, N), lineup, A)
    order, offsets = ref.brute_plan(lineup.numpy(), A)
    assert plan.order.dtype == torch.int32 and plan.order.shape == (K * N,)
    assert plan.offsets.dtype == torch.int64 and plan.offsets.shape == (A + 1,)
    assert plan.order.tolist() == order and plan.offsets.tolist() == offsets
    assert plan.num_policies == A and plan.lineup is lineup and plan.order.device == lineup.device
    assert sorted(order) == list(range(K * N))                      # every row once
    if kind == 'one':
        assert offsets == [0] * A + [K * N]
    if kind != 'random' and A > 2:
        assert offsets[1] == offsets[A - 1]                           # policies 1 .. A - 2 have no rows
    # the dtype of the line-up does not matter
    assert torch.equal(_multi_league.league_plan(_Env(K, N), lineup.to(torch.int32), A).order, plan.order)


def test_block_lineup_is_the_species_formula():
    for K, P in [(2, 2), (3, 2), (4, 1), (5, 3)]:
        lineup = _multi_league.block_lineup(K, 4, P)
        assert lineup.shape == (K, 4) and lineup.is_contiguous()
        assert lineup[:, 0].tolist() == [_multi_act.species_of(k, K, P) for k in range(K)]
        assert bool((lineup == lineup[:, :1]).all())


def test_plan_refusals():
    env, good = _Env(2, 3), torch.zeros((2, 3), dtype=torch.long)
    plan = _multi_league.league_plan
    with pytest.raises(RuntimeError, match='list'):
        plan(env, [[0, 0, 0], [0, 0, 0]], 1)
    with pytest.raises(RuntimeError, match='float32'):
        plan(env, good.float(), 1)
    with pytest.raises(RuntimeError, match='bool'):
        plan(env, good.bool(), 1)
    for bad in (torch.zeros((3, 2), dtype=torch.long), torch.zeros(6, dtype=torch.long),
                torch.zeros((2, 3, 1), dtype=torch.long), torch.zeros((2, 4), dtype=torch.long)):
        with pytest.raises(RuntimeError, match=r'expected \(num_snakes, num_envs\) = \(2, 3\)'):
            plan(env, bad, 1)
    with pytest.raises(RuntimeError, match=r'\[0, 2\], outside \[0, num_policies = 2\)'):
        plan(env, torch.tensor([[0, 1, 2], [0, 0, 0]]), 2)
    with pytest.raises(RuntimeError, match=r'\[-1, 1\]'):
        plan(env, torch.tensor([[0, 1, -1], [0, 0, 0]]), 2)
    for A in (0, -3):
        with pytest.raises(RuntimeError, match='num_policies must lie'):
            plan(env, good, A)
    with pytest.raises(RuntimeError, match='num_policies must be an int'):
        plan(env, good, 2.0)


def test_python_refusals():
    P = _multi_act.num_policy_params(E2)
    params, obs = torch.zeros((4, P)), torch.zeros((2, 3, E2))
    cpu_plan = _multi_league.league_plan(_Env(), torch.zeros((2, 3), dtype=torch.long), 4)
    act, window = _multi_league.act_league, _multi_league.league_window
    # what `act` refuses, in its words
    for mode in ('full', 'partial_7', 'positions'):
        with pytest.raises(NotImplementedError, match=mode):
            act(_Env(mode=mode), params, obs, cpu_plan)
        with pytest.raises(NotImplementedError, match=mode):
            window(_Env(mode=mode), params, obs, 0, cpu_plan)
    with pytest.raises(NotImplementedError, match='float16'):
        act(_Env(dtype=torch.half), params, obs, cpu_plan)
    with pytest.raises(RuntimeError, match='list'):
        act(_Env(), [1.0], obs, cpu_plan)
    with pytest.raises(RuntimeError, match='float64'):
        act(_Env(), params.double(), obs, cpu_plan)
    with pytest.raises(RuntimeError, match=str(P - 1)):
        act(_Env(), params[:, :-1].contiguous(), obs, cpu_plan)
    with pytest.raises(RuntimeError, match='contiguous'):
        act(_Env(), torch.zeros((P, 4)).t(), obs, cpu_plan)
    with pytest.raises(_lib.WurmHipError, match='cpu'):      # CPU tensors: there is no CPU path
        act(_Env(), params, obs, cpu_plan)
    with pytest.raises(_lib.WurmHipError, match='cpu'):
        window(_Env(), params, obs, 0, cpu_plan)
    with pytest.raises(RuntimeError, match='negative'):
        window(_Env(), params, obs, -1, cpu_plan)
    # the plan against the env, the batch and params (behind the tensors' own checks: `_checked` is what both calls run)
    chk = _multi_league._checked
    with pytest.raises(RuntimeError, match='must come from league_plan'):
        chk(_Env(), (cpu_plan.order, cpu_plan.offsets), 4, 3, 'act_league')
    with pytest.raises(RuntimeError, match=r'shape \(2, 3\), the observations for \(2, 5\)'):
        chk(_Env(), cpu_plan, 4, 5, 'act_league')
    with pytest.raises(RuntimeError, match='the plan is on cpu'):
        chk(_Env(), cpu_plan, 4, 3, 'act_league')
    with pytest.raises(RuntimeError, match='names 4 policies but params has 3 rows'):
        chk(_HostEnv(), cpu_plan, 3, 3, 'act_league')
    assert chk(_HostEnv(), cpu_plan, 4, 3, 'act_league') == 4


class _HostEnv(_Env):
    device = torch.device('cpu')


def test_table_refusals():
    with pytest.raises(RuntimeError, match='positive'):
        LeagueTable(0, 'cpu')
    table = LeagueTable(4, 'cpu')
    assert table.table.shape == (4, 8) and table.table.dtype == torch.float64
    plan = _multi_league.league_plan(_Env(), torch.zeros((2, 3), dtype=torch.long), 4)
    T = 2
    out = {'rewards': torch.zeros((T, 6)), 'dones': torch.zeros((T, 6), dtype=torch.bool)}
    info = {'food': torch.zeros((T, 6)), 'size': torch.zeros((T, 6)), 'boost': torch.zeros((T, 6), dtype=torch.bool),
            'snake_collision': torch.zeros((T, 6), dtype=torch.bool), 'edge_collision': torch.zeros((T, 6), dtype=torch.bool)}
    with pytest.raises(RuntimeError, match='must come from league_plan'):
        table.update(None, out)
    with pytest.raises(RuntimeError, match='names 4 policies, the table has 3'):
        LeagueTable(3, 'cpu').update(plan, out)
    with pytest.raises(RuntimeError, match="no 'dones'"):
        table.update(plan, {'rewards': out['rewards']})
    with pytest.raises(RuntimeError, match='not the other info=True keys'):
        table.update(plan, dict(out, food=info['food']))
    with pytest.raises(RuntimeError, match=r'rewards has shape \(2, 5\)'):
        table.update(plan, dict(out, rewards=torch.zeros((T, 5))))
    with pytest.raises(RuntimeError, match=r'dones has shape \(1, 6\)'):
        table.update(plan, dict(out, dones=out['dones'][:1]))
    with pytest.raises(RuntimeError, match='rewards must be torch.float32'):
        table.update(plan, dict(out, rewards=out['rewards'].double()))
    with pytest.raises(RuntimeError, match='size must be torch.float32'):
        table.update(plan, dict(out, **dict(info, size=info['size'].long())))
    with pytest.raises(RuntimeError, match='dones is on meta'):
        table.update(plan, dict(out, dones=out['dones'].to('meta')))
    for window in (out, dict(out, **info)):                 # everything in order, but on the CPU: there is no CPU path
        with pytest.raises(_lib.WurmHipError, match='runs on the GPU'):
            table.update(plan, window)
    assert not bool(table.table.any())
    # what read() makes of a row
    row = league_table.row_dict([20.0, -3.0, 4.0, 5.0, 1.0, 3.0, 2.0, 90.0])
    assert [row[c] for c in ref.COLUMNS] == [20.0, -3.0, 4.0, 5.0, 1.0, 3.0, 2.0, 90.0]
    assert row['reward_per_step'] == -3.0 / 20.0 and row['size_mean'] == 4.5 and row['life_length_mean'] == 5.0
    assert row['reward_per_life'] == -0.75 and row['food_per_life'] == 1.25 and row['deaths_per_step'] == 0.2
    never = league_table.row_dict([0.0] * 8)
    assert all(np.isnan(never[k]) for k in ('reward_per_step', 'size_mean', 'reward_per_life', 'life_length_mean'))
    assert league_table.COLUMNS == ref.COLUMNS


def _act(params=1, obs=1, order=1, offsets=1, actions=1, N=4, K=2, A=3, E=E2):
    """wurm_multi_act_league with host buffers standing in for device pointers: every case must return before any HIP call"""
    keep = [np.zeros(8, np.float32) if x == 1 else None for x in (params, obs, order, offsets, actions)]
    p = [k.ctypes.data if k is not None else None for k in keep]
    return _lib.lib().wurm_multi_act_league(p[0], p[1], p[2], p[3], p[4], None, None, N, K, A, E, 1, 0, 0, None)


def _scores(rewards=1, dones=1, order=1, offsets=1, table=1, R=8, T=2, A=3):
    keep = [np.zeros(8, np.float32) if x == 1 else None for x in (rewards, dones, order, offsets, table)]
    p = [k.ctypes.data if k is not None else None for k in keep]
    return _lib.lib().wurm_multi_league_scores(p[0], p[1], None, None, None, None, None, p[2], p[3], p[4], R, T, A, None)


def test_abi_refusals_need_no_device():
    assert _act(N=-1) == _lib.ERR_INVALID_ARG
    assert _act(K=-1) == _lib.ERR_INVALID_ARG
    assert _act(E=-75) == _lib.ERR_INVALID_ARG
    assert _act(A=0) == _lib.ERR_INVALID_ARG
    assert _act(A=-2) == _lib.ERR_INVALID_ARG
    for missing in ('params', 'obs', 'order', 'offsets', 'actions'):
        assert _act(**{missing: None}) == _lib.ERR_INVALID_ARG, missing
    for E in (0, 4, 74, 76, 3 * 15 * 15, 508):            # n = 7 is 3 * 15^2
        assert _act(E=E) == _lib.ERR_UNSUPPORTED, E
    assert _act(N=2 ** 30, K=2) == _lib.ERR_UNSUPPORTED   # 2^31 rows do not fit the int32 list
    assert _scores(R=-1) == _lib.ERR_INVALID_ARG
    assert _scores(T=-1) == _lib.ERR_INVALID_ARG
    assert _scores(A=0) == _lib.ERR_INVALID_ARG
    for missing in ('rewards', 'dones', 'order', 'offsets', 'table'):
        assert _scores(**{missing: None}) == _lib.ERR_INVALID_ARG, missing
    assert _scores(R=2 ** 31) == _lib.ERR_UNSUPPORTED
    # nothing to do: a successful no-op that launches nothing, null pointers included
    before = _lib.lib().wurm_launch_count()
    for E in (27, 75, 147, 243, 363, 507):
        assert _act(params=None, obs=None, order=None, offsets=None, actions=None, N=0, E=E) == _lib.OK
    assert _act(params=None, obs=None, order=None, offsets=None, actions=None, K=0) == _lib.OK
    assert _scores(rewards=None, dones=None, order=None, offsets=None, table=None, R=0) == _lib.OK
    assert _scores(rewards=None, dones=None, order=None, offsets=None, table=None, T=0) == _lib.OK
    assert _lib.lib().wurm_launch_count() == before


def test_symbols_are_declared_and_exported():
    for name, nargs in (('wurm_multi_act_league', 15), ('wurm_multi_league_scores', 14)):
        assert name in _lib.SYMBOLS
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs


def test_methods_exist_on_the_class():
    from wurm_amd.envs import MultiSnake
    assert callable(MultiSnake.league_plan) and callable(MultiSnake.act_league) and callable(MultiSnake.league_window)
