"""The league's matchmaking without a device: the Python restatement (tests/league_draw_ref.py) on hand-computed cases,
every refusal of `MultiSnake.league_draw` / `league_plan(sync=False)` and of wurm_multi_league_draw /
wurm_multi_league_plan (all made before any HIP call), `league_plan(sync=True)` against a verbatim copy of the torch
lines it had before the keyword, and one distribution check of the restatement itself."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import league_draw_ref as ref
from wurm_amd import _lib
from wurm_amd.envs import _multi_league

SEED = 11


class _Env(object):
    """what `league_draw` / `league_plan` read of a MultiSnake before they launch anything"""
    seed, env_offset, policy_calls, league_draws, league_dropped = SEED, 0, 0, 0, None

    def __init__(self, K=2, N=3, device=torch.device('cuda', 0)):
        self.num_snakes, self.num_envs, self.device = K, N, device


# ------------------------------------------------------------------ the restatement on cases worked out by hand

def test_the_only_ticket_holder_is_always_picked():
    for call in range(3):
        assert (ref.draw(1, 50, 3, SEED, call, tickets=[0, 0, 5]) == 2).all()
        assert (ref.draw(2, 50, 3, SEED, call, tickets=[0, 0, 5], replacement=True) == 2).all()


def test_negative_tickets_count_as_zero():
    assert (ref.draw(1, 50, 3, SEED, 0, tickets=[-7, 4, -1]) == 1).all()
    assert np.array_equal(ref.draw(2, 40, 4, SEED, 0, tickets=[-7, 4, -1, 2]), ref.draw(2, 40, 4, SEED, 0, tickets=[0, 4, 0, 2]))


def test_a_pool_without_tickets_is_drawn_from_uniformly():
    zero, ones = ref.draw(2, 64, 5, SEED, 0, tickets=[0] * 5), ref.draw(2, 64, 5, SEED, 0, tickets=[1] * 5)
    assert np.array_equal(zero, ones) and np.array_equal(zero, ref.draw(2, 64, 5, SEED, 0))
    assert len(set(zero.ravel().tolist())) == 5
    # the fall-back is per seat: once the only holder sits, the rest of the pool has no tickets left
    got = ref.draw(3, 64, 3, SEED, 0, tickets=[0, 0, 5])
    assert (got[0] == 2).all() and set(got[1].tolist()) == {0, 1} and (got[1] + got[2] == 1).all()


def test_the_walk_by_hand():
    """r = mulhi64(x, total) falls into the running sums 2 | 2 + 0 | 2 + 0 + 6: policy 0 for r < 2, policy 2 above"""
    tickets, total = [2, 0, 6], 8
    for i in range(64):
        w = ref.rng_words(SEED, 4, 1000 + i, ref.RNG_LEAGUE, 0)
        r = (((w[0] << 32) | w[1]) * total) >> 64
        assert ref.draw_env(1000 + i, 1, 3, SEED, 4, tickets) == [0 if r < 2 else 2]


def test_as_many_seats_as_policies_is_a_permutation():
    got = ref.draw(4, 80, 4, SEED, 2, tickets=[5, 1, 0, 2])
    assert (np.sort(got, axis=0) == np.arange(4)[:, None]).all()
    assert len(set(map(tuple, got.T.tolist()))) > 4          # (and not the same one everywhere)


def test_a_pinned_policy_never_sits_in_a_free_seat():
    pinned = [-1, 3, -1, 0]
    got = ref.draw(4, 80, 6, SEED, 0, tickets=[9, 1, 1, 9, 1, 1], pinned=pinned)
    assert (got[1] == 3).all() and (got[3] == 0).all()
    assert not np.isin(got[[0, 2]], [0, 3]).any() and (got[0] != got[2]).all()
    # with replacement the pool stays whole: the heavy pinned policies show up in the free seats too
    again = ref.draw(4, 80, 6, SEED, 0, tickets=[9, 1, 1, 9, 1, 1], replacement=True, pinned=pinned)
    assert (again[1] == 3).all() and (again[3] == 0).all() and np.isin(again[[0, 2]], [0, 3]).any()


def test_with_replacement_repeats_occur():
    got = ref.draw(3, 80, 3, SEED, 0, replacement=True)
    assert (got[0] == got[1]).any() and (got[0] != got[1]).any()
    assert not (ref.draw(3, 80, 3, SEED, 0)[0] == ref.draw(3, 80, 3, SEED, 0)[1]).any()


def test_an_env_does_not_depend_on_the_batch():
    whole = ref.draw(3, 40, 7, SEED, 5, tickets=[3, 0, 2, 2, 9, 1, 1])
    assert np.array_equal(ref.draw(3, 10, 7, SEED, 5, env_offset=25, tickets=[3, 0, 2, 2, 9, 1, 1]), whole[:, 25:35])
    assert not np.array_equal(ref.draw(3, 40, 7, SEED, 6, tickets=[3, 0, 2, 2, 9, 1, 1]), whole)


def test_distribution_of_the_restatement():
    """tickets [1, 3], one seat, 4096 envs: policy 1's share within four binomial standard deviations of 3 / 4"""
    N = 4096
    share = float((ref.draw(1, N, 2, 2026, 0, tickets=[1, 3]) == 1).mean())
    assert abs(share - 0.75) <= 4 * math.sqrt(0.75 * 0.25 / N), share


def test_plan_rule_with_dropped_rows():
    order, offsets, dropped = ref.plan(np.array([[2, 0, 5], [-1, 2, 0]]), 3)
    assert (order, offsets, dropped) == ([1, 5, 0, 4, -1, -1], [0, 2, 2, 4], 2)


# ------------------------------------------------------------------ sync=True is the code it was

def _plan_as_it_was(lineup, A):
    flat = lineup.reshape(-1).to(torch.long)
    order = torch.sort(flat, stable=True).indices.to(torch.int32)
    counts = torch.bincount(flat, minlength=A)
    offsets = torch.zeros(A + 1, dtype=torch.long, device=lineup.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    return order, offsets


@pytest.mark.parametrize('K,N,A', [(1, 1, 1), (2, 33, 5), (4, 257, 300), (3, 64, 2)])
def test_sync_true_is_unchanged(K, N, A):
    lineup = torch.randint(A, (K, N), generator=torch.Generator().manual_seed(K + N + A))
    for plan in (_multi_league.league_plan(_Env(K, N), lineup, A), _multi_league.league_plan(_Env(K, N), lineup, A, True),
                 _multi_league.league_plan(_Env(K, N), lineup.to(torch.int16), A, sync=True)):
        order, offsets = _plan_as_it_was(lineup, A)
        assert torch.equal(plan.order, order) and torch.equal(plan.offsets, offsets) and plan.num_policies == A
        want = ref.plan(lineup.numpy(), A)
        assert (plan.order.tolist(), plan.offsets.tolist()) == want[:2] and want[2] == 0
    with pytest.raises(RuntimeError, match=r'\[0, 2\], outside'):
        _multi_league.league_plan(_Env(1, 2), torch.tensor([[0, 2]]), 2, sync=True)


# ------------------------------------------------------------------ the host layer's refusals (nothing is launched)

def test_draw_refusals():
    draw = _multi_league.league_draw
    env = _Env(2, 3)
    for A in (0, -1, 2 ** 31):
        with pytest.raises(RuntimeError, match='num_policies must lie'):
            draw(env, A)
    for A in (2.0, '3', None):
        with pytest.raises(RuntimeError, match='num_policies must be an int'):
            draw(env, A)
    with pytest.raises(RuntimeError, match='tickets must be a tensor'):
        draw(env, 4, tickets=[1, 1, 1, 1])
    for dtype in (torch.int64, torch.float32, torch.uint8):
        with pytest.raises(RuntimeError, match='tickets must be int32'):
            draw(env, 4, tickets=torch.ones(4, dtype=dtype))
    for shape in ((3,), (5,), (4, 1), ()):
        with pytest.raises(RuntimeError, match=r'expected a contiguous \(num_policies,\) = \(4,\)'):
            draw(env, 4, tickets=torch.ones(shape, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='contiguous'):
        draw(env, 4, tickets=torch.ones(8, dtype=torch.int32)[::2])
    with pytest.raises(RuntimeError, match='tickets is on cpu'):
        draw(env, 4, tickets=torch.ones(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='pinned has 3 entries'):
        draw(env, 4, pinned=[0, -1, -1])
    with pytest.raises(RuntimeError, match='pinned must be a sequence of ints'):
        draw(env, 4, pinned=[0.5, -1])
    with pytest.raises(RuntimeError, match='pinned must be a sequence of ints'):
        draw(env, 4, pinned=7)
    for bad in ([4, -1], [-2, 0]):
        with pytest.raises(RuntimeError, match=r'outside \[-1, num_policies = 4\)'):
            draw(env, 4, pinned=bad)
    with pytest.raises(RuntimeError, match='pinned twice'):
        draw(env, 4, pinned=[1, 1])
    with pytest.raises(RuntimeError, match='at least as many policies'):
        draw(_Env(3, 3), 2)
    with pytest.raises(RuntimeError, match='at least as many policies'):
        draw(_Env(3, 3), 2, pinned=[0, 1, -1])
    with pytest.raises(RuntimeError, match='the env is on cpu'):
        draw(_Env(2, 3, torch.device('cpu')), 4)
    with pytest.raises(RuntimeError, match='the env is on cpu'):
        draw(_Env(3, 3, torch.device('cpu')), 2, replacement=True, pinned=[1, 1, -1])   # (legal but for the device)
    with pytest.raises(NotImplementedError, match='at most 64 snakes per env, got 65'):
        draw(_Env(65, 3), 100)
    assert env.league_draws == 0   # (a refused call draws nothing)


def test_device_plan_refusals():
    plan = _multi_league.league_plan
    env, good = _Env(2, 3), torch.zeros((2, 3), dtype=torch.long)
    with pytest.raises(RuntimeError, match='lineup is on cpu'):
        plan(env, good, 2, sync=False)
    with pytest.raises(RuntimeError, match='the env is on cpu'):
        plan(_Env(2, 3, torch.device('cpu')), good, 2, sync=False)
    with pytest.raises(RuntimeError, match='float32'):
        plan(env, good.float(), 2, sync=False)
    with pytest.raises(RuntimeError, match=r'expected \(num_snakes, num_envs\) = \(2, 3\)'):
        plan(env, good.t(), 2, sync=False)
    with pytest.raises(RuntimeError, match='num_policies must lie'):
        plan(env, good, 0, sync=False)


# ------------------------------------------------------------------ the entry points' refusals (before any HIP call)

def _draw_block(**kw):
    pins = (ctypes.c_int32 * 2)(-1, -1)
    c = _lib.LeagueDraw(tickets=0x1000, lineup=0x2000, pinned=ctypes.addressof(pins), num_envs=8, env_offset=0, seed=1,
                        call=0, num_snakes=2, num_policies=4, replacement=0, stream=None)
    c._pins = pins
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _pins(*values):
    return (ctypes.c_int32 * len(values))(*values)


def test_draw_entry_point_refusals():
    fn = _lib.lib().wurm_multi_league_draw

    def call(**kw):
        block = _draw_block(**kw)   # (kept alive across the call: `addressof` holds no reference)
        return fn(ctypes.addressof(block))

    assert fn(None) == _lib.ERR_INVALID_ARG
    assert call(num_envs=0) == _lib.OK and call(num_envs=0, lineup=None, tickets=None, pinned=None) == _lib.OK
    for kw in (dict(num_envs=-1), dict(env_offset=-1), dict(num_snakes=0), dict(num_snakes=-2), dict(num_policies=0),
               dict(num_policies=-4), dict(lineup=None), dict(num_policies=1), dict(num_snakes=5)):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    for values in ((4, -1), (-2, 0), (1, 1)):
        p = _pins(*values)
        assert call(pinned=ctypes.addressof(p)) == _lib.ERR_INVALID_ARG, values
    for kw in (dict(num_snakes=65, num_policies=100), dict(num_envs=2 ** 30), dict(env_offset=2 ** 32 - 7),
               dict(num_snakes=65, num_policies=100, num_envs=0)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
    p = _pins(1, 1)    # with replacement a policy may be pinned twice, and fewer policies than seats will do: but no rows
    assert call(pinned=ctypes.addressof(p), replacement=1, num_envs=0) == _lib.OK
    assert call(num_policies=1, replacement=1, num_envs=0) == _lib.OK


def _plan_block(**kw):
    c = _lib.LeaguePlanCall(lineup=0x1000, order=0x2000, offsets=0x3000, dropped=0x4000, workspace=0x5000,
                            workspace_bytes=1 << 20, num_rows=24, num_policies=4, lineup_dtype=_lib.LINEUP_I64, stream=None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_plan_entry_point_refusals():
    l = _lib.lib()
    fn, size = l.wurm_multi_league_plan, l.wurm_multi_league_plan_workspace_bytes

    def call(**kw):
        block = _plan_block(**kw)   # (kept alive across the call: `addressof` holds no reference)
        return fn(ctypes.addressof(block))

    assert fn(None) == _lib.ERR_INVALID_ARG
    assert call(num_rows=0) == _lib.OK
    assert call(num_rows=0, lineup=None, order=None, offsets=None, dropped=None, workspace=None, workspace_bytes=0) == _lib.OK
    need = size(24, 4)
    for kw in (dict(num_rows=-1), dict(num_policies=0), dict(num_policies=-1), dict(lineup_dtype=-1), dict(lineup_dtype=5),
               dict(lineup=None), dict(order=None), dict(offsets=None), dict(dropped=None), dict(workspace=None),
               dict(workspace=0x5004), dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace_bytes=-8)):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(num_rows=2 ** 31) == _lib.ERR_UNSUPPORTED
    # the query: sized from the two numbers alone, 0 for what the call refuses
    assert need == 24   # one chunk of 4 counts and one tile sum, rounded up to 8 bytes
    assert size(64, 300) == (300 + 2) * 4 and size(65, 300) == (2 * 300 + 2) * 4
    assert size(16384, 256) == (256 * 256 + 1) * 4 + 4 and size(16385, 256) == (129 * 256 + 1) * 4 + 4
    assert size(-1, 4) == 0 and size(2 ** 31, 4) == 0 and size(24, 0) == 0 and size(0, 4) == 8
    assert size(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 40


def test_symbols_and_constants():
    assert {'wurm_multi_league_draw', 'wurm_multi_league_plan', 'wurm_multi_league_plan_workspace_bytes'} <= set(_lib.SYMBOLS)
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), 'include', 'wurm_hip.h')).read()
    assert f'#define WURM_LEAGUE_PLAN_LAUNCHES {_lib.LEAGUE_PLAN_LAUNCHES}\n' in header
    for name, value in (('I64', _lib.LINEUP_I64), ('I32', _lib.LINEUP_I32), ('I16', _lib.LINEUP_I16),
                        ('I8', _lib.LINEUP_I8), ('U8', _lib.LINEUP_U8)):
        assert f'#define WURM_LINEUP_{name} {value}\n' in header
    assert ctypes.sizeof(_lib.LeagueDraw) == 80 and ctypes.sizeof(_lib.LeaguePlanCall) == 72
