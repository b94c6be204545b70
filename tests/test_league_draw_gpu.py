"""The league's matchmaking on the GPU (include/wurm_hip.h: wurm_multi_league_draw, wurm_multi_league_plan; kernels:
wurm_amd/csrc/multi_matchmaking.hpp): `MultiSnake.league_draw` equal to the Python restatement (tests/league_draw_ref.py)
entry for entry, its counters, `league_plan(sync=False)` equal to the torch path bit for bit with rows out of range dropped
and counted, the number of launches the header states, a league window, update and table on a drawn plan equal to the
same on the torch plan of that line-up, and both calls and both entry points behind the stream gate
(tests/stream_gate.py) — their stream cases live here, not in tests/stream_cases.py: the prototypes take an argument
block, whose last member is the stream."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from tests import league_draw_ref as ref
from tests import stream_gate
from tests.stream_gate import Case
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.envs import MultiSnake
from wurm_amd.envs._multi_league import LeaguePlan
from wurm_amd.rl import FusedA2CPopulation, LeagueTable

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 7
PLAN_LAUNCHES = _lib.LEAGUE_PLAN_LAUNCHES


def _env(K, N, seed=SEED, size=12, **kw):
    return MultiSnake(num_envs=N, num_snakes=K, size=size, observation_mode='partial_2', device=DEV, seed=seed,
                      boost=False, food_mode='random_rate', food_rate=0.02, respawn_mode='any', **kw)


def _count():
    return _lib.lib().wurm_launch_count()


# ------------------------------------------------------------------ the drawn line-up

# (K, N, A): one env, more than a workgroup of envs, policies beyond the 256 the kernel stages in LDS, K above 4 (the
# kernel with 16 seats)
SHAPES = [(1, 1, 1), (2, 1, 2), (3, 65, 3), (4, 257, 16), (2, 700, 300), (10, 64, 12)]


def _tickets(A, seed):
    """zeros and negatives among them; A = 1: the lone policy without a ticket (the uniform fall-back)"""
    t = np.random.default_rng(seed).choice([-3, 0, 0, 1, 2, 7, 50], size=A)
    if A > 2:
        t[0], t[1], t[A - 1] = 0, -5, 9
    return [int(x) for x in t]


def _pins(K, A):
    pins = [-1] * K
    pins[K - 1] = A - 1
    if K >= 3:
        pins[0] = 0
    return pins


# what, tickets, pins
VARIANTS = [('plain', False, False), ('tickets', True, False), ('pins', False, True), ('tickets+pins', True, True)]


@pytest.mark.parametrize('env_offset', [0, 1000])
@pytest.mark.parametrize('variant', VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize('replacement', [False, True], ids=['distinct', 'replacement'])
@pytest.mark.parametrize('K,N,A', SHAPES)
def test_lineup_equals_the_restatement(K, N, A, replacement, variant, env_offset):
    _, with_tickets, with_pins = variant
    tickets = _tickets(A, K + N + A) if with_tickets else None
    pins = _pins(K, A) if with_pins else None
    env = _env(K, N, env_offset=env_offset, size=12 if K <= 6 else 25 if K <= 16 else 36)
    dev_tickets = None if tickets is None else torch.tensor(tickets, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    before = _count()
    plan = env.league_draw(A, tickets=dev_tickets, replacement=replacement, pinned=pins)
    assert _count() - before == 1 + PLAN_LAUNCHES and env.league_draws == 1
    want = ref.draw(K, N, A, SEED, 0, env_offset, tickets, replacement, pins)
    assert isinstance(plan, LeaguePlan) and plan.num_policies == A
    assert plan.lineup.dtype == torch.int64 and plan.lineup.shape == (K, N) and plan.lineup.device == env.device
    assert torch.equal(plan.lineup.cpu(), torch.from_numpy(want))
    order, offsets, dropped = ref.plan(want, A)
    assert dropped == 0 and int(env.league_dropped) == 0
    assert plan.order.dtype == torch.int32 and plan.order.tolist() == order
    assert plan.offsets.dtype == torch.int64 and plan.offsets.tolist() == offsets
    if not replacement:
        assert all(len(set(col)) == K for col in want.T.tolist())


@pytest.mark.parametrize('replacement', [False, True], ids=['distinct', 'replacement'])
@pytest.mark.parametrize('K,N,A', [(17, 5, 20), (33, 3, 40)])
def test_more_than_16_seats(K, N, A, replacement):
    """league_draw_kernel<64> serves 17 .. 64 snakes per env: tickets, pins and an env_offset at once"""
    test_lineup_equals_the_restatement(K, N, A, replacement, VARIANTS[3], 1000)
    test_lineup_equals_the_restatement(K, N, A, replacement, VARIANTS[0], 0)


def test_a_shard_draws_its_rows_of_the_whole_batch():
    K, A, tickets = 3, 5, torch.tensor([4, 0, 1, 1, 9], dtype=torch.int32, device=DEV)
    whole = _env(K, 100).league_draw(A, tickets=tickets, pinned=[-1, 2, -1]).lineup
    shard = _env(K, 30, env_offset=40).league_draw(A, tickets=tickets, pinned=[-1, 2, -1]).lineup
    assert torch.equal(shard, whole[:, 40:70])
    assert not torch.equal(_env(K, 30, env_offset=41).league_draw(A, tickets=tickets, pinned=[-1, 2, -1]).lineup, shard)


def test_counters():
    K, N, A = 3, 40, 6
    env = _env(K, N)
    env.reset()
    twin = copy.deepcopy(env)
    call, policy_calls = env._call, env.policy_calls
    first, second = env.league_draw(A), env.league_draw(A)
    assert env.league_draws == 2 and (env._call, env.policy_calls) == (call, policy_calls)
    assert not torch.equal(first.lineup, second.lineup)                 # two chained draws differ
    assert torch.equal(twin.league_draw(A).lineup, first.lineup)        # a twin at the same counter matches
    restored = pickle.loads(pickle.dumps(twin))
    assert restored.league_draws == twin.league_draws == 1
    assert torch.equal(restored.league_draw(A).lineup, second.lineup)
    assert torch.equal(second.lineup.cpu(), torch.from_numpy(ref.draw(K, N, A, SEED, 1)))
    with pytest.raises(RuntimeError, match='pinned twice'):
        env.league_draw(A, pinned=[1, 1, -1])
    assert env.league_draws == 2                                        # (a refused call draws nothing)
    # a state saved before there was a draw counter: it starts at 0
    state = twin.__getstate__()
    del state['league_draws'], state['league_dropped']
    old = MultiSnake.__new__(MultiSnake)
    old.__setstate__(state)
    assert old.league_draws == 0 and old.league_dropped is None
    assert torch.equal(old.league_draw(A).lineup, first.lineup) and int(old.league_dropped) == 0


STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours')


def test_a_draw_leaves_the_env_alone():
    """A steps, postpones its reset, draws, steps on; B never draws: the same trajectory, and the reset postponed in
    front of a draw is still postponed behind it"""
    K, N, A_ = 3, 6, 5
    A, B = _env(K, N, seed=21), _env(K, N, seed=21)
    A.reset(), B.reset()
    g = torch.Generator().manual_seed(3)
    postponed = 0
    for t in range(6):
        actions = {f'agent_{k}': torch.randint(4, (N,), generator=g).to(DEV) for k in range(K)}
        out_a, out_b = A.step(actions), B.step({k: v.clone() for k, v in actions.items()})
        A.reset(out_a[2]['__all__'], return_observations=False)
        B.reset(out_b[2]['__all__'], return_observations=False)
        pending, call = A._pending, A._call
        A.league_draw(A_)
        assert A._pending == pending and A._call == call and A.league_draws == t + 1
        postponed += bool(pending)
        for x, y in zip(out_a[:3], out_b[:3]):
            for key in x:
                assert torch.equal(x[key], y[key]), (t, key)
    for name in STATE:
        assert torch.equal(getattr(A, name), getattr(B, name)), name
    assert A._call == B._call and A.policy_calls == B.policy_calls == 0 and B.league_draws == 0 and postponed >= 4


# ------------------------------------------------------------------ league_plan(sync=False)

ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 4097]


class _Shape(object):
    """what the two forms of `league_plan` read of an env (num_snakes, num_envs, device; `league_dropped` is given to
    it): the builder is a function of the line-up alone, and no MultiSnake has to be made for 4097 rows"""
    league_dropped = None
    league_plan = MultiSnake.league_plan

    def __init__(self, K, N):
        self.num_snakes, self.num_envs, self.device = K, N, torch.device(DEV)


def _shape_of(rows):
    """(K, N) with K N = rows, K > 1 where rows allows"""
    for K in (4, 3, 5, 17, 241):
        if rows % K == 0 and rows > K:
            return K, rows // K
    return 1, rows


def _lineup(rows, A, kind, seed):
    g = np.random.default_rng(seed)
    if kind == 'random':
        flat = g.integers(0, A, rows)
    elif kind == 'one':           # all rows on one policy
        flat = np.full(rows, A - 1)
    elif kind == 'sparse':        # policies without rows
        flat = g.integers(0, 2, rows) * (A - 1)
    else:
        raise ValueError(kind)
    return flat.astype(np.int64)


def _same_plan(got, want, what):
    assert got.order.dtype == want.order.dtype == torch.int32 and got.offsets.dtype == want.offsets.dtype == torch.int64, what
    assert torch.equal(got.order, want.order), what
    assert torch.equal(got.offsets, want.offsets), what
    assert got.num_policies == want.num_policies and got.order.device == want.order.device


@pytest.mark.parametrize('A,kind', [(1, 'one'), (2, 'random'), (7, 'random'), (7, 'one'), (7, 'sparse'), (300, 'random'),
                                    (300, 'sparse'), (5000, 'random')])
@pytest.mark.parametrize('rows', ROWS)
def test_device_plan_equals_the_torch_plan(rows, A, kind):
    K, N = _shape_of(rows)
    env = _Shape(K, N)
    lineup = torch.from_numpy(_lineup(rows, A, kind, rows + A).reshape(K, N)).to(DEV)
    want = env.league_plan(lineup, A)
    torch.cuda.synchronize()
    before = _count()
    got = env.league_plan(lineup, A, sync=False)
    assert _count() - before == PLAN_LAUNCHES
    _same_plan(got, want, (rows, A, kind))
    assert got.lineup is lineup and int(env.league_dropped) == 0
    assert (got.order.tolist(), got.offsets.tolist(), 0) == ref.plan(lineup.cpu().numpy(), A)


# Above 16384 rows a chunk has more than 64 rows (L = 128, 192 and 448 here) and its wave makes several steps: a step reads
# the counts the step before moved on, through global memory.  Few policies: every step has many lanes per policy.
LONG_ROWS = [16385, 40000, 99999]


@pytest.mark.parametrize('A,kind', [(1, 'one'), (2, 'random'), (3, 'random'), (3, 'sparse'), (300, 'random')])
@pytest.mark.parametrize('rows', LONG_ROWS)
def test_chunks_of_several_steps(rows, A, kind):
    chunks = (_lib.lib().wurm_multi_league_plan_workspace_bytes(rows, 3) // 4 - 1) // 3   # (C * 3 + 1 words, rounded up to 8 bytes)
    assert chunks <= 256 and chunks * 64 < rows                                             # a chunk is more than one step
    test_device_plan_equals_the_torch_plan(rows, A, kind)


def test_twelve_rows_among_300_policies():
    env = _Shape(3, 4)
    lineup = torch.from_numpy(_lineup(12, 300, 'random', 5).reshape(3, 4)).to(DEV)
    _same_plan(env.league_plan(lineup, 300, sync=False), env.league_plan(lineup, 300), 'a300')


@pytest.mark.parametrize('dtype', [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_every_integer_dtype(dtype):
    K, N, A = 3, 43, 100
    env = _Shape(K, N)
    lineup = torch.from_numpy(_lineup(K * N, A, 'random', 9).reshape(K, N)).to(DEV).to(dtype)
    _same_plan(env.league_plan(lineup, A, sync=False), env.league_plan(lineup, A), dtype)
    # a wide type with entries far outside the range, a byte that would be negative as a signed one
    if dtype == torch.uint8:
        lineup[0, :5] = 200
        got = env.league_plan(lineup, 201, sync=False)
        _same_plan(got, env.league_plan(lineup, 201), 'uint8 200')
        assert int(env.league_dropped) == 0 and int(got.offsets[201] - got.offsets[200]) == 5


@pytest.mark.parametrize('rows', [1, 65, 1025, 4097] + LONG_ROWS)
@pytest.mark.parametrize('A', [3, 300])
def test_rows_out_of_range_are_dropped_and_counted(rows, A):
    K, N = _shape_of(rows)
    env = _Shape(K, N)
    flat = _lineup(rows, A, 'random', rows * A)
    bad = np.random.default_rng(rows).random(rows) < 0.3
    bad[0] = True
    flat[bad] = np.random.default_rng(A).choice([-1, -2 ** 40, A, A + 1, 2 ** 31, 2 ** 62], size=int(bad.sum()))
    lineup = torch.from_numpy(flat.reshape(K, N)).to(DEV)
    got = env.league_plan(lineup, A, sync=False)
    order, offsets, dropped = ref.plan(flat, A)
    assert dropped == int(bad.sum()) and int(env.league_dropped) == dropped
    assert got.order.tolist() == order and got.offsets.tolist() == offsets
    assert got.order.shape == (rows,) and (got.order[offsets[A]:] == -1).all() and (got.order[:offsets[A]] >= 0).all()
    # the lists are the torch plan's of the rows that are left
    keep = torch.from_numpy(~bad)
    kept = torch.from_numpy(flat)[keep]
    rows_kept = torch.arange(rows)[keep]
    assert torch.equal(got.order[:offsets[A]].cpu().long(), rows_kept[torch.sort(kept, stable=True).indices])
    # ... and a call on a line-up in range rewrites the count
    env.league_plan(torch.zeros((K, N), dtype=torch.long, device=DEV), A, sync=False)
    assert int(env.league_dropped) == 0


def test_no_rows_is_a_plan_without_a_launch():
    env = _Shape(2, 0)
    before = _count()
    got = env.league_plan(torch.zeros((2, 0), dtype=torch.long, device=DEV), 3, sync=False)
    assert _count() == before and got.order.shape == (0,) and got.offsets.tolist() == [0, 0, 0, 0]
    assert int(env.league_dropped) == 0


# ------------------------------------------------------------------ end to end

def test_a_drawn_plan_plays_learns_and_scores_as_the_torch_plan_of_its_lineup():
    K, N, A, T, E = 2, 8, 4, 3, 75
    results = []
    for drawn in (True, False):
        env = _env(K, N, seed=33)
        agents = []
        for a in range(A):
            torch.manual_seed(20 + a)
            agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
        pop, table = FusedA2CPopulation(agents, lr=1e-3, gamma=0.99, entropy_coef=0.01), LeagueTable(A, env.device)
        plan = env.league_draw(A, tickets=torch.tensor([3, 1, 0, 2], dtype=torch.int32, device=DEV))
        if not drawn:
            plan = env.league_plan(plan.lineup.clone(), A)
        state = env.reset()
        for _ in range(2):
            out = env.league_window(pop.params, state, T, plan, info=True)
            res = pop.update(state, out, plan=plan)
            table.update(plan, out)
            state = out['state']
        results.append((plan, out, res, pop.params.clone(), table.table.clone()))
    (plan_a, out_a, res_a, params_a, table_a), (plan_b, out_b, res_b, params_b, table_b) = results
    _same_plan(plan_a, plan_b, 'plans')
    assert torch.equal(plan_a.lineup, plan_b.lineup) and len(set(plan_a.lineup.reshape(-1).tolist())) > 1
    for key in out_a:
        if key != 'state':
            assert torch.equal(out_a[key], out_b[key]), key
    for key in res_a:
        if isinstance(res_a[key], torch.Tensor):
            assert torch.equal(stream_gate._bits(res_a[key]), stream_gate._bits(res_b[key])), key
    assert torch.equal(params_a, params_b) and torch.equal(table_a, table_b) and float(table_a[:, 0].sum()) == 2 * T * K * N


# ------------------------------------------------------------------ behind the stream gate

_K, _N, _A = 3, 70, 9


def _ticket_inputs(seed):
    return (torch.tensor(_tickets(_A, seed), dtype=torch.int32, device=DEV),)


def _lineup_inputs(seed):
    flat = _lineup(_K * _N, _A, 'random', seed)
    flat[seed::7] = _A + seed      # rows out of range: `dropped` is an output too
    return (torch.from_numpy(flat.reshape(_K, _N)).to(DEV),)


def _plan_dict(env, plan):
    return dict(lineup=plan.lineup, order=plan.order, offsets=plan.offsets, dropped=env.league_dropped)


def _raw_draw(x, inputs):
    pins = (ctypes.c_int32 * _K)(-1, 4, -1)
    c = _lib.LeagueDraw(_lib.ptr(inputs[0]), _lib.ptr(x['lineup']), ctypes.addressof(pins), _N, 5, 99, 2, _K, _A, 0,
                        _lib.stream_ptr(0))
    assert _lib.lib().wurm_multi_league_draw(ctypes.addressof(c)) == _lib.OK
    return dict(x)


def _raw_plan_buffers():
    nbytes = _lib.lib().wurm_multi_league_plan_workspace_bytes(_K * _N, _A)
    return dict(order=torch.zeros(_K * _N, dtype=torch.int32, device=DEV), offsets=torch.zeros(_A + 1, dtype=torch.long, device=DEV),
                dropped=torch.zeros((), dtype=torch.int32, device=DEV), workspace=torch.zeros(nbytes // 8, dtype=torch.long, device=DEV))


def _raw_plan(x, inputs):
    c = _lib.LeaguePlanCall(_lib.ptr(inputs[0]), _lib.ptr(x['order']), _lib.ptr(x['offsets']), _lib.ptr(x['dropped']),
                            _lib.ptr(x['workspace']), x['workspace'].numel() * 8, _K * _N, _A, _lib.LINEUP_I64, _lib.stream_ptr(0))
    assert _lib.lib().wurm_multi_league_plan(ctypes.addressof(c)) == _lib.OK
    return {k: v for k, v in x.items() if k != 'workspace'}


_BOTH = ('wurm_multi_league_draw', 'wurm_multi_league_plan')
STREAM_CASES = [
    Case('MultiSnake.league_draw', lambda: _env(_K, _N),
         lambda env, inputs: _plan_dict(env, env.league_draw(_A, tickets=inputs[0], pinned=[-1, 4, -1])),
         lambda: _ticket_inputs(1), lambda: _ticket_inputs(2), _BOTH, min_launches=1 + PLAN_LAUNCHES),
    Case('MultiSnake.league_plan(sync=False)', lambda: _env(_K, _N),
         lambda env, inputs: _plan_dict(env, env.league_plan(inputs[0], _A, sync=False)),
         lambda: _lineup_inputs(1), lambda: _lineup_inputs(2), _BOTH[1:], min_launches=PLAN_LAUNCHES),
    Case('abi wurm_multi_league_draw', lambda: dict(lineup=torch.zeros((_K, _N), dtype=torch.long, device=DEV)), _raw_draw,
         lambda: _ticket_inputs(1), lambda: _ticket_inputs(2), _BOTH[:1], min_launches=1),
    Case('abi wurm_multi_league_plan', _raw_plan_buffers, _raw_plan, lambda: _lineup_inputs(1), lambda: _lineup_inputs(2),
         _BOTH[1:], min_launches=PLAN_LAUNCHES),
]


@pytest.mark.parametrize('case', STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_stream_case(case):
    """gate still closed on return, outputs equal to the default-stream run (tests/test_stream_gate_gpu.py: test_case)"""
    try:
        stream_gate.run_case(case)
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):   # nothing more is started on a device that faulted
            pytest.exit(f'{case.name}: {e}', returncode=3)
        raise


def test_the_stream_cases_cover_both_entry_points():
    covered = set()
    for case in STREAM_CASES:
        covered.update(case.covers)
    assert covered == set(_BOTH)
