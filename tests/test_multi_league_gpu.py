"""The league on the GPU (include/wurm_hip.h: wurm_multi_act_league, wurm_multi_league_scores; wurm_amd/csrc/multi_league.hpp):
`MultiSnake.act_league` row for row bit for bit the CPU oracle's (oracle/policy.c: oracle_policy_forward with the policy of
the row, oracle_policy_sample with the row's own stream), a row independent of the rest of the line-up, the block line-up
equal to `act`, one launch per call with the env left alone, `league_window` equal to the hand-written loop, and
`LeagueTable` equal to its numpy float64 restatement."""
import copy

import numpy as np
import pytest
import torch

from tests import multi_act_ref as act_ref
from tests import multi_league_ref as ref
from wurm_amd import _lib
from wurm_amd.envs import MultiSnake, _multi_act, _multi_league
from wurm_amd.rl import LeagueTable

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 7
ES = (27, 75, 363, 507)


def _env(n, K, N, seed=3, size=12, **kw):
    return MultiSnake(num_envs=N, num_snakes=K, size=size, observation_mode=f'partial_{n}', device=DEV, seed=seed,
                      boost=False, food_mode='random_rate', food_rate=0.02, respawn_mode='any', **kw)


def _league_params(A, E, used):
    """(A, num_params) numpy: sharp policies (tests/multi_act_ref.py) in the rows `used`, NaN in the rows nobody plays — a
    kernel that read one of those would show it"""
    used = sorted(set(int(a) for a in used))
    params = np.full((A, _multi_act.num_policy_params(E)), np.nan, np.float32)
    params[used] = act_ref.sharp_params(len(used), E)
    return params


def _counts_lineup(K, N, counts, seed):
    """(K, N) numpy line-up in which policy a plays counts[a] rows, scattered"""
    flat = np.repeat(np.arange(len(counts)), counts)
    assert flat.size == K * N
    return np.random.default_rng(seed).permutation(flat).reshape(K, N)


def _random_lineup(K, N, choices, seed):
    return np.random.default_rng(seed).choice(np.asarray(choices), size=(K, N))


# name -> (K, N, A, line-up, env_offset).  A workgroup takes 8 rows per pass (multi_act.hpp: MULTI_ACT_WAVES) and a policy
# gets wgps = min(ceil(K N / 8), max(1, 256 // A)) workgroups (multi_league.hpp).
SHAPES = {
    'k3_n5_a2': (3, 5, 2, _random_lineup(3, 5, [0, 1], 1), 0),
    'a5_above_k_one_unused': (2, 4, 5, _random_lineup(2, 4, [0, 1, 2, 4], 2), 0),    # (policy 3 has no rows)
    'a300_grid_above_256': (3, 4, 300, _random_lineup(3, 4, list(range(300)), 3), 0),  # 300 workgroups, >= 288 of them empty
    'rows_7_8_9': (3, 8, 3, _counts_lineup(3, 8, [7, 8, 9], 4), 0),                    # below, at, above one pass of 8 waves
    'one_policy_of_64_loops': (1, 70, 64, np.full((1, 70), 37), 0),  # wgps = 4: 32 rows per pass, 70 rows: waves loop
    'env_offset': (3, 5, 2, _random_lineup(3, 5, [0, 1], 5), 1000),
}


def _check_rows(got, params, x, lineup, call, env_offset, what):
    probs, values, actions = ref.expected_rows(params, x, lineup, SEED, call, env_offset)
    assert np.array_equal(got['probs'].cpu().numpy(), probs), (what, 'probs')
    assert np.array_equal(got['values'].cpu().numpy(), values), (what, 'values')
    assert np.array_equal(got['actions_t'].cpu().numpy(), actions), (what, 'actions')
    K, N = lineup.shape
    assert list(got['actions']) == [f'agent_{k}' for k in range(K)]
    for k in range(K):
        a = got['actions'][f'agent_{k}']
        assert a.data_ptr() == got['actions_t'][k].data_ptr() and a.shape == (N,) and a.dtype == torch.long
    return probs, actions


@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('E', ES)
def test_rows_equal_the_oracle_in_one_launch(E, shape):
    K, N, A, lineup, env_offset = SHAPES[shape]
    assert shape != 'a5_above_k_one_unused' or 3 not in lineup
    n = act_ref.OBS_N[E]
    params = _league_params(A, E, lineup.ravel())
    env = _env(n, K, N, seed=SEED, env_offset=env_offset)
    dev_params = torch.from_numpy(params).to(DEV)
    x = act_ref.random_rows(K, N, E, seed=E)
    plan = env.league_plan(torch.from_numpy(lineup).to(DEV), A)
    count = _lib.lib().wurm_launch_count
    torch.cuda.synchronize()
    before = count()
    got = env.act_league(dev_params, torch.from_numpy(x).to(DEV), plan)
    assert count() - before == 1 and env.policy_calls == 1
    _check_rows(got, params, x, lineup, 0, env_offset, shape)
    got = env.act_league(dev_params, torch.from_numpy(x).to(DEV).view(K, N, 3, 2 * n + 1, 2 * n + 1), plan)   # the image form
    assert env.policy_calls == 2
    _check_rows(got, params, x, lineup, 1, env_offset, shape + ', second call')


def test_a_row_does_not_depend_on_the_rest_of_the_lineup():
    """The rows of envs 0 .. 2 keep their policies (0 and 1); the other envs' line-up changes, then the order of the
    policies nobody in envs 0 .. 2 plays (2 and 3) in `params`."""
    E, K, N, A, keep = 75, 3, 7, 4, 3
    params = act_ref.sharp_params(A, E, scale=1.0)
    x = torch.from_numpy(act_ref.random_rows(K, N, E, seed=11)).to(DEV)
    lineup = np.concatenate([_random_lineup(K, keep, [0, 1], 6), _random_lineup(K, N - keep, [2, 3], 7)], axis=1)
    other = lineup.copy()
    other[:, keep:] = _random_lineup(K, N - keep, [0, 1, 2, 3], 8)
    assert (other[:, keep:] != lineup[:, keep:]).any()
    swapped = params[[0, 1, 3, 2]]
    env = _env(2, K, N, seed=SEED)
    results = []
    for p, l in ((params, lineup), (params, other), (swapped, lineup)):
        twin = copy.deepcopy(env)
        got = twin.act_league(torch.from_numpy(np.ascontiguousarray(p)).to(DEV), x, twin.league_plan(torch.from_numpy(l).to(DEV), A))
        results.append(got)
        _check_rows(got, p, x.cpu().numpy(), l, 0, 0, 'variant')
    first = results[0]
    for got in results[1:]:
        for key in ('probs', 'values', 'actions_t'):
            assert torch.equal(got[key][:, :keep], first[key][:, :keep]), key
    # ... and the inputs do tell the variants apart: the rows whose policy changed differ
    assert not torch.equal(results[2]['probs'][:, keep:], first['probs'][:, keep:])
    assert env.policy_calls == 0


def _played(n, K, N, steps=4):
    """(env, observations) after a few random steps with their resets: dead and respawned snakes occur"""
    env = _env(n, K, N, seed=SEED)
    obs = env.reset()
    g = torch.Generator().manual_seed(n + K + N)
    for _ in range(steps):
        actions = {f'agent_{k}': torch.randint(4, (N,), generator=g).to(DEV) for k in range(K)}
        obs, _, dones, _ = env.step(actions)
        env.reset(dones['__all__'], return_observations=False)
    return env, obs


@pytest.mark.parametrize('K,P', [(2, 2), (3, 2), (4, 1)])
def test_block_lineup_is_act(K, P):
    n, E, N = 2, 75, 9
    params = torch.from_numpy(act_ref.sharp_params(P, E)).to(DEV)
    env, obs = _played(n, K, N)
    twin = copy.deepcopy(env)
    obs_twin = {k: v.clone() for k, v in obs.items()}
    plan = env.league_plan(_multi_league.block_lineup(K, N, P, DEV), P)
    for call in range(2):
        got, want = env.act_league(params, obs, plan), twin.act(params, obs_twin)
        for key in ('actions_t', 'probs', 'values'):
            assert torch.equal(got[key], want[key]), (call, key)
        assert list(got) == list(want) and list(got['actions']) == list(want['actions'])
    assert env.policy_calls == twin.policy_calls == 2


def _same_dicts(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours')


@pytest.mark.parametrize('look_at_state', [True, False])
def test_act_league_leaves_the_env_alone(look_at_state):
    """tests/test_multi_act_gpu.py::test_act_leaves_the_env_alone with `act_league`: A acts, steps and resets; B steps the
    same actions and resets.  look_at_state: the state tensors are compared at every step (reading them applies a
    postponed reset); else only at the end, and the reset postponed behind each step must still be postponed across the
    `act_league` that follows it."""
    K, N, E, A_ = 4, 6, 75, 5
    params = torch.from_numpy(act_ref.sharp_params(A_, E)).to(DEV)
    A, B = _env(2, K, N, seed=21), _env(2, K, N, seed=21)
    plan = A.league_plan(torch.from_numpy(_random_lineup(K, N, list(range(A_)), 9)).to(DEV), A_)
    obs_a, obs_b = A.reset(), B.reset()
    _same_dicts(obs_a, obs_b, 'reset')
    count = _lib.lib().wurm_launch_count
    postponed = 0
    for t in range(6):
        pending, call = A._pending, A._call
        before = count()
        a = A.act_league(params, obs_a, plan)
        assert count() - before == 1
        assert A._pending == pending and A._call == call and A.policy_calls == t + 1
        postponed += bool(pending)
        before = count()
        out_a = A.step(a['actions'])
        if pending:
            assert count() - before == 1   # the step and the reset postponed behind the last one: still one launch
        out_b = B.step({k: v.clone() for k, v in a['actions'].items()})
        for x, y, what in zip(out_a, out_b, ('observations', 'rewards', 'dones', 'info')):
            _same_dicts(dict(x.items()), dict(y.items()), (t, what))
        A.reset(out_a[2]['__all__'], return_observations=False)
        B.reset(out_b[2]['__all__'], return_observations=False)
        obs_a = out_a[0]
        if look_at_state or t == 5:
            for name in STATE:
                assert torch.equal(getattr(A, name), getattr(B, name)), (t, name)
    assert A._call == B._call and B.policy_calls == 0
    if not look_at_state:
        assert postponed >= 4


def test_device_refusals_draw_nothing():
    E, K, N = 75, 3, 5
    env = _env(2, K, N, seed=SEED)
    params = torch.from_numpy(act_ref.sharp_params(2, E)).to(DEV)
    x = torch.from_numpy(act_ref.random_rows(K, N, E, seed=1)).to(DEV)
    plan = env.league_plan(torch.zeros((K, N), dtype=torch.long, device=DEV), 2)
    with pytest.raises(RuntimeError, match='names 3 policies but params has 2 rows'):
        env.act_league(params, x, env.league_plan(torch.zeros((K, N), dtype=torch.long, device=DEV), 3))
    with pytest.raises(RuntimeError, match='the plan is on cpu'):
        env.act_league(params, x, env.league_plan(torch.zeros((K, N), dtype=torch.long), 2))
    with pytest.raises(RuntimeError, match=r'the observations for \(3, 4\)'):
        env.act_league(params, x[:, :4].contiguous(), plan)
    with pytest.raises(RuntimeError, match=r'\[2, 2\], outside'):
        env.league_plan(torch.full((K, N), 2, device=DEV), 2)
    with pytest.raises(NotImplementedError, match='full'):
        MultiSnake(num_envs=2, num_snakes=2, size=12, device=DEV).act_league(params, None, plan)
    with pytest.raises(NotImplementedError, match='float16'):
        _env(2, 2, 2, dtype=torch.half).act_league(params, None, plan)
    with pytest.raises(_lib.WurmHipError):
        env.act_league(params.cpu(), x, plan)
    assert env.policy_calls == 0   # (a refused call draws nothing)
    one = env.act_league(params[0], x, env.league_plan(torch.zeros((K, N), dtype=torch.long, device=DEV), 1))   # 1-D params
    assert torch.equal(one['probs'], env.act_league(params, x, plan)['probs'])


# (T, N, size, n of partial_n, info)
WINDOWS = [(0, 3, 8, 1, False), (0, 1, 12, 2, True), (1, 1, 9, 2, True), (1, 65, 8, 1, False), (5, 3, 10, 1, True),
           (5, 65, 11, 2, False), (5, 65, 12, 2, True)]


@pytest.mark.parametrize('T,N,size,n,info', WINDOWS)
def test_league_window_is_the_loop(T, N, size, n, info):
    K, A = (2 if size < 10 else 3), 4     # (three snakes do not always find room on the 6 x 6 inside of size 8)
    E = 3 * (2 * n + 1) ** 2
    params = torch.from_numpy(act_ref.sharp_params(A, E)).to(DEV)
    env, twin = _env(n, K, N, seed=33, size=size), _env(n, K, N, seed=33, size=size)
    plan = env.league_plan(torch.from_numpy(_random_lineup(K, N, list(range(A)), T + N)).to(DEV), A)
    state0 = env.reset()
    count = _lib.lib().wurm_launch_count
    before = count()
    out = env.league_window(params, state0, T, plan, info=info)
    assert count() - before == 2 * T
    shapes = {'observations': (T, K * N, E), 'actions': (T, K * N), 'probs': (T, K * N, 4), 'values': (T, K * N),
              'rewards': (T, K * N), 'dones': (T, K * N), 'all_done': (T, N)}
    if info:
        shapes.update({name: (T, K * N) for name, _, _ in _multi_act.INFO_KEYS})
    assert {k: tuple(v.shape) for k, v in out.items() if k != 'state'} == shapes
    assert [out[name].dtype for name, _, _ in _multi_act.INFO_KEYS if info] == [d for _, _, d in _multi_act.INFO_KEYS if info]
    state = twin.reset()
    _same_dicts(state0, state, 'reset')
    rows = lambda d, prefix='agent_': torch.stack([d[f'{prefix}{k}'] for k in range(K)]).reshape(K * N, -1).squeeze(-1)
    for t in range(T):
        a = twin.act_league(params, state, plan)
        sampled = a['actions_t'].clone()
        obs, rewards, dones, step_info = twin.step(a['actions'])
        twin.reset(dones['__all__'], return_observations=False)
        assert torch.equal(out['actions'][t], sampled.reshape(-1)), t
        assert torch.equal(out['probs'][t], a['probs'].reshape(K * N, 4)), t
        assert torch.equal(out['values'][t], a['values'].reshape(-1)), t
        assert torch.equal(out['observations'][t], rows(obs)), t
        assert torch.equal(out['rewards'][t], rows(rewards)), t
        assert torch.equal(out['dones'][t], rows(dones)), t
        assert torch.equal(out['all_done'][t], dones['__all__']), t
        if info:
            for name, prefix, _ in _multi_act.INFO_KEYS:
                assert torch.equal(out[name][t], rows(step_info, prefix)), (t, name)
        state = obs
    _same_dicts(out['state'], state, 'last observations')
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    assert env.policy_calls == twin.policy_calls == T and env._call == twin._call


@pytest.mark.parametrize('K,P,info', [(2, 2, True), (3, 2, False), (4, 1, True)])
def test_block_lineup_window_is_act_window(K, P, info):
    T, N, n, E = 5, 6, 2, 75
    params = torch.from_numpy(act_ref.sharp_params(P, E)).to(DEV)
    env, twin = _env(n, K, N, seed=34), _env(n, K, N, seed=34)
    plan = env.league_plan(_multi_league.block_lineup(K, N, P, DEV), P)
    got = env.league_window(params, env.reset(), T, plan, info=info)
    want = twin.act_window(params, twin.reset(), T, info=info)
    assert list(got) == list(want)
    for key in want:
        if key == 'state':
            _same_dicts(got[key], want[key], key)
        else:
            assert torch.equal(got[key], want[key]), key


def test_record_frames_takes_the_window():
    T, K, N, A, n, E = 4, 3, 5, 4, 2, 75
    params = torch.from_numpy(act_ref.sharp_params(A, E)).to(DEV)
    env = _env(n, K, N, seed=35)
    plan = env.league_plan(torch.from_numpy(_random_lineup(K, N, list(range(A)), 10)).to(DEV), A)
    state = env.reset()
    select = [4, 0, 2]
    first = env._get_env_images()[select].clone()
    rec = env.record_start(select)
    out = env.league_window(params, state, T, plan)
    res = env.record_frames(rec, out['actions'])
    assert res['status'].tolist() == [0, 0, 0] and res['frames'].shape[:2] == (T + 1, 3)
    assert torch.equal(res['frames'][0], first.to(res['frames'].dtype))
    assert torch.equal(res['frames'][T], env._get_env_images()[select].to(res['frames'].dtype))


def _numpy_window(out):
    return {k: v.cpu().numpy() for k, v in out.items() if k != 'state'}


def test_league_table_is_the_float64_restatement():
    """Counts, sizes and rewards from {-1, 0, 1} (reward_on_death = -1, the default): every sum is exact in double, so the
    table equals the numpy restatement whatever the order of either: ==, no tolerance."""
    T, K, N, A, n, E = 12, 2, 65, 6, 1, 27
    params = torch.from_numpy(_league_params(A, E, [0, 1, 2, 4, 5])).to(DEV)
    lineup = _random_lineup(K, N, [0, 1, 2, 4, 5], 12)     # (policy 3 has no rows)
    tables, windows = [], []
    for run in range(2):
        env = _env(n, K, N, seed=36, size=8)
        plan = env.league_plan(torch.from_numpy(lineup).to(DEV), A)
        table = LeagueTable(A, DEV)
        state = env.reset()
        count = _lib.lib().wurm_launch_count
        for w in range(2):
            out = env.league_window(params, state, T, plan, info=True)
            before = count()
            table.update(plan, out)
            assert count() - before == 1
            state = out['state']
            if run == 0:
                windows.append(_numpy_window(out))
        tables.append(table.table.clone())
    want = ref.score_table(lineup, A, windows)
    for w in windows:   # what makes the sums exact, and the window worth summing
        assert set(np.unique(w['rewards'])) <= {-1.0, 0.0, 1.0}
        assert np.array_equal(w['size'], np.round(w['size']))
    assert want[:, 2].sum() > 0 and want[:, 3].sum() > 0 and (want[:, 1] != 0).any() and want[:, 5].sum() > 0
    got = tables[0].cpu().numpy()
    print(np.array2string(got, max_line_width=200))
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert torch.equal(tables[0], tables[1])                                 # two runs: the same bits
    assert not got[3].any() and want[[0, 1, 2, 4, 5], 0].tolist() == [float(2 * T * (lineup == a).sum()) for a in (0, 1, 2, 4, 5)]
    rows = table.read()
    assert len(rows) == A and [rows[4][c] for c in ref.COLUMNS] == want[4].tolist()
    assert rows[4]['reward_per_step'] == want[4, 1] / want[4, 0] and np.isnan(rows[3]['reward_per_step'])
    # a window without the info=True keys adds to steps, reward and deaths only
    plain = LeagueTable(A, DEV)
    out = env.league_window(params, state, 3, plan)
    plain.update(plan, out)
    got = plain.table.cpu().numpy()
    assert np.array_equal(got, ref.score_table(lineup, A, [_numpy_window(out)])) and not got[:, 3:].any() and got[:, 0].any()
    plain.reset()
    assert not bool(plain.table.any())
    before = count()
    plain.update(plan, env.league_window(params, state, 0, plan))           # an empty window: nothing to add, no launch
    assert count() - before == 0 and not bool(plain.table.any())
