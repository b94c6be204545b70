"""MultiSnake.policy_window — act, step and reset a whole window in one launch — against `act_window`.

The reference of every comparison is a `copy.deepcopy` twin of the env driven through `act_window` with the same `params`;
every key of the two dicts is compared with `torch.equal`: no tolerance anywhere.  Shapes are the smallest at which the
kernel can go wrong: one env, fewer envs than waves of a workgroup, one env past a workgroup multiple (`_policy_window_wpb`
forces 2 and 4 envs per workgroup on batches this small), K = 1 .. 4, every P the env accepts including the uneven K = 3,
P = 2, sizes 8 .. 12, partial_0 .. partial_3, T = 0, 1, 5 and 70, the RESIDENT form with 1, 2 and 4 heads and the RELOAD
form (4 species at partial_3).

Event coverage is a condition on the inputs, asserted on the TWIN's output (`_events`): the event cases are crowded boards
(3 - 4 snakes on 8 x 8 and 9 x 9, 65 / 130 envs, T = 70) on which snakes die, whole envs are rebuilt and food is eaten within
a handful of steps whatever the policy; one of them acts with sharpened policies (weights x 4), whose snakes hold a course.
"""
import copy

import pytest
import torch

from wurm_amd import _lib
from wurm_amd.envs import MultiSnake, _multi_act, _multi_frames

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours', 'boost_this_step')
INFO = tuple(name for name, _, _ in _multi_act.INFO_KEYS)
BASE = ('observations', 'actions', 'probs', 'values', 'rewards', 'dones', 'all_done', 'state')


def launches():
    return int(_lib.lib().wurm_launch_count())


def make_env(K, S, N, mode, seed, env_offset=0, **options):
    # manual_setup + reset: the constructor's own two calls without its RuntimeError for a snake that found no room
    env = MultiSnake(num_envs=N, num_snakes=K, size=S, observation_mode=mode, device=DEV, seed=seed, env_offset=env_offset,
                     manual_setup=True, **options)
    env.reset(torch.ones(N, dtype=torch.bool, device=DEV), return_observations=False)
    return env


def make_params(P, mode, seed, scale=0.3):
    E = 3 * (2 * int(mode.split('_')[1]) + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((P, _multi_act.num_policy_params(E)), generator=g) * scale).to(DEV)


def same(out, ref, info):
    assert set(out) == set(ref) == set(BASE) | (set(INFO) if info else set())
    for k, v in ref.items():
        if k == 'state':
            assert list(out[k]) == list(v)
            for a in v:
                assert out[k][a].shape == v[a].shape and out[k][a].dtype == v[a].dtype and torch.equal(out[k][a], v[a]), (k, a)
        else:
            assert out[k].shape == v.shape and out[k].dtype == v.dtype, k
            assert torch.equal(out[k], v), k


def verdict(env):
    try:
        env.check_consistency()
        return 'ok'
    except RuntimeError as e:
        return str(e)


def same_env(env, twin):
    assert env.policy_calls == twin.policy_calls and int(env._fs.call) == int(twin._fs.call)
    assert verdict(env) == verdict(twin)
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    assert torch.equal(env.rewards, twin.rewards)


def _events(out):
    """(snakes that died, all_done resets, meals) of a window's output"""
    d = out['dones']
    died = int(d[0].sum()) + int((d[1:] & ~d[:-1]).sum())
    return died, int(out['all_done'].sum()), int((out['food'] > 0).sum()) if 'food' in out else -1


# (id, K, S, N, mode, P, T, envs per workgroup (0 = by batch size: 1), seed, env_offset, options, info, weight scale, events)
CASES = [
    ('one_env', 1, 8, 1, 'partial_0', 1, 5, 0, 11, 0, {}, False, 0.3, False),
    ('three_envs_of_four_waves', 2, 9, 3, 'partial_1', 2, 5, 4, 12, 0, {}, True, 0.3, False),
    ('past_a_workgroup_multiple', 2, 12, 65, 'partial_2', 1, 1, 4, 13, 0, {}, False, 0.3, False),
    ('uneven_species', 3, 10, 65, 'partial_2', 2, 5, 2, 14, 0, {}, True, 0.3, False),
    ('one_step', 4, 11, 3, 'partial_3', 2, 1, 0, 15, 0, {}, False, 0.3, False),
    ('no_steps', 2, 12, 3, 'partial_2', 2, 0, 0, 16, 0, {}, True, 0.3, False),
    ('four_heads', 4, 10, 130, 'partial_2', 4, 5, 4, 17, 0, {}, False, 0.3, False),
    ('three_species', 3, 9, 3, 'partial_1', 3, 5, 2, 18, 0, {}, False, 0.3, False),
    ('reload_form', 4, 12, 3, 'partial_3', 4, 5, 0, 19, 0, {}, True, 0.3, False),
    ('events_crowded', 4, 8, 65, 'partial_2', 2, 70, 4, 20, 0, {}, True, 0.3, True),
    ('events_sharp_shard', 3, 9, 130, 'partial_3', 3, 70, 2, 21, 1000, dict(agent_colours='fixed'), True, 1.2, True),
    ('training_defaults', 4, 12, 65, 'partial_3', 2, 70, 4, 22, 0, dict(food_mode='random_rate', respawn_mode='any'), True,
     0.3, True),
    ('boost', 2, 10, 65, 'partial_2', 2, 70, 4, 23, 0, dict(boost=True), True, 0.3, True),
    ('no_boost_no_death_food', 2, 9, 3, 'partial_0', 1, 70, 0, 24, 7, dict(boost=False, food_on_death_prob=0.0), True, 0.3,
     False),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_equals_act_window(case):
    _, K, S, N, mode, P, T, wpb, seed, off, options, info, scale, events = case
    env = make_env(K, S, N, mode, seed, off, **options)
    env._policy_window_wpb = wpb
    assert env.policy_window_fused(P)
    params = make_params(P, mode, seed, scale)
    state = env._observe()
    twin, again = copy.deepcopy(env), copy.deepcopy(env)
    n0 = launches()
    out = env.policy_window(params, state, T, num_species=P, info=info)
    assert launches() - n0 == (1 if T else 0)
    ref = twin.act_window(params, state, T, num_species=P, info=info)
    if events:
        died, resets, meals = _events(ref)
        print(f'{case[0]}: {died} deaths, {resets} all_done resets, {meals} meals in the twin\'s window')
        assert died > 0 and resets > 0 and meals > 0
    same(out, ref, info)
    same_env(env, twin)
    # two runs from equal copies give equal bits
    out2 = again.policy_window(params, state, T, num_species=P, info=info)
    same(out2, out, info)


def _hand_step(e, t):
    """one hand-made step + reset(done): leaves that reset postponed"""
    K, N = e.num_snakes, e.num_envs
    g = torch.Generator().manual_seed(100 + t)
    a = torch.randint(0, 8, (K, N), generator=g).to(DEV)
    obs, rewards, dones, _ = e.step({f'agent_{k}': a[k] for k in range(K)})
    e.reset(dones['__all__'], return_observations=False)
    return obs, torch.stack(list(rewards.values())), dones['__all__']


@pytest.mark.parametrize('K,S,N,mode,P,wpb', [(2, 12, 65, 'partial_2', 2, 4), (3, 8, 5, 'partial_1', 1, 0)])
def test_three_chained_windows(K, S, N, mode, P, wpb):
    T = 5
    env = make_env(K, S, N, mode, 31, boost=True)
    env._policy_window_wpb = wpb
    params = make_params(P, mode, 31)
    twin = copy.deepcopy(env)
    state = state_t = env._observe()
    for w in range(3):
        n0 = launches()
        out = env.policy_window(params, state, T, num_species=P, info=True)
        n1 = launches()
        ref = twin.act_window(params, state_t, T, num_species=P, info=True)
        if w > 0:  # (this window started behind the postponed reset of the hand-made step below: it went into the launch)
            assert n1 - n0 == 1 and launches() - n1 == 2 * T
        same(out, ref, True)
        same_env(env, twin)
        (obs, r, d), (obs_t, r_t, d_t) = _hand_step(env, w), _hand_step(twin, w)
        assert env._fs.pending and twin._fs.pending
        assert torch.equal(r, r_t) and torch.equal(d, d_t)
        for a in obs:
            assert torch.equal(obs[a], obs_t[a])
        state, state_t = obs, obs_t
    same_env(env, twin)
    # the other entry points behind a fused window: rollout, act, a reset of everything
    tape = torch.randint(0, 8, (3, K, N), generator=torch.Generator().manual_seed(5)).to(DEV)
    ro, ro_t = env.rollout(tape), twin.rollout(tape)
    for k in ro:
        assert torch.equal(ro[k], ro_t[k]), k
    a, a_t = env.act(params, env._observe(), P), twin.act(params, twin._observe(), P)
    assert torch.equal(a['actions_t'], a_t['actions_t']) and torch.equal(a['probs'], a_t['probs'])
    o, o_t = env.reset(), twin.reset()
    assert all(torch.equal(o[k], o_t[k]) for k in o)
    same_env(env, twin)


def test_fused_a2c_population_takes_the_output():
    from wurm_amd.agents import FeedforwardAgent
    from wurm_amd.rl import FusedA2CPopulation
    K, S, N, mode, P, T, E = 2, 12, 8, 'partial_2', 2, 5, 75
    env = make_env(K, S, N, mode, 41, boost=False)
    twin = copy.deepcopy(env)
    learners = []
    for _ in range(2):
        torch.manual_seed(3)
        agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV) for _ in range(P)]
        learners.append(FusedA2CPopulation(agents, lr=1e-3, gamma=0.99, entropy_coef=0.01))
    assert torch.equal(learners[0].params, learners[1].params)
    state = env._observe()
    x0 = torch.stack(list(state.values())).reshape(K * N, E)
    out = env.policy_window(learners[0].params, state, T)
    ref = twin.act_window(learners[1].params, state, T)
    same(out, ref, False)
    learners[0].update(x0, out)
    learners[1].update(x0, ref)
    assert torch.equal(learners[0].params, learners[1].params)


def test_multi_rollout_stats_takes_the_output():
    from wurm_amd.rl import MultiRolloutStats
    K, S, N, mode, P, T = 3, 9, 16, 'partial_1', 3, 20
    env = make_env(K, S, N, mode, 42)
    twin = copy.deepcopy(env)
    params = make_params(P, mode, 42)
    stats, stats_t = MultiRolloutStats(env), MultiRolloutStats(twin)
    state = env._observe()
    stats.update(env.policy_window(params, state, T, info=True))
    stats_t.update(twin.act_window(params, state, T, info=True))
    rows, rows_t = stats.read(), stats_t.read()
    assert rows[0]['steps'] == T * N and repr(rows) == repr(rows_t)


def test_record_frames_replays_a_fused_window():
    K, S, N, mode, P, T = 3, 9, 16, 'partial_2', 2, 20
    env = make_env(K, S, N, mode, 43)
    twin = copy.deepcopy(env)
    params = make_params(P, mode, 43)
    select = [N - 1, 0, 5]
    state = env._observe()
    rec, rec_t = env.record_start(select), twin.record_start(select)
    out = env.policy_window(params, state, T, num_species=P)
    ref = twin.act_window(params, state, T, num_species=P)
    res, res_t = env.record_frames(rec, out['actions']), twin.record_frames(rec_t, ref['actions'])
    assert torch.equal(res['frames'], res_t['frames']) and not res['status'].any()
    idx = torch.as_tensor(select, device=DEV)
    aidx = (idx[:, None] * K + torch.arange(K, device=DEV)).reshape(-1)
    for name, attr in zip(_multi_frames.STATE_NAMES, STATE):
        own = getattr(env, attr).index_select(0, idx if attr == 'foods' else aidx)
        assert torch.equal(res['final'][name], own), name
        assert torch.equal(res['final'][name], res_t['final'][name]), name


@pytest.mark.parametrize('how', ['partial_4', 'half', 'forced'])
def test_fallback(how):
    K, S, N, P, T = 2, 12, 8, 2, 3
    mode = 'partial_4' if how == 'partial_4' else 'partial_2'
    env = make_env(K, S, N, mode, 44, **(dict(dtype=torch.half) if how == 'half' else {}))
    if how == 'forced':
        assert env.policy_window_fused(P)
        env._force_act_window = True
    assert not env.policy_window_fused(P)
    params = make_params(P, mode, 44)
    state = env._observe()
    twin = copy.deepcopy(env)
    if how == 'half':  # what act_window refuses, policy_window refuses
        with pytest.raises(NotImplementedError):
            env.policy_window(params, state, T)
        return
    n0 = launches()
    out = env.policy_window(params, state, T, info=True)
    assert launches() - n0 == 2 * T
    same(out, twin.act_window(params, state, T, info=True), True)
    same_env(env, twin)
