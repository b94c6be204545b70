"""`MultiSnake.act` / `act_window` on the GPU (include/wurm_hip.h: wurm_multi_act; wurm_amd/csrc/multi_act.hpp): every row
bit for bit the CPU oracle's (oracle/policy.c: oracle_policy_forward, oracle_policy_sample), one launch per call, the env
left alone, the window equal to the hand-written loop and accepted by FusedA2CPopulation."""
import copy

import numpy as np
import pytest
import torch

from tests import a2c_learner_ref as learner_ref
from tests import multi_act_ref as ref
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.envs import MultiSnake
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 7
ES = sorted(ref.OBS_N)

# (K, N, num_species).  A workgroup takes 8 rows per pass (multi_act.hpp: MULTI_ACT_WAVES) and a species gets at most
# 256 // num_species workgroups: K N = 7, 8, 9 rows of one species sit below, at and one above one pass of one workgroup;
# (2, 4, 2) is two species of half a pass; (5, 500, 5) and (1, 2100, 1) have more rows per species than one pass of all its
# workgroups (51 x 8 = 408, 256 x 8 = 2048), so waves walk to a second row — some of them, and all of them plus a few.
CASES = [(2, 3, 2), (4, 1, 1), (3, 7, 3), (4, 17, 2), (5, 13, 1), (5, 13, 2), (5, 13, 5),
         (1, 7, 1), (2, 4, 1), (3, 3, 1), (2, 4, 2), (5, 500, 5), (1, 2100, 1)]
ENV_CASES = [(3, 7, 3), (4, 17, 2)]   # also on the observations of a real env


def _env(n, K, N, seed=3, **kw):
    return MultiSnake(num_envs=N, num_snakes=K, size=12, observation_mode=f'partial_{n}', device=DEV, seed=seed,
                      boost=False, food_mode='random_rate', food_rate=0.02, respawn_mode='any', **kw)


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


def _check_rows(got, params, x, P, call, env_offset, what):
    probs, values, actions = ref.expected_rows(params, x, P, SEED, call, env_offset)
    assert np.array_equal(got['probs'].cpu().numpy(), probs), (what, 'probs')
    assert np.array_equal(got['values'].cpu().numpy(), values), (what, 'values')
    assert np.array_equal(got['actions_t'].cpu().numpy(), actions), (what, 'actions')
    K = x.shape[0]
    assert list(got['actions']) == [f'agent_{k}' for k in range(K)]
    for k in range(K):
        a = got['actions'][f'agent_{k}']
        assert a.data_ptr() == got['actions_t'][k].data_ptr() and a.shape == (x.shape[1],) and a.dtype == torch.long
    return probs, actions


@pytest.mark.parametrize('K,N,P', CASES)
@pytest.mark.parametrize('E', ES)
def test_rows_equal_the_oracle_in_one_launch(E, K, N, P):
    n = ref.OBS_N[E]
    params = ref.sharp_params(P, E)
    env = _env(n, K, 2, seed=SEED)     # (the tensor form takes its N from the tensor)
    dev_params = torch.from_numpy(params).to(DEV)
    x = ref.random_rows(K, N, E, seed=E)
    count = _lib.lib().wurm_launch_count
    before = count()
    got = env.act(dev_params, torch.from_numpy(x).to(DEV))
    assert count() - before == 1 and env.policy_calls == 1
    probs, actions = _check_rows(got, params, x, P, 0, 0, 'random rows')
    if (K, N, P) == (4, 17, 2):   # the inputs exercise the sampler: every action, and probabilities far from uniform
        assert set(actions.ravel()) == {0, 1, 2, 3} and probs.min() < 1e-3
    if (K, N, P) in ENV_CASES:
        penv, obs = _played(n, K, N)
        before = count()
        got = penv.act(dev_params, obs)                                    # the dict `step` returned, in place
        assert count() - before == 1
        x = torch.stack(list(obs.values())).reshape(K, N, E)
        _check_rows(got, params, x.cpu().numpy(), P, 0, 0, 'env rows (dict)')
        got = penv.act(dev_params, x.view(K, N, 3, 2 * n + 1, 2 * n + 1))  # the image form of the tensor
        _check_rows(got, params, x.cpu().numpy(), P, 1, 0, 'env rows (tensor)')
        loose = {k: v.clone() for k, v in obs.items()}                     # not one buffer: stacked once
        got = penv.act(dev_params, loose)
        _check_rows(got, params, x.cpu().numpy(), P, 2, 0, 'env rows (loose dict)')


def test_single_species_params_may_be_one_dimensional():
    E, K, N = 75, 3, 5
    params = ref.sharp_params(1, E)
    env = _env(2, K, N, seed=SEED)
    x = ref.random_rows(K, N, E, seed=1)
    got = env.act(torch.from_numpy(params[0]).to(DEV), torch.from_numpy(x).to(DEV))
    _check_rows(got, params, x, 1, 0, 0, '1-D params')
    with pytest.raises(RuntimeError, match='num_species 4'):
        env.act(torch.from_numpy(params).to(DEV), torch.from_numpy(x).to(DEV), num_species=4)
    with pytest.raises(RuntimeError, match=r'\(2, 5, 75\)'):
        env.act(torch.from_numpy(params).to(DEV), torch.from_numpy(x[:2]).to(DEV))
    with pytest.raises(NotImplementedError, match='full'):
        MultiSnake(num_envs=2, num_snakes=2, size=12, device=DEV).act(torch.from_numpy(params).to(DEV), None)
    with pytest.raises(NotImplementedError, match='float16'):
        _env(2, 2, 2, dtype=torch.half).act(torch.from_numpy(params).to(DEV), None)
    with pytest.raises(_lib.WurmHipError):
        env.act(torch.from_numpy(params), torch.from_numpy(x).to(DEV))
    assert env.policy_calls == 1   # (a refused call draws nothing)


def test_counter_offset_and_repeatability():
    E, K, N, P = 147, 4, 9, 2
    params = ref.sharp_params(P, E, scale=1.0)   # (probabilities near uniform: other uniforms give other actions — the
                                                 # oracle differs in 23 of the 36 rows between calls, in 27 with the offset)
    dev_params = torch.from_numpy(params).to(DEV)
    x = ref.random_rows(K, N, E, seed=2)
    dev_x = torch.from_numpy(x).to(DEV)
    env = _env(3, K, N, seed=SEED)
    first, second = env.act(dev_params, dev_x), env.act(dev_params, dev_x)
    assert env.policy_calls == 2
    _check_rows(first, params, x, P, 0, 0, 'call 0')
    _check_rows(second, params, x, P, 1, 0, 'call 1')
    assert torch.equal(first['probs'], second['probs']) and not torch.equal(first['actions_t'], second['actions_t'])
    shifted = _env(3, K, N, seed=SEED, env_offset=1000)
    got = shifted.act(dev_params, dev_x)
    _check_rows(got, params, x, P, 0, 1000, 'env_offset 1000')
    assert not torch.equal(got['actions_t'], first['actions_t'])
    again = _env(3, K, N, seed=SEED)
    for want in (first, second):
        got = again.act(dev_params, dev_x)
        assert all(torch.equal(got[k], want[k]) for k in ('actions_t', 'probs', 'values'))
    # the counter travels with a copy of the env
    assert copy.deepcopy(env).policy_calls == 2


def test_no_rows_no_launch():
    E, K = 75, 3
    env = _env(2, K, 4)
    params = torch.from_numpy(ref.sharp_params(2, E)).to(DEV)
    before = _lib.lib().wurm_launch_count()
    got = env.act(params, torch.empty((K, 0, E), device=DEV))
    assert _lib.lib().wurm_launch_count() == before
    assert got['actions_t'].shape == (K, 0) and got['probs'].shape == (K, 0, 4) and got['values'].shape == (K, 0)
    assert [a.shape for a in got['actions'].values()] == [(0,)] * K


def _same_dicts(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours')


@pytest.mark.parametrize('look_at_state', [True, False])
def test_act_leaves_the_env_alone(look_at_state):
    """A acts, steps and resets; B steps the same actions and resets.  look_at_state: the state tensors are compared at
    every step (reading them applies a postponed reset); else only at the end, and the reset postponed behind each step
    must still be postponed across the `act` that follows it."""
    K, N, E = 4, 6, 75
    params = torch.from_numpy(ref.sharp_params(2, E)).to(DEV)
    A, B = _env(2, K, N, seed=21), _env(2, K, N, seed=21)
    obs_a, obs_b = A.reset(), B.reset()
    _same_dicts(obs_a, obs_b, 'reset')
    count = _lib.lib().wurm_launch_count
    postponed = 0
    for t in range(6):
        pending, call = A._pending, A._call
        a = A.act(params, obs_a)
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


def _agents(P, E):
    agents = []
    for p in range(P):
        torch.manual_seed(10 + p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
    return agents


def test_act_window_is_the_loop_and_feeds_the_population():
    T, K, N, P, E = 5, 4, 6, 2, 75
    pop = FusedA2CPopulation(_agents(P, E), entropy_coef=0.01)
    env, twin = _env(2, K, N, seed=33), _env(2, K, N, seed=33)
    state0 = env.reset()
    count = _lib.lib().wurm_launch_count
    before = count()
    out = env.act_window(pop.params, state0, T)
    assert count() - before == 2 * T
    assert {k: tuple(v.shape) for k, v in out.items() if k != 'state'} == {
        'observations': (T, K * N, E), 'actions': (T, K * N), 'probs': (T, K * N, 4), 'values': (T, K * N),
        'rewards': (T, K * N), 'dones': (T, K * N), 'all_done': (T, N)}
    state = twin.reset()
    _same_dicts(state0, state, 'reset')
    for t in range(T):
        a = twin.act(pop.params, state)
        sampled = a['actions_t'].clone()
        obs, rewards, dones, _ = twin.step(a['actions'])
        twin.reset(dones['__all__'], return_observations=False)
        rows = lambda d: torch.stack([d[f'agent_{k}'] for k in range(K)]).reshape(K * N, -1).squeeze(-1)
        assert torch.equal(out['actions'][t], sampled.reshape(-1)), t
        assert torch.equal(out['probs'][t], a['probs'].reshape(K * N, 4)), t
        assert torch.equal(out['values'][t], a['values'].reshape(-1)), t
        assert torch.equal(out['observations'][t], rows(obs)), t
        assert torch.equal(out['rewards'][t], rows(rewards)), t
        assert torch.equal(out['dones'][t], rows(dones)), t
        assert torch.equal(out['all_done'][t], dones['__all__']), t
        state = obs
    _same_dicts(out['state'], state, 'last observations')
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    assert env.policy_calls == twin.policy_calls == T and env._call == twin._call

    # the window is the member layout of the learner that exists: one member per species
    x0 = torch.stack(list(state0.values())).reshape(K * N, E)
    grad, losses = pop.grad(x0, out)
    assert grad.shape == pop.params.shape and bool(torch.isfinite(grad).all())
    M = K // P * N
    # species 0 as a learner of its own on its columns: what tests/test_a2c_population_gpu.py compares, bit for bit
    single = FusedA2CLearner(copy.deepcopy(pop.agents[0]), entropy_coef=0.01)
    keys = ('observations', 'actions', 'rewards', 'dones')
    _, alone = single.grad(x0[:M].contiguous(), {k: out[k][:, :M].contiguous() for k in keys})
    assert torch.equal(losses['values'][:, :M], alone['values'])
    # ... and the values the window acted on, against the learner's recomputation of them: the bound of
    # tests/test_a2c_learner_gpu.py::test_three_rounds_with_an_env for this comparison, 4 x (the error of torch's own fp32
    # forward against float64 on these inputs) + 1e-6, relative to the largest value
    inputs = torch.cat([x0[:M].unsqueeze(0), out['observations'][:-1, :M]])
    with torch.no_grad():
        v32 = pop.agents[0](inputs)[1].squeeze(-1)
        v64 = copy.deepcopy(pop.agents[0]).double()(inputs.double())[1].squeeze(-1)
    bound = 4 * learner_ref.rel_err(v32, v64) + 1e-6
    err = learner_ref.rel_err(out['values'][:, :M], losses['values'][:, :M])
    print(f'window values against the learner: {err:.3e} (bound {bound:.3e})')
    assert err <= bound
    res = pop.update(x0, out)
    assert pop.step == 1 and bool(torch.isfinite(res['grad_norm']).all())


@pytest.mark.parametrize('E', ES)
def test_agrees_with_the_torch_agent(E):
    """probs / values against FeedforwardAgent in fp32 torch on the same rows, to the tolerances of
    tests/test_policy_rollout.py::test_python_api for the single-agent actor (2e-6 on probabilities, 2e-5 on values) —
    like there, with the weights torch initialises and the observations of an env"""
    n, K, N, P = ref.OBS_N[E], 4, 17, 2
    pop = FusedA2CPopulation(_agents(P, E))
    env, obs = _played(n, K, N)
    got = env.act(pop.params, obs)
    x = torch.stack(list(obs.values())).reshape(K, N, E)
    with torch.no_grad():
        for k in range(K):
            probs, values = pop.agents[k * P // K](x[k])
            dp = (probs - got['probs'][k]).abs().max().item()
            dv = (values.squeeze(-1) - got['values'][k]).abs().max().item()
            print(f'E={E} snake {k}: probs {dp:.3e} values {dv:.3e}')
            assert dp < 2e-6 and dv < 2e-5
