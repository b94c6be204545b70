"""`FusedA2CPopulation`: P independent A2C updates in the three launches of one (include/wurm_hip.h: wurm_a2c_ff_pop_*).
Everything member p computes must equal, bit for bit, what a `FusedA2CLearner` of its own (a deep copy of the same agent,
its own lr / gamma / entropy_coef / gae_lambda) computes from contiguous copies of the member's columns."""
import copy

import pytest
import torch

from tests import a2c_learner_ref as ref
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# per-member hyper-parameters, all different (member 0 has the lambda = 0.95 of the single-agent tests)
LR, GAMMA, ENTROPY, LAMBDA = [1e-3, 3e-4, 2e-3], [0.99, 0.95, 0.9], [0.01, 0.0, 0.05], [0.95, 0.9, 0.8]
# (P, M, T): two envs per member; more than one env per group; more envs than groups (M > 256); a workgroup with more
# than one 64-row tile (600 envs over 256 groups: 3 envs x 41 rows)
SHAPES = [(3, 2, 5), (2, 5, 20), (2, 300, 20), (2, 600, 40)]


def _agents(P, E):
    agents = []
    for p in range(P):
        torch.manual_seed(10 + p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
    return agents


def _hyper(P, use_gae, value_loss):
    shared = dict(value_loss=value_loss, use_gae=use_gae, max_grad_norm=0.5)
    pop = dict(lr=LR[:P], gamma=GAMMA[:P], entropy_coef=ENTROPY[:P], gae_lambda=LAMBDA[:P] if use_gae else None, **shared)
    single = [dict(lr=LR[p], gamma=GAMMA[p], entropy_coef=ENTROPY[p], gae_lambda=LAMBDA[p] if use_gae else None, **shared)
              for p in range(P)]
    return pop, single


_INPUTS = {}


def _inputs(E, P, M, T):
    """(state, out) of a population of P x M envs over T steps, made once per shape: from a population rollout at
    E = 75 (SingleSnake 9 x 9 partial_2) and E = 4 (SingleSnake 9 x 9 positions), random tensors at E = 507"""
    key = (E, P, M, T)
    if key not in _INPUTS:
        N = P * M
        if E == 507:
            g = torch.Generator().manual_seed(E + N + T)
            state = (torch.rand((N, 3, 13, 13), generator=g) < 0.3).float().to(DEV)
            out = dict(observations=(torch.rand((T, N, 3, 13, 13), generator=g) < 0.3).float().to(DEV),
                       actions=torch.randint(4, (T, N), generator=g).to(DEV),
                       rewards=(torch.rand((T, N), generator=g) < 0.2).float().to(DEV),
                       dones=(torch.rand((T, N), generator=g) < 0.1).to(DEV))
        else:
            from wurm_amd.envs import SingleSnake
            env = SingleSnake(num_envs=N, size=9, observation_mode='partial_2' if E == 75 else 'positions', device=DEV,
                              seed=5, env_offset=40)
            state = env.reset()
            acting = FusedA2CPopulation(_agents(P, E))
            state = env.policy_rollout(acting.params, state, 30, population=P)['state']  # (deaths and meals before the window)
            out = env.policy_rollout(acting.params, state, T, population=P)
            assert not out['status'].any()
        _INPUTS[key] = (state, out)
    return _INPUTS[key]


def _member_inputs(state, out, sl):
    keys = ('observations', 'actions', 'rewards', 'dones')
    return state[sl].contiguous(), {k: out[k][:, sl].contiguous() for k in keys}


def _compare(res, refs, M, keys, what):
    for p, ref in enumerate(refs):
        sl = slice(p * M, (p + 1) * M)
        for k in keys:
            got = res[k][:, sl] if k in ('values', 'returns') else res[k][p]
            assert got.shape == ref[k].shape, (what, p, k)
            assert torch.equal(got, ref[k]), (what, p, k)


@pytest.mark.parametrize('use_gae,value_loss', [(False, 'smooth_l1'), (False, 'mse'), (True, 'smooth_l1'), (True, 'mse')])
@pytest.mark.parametrize('P,M,T', SHAPES)
@pytest.mark.parametrize('E', [4, 75, 507])
def test_members_equal_stand_alone_learners(E, P, M, T, use_gae, value_loss):
    state, out = _inputs(E, P, M, T)
    agents = _agents(P, E)
    kw_pop, kw_single = _hyper(P, use_gae, value_loss)
    singles = [FusedA2CLearner(copy.deepcopy(a), **kw) for a, kw in zip(agents, kw_single)]
    pop = FusedA2CPopulation(agents, **kw_pop)
    assert pop.params.shape == (P, singles[0].params.numel())
    member = [_member_inputs(state, out, slice(p * M, (p + 1) * M)) for p in range(P)]
    loss_keys = ['value_loss', 'policy_loss', 'entropy', 'values'] + (['returns'] if use_gae else [])

    grad, losses = pop.grad(state, out)
    assert grad.shape == pop.params.shape and losses['value_loss'].shape == (P,) and losses['values'].shape == (T, P * M)
    refs = []
    for s, (x, o) in zip(singles, member):
        g, l = s.grad(x, o)
        refs.append(dict(l, grad=g))
    _compare(dict(losses, grad=grad), refs, M, loss_keys + ['grad'], 'grad')

    for i in range(3):
        res = pop.update(state, out)
        refs = [s.update(x, o) for s, (x, o) in zip(singles, member)]
        assert res['grad_norm'].shape == (P,) and res['grad'].shape == pop.params.shape
        _compare(res, refs, M, loss_keys + ['grad', 'grad_norm'], ('update', i))
        for p, s in enumerate(singles):
            assert torch.equal(pop.params[p], s.params), ('params', i, p)
            assert torch.equal(pop.exp_avg[p], s.exp_avg), ('exp_avg', i, p)
            assert torch.equal(pop.exp_avg_sq[p], s.exp_avg_sq), ('exp_avg_sq', i, p)
    assert pop.step == 3
    assert not torch.equal(pop.params[0], pop.params[1])


@pytest.mark.parametrize('use_gae', [False, True])
def test_grad_then_apply_is_update_in_three_launches(use_gae):
    E, P, M, T = 75, 3, 2, 5
    state, out = _inputs(E, P, M, T)
    kw = _hyper(P, use_gae, 'smooth_l1')[0]
    one, two = FusedA2CPopulation(_agents(P, E), **kw), FusedA2CPopulation(_agents(P, E), **kw)
    for pop in (one, two):  # a state that is not the initial one
        pop.step = 3
        pop.exp_avg.fill_(1e-3)
        pop.exp_avg_sq.fill_(1e-5)
    before = _lib.lib().wurm_launch_count()
    res = one.update(state, out)
    assert _lib.lib().wurm_launch_count() - before == 3
    grad, losses = two.grad(state, out)
    norm = two.apply(grad)
    assert one.step == 4 and two.step == 4
    assert torch.equal(one.params, two.params) and torch.equal(one.exp_avg, two.exp_avg)
    assert torch.equal(one.exp_avg_sq, two.exp_avg_sq)
    assert torch.equal(res['grad'], grad) and torch.equal(res['grad_norm'], norm)
    assert all(torch.equal(res[k], losses[k]) for k in losses)


@pytest.mark.parametrize('stem', ref.ENTRY_POINT_STEMS)
def test_optional_outputs_may_be_null(stem):
    """values_out, grad_norm and returns_out are optional in the C ABI and FusedA2CPopulation always hands them over:
    every launching population entry point once without and once with them (P = 3, M = 2, two learning rates), on the
    same inputs, writes the same bits everywhere else."""
    without, given = (ref.run_entry_point(stem, g, DEV, E=4, T=2, N=6, members=3, lrs=(1e-3, 3e-4, 1e-3))
                      for g in (False, True))
    for k in ('grad', 'losses', 'params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(without[k], given[k]), k


def test_agents_show_the_updated_weights():
    E, P, M, T = 75, 3, 2, 5
    state, out = _inputs(E, P, M, T)
    agents = _agents(P, E)
    pop = FusedA2CPopulation(agents, lr=LR)
    before = [a.feedforward[0][0].weight.clone() for a in agents]
    pop.update(state, out)
    x = torch.rand(9, E, device=DEV)
    for p, a in enumerate(agents):
        w = a.feedforward[0][0].weight
        assert w.data_ptr() == pop.params[p].data_ptr() and not torch.equal(w, before[p])
        assert torch.equal(w.reshape(-1), pop.params[p, :64 * E])
        assert torch.equal(a.value_head.bias, pop.params[p, -1:])
        single = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV)
        FusedA2CLearner(single).params.copy_(pop.params[p])
        assert all(torch.equal(u, v) for u, v in zip(a(x), single(x)))


@pytest.mark.parametrize('use_gae', [False, True])
def test_four_windows_of_rollout_and_update_equal_separate_loops(use_gae):
    from wurm_amd.envs import SingleSnake
    P, M, T, seed, base = 3, 8, 5, 3, 200
    kw_pop, kw_single = _hyper(P, use_gae, 'smooth_l1')
    make = lambda n, off: SingleSnake(num_envs=n, size=9, observation_mode='partial_2', device=DEV, seed=seed, env_offset=off)
    agents = _agents(P, 75)
    singles = [FusedA2CLearner(copy.deepcopy(a), **kw) for a, kw in zip(agents, kw_single)]
    pop = FusedA2CPopulation(agents, **kw_pop)
    env = make(P * M, base)
    state = env.reset()
    for _ in range(4):
        out = env.policy_rollout(pop.params, state, T, population=P)
        pop.update(state, out)
        state = out['state']
    for p, s in enumerate(singles):
        e = make(M, base + p * M)
        x = e.reset()
        for _ in range(4):
            o = e.policy_rollout(s.params, x, T)
            s.update(x, o)
            x = o['state']
        assert torch.equal(pop.params[p], s.params), p
        assert torch.equal(pop.exp_avg_sq[p], s.exp_avg_sq), p
        assert torch.equal(env.envs[p * M:(p + 1) * M], e.envs), p
