"""The fused A2C learner's GAE mode on the GPU (a2c_ff_main_kernel<true> of wurm_amd/csrc/a2c_learner.hpp through
wurm_amd.rl.FusedA2CLearner(use_gae=True, gae_lambda=...)) against the float64 specification of tests/a2c_gae_ref.py,
under the rule of tests/test_a2c_learner_gpu.py: per parameter block, err(fused) <= 4 * err(torch fp32 autograd of the
same loss on the GPU) + 1e-6.

The shapes are that file's GRAD_CASES (a single env, unevenly filled workgroups, the single-tile path that keeps H1 / H2
in LDS, the two-tile path that forwards twice, E from 3 to 507); in every fixture env 0 is done at every step and env 1
never, so the scan meets the cut chain (nd = 0), the uncut one and T = 1."""
import functools
import math

import pytest
import torch

from tests import a2c_gae_ref as gae
from tests import a2c_learner_ref as ref
from tests.test_a2c_learner_gpu import DEV, GRAD_CASES, assert_within_bound, bound
from wurm_amd import _lib
from wurm_amd.rl import FusedA2CLearner
from wurm_amd.rl.a2c import a2c_returns

pytestmark = pytest.mark.gpu

SMALL, TWO_TILES = GRAD_CASES[2], GRAD_CASES[6]
assert SMALL[:3] == (27, 5, 65) and TWO_TILES[:3] == (27, 20, 1031)
GAE_CASES = [c + (0.95,) for c in GRAD_CASES] + [c + (lam,) for c in (SMALL, TWO_TILES) for lam in (0.0, 0.5, 1.0)]


@functools.lru_cache(maxsize=None)
def references(E, T, N, value_loss, entropy_coef, scale, gae_lambda):
    """(float64 specification, torch fp32 autograd on the GPU) of a case: computed once, shared, never modified"""
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    return (gae.spec_float64_gae(fx, gae_lambda, entropy_coef, value_loss),
            gae.example_loss_gae(fx, torch.float32, DEV, gae_lambda, entropy_coef, value_loss))


def fused_gae(fx, entropy_coef, value_loss, gae_lambda):
    agent, state, out = ref.to_device(fx, DEV)
    learner = FusedA2CLearner(agent, gamma=fx['gamma'], entropy_coef=entropy_coef, value_loss=value_loss, use_gae=True,
                              gae_lambda=gae_lambda)
    g, losses = learner.grad(state, out)
    return learner, state, out, g, losses


@pytest.mark.parametrize('E,T,N,value_loss,entropy_coef,scale,gae_lambda', GAE_CASES)
def test_gradient_losses_and_values(E, T, N, value_loss, entropy_coef, scale, gae_lambda):
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    learner, state, out, g, losses = fused_gae(fx, entropy_coef, value_loss, gae_lambda)
    spec, t32 = references(E, T, N, value_loss, entropy_coef, scale, gae_lambda)
    assert_within_bound(fx, g, losses, spec, t32, f'gae {gae_lambda}')
    g2, losses2 = learner.grad(state, out)  # no atomics: the same bits
    assert torch.equal(g, g2) and all(torch.equal(losses[k], losses2[k]) for k in losses)


@pytest.mark.parametrize('E,T,N,value_loss,entropy_coef,scale,gae_lambda', GAE_CASES)
def test_returns_are_those_of_the_scan_kernel(E, T, N, value_loss, entropy_coef, scale, gae_lambda):
    """`returns` == wurm_amd.rl.a2c.a2c_returns (rl.hip, GAE) of the fused values, bit for bit.  The bootstrap value is
    taken from a second `grad` call on the window shifted to the last observation (one step, whose only policy input is
    obs[T-1]): a row's forward pass does not depend on where the row sits, so this is the value the first call used, and
    nothing had to be added to the interface for it."""
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    learner, state, out, _, losses = fused_gae(fx, entropy_coef, value_loss, gae_lambda)
    last = {k: out[k][:1].contiguous() for k in ('observations', 'actions', 'rewards', 'dones')}
    bootstrap = learner.grad(out['observations'][T - 1], last)[1]['values'][0]
    expected = a2c_returns(bootstrap, out['rewards'], losses['values'], out['dones'], fx['gamma'], True, gae_lambda)
    assert losses['returns'].shape == (T, N) and torch.equal(losses['returns'], expected)
    spec, t32 = references(E, T, N, value_loss, entropy_coef, scale, gae_lambda)  # and the specification's, to fp32
    ef, et = ref.rel_err(losses['returns'], spec['returns']), ref.rel_err(t32['returns'], spec['returns'])
    print(f'returns E={E} T={T} N={N} lambda={gae_lambda}: fused {ef:.3e} torch32 {et:.3e}')
    assert ef <= bound(et)


@pytest.mark.parametrize('case', [SMALL, TWO_TILES])
def test_lambda_one_is_the_n_step_learner(case):
    """At lambda = 1 the two instantiations compute the same gradient by different arithmetic (R = gae + v against the
    plain discounted sum; an `extra` that is rounding noise against none): they agree within the bound of the torch fp32
    error."""
    E, T, N, value_loss, entropy_coef, scale = case
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    _, state, out, g, losses = fused_gae(fx, entropy_coef, value_loss, 1.0)
    agent, _, _ = ref.to_device(fx, DEV)
    g0, losses0 = FusedA2CLearner(agent, gamma=fx['gamma'], entropy_coef=entropy_coef, value_loss=value_loss).grad(
        state, out)
    assert 'returns' not in losses0 and torch.equal(losses0['values'], losses['values'])
    spec, t32 = references(E, T, N, value_loss, entropy_coef, scale, 1.0)
    et = ref.block_errors(t32['grad'], spec['grad'], E)
    err = ref.block_errors(g, g0, E)
    for k in err:
        print(f'lambda 1 against n-step E={E} T={T} N={N} {k}: {err[k]:.3e} torch32 {et[k]:.3e}')
    for k in err:
        assert err[k] <= bound(et[k]), (k, err[k], et[k])


def test_update_is_grad_then_apply():
    fx = ref.make_fixture(75, 5, 65, seed=4, reward_scale=3.0)
    a1, state, out = ref.to_device(fx, DEV)
    a2, _, _ = ref.to_device(fx, DEV)
    kw = dict(gamma=fx['gamma'], entropy_coef=0.01, lr=1e-3, use_gae=True, gae_lambda=0.95)
    l1, l2 = FusedA2CLearner(a1, **kw), FusedA2CLearner(a2, **kw)
    for l in (l1, l2):  # a state that is not the initial one
        l.step = 3
        l.exp_avg = torch.full_like(l.params, 1e-3)
        l.exp_avg_sq = torch.full_like(l.params, 1e-5)
    before = _lib.lib().wurm_launch_count()
    res = l1.update(state, out)
    assert _lib.lib().wurm_launch_count() - before <= 3
    g, losses = l2.grad(state, out)
    norm = l2.apply(g)
    assert l1.step == 4 and l2.step == 4
    assert torch.equal(l1.params, l2.params) and torch.equal(l1.exp_avg, l2.exp_avg)
    assert torch.equal(l1.exp_avg_sq, l2.exp_avg_sq) and torch.equal(res['grad'], g) and torch.equal(res['grad_norm'], norm)
    assert 'returns' in losses and all(torch.equal(res[k], losses[k]) for k in losses)
    assert not torch.equal(l1.params, fx['params'].to(DEV))
    # and it is the GAE gradient that was applied, not the n-step one
    a3, _, _ = ref.to_device(fx, DEV)
    g0, _ = FusedA2CLearner(a3, gamma=fx['gamma'], entropy_coef=0.01).grad(state, out)
    assert ref.block_errors(g, g0, 75)['Wv'] > 1e-3


def test_three_rounds_with_an_env():
    from wurm_amd.agents import FeedforwardAgent
    from wurm_amd.envs import SingleSnake
    torch.manual_seed(0)
    env = SingleSnake(num_envs=64, size=9, observation_mode='partial_2', device=DEV, seed=5)
    agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75).to(DEV)
    learner = FusedA2CLearner(agent, entropy_coef=0.01, use_gae=True, gae_lambda=0.95)
    params = learner.params
    state = env.reset()
    for rnd in range(3):
        before = learner.params.clone()
        out = env.policy_rollout(learner.params, state, 5)
        res = learner.update(state, out)
        assert all(bool(torch.isfinite(res[k]).all()) for k in res) and learner.step == rnd + 1
        assert all(math.isfinite(float(res[k])) for k in ('value_loss', 'policy_loss', 'entropy', 'grad_norm'))
        assert res['returns'].shape == (5, 64) and not torch.equal(learner.params, before)
        # the buffer the actor reads is still the learner's and still the module's
        assert learner.params is params and agent.feedforward[0][0].weight.data_ptr() == params.data_ptr()
        state = out['state']
