"""The fused A2C learner on the GPU (wurm_amd/csrc/a2c_learner.hpp through wurm_amd.rl.FusedA2CLearner) against the
float64 specification of tests/a2c_learner_ref.py.

The bound is not a fixed number: for every parameter block, err = max|g - g64| / max|g64|, and the fused learner must
satisfy err(fused) <= 4 * err(torch fp32 autograd of the same loss on the GPU) + 1e-6 (the factor covers another summation
order over the batch, the floor is the 1.5e-7 * sum|ab| error of an fp32 chain where torch happens to be exact)."""
import ctypes
import math
import os
import sys

import pytest
import torch

from tests import a2c_learner_ref as ref
from wurm_amd import _lib
from wurm_amd.rl import FusedA2CLearner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))


def bound(torch_err):
    return 4 * torch_err + 1e-6


def fused_and_references(fx, entropy_coef, value_loss):
    agent, state, out = ref.to_device(fx, DEV)
    learner = FusedA2CLearner(agent, gamma=fx['gamma'], entropy_coef=entropy_coef, value_loss=value_loss)
    g, losses = learner.grad(state, out)
    spec = ref.spec_float64(fx, entropy_coef, value_loss)
    t32 = ref.example_loss(fx, torch.float32, DEV, entropy_coef, value_loss)
    return learner, (state, out), g, losses, spec, t32


def assert_within_bound(fx, g, losses, spec, t32, what=''):
    E = fx['E']
    ef, et = ref.block_errors(g, spec['grad'], E), ref.block_errors(t32['grad'], spec['grad'], E)
    l = torch.stack([losses['value_loss'], losses['policy_loss'], losses['entropy']])
    ef['losses'], et['losses'] = ref.rel_err(l, spec['losses']), ref.rel_err(t32['losses'], spec['losses'])
    ef['values'], et['values'] = ref.rel_err(losses['values'], spec['values']), ref.rel_err(t32['values'], spec['values'])
    for k in ef:
        print(f"{what} E={E} T={fx['T']} N={fx['N']} {k}: fused {ef[k]:.3e} torch32 {et[k]:.3e}")
    for k in ef:
        assert math.isfinite(ef[k]) and ef[k] <= bound(et[k]), (k, ef[k], et[k])
    return et


# (E, T, N, value_loss, entropy_coef, reward scale).  Every E of {3, 4, 27, 75, 507}, T of {1, 2, 5, 20} and N of
# {1, 63, 65} at least once, plus two N of the builder's choice.  The 256 workgroups of the main kernel take the envs
# [w N / 256, (w + 1) N / 256) and cut their (T + 1) * nenv rows into tiles of 64:
#   N = 601 (with E = 507):  256 workgroups contribute partials, 2 or 3 envs each (so they are unevenly filled, the last
#                            one with 3), every one a single partly filled tile — the path that keeps H1 / H2 in LDS;
#   N = 1031, T = 20:        4 or 5 envs = 84 or 105 rows per workgroup: two tiles, the second partly filled — the path
#                            that recomputes the forward pass and accumulates dW1 in the workspace across tiles.
GRAD_CASES = [(3, 1, 1, 'smooth_l1', 0.0, 1.0), (4, 2, 63, 'mse', 0.01, 3.0), (27, 5, 65, 'smooth_l1', 0.01, 3.0),
              (75, 20, 65, 'mse', 0.0, 1.0), (75, 5, 63, 'smooth_l1', 0.01, 1.0), (507, 2, 601, 'smooth_l1', 0.01, 3.0),
              (27, 20, 1031, 'smooth_l1', 0.0, 3.0)]


@pytest.mark.parametrize('E,T,N,value_loss,entropy_coef,scale', GRAD_CASES)
def test_gradient_losses_and_values(E, T, N, value_loss, entropy_coef, scale):
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    learner, (state, out), g, losses, spec, t32 = fused_and_references(fx, entropy_coef, value_loss)
    assert_within_bound(fx, g, losses, spec, t32, 'grad')
    g2, losses2 = learner.grad(state, out)  # no atomics: the same bits
    assert torch.equal(g, g2) and all(torch.equal(losses[k], losses2[k]) for k in losses)


def test_sharp_policy_matches_the_clamped_formula():
    """Wp x 30 and planted saturated rows: sampled actions with p < eps32 / 4 and with p > 1 - eps32 / 4 (asserted on
    the reference).  Their policy gradient is zero in the clamped formula and non-zero without the clamp."""
    fx = ref.make_fixture(27, 5, 65, seed=3, wp_scale=30.0)
    learner, _, g, losses, spec, t32 = fused_and_references(fx, 0.01, 'smooth_l1')
    assert bool((spec['p_action'] < ref.EPS32 / 4).any()) and bool((spec['p_action'] > 1 - ref.EPS32 / 4).any())
    assert_within_bound(fx, g, losses, spec, t32, 'sharp')
    plain = ref.spec_float64(fx, 0.01, clamp=False)
    assert max(ref.block_errors(g, plain['grad'], 27).values()) > 1e-3


def test_gradient_is_the_weighted_sum_over_a_split_batch():
    """grad over N envs == (B1 grad(first envs) + B2 grad(the others)) / B: partial sums across workgroup counts"""
    fx = ref.make_fixture(75, 5, 65, seed=4, reward_scale=3.0)
    _, _, g, losses, spec, t32 = fused_and_references(fx, 0.01, 'smooth_l1')
    et = assert_within_bound(fx, g, losses, spec, t32, 'whole')
    parts = []
    for lo, hi in ((0, 32), (32, 65)):
        half = dict(fx, N=hi - lo, obs0=fx['obs0'][lo:hi].contiguous(), obs=fx['obs'][:, lo:hi].contiguous(),
                    **{k: fx[k][:, lo:hi].contiguous() for k in ('actions', 'rewards', 'dones')})
        agent, state, out = ref.to_device(half, DEV)
        gh, _ = FusedA2CLearner(agent, gamma=fx['gamma'], entropy_coef=0.01).grad(state, out)
        parts.append(gh.double() * (hi - lo))
    combined = (parts[0] + parts[1]) / 65
    err = ref.block_errors(g, combined, 75)
    for k in err:
        assert err[k] <= bound(et[k]), (k, err[k], et[k])


# ------------------------------------------------------------------------------------------------ clip + Adam

def torch_adam(theta, g, m, u, step, dtype, max_norm, lr=1e-3):
    p = torch.nn.Parameter(theta.to(dtype).clone())
    p.grad = g.to(dtype).clone()
    opt = torch.optim.Adam([p], lr=lr)
    opt.state[p] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.to(dtype).clone(),
                    'exp_avg_sq': u.to(dtype).clone()}
    norm = torch.nn.utils.clip_grad_norm_([p], max_norm if max_norm > 0 else float('inf'))
    opt.step()
    return p.data.double() - theta.double(), norm.double(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']


def fused_apply(theta, g, m, u, step, max_norm, lr=1e-3):
    theta, m, u = theta.clone(), m.clone(), u.clone()
    norm = torch.zeros(1, device=DEV)
    F32 = ctypes.c_float
    rc = _lib.lib().wurm_a2c_ff_apply(theta.data_ptr(), g.data_ptr(), m.data_ptr(), u.data_ptr(), norm.data_ptr(),
                                      step, F32(lr), F32(0.9), F32(0.999), F32(1e-8), F32(max_norm), theta.numel(),
                                      _lib.stream_ptr(theta.device.index))
    assert rc == _lib.OK
    return theta, norm[0].double(), m, u


@pytest.mark.parametrize('P', [1481, 36929])
@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('kind', ['small', 'large', 'zeros'])
def test_clip_and_adam(P, step, kind):
    gen = torch.Generator().manual_seed(P + step)
    theta = (torch.rand(P, generator=gen) - 0.5).to(DEV)
    g = torch.randn(P, generator=gen) * {'small': 1e-3, 'large': 10.0, 'zeros': 1e-2}[kind]
    m, u = torch.randn(P, generator=gen) * 1e-2, torch.rand(P, generator=gen) * 1e-3
    if kind == 'zeros':  # zero gradients, and zero state under some of them: the step is m / (0 + eps)
        g[:P // 3] = 0
        m[:P // 6] = 0
        u[:P // 6] = 0
    g, m, u = g.to(DEV), m.to(DEV), u.to(DEV)
    g_before = g.clone()
    new, norm, m2, u2 = fused_apply(theta, g, m, u, step, 0.5)
    assert torch.equal(g, g_before)
    d64, n64, m64, u64 = torch_adam(theta, g, m, u, step, torch.float64, 0.5)
    d32, n32, _, _ = torch_adam(theta, g, m, u, step, torch.float32, 0.5)
    lr = 1e-3
    ef = float(((new.double() - theta.double()) - d64).abs().max() / lr)
    et = float((d32 - d64).abs().max() / lr)
    nf, nt = float((norm - n64).abs() / n64), float((n32 - n64).abs() / n64)
    print(f'apply P={P} step={step} {kind}: dtheta/lr fused {ef:.3e} torch32 {et:.3e}; norm fused {nf:.3e} torch32 {nt:.3e}')
    assert ef <= bound(et) and nf <= bound(nt)
    assert ref.rel_err(m2, m64) <= 1e-6 and ref.rel_err(u2, u64) <= 1e-6
    if kind == 'small':
        assert float(n64) < 0.5  # not clipped
    elif kind == 'large':
        assert float(n64) > 50  # clipped hard
    else:
        assert int((g == 0).sum()) >= P // 3 and float(n64) > 0  # the eps path is taken, the norm is not 0 / 0
    # max_grad_norm = 0: g is used unscaled
    new0, _, _, _ = fused_apply(theta, g, m, u, step, 0.0)
    e64, _, _, _ = torch_adam(theta, g, m, u, step, torch.float64, 0.0)
    e32, _, _, _ = torch_adam(theta, g, m, u, step, torch.float32, 0.0)
    assert float(((new0.double() - theta.double()) - e64).abs().max() / lr) <= bound(float((e32 - e64).abs().max() / lr))


@pytest.mark.parametrize('stem', ref.ENTRY_POINT_STEMS)
def test_optional_outputs_may_be_null(stem):
    """values_out, grad_norm and returns_out are optional in the C ABI and FusedA2CLearner always hands them over: every
    launching entry point once without and once with them, on the same inputs, writes the same bits everywhere else."""
    without, given = (ref.run_entry_point(stem, g, DEV, E=4, T=2, N=3) for g in (False, True))
    for k in ('grad', 'losses', 'params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(without[k], given[k]), k


# ------------------------------------------------------------------------------------------------ composition

def test_update_is_grad_then_apply():
    fx = ref.make_fixture(75, 5, 65, seed=4, reward_scale=3.0)
    a1, state, out = ref.to_device(fx, DEV)
    a2, _, _ = ref.to_device(fx, DEV)
    kw = dict(gamma=fx['gamma'], entropy_coef=0.01, lr=1e-3)
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
    assert all(torch.equal(res[k], losses[k]) for k in losses)
    assert not torch.equal(l1.params, fx['params'].to(DEV))
    x = torch.rand(9, 75, device=DEV)
    w = ref.split(l1.params, 75)
    _, _, p, v = ref.forward(w, x)
    pa, va = a1(x)  # the module runs on the updated buffer
    assert torch.allclose(pa, p, atol=1e-6) and torch.allclose(va.squeeze(-1), v, atol=1e-6)
    assert a1.feedforward[0][0].weight.data_ptr() == l1.params.data_ptr()


def test_shape_and_device_errors():
    fx = ref.make_fixture(27, 2, 65, seed=0)
    agent, state, out = ref.to_device(fx, DEV)
    learner = FusedA2CLearner(agent)
    with pytest.raises(RuntimeError):
        learner.grad(state[:-1], out)
    with pytest.raises(RuntimeError):
        learner.grad(state, dict(out, actions=out['actions'].int()))
    with pytest.raises(RuntimeError):
        learner.grad(state, dict(out, rewards=out['rewards'].cpu()))
    with pytest.raises(RuntimeError):
        learner.update(state, dict(out, dones=out['dones'][:1]))
    learner.grad(state, out)
    assert len(learner._workspace) == 1  # allocated once per (N, T, E)
    learner.grad(state, out)
    assert len(learner._workspace) == 1


def _clean_copy(state, out, params, E):
    """This round's tensors as a fixture on the CPU, with the observation of any row near a kink (float64) replaced by
    that of a row that is not: real crops can sit on a ReLU boundary, where fp32 may take the other side."""
    T, N = out['rewards'].shape
    x = torch.cat([state.reshape(1, N, E), out['observations'].reshape(T, N, E)]).cpu().reshape(-1, E).clone()
    w = ref.split(params.double().cpu(), E)
    bad = ref._near_kink(w, x.double())
    assert float(bad.float().mean()) <= 0.10
    x[bad] = x[~bad][0]
    x = x.view(T + 1, N, E)
    return {'E': E, 'T': T, 'N': N, 'gamma': 0.99, 'params': params.detach().cpu().clone(), 'obs0': x[0].contiguous(),
            'obs': x[1:].contiguous(), 'actions': out['actions'].cpu(), 'rewards': out['rewards'].cpu(),
            'dones': out['dones'].cpu()}


@pytest.mark.parametrize('family', ['snake', 'gridworld'])
def test_three_rounds_with_an_env(family):
    """policy_rollout(learner.params) -> update, three times.  Each round's gradient is checked on the re-drawn copy of
    that round's tensors (_clean_copy: identical to them unless a row sits near a kink), the rollout's own values
    against values_out on the real ones."""
    from wurm_amd.agents import FeedforwardAgent
    from wurm_amd.envs import SimpleGridworld, SingleSnake
    torch.manual_seed(0)
    if family == 'snake':
        env, E = SingleSnake(num_envs=64, size=9, observation_mode='partial_2', device=DEV, seed=5), 75
    else:
        env, E = SimpleGridworld(num_envs=64, size=5, observation_mode='positions', start_location=(2, 2), device=DEV,
                                 seed=5), 4
    agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV)
    learner = FusedA2CLearner(agent, entropy_coef=0.01)
    state = env.reset()
    for rnd in range(3):
        out = env.policy_rollout(learner.params, state, 5)
        fx = _clean_copy(state, out, learner.params, E)
        a2, s2, o2 = ref.to_device(fx, DEV)
        g, losses = FusedA2CLearner(a2, entropy_coef=0.01).grad(s2, o2)
        et = assert_within_bound(fx, g, losses, ref.spec_float64(fx, 0.01),
                                 ref.example_loss(fx, torch.float32, DEV, 0.01), f'{family} round {rnd}')
        res = learner.update(state, out)
        assert ref.rel_err(out['values'], res['values']) <= bound(et['values'])
        assert all(bool(torch.isfinite(res[k]).all()) for k in res) and learner.step == rnd + 1
        state = out['state']


def test_a2c_with_the_fused_learner_runs():
    import a2c_fused_learner
    hist = a2c_fused_learner.run(num_envs=256, size=9, observation='partial_2', steps=3000, update_steps=5,
                                 log_interval=1000, lr=1e-3, verbose=False)
    assert len(hist) >= 3
    for row in hist:
        assert all(math.isfinite(v) for v in row.values())
        assert 0 < row['done_rate'] < 0.4 and row['reward_rate'] > 0
