"""Shared by tests/test_a2c_gae_cpu.py and tests/test_a2c_gae_gpu.py: the float64 specification of the fused A2C learner
with generalised advantage estimation (include/wurm_hip.h: wurm_a2c_ff_grad_gae) and the same loss written the way a
user of wurm.rl.A2C(gamma, use_gae=True, gae_lambda=...) writes it, for any dtype / device.  Forward pass, clamp rule,
fixtures and error measures are those of tests/a2c_learner_ref.py.

What GAE changes against the n-step loss: R_t is built from the values, which carry gradient (the reference does not
detach `returns`: wurm/rl/a2c.py:66-71), and from the bootstrap value, which does not (experiments/main.py:233-234).  So
the value loss l(v - R) sends gradient into v through R as well; the advantage R - v of the policy term stays detached."""
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from tests import a2c_learner_ref as ref


def gae_returns(bootstrap, rewards, values, dones, gamma, gae_lambda):
    """delta_t = r_t + gamma v_{t+1} !done_t - v_t with v_T = bootstrap; gae_t = delta_t + gamma lambda !done_t gae_{t+1};
    R_t = gae_t + v_t.  Differentiable in `values` and `bootstrap`."""
    nd = (~dones.bool()).to(rewards.dtype)
    delta = rewards + gamma * torch.cat([values[1:], bootstrap[None]]) * nd - values
    gae, out = torch.zeros_like(bootstrap), []
    for t in range(rewards.shape[0] - 1, -1, -1):
        gae = delta[t] + gamma * gae_lambda * nd[t] * gae
        out.append(gae + values[t])
    return torch.stack(out[::-1])


def spec_float64_gae(fx, gae_lambda, entropy_coef=0.0, value_loss='smooth_l1'):
    """The specification in float64: tests.a2c_learner_ref.spec_float64 with GAE returns.  Returns grad (P), losses (3),
    values (T,N) and returns (T,N)."""
    E = fx['E']
    params = fx['params'].double().clone().requires_grad_(True)
    w = ref.split(params, E)
    x = torch.cat([fx['obs0'][None], fx['obs'][:-1]]).double()
    _, _, p, v = ref.forward(w, x)                                        # (T,N,4), (T,N)
    with torch.no_grad():
        boot = ref.forward(w, fx['obs'][-1].double())[3]
    R = gae_returns(boot, fx['rewards'].double(), v, fx['dones'], fx['gamma'], gae_lambda)   # carries d/dv
    d = v - R
    if value_loss == 'smooth_l1':
        vl = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).mean()
    else:
        vl = (d * d).mean()
    inside = (p > ref.EPS32) & (p < 1 - ref.EPS32)
    logp = torch.log(torch.where(inside, p, p.detach().clamp(ref.EPS32, 1 - ref.EPS32)))
    logp_a = logp.gather(-1, fx['actions'][..., None]).squeeze(-1)
    pl = -((R - v).detach() * logp_a).mean()
    ent = -(p * logp).sum(-1).mean()
    loss = vl + pl - entropy_coef * ent
    (g,) = torch.autograd.grad(loss, params)
    return {'grad': g, 'losses': torch.stack([vl, pl, ent]).detach(), 'values': v.detach(), 'returns': R.detach()}


def example_loss_gae(fx, dtype, device, gae_lambda, entropy_coef=0.0, value_loss='smooth_l1'):
    """The loss through Categorical, the loops of wurm/rl/a2c.py:50-59 restated in torch ops (one step at a time, the
    last step on the bootstrap value) and smooth_l1_loss / mse_loss, by torch autograd in `dtype` on `device`."""
    E = fx['E']
    params = fx['params'].to(device=device, dtype=dtype).clone().requires_grad_(True)
    w = ref.split(params, E)
    inputs = torch.cat([fx['obs0'][None], fx['obs'][:-1]]).to(device=device, dtype=dtype)
    actions, dones = fx['actions'].to(device), fx['dones'].to(device).bool()
    rewards = fx['rewards'].to(device=device, dtype=dtype)
    gamma = fx['gamma']
    _, _, probs, values = ref.forward(w, inputs)
    dist = Categorical(probs, validate_args=False)
    log_probs = dist.log_prob(actions)
    entropies = dist.entropy().mean(-1)
    with torch.no_grad():
        bootstrap_values = ref.forward(w, fx['obs'][-1].to(device=device, dtype=dtype))[3]
    returns, gae = [], 0
    for t in reversed(range(rewards.size(0))):                             # a2c.py:52-59
        if t == rewards.size(0) - 1:
            delta = rewards[t] + gamma * bootstrap_values * (~dones[t]).to(dtype) - values[t]
        else:
            delta = rewards[t] + gamma * values[t + 1] * (~dones[t]).to(dtype) - values[t]
        gae = delta + gamma * gae_lambda * (~dones[t]).to(dtype) * gae
        returns.insert(0, gae + values[t])
    returns = torch.stack(returns)
    loss_fn = F.smooth_l1_loss if value_loss == 'smooth_l1' else F.mse_loss
    vl = loss_fn(values, returns).mean()
    pl = -((returns - values).detach() * log_probs).mean()
    loss = vl + pl - entropy_coef * entropies.mean()
    (g,) = torch.autograd.grad(loss, params)
    return {'grad': g, 'losses': torch.stack([vl, pl, entropies.mean()]).detach(), 'values': values.detach(),
            'returns': returns.detach()}
