"""Shared by tests/test_a2c_returns_cpu.py and tests/test_a2c_returns_gpu.py: the specification of the A2C return scan
(wurm_amd/csrc/rl.hip: wurm_a2c_returns, wurm_a2c_returns_backward) and of wurm_amd.rl.A2C.loss on top of it, as plain
torch ops in whatever dtype and device the inputs have, and the seeded case builder.

Called in float64 the two functions are the specification.  Called in float32 they are the yardstick: what torch makes of
the same loops (wurm/rl/a2c.py:49-73) in the kernels' own precision, in the reference's operation order — on the CPU the
float32 returns equal the oracle's bit for bit (tests/test_a2c_returns_cpu.py)."""
import functools

import torch
import torch.nn.functional as F

from tests.a2c_gae_ref import gae_returns
from tests.a2c_learner_ref import rel_err  # noqa: F401  (the error measure of every comparison with float64)

EPS = 1e-8


def returns_spec(bootstrap, rewards, values, dones, gamma, use_gae=False, gae_lambda=None):
    """(T,N) returns of wurm/rl/a2c.py:49-66 from bootstrap (N), rewards / values / dones (T,N); differentiable in
    `values` (GAE; the n-step returns do not depend on them) and `bootstrap`."""
    if use_gae:
        return gae_returns(bootstrap, rewards, values, dones, gamma, gae_lambda)
    T = rewards.shape[0]
    nd = (~dones.bool()).to(rewards.dtype)
    R = bootstrap * nd[T - 1]
    out = []
    for t in range(T - 1, -1, -1):
        R = rewards[t] + gamma * R * nd[t]
        out.append(R)
    return torch.stack(out[::-1])


def loss_spec(bootstrap, rewards, values, log_probs, dones, gamma, use_gae=False, gae_lambda=None,
              normalise_returns=False, value_loss_fn=F.smooth_l1_loss):
    """(value_loss, policy_loss, returns) of wurm/rl/a2c.py:49-73; `returns` as the losses see them (normalised if asked)."""
    R = returns_spec(bootstrap, rewards, values, dones, gamma, use_gae, gae_lambda)
    if normalise_returns:
        R = (R - R.mean()) / (R.std() + EPS)
    value_loss = value_loss_fn(values, R).mean()
    policy_loss = -((R - values).detach() * log_probs).mean()
    return value_loss, policy_loss, R


def grads_spec(bootstrap, rewards, values, dones, G, gamma, use_gae=False, gae_lambda=None):
    """(returns, d<G, returns>/d values, d<G, returns>/d bootstrap) by torch autograd of returns_spec in the dtype and on the
    device of the inputs; zeros where the returns do not depend on an input."""
    v, b = values.detach().clone().requires_grad_(True), bootstrap.detach().clone().requires_grad_(True)
    R = returns_spec(b, rewards, v, dones, gamma, use_gae, gae_lambda)
    gv, gb = torch.autograd.grad(R, (v, b), G, allow_unused=True)
    return R.detach(), torch.zeros_like(v) if gv is None else gv, torch.zeros_like(b) if gb is None else gb


@functools.lru_cache(maxsize=None)
def make_case(T, N, seed=0):
    """Seeded float32 CPU case (shared, never modified: callers copy what they change).  bootstrap (N) and values (T,N)
    ~ N(0,1); rewards in {-1, 0, 1} drawn as tests/golden/make_golden_rl.py draws them; log_probs in [-2, 0]; dones
    Bernoulli(0.2) with planted columns wherever the env exists: env 0 done at every step, env 1 never, env 2 only at
    T - 1, env 3 only at t = 0 (a single env cannot be planted both ways and keeps its draw, as in
    tests/a2c_learner_ref.py); G ~ N(0,1) (T,N), an upstream gradient that is the gradient of no mean."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * T + N)
    rewards = (torch.rand((T, N), generator=g) < 0.15).float() - (torch.rand((T, N), generator=g) < 0.05).float()
    values = torch.randn((T, N), generator=g)
    log_probs = -torch.rand((T, N), generator=g) * 2
    dones = torch.rand((T, N), generator=g) < 0.2
    bootstrap = torch.randn(N, generator=g)
    G = torch.randn((T, N), generator=g)
    if N >= 2:
        dones[:, 0] = True
        dones[:, 1] = False
    if N >= 3:
        dones[:, 2] = False
        dones[T - 1, 2] = True
    if N >= 4:
        dones[:, 3] = False
        dones[0, 3] = True
    return {'T': T, 'N': N, 'bootstrap': bootstrap, 'rewards': rewards, 'values': values, 'log_probs': log_probs,
            'dones': dones, 'G': G}


def to(case, dtype, device='cpu'):
    """the case's tensors in `dtype` on `device` (dones stay bool)"""
    out = {k: v.to(device=device, dtype=dtype) for k, v in case.items() if k not in ('T', 'N', 'dones')}
    out['dones'] = case['dones'].to(device)
    return out
