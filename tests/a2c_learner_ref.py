"""Shared by tests/test_a2c_learner_cpu.py, tests/test_a2c_learner_gpu.py and tools/a2c_learner_accuracy.py: the float64
restatement of the fused A2C learner's specification (include/wurm_hip.h: wurm_a2c_ff_grad), the same loss written the way
examples/a2c_fused_actor.py writes it (Categorical, smooth_l1_loss) for any dtype / device, and the fixture builder.

Fixtures are seeded and keep the kinks at a distance: a row whose float64 forward has a hidden pre-activation within 1e-4 of
0, or a probability within a factor 4 of eps32 or of 1 - eps32, is drawn again — there an fp32 forward may take the other
side of a discontinuous derivative, which is no error of a kernel."""
import functools

import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from wurm_amd.agents import FeedforwardAgent, pack_policy_params

EPS32 = torch.finfo(torch.float32).eps
BLOCKS = ('W1', 'b1', 'W2', 'b2', 'Wp', 'bp', 'Wv', 'bv')


def num_params(E):
    return 64 * E + 64 + 4096 + 64 + 256 + 4 + 64 + 1


def split(flat, E):
    """the eight blocks of a flat parameter / gradient vector in pack_policy_params order"""
    sizes = (64 * E, 64, 4096, 64, 256, 4, 64, 1)
    shapes = ((64, E), (64,), (64, 64), (64,), (4, 64), (4,), (64,), (1,))
    return {n: p.view(s) for n, p, s in zip(BLOCKS, flat.split(sizes), shapes)}


def forward(w, x):
    """(z1, z2, probs, values) of the spec's forward pass; w = split(params)"""
    z1 = x @ w['W1'].T + w['b1']
    z2 = torch.relu(z1) @ w['W2'].T + w['b2']
    h2 = torch.relu(z2)
    return z1, z2, torch.softmax(h2 @ w['Wp'].T + w['bp'], -1), h2 @ w['Wv'] + w['bv']


def returns_of(bootstrap, rewards, dones, gamma):
    """R_T = v_boot * !done[T-1]; R_t = r_t + gamma R_{t+1} * !done_t (wurm/rl/a2c.py:60-64); constants"""
    nd = (~dones.bool()).to(rewards.dtype)
    R = bootstrap * nd[-1]
    out = []
    for t in range(rewards.shape[0] - 1, -1, -1):
        R = rewards[t] + gamma * R * nd[t]
        out.append(R)
    return torch.stack(out[::-1])


def _grad_of(loss, params):
    (g,) = torch.autograd.grad(loss, params)
    return g


def spec_float64(fx, entropy_coef=0.0, value_loss='smooth_l1', clamp=True):
    """The specification in float64, written out: log p~ = log(clamp(p, eps32, 1 - eps32)) with gradient strictly inside
    the range only (clamp=False: the plain log, to show what the clamp changes).  Returns grad (P), losses (3), values
    (T,N) and the probabilities of the sampled actions."""
    E = fx['E']
    params = fx['params'].double().clone().requires_grad_(True)
    w = split(params, E)
    x = torch.cat([fx['obs0'][None], fx['obs'][:-1]]).double()
    _, _, p, v = forward(w, x)                                            # (T,N,4), (T,N)
    with torch.no_grad():
        boot = forward(w, fx['obs'][-1].double())[3]
        R = returns_of(boot, fx['rewards'].double(), fx['dones'], fx['gamma'])
    d = v - R
    if value_loss == 'smooth_l1':
        vl = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).mean()
    else:
        vl = (d * d).mean()
    if clamp:
        inside = (p > EPS32) & (p < 1 - EPS32)
        logp = torch.log(torch.where(inside, p, p.detach().clamp(EPS32, 1 - EPS32)))
    else:
        logp = torch.log(p)
    logp_a = logp.gather(-1, fx['actions'][..., None]).squeeze(-1)
    pl = -((R - v).detach() * logp_a).mean()
    ent = -(p * logp).sum(-1).mean()
    loss = vl + pl - entropy_coef * ent
    return {'grad': _grad_of(loss, params), 'losses': torch.stack([vl, pl, ent]).detach(), 'values': v.detach(),
            'p_action': p.detach().gather(-1, fx['actions'][..., None]).squeeze(-1)}


def example_loss(fx, dtype, device, entropy_coef=0.0, value_loss='smooth_l1'):
    """The loss as examples/a2c_fused_actor.py:38-52 writes it (Categorical, A2C.loss with its return scan restated in
    torch ops, smooth_l1_loss) through torch autograd in `dtype` on `device`: grad, losses, values."""
    E = fx['E']
    params = fx['params'].to(device=device, dtype=dtype).clone().requires_grad_(True)
    w = split(params, E)
    model = lambda x: (lambda f: (f[2], f[3]))(forward(w, x))
    inputs = torch.cat([fx['obs0'][None], fx['obs'][:-1]]).to(device=device, dtype=dtype)
    actions, dones = fx['actions'].to(device), fx['dones'].to(device)
    rewards = fx['rewards'].to(device=device, dtype=dtype)
    probs, values = model(inputs)
    dist = Categorical(probs, validate_args=False)
    log_probs = dist.log_prob(actions)
    entropies = dist.entropy().mean(-1)
    with torch.no_grad():
        _, boot = model(fx['obs'][-1].to(device=device, dtype=dtype))
    returns = returns_of(boot, rewards, dones, fx['gamma'])
    loss_fn = F.smooth_l1_loss if value_loss == 'smooth_l1' else F.mse_loss
    vl = loss_fn(values, returns).mean()
    pl = -((returns - values).detach() * log_probs).mean()
    loss = vl + pl - entropy_coef * entropies.mean()
    return {'grad': _grad_of(loss, params), 'losses': torch.stack([vl, pl, entropies.mean()]).detach(),
            'values': values.detach()}


def block_errors(g, g64, E):
    """err per parameter block: max|g - g64| / max|g64|"""
    a, b = split(g.detach().double().cpu(), E), split(g64.detach().double().cpu(), E)
    return {n: float((a[n] - b[n]).abs().max() / b[n].abs().max().clamp_min(1e-300)) for n in BLOCKS}


def rel_err(x, x64):
    x, x64 = x.detach().double().cpu(), x64.detach().double().cpu()
    return float((x - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def _near_kink(w, x):
    z1, z2, p, _ = forward(w, x)
    near0 = (z1.abs().min(-1).values < 1e-4) | (z2.abs().min(-1).values < 1e-4)
    lo = (p > EPS32 / 4) & (p < EPS32 * 4)
    hi = (1 - p > EPS32 / 4) & (1 - p < EPS32 * 4)
    return near0 | lo.any(-1) | hi.any(-1)


@functools.lru_cache(maxsize=None)
def make_fixture(E, T, N, seed=0, reward_scale=1.0, wp_scale=1.0, gamma=0.99):
    """Seeded CPU fixture (shared, never modified: callers copy what they change).  obs in {0, 1} like crops (uniform
    [0, 1) for E = 4); default nn.Linear init with W1 doubled so that both live and dead units occur; rewards in
    {-1, 0, 1} * reward_scale, sparse; dones Bernoulli(0.2) with env 0 done at every step and env 1 never (N >= 2; a
    single env cannot be both and keeps its draw), which also gives done[T-1] both ways.
    wp_scale > 1 (the sharp policy): Wp is scaled, and eight rows get dense crops (most cells set) picked from a seeded pool
    for a winning probability above 1 - eps32 / 8; four of them take the winning action and four the least likely one, so
    that sampled actions sit beyond both clamps while the other rows keep clear of them."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * E + 31 * T + N)
    torch.manual_seed(seed + E)
    agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)
    with torch.no_grad():
        agent.feedforward[0][0].weight.mul_(2.0)
        agent.action_head.weight.mul_(wp_scale)
    params = pack_policy_params(agent)
    w = split(params.double(), E)

    def draw(n):
        if E == 4:
            return torch.rand((n, E), generator=gen)
        return (torch.rand((n, E), generator=gen) < 0.3).float()

    x = draw((T + 1) * N)
    redrawn = torch.zeros((T + 1) * N, dtype=torch.bool)
    for _ in range(20):
        bad = _near_kink(w, x.double())
        if not bool(bad.any()):
            break
        redrawn |= bad
        x[bad] = draw(int(bad.sum()))
    assert not bool(_near_kink(w, x.double()).any()), 'rows near a kink remain'
    assert float(redrawn.float().mean()) <= 0.10, 'more than 10 % of the rows were re-drawn'
    x = x.view(T + 1, N, E)
    actions = torch.randint(0, 4, (T, N), generator=gen)
    if wp_scale > 1:
        assert E != 4 and T * N >= 16
        pool = (torch.rand((4096, E), generator=gen) < 0.5 + 0.5 * torch.rand((4096, 1), generator=gen)).float()
        p = forward(w, pool.double())[2]
        pool, p = pool[(p.max(-1).values > 1 - EPS32 / 8) & ~_near_kink(w, pool.double())][:8], None
        assert len(pool) == 8, 'the pool has too few saturated rows'
        p = forward(w, pool.double())[2]
        for i, row in enumerate(torch.randperm(T * N, generator=gen)[:8].tolist()):
            x[row // N, row % N] = pool[i]
            actions[row // N, row % N] = p[i].argmax() if i < 4 else p[i].argmin()
    r = torch.randint(-1, 2, (T, N), generator=gen).float() * (torch.rand((T, N), generator=gen) < 0.4).float()
    dones = torch.rand((T, N), generator=gen) < 0.2
    if N >= 2:
        dones[:, 0] = True
        dones[:, 1] = False
    fx = {'E': E, 'T': T, 'N': N, 'gamma': gamma, 'params': params, 'obs0': x[0].contiguous(),
          'obs': x[1:].contiguous(), 'actions': actions,
          'rewards': (r * reward_scale).contiguous(), 'dones': dones, 'reward_scale': reward_scale,
          'redrawn': float(redrawn.float().mean())}
    z1, z2, _, v = forward(w, x[:-1].double())
    fx['live'] = float(torch.cat([z1.flatten(), z2.flatten()]).gt(0).double().mean())
    R = returns_of(forward(w, x[-1].double())[3], fx['rewards'].double(), dones, gamma)
    fx['linear_branch'] = float(((v - R).abs() > 1).double().mean())
    assert 0.05 <= fx['live'] <= 0.95, f"live hidden units: {fx['live']}"
    if reward_scale > 1 and T * N >= 64:
        assert 0.05 <= fx['linear_branch'] <= 0.95, f"|v - R| > 1 in {fx['linear_branch']} of the samples"
    return fx


def to_device(fx, device):
    """(state, out) as FusedA2CLearner.grad takes them, and a learner-ready agent holding the fixture's weights"""
    from wurm_amd.rl import FusedA2CLearner  # noqa: F401  (imported here: the CPU tests of the helper need no library)
    agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=fx['E'])
    with torch.no_grad():
        for p, q in zip([agent.feedforward[0][0].weight, agent.feedforward[0][0].bias, agent.feedforward[1][0].weight,
                         agent.feedforward[1][0].bias, agent.action_head.weight, agent.action_head.bias,
                         agent.value_head.weight, agent.value_head.bias], split(fx['params'], fx['E']).values()):
            p.copy_(q.view(p.shape))
    out = {k: fx[k].to(device) for k in ('actions', 'rewards', 'dones')}
    out['observations'] = fx['obs'].to(device)
    return agent.to(device), fx['obs0'].to(device), out


ENTRY_POINT_STEMS = ('grad', 'grad_gae', 'update', 'update_gae', 'apply')


def build_entry_point(stem, given, device, E, T, N, members=0, lrs=(1e-3,)):
    """What one call of wurm_a2c_ff_<stem> (members == 0) or wurm_a2c_ff_pop_<stem> through ctypes takes, on inputs that
    depend on the shape only: (launch, t, window, optional) — `launch(stream)` makes the call with the arguments in the
    entry point's order and returns its code, without synchronising; `t` the tensors it may write; `window` the rollout
    window it reads (obs0, obs, rewards, actions, dones); `optional` the outputs values_out, returns_out and grad_norm
    (`given`: filled with NaN; else None and handed over as null).  Every tensor stays alive as long as the result."""
    import ctypes

    import numpy as np

    from wurm_amd import _lib
    lib, pop, gae, rows, P = _lib.lib(), members > 0, stem.endswith('_gae'), max(members, 1), num_params(E)
    gen = torch.Generator().manual_seed(E + T + N)
    rnd = lambda *shape: torch.rand(shape, generator=gen)
    t = {'params': (rnd(rows, P) - 0.5) * 0.5, 'grad': rnd(rows, P) - 0.5, 'exp_avg': (rnd(rows, P) - 0.5) * 1e-2,
         'exp_avg_sq': rnd(rows, P) * 1e-3, 'losses': torch.zeros(rows, 3)}
    t = {k: v.to(device) for k, v in t.items()}
    obs0, obs, rewards = rnd(N, E).to(device), rnd(T, N, E).to(device), rnd(T, N).to(device)
    actions, dones = torch.randint(4, (T, N), generator=gen).to(device), (rnd(T, N) < 0.3).to(device)
    opt = lambda *shape: torch.full(shape, float('nan'), device=device) if given else None
    values, returns, norm = opt(T, N), opt(T, N), opt(rows)
    ptr = lambda x: None if x is None else x.data_ptr()
    if pop:
        table = np.zeros((members, 4), dtype=np.float64)
        lam = [float(np.float32(0.99 * 0.95))] * members
        cols = [(ctypes.c_float * members)(*v) for v in (lrs, [0.99] * members, [0.01] * members, lam)]
        assert lib.wurm_a2c_ff_pop_hyper(*[ctypes.addressof(c) for c in cols], members, table.ctypes.data) == _lib.OK
        hyper = torch.from_numpy(table).to(device)
        nbytes = lib.wurm_a2c_ff_pop_workspace_bytes(N, T, E, members)
        hyp, lr, mem, lam_tail = (ptr(hyper),), (), (members,), ()
    else:
        nbytes = lib.wurm_a2c_ff_workspace_bytes(N, T, E)
        hyp, lr, mem, lam_tail = (0.99, 0.01), (lrs[0],), (), (float(np.float32(0.99 * 0.95)),)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    window = {'obs0': obs0, 'obs': obs, 'rewards': rewards, 'actions': actions, 'dones': dones}
    optional = {'values_out': values, 'returns_out': returns, 'grad_norm': norm, 'workspace': ws, 'hyper': hyper if pop else None}

    def launch(stream):
        return _launch(lib, stem, pop, gae, P, t, window, optional, nbytes, N, T, E, hyp, lr, mem, lam_tail, stream)

    return launch, t, window, optional


def _launch(lib, stem, pop, gae, P, t, window, optional, nbytes, N, T, E, hyp, lr, mem, lam_tail, stream):
    """the call of build_entry_point, arguments in the order of include/wurm_hip.h"""
    ptr = lambda x: None if x is None else x.data_ptr()
    obs0, obs, rewards, actions, dones = (window[k] for k in ('obs0', 'obs', 'rewards', 'actions', 'dones'))
    values, returns, norm, ws = (optional[k] for k in ('values_out', 'returns_out', 'grad_norm', 'workspace'))
    head = (ptr(t['params']), ptr(obs0), ptr(obs), ptr(actions), ptr(rewards), ptr(dones), *hyp, 0, ptr(t['grad']),
            ptr(t['losses']), ptr(values), ptr(ws), nbytes, N, T, E, *mem)
    state = (ptr(t['exp_avg']), ptr(t['exp_avg_sq']), ptr(norm))
    adam = (3, *lr, 0.9, 0.999, 1e-8, 0.5)
    tail = (*lam_tail, ptr(returns)) if gae else ()
    fn = getattr(lib, 'wurm_a2c_ff_' + ('pop_' if pop else '') + stem)
    if stem == 'apply':
        rc = fn(ptr(t['params']), ptr(t['grad']), *state, *(hyp if pop else ()), *adam, P, *mem, stream)
    elif stem.startswith('grad'):
        rc = fn(*head, stream, *tail)
    else:
        rc = fn(*head, *state, *adam, stream, *tail)
    return rc


def run_entry_point(stem, given, device, E, T, N, members=0, lrs=(1e-3,)):
    """One call of wurm_a2c_ff_<stem> (members == 0) or wurm_a2c_ff_pop_<stem> through ctypes (build_entry_point), with
    the optional outputs values_out, grad_norm and returns_out handed over (`given`: filled with NaN before, asserted
    written after) or null.  Returns every tensor the call writes whether they are given or not."""
    from wurm_amd import _lib
    launch, t, window, optional = build_entry_point(stem, given, device, E, T, N, members, lrs)
    values, returns, norm = (optional[k] for k in ('values_out', 'returns_out', 'grad_norm'))
    gae = stem.endswith('_gae')
    before = {k: v.clone() for k, v in t.items()}
    rc = launch(_lib.stream_ptr(torch.device(device).index))
    torch.cuda.synchronize()
    assert rc == _lib.OK
    written = ('grad', 'losses') if stem.startswith('grad') else ('params', 'exp_avg', 'exp_avg_sq') if stem == 'apply' \
        else tuple(t)
    for k in t:  # the call did its work, and nothing else
        assert torch.equal(t[k], before[k]) == (k not in written), k
    if given:
        assert stem == 'apply' or bool(torch.isfinite(values).all())
        assert stem.startswith('grad') or bool(torch.isfinite(norm).all())
        assert not gae or bool(torch.isfinite(returns).all())
    return t
