"""The A2C returns op on the GPU (wurm_amd/csrc/rl.hip: a2c_returns_kernel, a2c_returns_backward_kernel, single_stats_kernel;
wurm_amd/rl/a2c.py: _Returns, a2c_returns, A2C.loss) against the float64 specification of tests/a2c_returns_ref.py.

The forward scan is bit-equal to the oracle.  Everything else is held to the rule of tests/test_a2c_learner_gpu.py:
err(kernel) <= 4 * err(torch fp32 running the same specification on the GPU) + 1e-6, both errors max|x - x64| / max|x64|
against float64; every comparison prints both.  The cases of tests/a2c_returns_ref.make_case plant an env that is done at
every step, one that never is, one done only at T - 1 and one done only at t = 0, and their upstream gradient G is the
gradient of no mean."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import a2c_returns_ref as ref
from tests.backends import OracleBackend
from tests.test_a2c_learner_gpu import bound
from tests.test_a2c_returns_cpu import MODES, SHAPES, mode_id
from wurm_amd import _lib
from wurm_amd.rl import A2C, a2c_returns

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD, SENTINEL = 64, -777.0
NSTEP, GAE95 = MODES[0], MODES[3]
cases = lambda f: pytest.mark.parametrize('T,N', SHAPES)(pytest.mark.parametrize('mode', MODES, ids=mode_id)(f))


def f32(x):
    return float(np.float32(x))


def bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint32)


def within(what, got, t32, spec):
    """the rule; returns (err(kernel), err(torch fp32))"""
    ek, et = ref.rel_err(got, spec), ref.rel_err(t32, spec)
    print(f'{what}: kernel {ek:.3e} torch32 {et:.3e}')
    assert math.isfinite(ek) and ek <= bound(et), (what, ek, et)
    return ek, et


@functools.lru_cache(maxsize=None)
def references(T, N, mode):
    """Computed once per case and shared (never modified): the case on the GPU, the float64 specification's returns and
    gradients for the upstream gradient G, and torch fp32's on the GPU."""
    gae, lam, gamma = mode
    c = ref.make_case(T, N)
    c64, c32 = ref.to(c, torch.float64), ref.to(c, torch.float32, DEV)
    args = lambda d: (d['bootstrap'], d['rewards'], d['values'], d['dones'], d['G'], gamma, gae, lam)
    return {'cpu': c, 'gpu': c32, 'spec': ref.grads_spec(*args(c64)), 't32': ref.grads_spec(*args(c32))}


def c_forward(c, mode, values=True):
    """wurm_a2c_returns through the C ABI on the GPU case `c`"""
    gae, lam, gamma = mode
    T, N = c['rewards'].shape
    out = torch.full((T * N + PAD,), SENTINEL, device=DEV)
    d = c['dones'].to(torch.uint8)
    rc = _lib.lib().wurm_a2c_returns(_lib.ptr(c['bootstrap']), _lib.ptr(c['rewards']), _lib.ptr(c['values'] if values else None),
                                     _lib.ptr(d), f32(gamma), int(gae), f32(gamma * lam) if gae else 0.0, _lib.ptr(out), T, N,
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.OK
    assert torch.equal(out[T * N:], torch.full((PAD,), SENTINEL, device=DEV)), 'the forward scan wrote behind its output'
    return out[:T * N].view(T, N)


def c_backward(G, dones, mode, want_values=True, want_bootstrap=True):
    """wurm_a2c_returns_backward through the C ABI; each output it is asked for is followed by PAD sentinels that must stay"""
    gae, lam, gamma = mode
    T, N = dones.shape
    gv = torch.full((T * N + PAD,), SENTINEL, device=DEV) if want_values else None
    gb = torch.full((N + PAD,), SENTINEL, device=DEV) if want_bootstrap else None
    G = G.contiguous() if G.numel() else torch.zeros(1, device=DEV)
    d = dones.to(torch.uint8).contiguous() if dones.numel() else torch.zeros(1, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().wurm_a2c_returns_backward(_lib.ptr(G), _lib.ptr(d), f32(gamma), int(gae), f32(gamma * lam) if gae else 0.0,
                                              _lib.ptr(gv), _lib.ptr(gb), T, N, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.OK
    tail = torch.full((PAD,), SENTINEL, device=DEV)
    assert gv is None or torch.equal(gv[T * N:], tail), 'grad_values: written behind the (T,N) elements'
    assert gb is None or torch.equal(gb[N:], tail), 'grad_bootstrap: written behind the N elements'
    return (None if gv is None else gv[:T * N].view(T, N)), (None if gb is None else gb[:N])


# ---------------------------------------------------------------- forward
@cases
def test_forward_has_the_oracles_bits_and_is_within_the_bound(T, N, mode):
    gae, lam, gamma = mode
    r = references(T, N, mode)
    c, g = r['cpu'], r['gpu']
    want = oracle.a2c_returns(c['bootstrap'].numpy(), c['rewards'].numpy(), c['values'].numpy(), c['dones'].numpy(), gamma,
                              gae, lam)
    got = a2c_returns(g['bootstrap'], g['rewards'], g['values'], g['dones'], gamma, gae, lam)
    assert got.shape == (T, N) and got.dtype == torch.float32
    assert np.array_equal(bits(got), want.view(np.uint32))
    assert np.array_equal(bits(c_forward(g, mode)), want.view(np.uint32))
    within(f'returns T={T} N={N} {mode_id(mode)}', got, r['t32'][0], r['spec'][0])
    if not gae:   # the n-step scan never reads the values
        assert np.array_equal(bits(c_forward(g, mode, values=False)), want.view(np.uint32))
    # (T,N,1) inputs and every dtype of dones a2c_returns accepts
    col = a2c_returns(g['bootstrap'][:, None], g['rewards'][..., None], g['values'][..., None], g['dones'][..., None], gamma,
                      gae, lam)
    assert col.shape == (T, N, 1) and np.array_equal(bits(col).reshape(T, N), want.view(np.uint32))
    for dtype in (torch.uint8, torch.float32):
        other = a2c_returns(g['bootstrap'], g['rewards'], g['values'], g['dones'].to(dtype), gamma, gae, lam)
        assert np.array_equal(bits(other), want.view(np.uint32)), dtype


# ---------------------------------------------------------------- backward through the C ABI
@cases
def test_backward_is_within_the_bound_of_float64(T, N, mode):
    """grad_values and grad_bootstrap for the upstream gradient G against float64 autograd of the specification, the zeros
    the structure demands exactly, and the same bits from a second call.  At lambda = 1 the returns do not depend on the
    values: float64 itself leaves a rounding residue of 1e-16 there and both errors are ~1e9 (docs/HISTORY.md), so that
    case says only that the kernel's residue is no larger than four times torch's."""
    gae, lam, gamma = mode
    r = references(T, N, mode)
    g, (_, gv64, gb64), (_, gv32, gb32) = r['gpu'], r['spec'], r['t32']
    what = f'T={T} N={N} {mode_id(mode)}'
    gv, gb = c_backward(g['G'], g['dones'], mode)
    within('grad_bootstrap ' + what, gb, gb32, gb64)
    last_done = g['dones'][T - 1]
    assert torch.equal(gb[last_done], torch.zeros(int(last_done.sum()), device=DEV))
    if gae:
        within('grad_values ' + what, gv, gv32, gv64)
    else:
        assert torch.equal(gv, torch.zeros((T, N), device=DEV))
    if gae and lam == 0.0:   # R_t = r_t + gamma v_{t+1} !done_t: one product per element (the kernel's g - A is g - g)
        nd = (~r['cpu']['dones']).double()
        want = torch.cat([torch.zeros(1, N, dtype=torch.float64), gamma * nd[:-1] * r['cpu']['G'][:-1].double()])
        within('grad_values, lambda = 0 in closed form ' + what, gv, gv32, want)
    gv2, gb2 = c_backward(g['G'], g['dones'], mode)
    assert torch.equal(gv, gv2) and torch.equal(gb, gb2)


@pytest.mark.parametrize('mode', [NSTEP, GAE95], ids=mode_id)
@pytest.mark.parametrize('T,N', [(2, 63), (1, 257), (7, 513)])
def test_each_output_alone_has_the_bits_of_both(T, N, mode):
    """grad_values == NULL and grad_bootstrap == NULL, one at a time (c_backward asserts the sentinels behind the other)"""
    g = references(T, N, mode)['gpu']
    gv, gb = c_backward(g['G'], g['dones'], mode)
    gv1, none = c_backward(g['G'], g['dones'], mode, want_bootstrap=False)
    assert none is None and torch.equal(gv1, gv)
    none, gb1 = c_backward(g['G'], g['dones'], mode, want_values=False)
    assert none is None and torch.equal(gb1, gb)


@pytest.mark.parametrize('mode', [NSTEP, GAE95], ids=mode_id)
def test_backward_of_no_steps_writes_a_zero_bootstrap_gradient(mode):
    gv, gb = c_backward(torch.zeros((0, 5), device=DEV), torch.zeros((0, 5), dtype=torch.bool, device=DEV), mode)
    assert gv.numel() == 0 and torch.equal(gb, torch.zeros(5, device=DEV))


def _adjoint_defect(R, gv, gb, G, u_b, u_v, scale):
    lhs = (G.double() * R.double()).sum()
    rhs = (gb.double() * u_b.double()).sum() + (gv.double() * u_v.double()).sum()
    return float((lhs - rhs).abs().cpu() / scale)


@pytest.mark.parametrize('mode', [NSTEP, GAE95], ids=mode_id)
@pytest.mark.parametrize('T,N', [(5, 65), (7, 513)])
def test_the_two_kernels_are_adjoint(T, N, mode):
    """With rewards = 0 the forward is linear in u = (bootstrap, values): <G, forward(u)> == <backward(G), u>, both
    accumulated in float64 from the fp32 outputs, up to bound(e32) * sum|G R| where e32 is the same defect of torch fp32."""
    gae, lam, gamma = mode
    r = references(T, N, mode)
    g = dict(r['gpu'], rewards=torch.zeros((T, N), device=DEV))
    c64 = ref.to(r['cpu'], torch.float64)
    R64 = ref.returns_spec(c64['bootstrap'], torch.zeros_like(c64['rewards']), c64['values'], c64['dones'], gamma, gae, lam)
    scale = float((c64['G'] * R64).abs().sum())
    assert scale > 0
    R = c_forward(g, mode)
    gv, gb = c_backward(g['G'], g['dones'], mode)
    R32, gv32, gb32 = ref.grads_spec(g['bootstrap'], g['rewards'], g['values'], g['dones'], g['G'], gamma, gae, lam)
    ek = _adjoint_defect(R, gv, gb, g['G'], g['bootstrap'], g['values'], scale)
    et = _adjoint_defect(R32, gv32, gb32, g['G'], g['bootstrap'], g['values'], scale)
    print(f'adjoint defect T={T} N={N} {mode_id(mode)}: kernel {ek:.3e} torch32 {et:.3e}')
    assert math.isfinite(ek) and ek <= bound(et), (ek, et)


# ---------------------------------------------------------------- a2c_returns in the autograd graph
WHO = ['bootstrap', 'values', 'both', 'neither', 'strided', 'float64', 'column']


@pytest.mark.parametrize('who', WHO)
@pytest.mark.parametrize('mode', [NSTEP, GAE95], ids=mode_id)
@pytest.mark.parametrize('T,N', [(2, 63), (7, 513)])
def test_autograd_asks_for_what_it_needs(T, N, mode, who):
    """_Returns.backward: only one of the two gradients needed, both, none; an upstream gradient that is not contiguous;
    float64 leaves (gradients return in float64 through the cast); (T,N,1) leaves."""
    gae, lam, gamma = mode
    r = references(T, N, mode)
    g, (_, gv64, gb64), (_, gv32, gb32) = r['gpu'], r['spec'], r['t32']
    what = f'{who} T={T} N={N} {mode_id(mode)}'
    dtype = torch.float64 if who == 'float64' else torch.float32
    need_b, need_v = who not in ('values', 'neither'), who not in ('bootstrap', 'neither')
    b = g['bootstrap'].to(dtype).clone().requires_grad_(need_b)
    v = g['values'].to(dtype).clone().requires_grad_(need_v)
    rewards, dones, G = g['rewards'], g['dones'], g['G']
    if who == 'column':
        b, v = (x.detach()[..., None].requires_grad_(True) for x in (b, v))
        rewards, dones, G = rewards[..., None], dones[..., None], G[..., None]
    R = a2c_returns(b, rewards, v, dones, gamma, gae, lam)
    assert R.dtype == torch.float32 and R.shape == rewards.shape
    assert R.requires_grad == (who != 'neither')
    if who == 'neither':
        return
    if who == 'strided':
        W = G.t().contiguous()
        loss = (R.t() * W).sum()          # d loss / d R is W.t(): strides (1, T)
    else:
        loss = (R * G).sum()
    loss.backward()
    if need_b:
        assert b.grad.dtype == dtype and b.grad.shape == b.shape
        within('grad_bootstrap ' + what, b.grad.reshape(N), gb32, gb64)
    else:
        assert b.grad is None
    if need_v:
        assert v.grad.dtype == dtype and v.grad.shape == v.shape
        if gae:
            within('grad_values ' + what, v.grad.reshape(T, N), gv32, gv64)
        else:
            assert torch.equal(v.grad, torch.zeros_like(v))
    else:
        assert v.grad is None


# ---------------------------------------------------------------- A2C.loss
@pytest.mark.parametrize('fn', [F.smooth_l1_loss, F.mse_loss], ids=['smooth_l1', 'mse'])
@pytest.mark.parametrize('norm', [False, True], ids=['plain', 'normalised'])
@pytest.mark.parametrize('gae', [False, True], ids=['nstep', 'gae'])
@pytest.mark.parametrize('T,N', [(5, 65), (7, 513)])
def test_a2c_loss(T, N, gae, norm, fn):
    gamma, lam = 0.99, 0.95 if gae else None
    c = ref.make_case(T, N)
    what = f'T={T} N={N} {"gae" if gae else "nstep"} norm={norm} {fn.__name__}'

    def run(loss, d):
        b, v = d['bootstrap'].clone().requires_grad_(True), d['values'].clone().requires_grad_(True)
        vl, pl, R = loss(b, d['rewards'], v, d['log_probs'], d['dones'])
        gv, gb = torch.autograd.grad(vl + pl, (v, b))
        return {'value_loss': vl.detach(), 'policy_loss': pl.detach(), 'returns': R.detach(), 'grad_values': gv,
                'grad_bootstrap': gb}

    spec_loss = lambda b, r, v, lp, d: ref.loss_spec(b, r, v, lp, d, gamma, gae, lam, norm, fn)
    spec, t32 = run(spec_loss, ref.to(c, torch.float64)), run(spec_loss, ref.to(c, torch.float32, DEV))
    a2c = A2C(gamma=gamma, value_loss_fn=fn, normalise_returns=norm, use_gae=gae, gae_lambda=lam)
    got = run(lambda b, r, v, lp, d: a2c.loss(b, r, v, lp, d, return_returns=True), ref.to(c, torch.float32, DEV))
    for k in spec:
        assert bool(torch.isfinite(spec[k]).all()) and float(spec[k].abs().max()) > 0, k
    for k in spec:
        within(f'{k} {what}', got[k], t32[k], spec[k])


# ---------------------------------------------------------------- wurm_single_stats
STATS_N = [1, 3, 5, 32, 64, 301]      # grids of 1, 1, 2, 8, 16 and 76 workgroups of four envs
GUARD = 1234.5


def _reset(o, envs, done, rng):
    """the oracle's reset; at S <= 8, where the reference (and so the oracle) refuses to create an env, a fresh env as
    the reference lays it out: a snake of length 3 through an interior cell (body 1, 2, 3, head on the 3), one food"""
    N, _, S, _ = envs.shape
    if S > 8:
        o.single_reset(envs, done, 'none')
        return
    for i in np.flatnonzero(done):
        envs[i] = 0
        y, x, d = rng.randint(1, S - 1), rng.randint(1, S - 1), rng.randint(4)
        dy, dx = [(-1, 0), (0, 1), (1, 0), (0, -1)][d]
        envs[i, 2, y - dy, x - dx], envs[i, 2, y, x], envs[i, 2, y + dy, x + dx] = 1, 2, 3
        envs[i, 1, y + dy, x + dx] = 1
        free = np.flatnonzero(envs[i, 2].reshape(-1) == 0)
        envs[i, 0].reshape(-1)[free[rng.randint(len(free))]] = 1


@functools.lru_cache(maxsize=None)
def stats_states(S, N):
    """two consecutive steps' (state, reward, done, self_collision, edge_collision) from the oracle, after a reset and three
    steps of random actions; env 0 has all three flags planted, env 1 none (shared, never modified)"""
    rng = np.random.RandomState(100 * S + N)
    o = OracleBackend(seed=S + N)
    envs = np.zeros((N, 3, S, S), np.float32)
    _reset(o, envs, np.ones(N, np.uint8), rng)
    out = []
    for t in range(5):
        _, reward, done, sc, ec = o.single_step(envs, rng.randint(0, 4, N).astype(np.int64), 'none')
        if t >= 3:
            flags = [done.copy(), sc.copy(), ec.copy()]
            for f in flags:
                f[0] = 1
                if N > 1:
                    f[1] = 0
            out.append((envs.copy(), reward.copy(), *flags))
        _reset(o, envs, done, rng)
    return out


@pytest.mark.parametrize('N', STATS_N)
@pytest.mark.parametrize('S', [5, 9, 12, 25])
def test_single_stats(S, N):
    """Exactly the oracle's five sums, accumulated over two calls into a buffer that was not zero, with the three doubles
    behind it untouched.  The states are followed by cells of a larger value than any body cell, so a lane that read
    beyond the S * S cells of the last env (S = 5: 25 cells for 64 lanes) would change the maximum."""
    init = np.array([7.0, -3.0, 2.0, 1.0, 100.0])
    acc = torch.tensor(list(init) + [GUARD] * 3, dtype=torch.float64, device=DEV)
    want = init.copy()
    for envs, reward, done, sc, ec in stats_states(S, N):
        assert set(np.unique(reward).tolist()) <= {-1.0, 0.0, 1.0} and envs[:, 2].max() >= 2
        want += oracle.single_stats(envs, reward, done, sc, ec)
        buf = torch.full((envs.size + 256,), 1e6, device=DEV)
        buf[:envs.size] = torch.from_numpy(envs).to(DEV).flatten()
        dev = [torch.from_numpy(x).to(DEV) for x in (reward, done, sc, ec)]
        rc = _lib.lib().wurm_single_stats(_lib.ptr(buf), *[_lib.ptr(x) for x in dev], _lib.ptr(acc), N, S, _lib.stream_ptr())
        assert rc == _lib.OK
    got = acc.cpu().numpy()
    assert np.array_equal(got[:5], want), (got, want)
    assert np.array_equal(got[5:], [GUARD] * 3)
