"""The A2C returns op without a GPU: the specification of tests/a2c_returns_ref.py against the five recordings of the
reference (which pins it before anything on the GPU is compared with it) and, in float32, against the oracle bit for bit
(which pins the operation order of the yardstick); the structural facts of its gradient that the GPU tests demand exactly;
and what wurm_a2c_returns, wurm_a2c_returns_backward and wurm_single_stats refuse before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle
from tests import a2c_returns_ref as ref
from tests import replay
from wurm_amd import _lib

RL = ['a2c_nstep_t40_n64', 'a2c_nstep_t5_n512', 'a2c_gae_t40_n64', 'a2c_gae_t20_n128', 'a2c_nstep_norm_t30_n32']
SHAPES = [(1, 1), (1, 257), (2, 63), (5, 65), (7, 513), (40, 256)]
# (use_gae, lambda, gamma): n-step and GAE at every lambda of the GPU tests, and one case at another gamma each
MODES = [(False, None, 0.99), (True, 0.0, 0.99), (True, 0.5, 0.99), (True, 0.95, 0.99), (True, 1.0, 0.99),
         (False, None, 0.9), (True, 0.95, 0.9)]


def mode_id(m):
    return ('gae%g' % m[1] if m[0] else 'nstep') + '-g%g' % m[2]


def _recording(name, dtype):
    z = replay.load(name)
    T, N, gae, norm = (int(v) for v in z['meta'])
    t = {k: torch.from_numpy(z[k]).reshape(T, N).to(dtype) for k in ('rewards', 'values', 'log_probs')}
    t['dones'] = torch.from_numpy(z['dones']).reshape(T, N).bool()
    t['bootstrap'] = torch.from_numpy(z['bootstrap']).reshape(N).to(dtype)
    return z, t, bool(gae), bool(norm), float(z['gamma']), float(z['gae_lambda']) if gae else None


@pytest.mark.parametrize('name', RL)
def test_specification_reproduces_the_recordings(name):
    """float64 returns_spec / loss_spec against what the reference recorded in fp32, within the tolerances
    tests/test_rl_gpu.py applies to the same files (for the returns: the one it has that is not bit-equality)."""
    z, t, gae, norm, gamma, lam = _recording(name, torch.float64)
    T, N = t['rewards'].shape
    v, b = t['values'].requires_grad_(True), t['bootstrap'].requires_grad_(True)
    vl, pl, R = ref.loss_spec(b, t['rewards'], v, t['log_probs'], t['dones'], gamma, gae, lam, norm)
    assert np.allclose(R.detach().numpy(), z['returns'].reshape(T, N), rtol=0, atol=2e-6)
    assert abs(vl.item() - float(z['value_loss'])) <= 2e-6 * max(1.0, abs(float(z['value_loss'])))
    assert abs(pl.item() - float(z['policy_loss'])) <= 2e-6 * max(1.0, abs(float(z['policy_loss'])))
    gv, gb = torch.autograd.grad(vl + pl, (v, b), allow_unused=True)
    gb = torch.zeros(N, dtype=torch.float64) if gb is None else gb
    assert np.allclose(gv.numpy(), z['grad_values'].reshape(T, N), rtol=1e-4, atol=1e-7)
    assert np.allclose(gb.numpy(), z['grad_bootstrap'].reshape(N), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize('name', [n for n in RL if 'norm' not in n])
def test_float32_specification_has_the_recorded_bits(name):
    """the yardstick: returns_spec in float32 on the CPU is the reference's own op sequence"""
    z, t, gae, norm, gamma, lam = _recording(name, torch.float32)
    R = ref.returns_spec(t['bootstrap'], t['rewards'], t['values'], t['dones'], gamma, gae, lam).numpy()
    assert np.array_equal(R.view(np.uint32), z['returns'].reshape(R.shape).view(np.uint32))


@pytest.mark.parametrize('mode', MODES, ids=mode_id)
@pytest.mark.parametrize('T,N', SHAPES)
def test_float32_specification_is_the_oracle(T, N, mode):
    gae, lam, gamma = mode
    c = ref.make_case(T, N)
    R = ref.returns_spec(c['bootstrap'], c['rewards'], c['values'], c['dones'], gamma, gae, lam).numpy()
    want = oracle.a2c_returns(c['bootstrap'].numpy(), c['rewards'].numpy(), c['values'].numpy(), c['dones'].numpy(), gamma,
                              gae, lam)
    assert np.array_equal(R.view(np.uint32), want.view(np.uint32))


def test_case_has_the_planted_columns():
    d = ref.make_case(7, 513)['dones']
    assert bool(d[:, 0].all()) and not bool(d[:, 1].any())
    assert d[:, 2].tolist() == [False] * 6 + [True] and d[:, 3].tolist() == [True] + [False] * 6
    assert 0.1 < float(d[:, 4:].float().mean()) < 0.3
    assert ref.make_case(1, 1)['dones'].shape == (1, 1)
    r = ref.make_case(40, 256)['rewards']
    assert sorted(r.unique().tolist()) == [-1.0, 0.0, 1.0]


@pytest.mark.parametrize('mode', MODES, ids=mode_id)
@pytest.mark.parametrize('T,N', SHAPES)
def test_structure_of_the_gradient(T, N, mode):
    """What the GPU tests demand exactly of the backward kernel, in float64: d returns / d values == 0 for n-step returns;
    no gradient reaches the bootstrap value of an env whose last step is done; at lambda = 0 the return is
    r_t + gamma v_{t+1} !done_t, so grad_values[t] == gamma !done_{t-1} G_{t-1} (and grad_values[0] == 0)."""
    gae, lam, gamma = mode
    c = ref.to(ref.make_case(T, N), torch.float64)
    _, gv, gb = ref.grads_spec(c['bootstrap'], c['rewards'], c['values'], c['dones'], c['G'], gamma, gae, lam)
    nd = (~c['dones']).double()
    if not gae:
        assert torch.equal(gv, torch.zeros_like(gv))
    assert torch.equal(gb[c['dones'][T - 1]], torch.zeros(int(c['dones'][T - 1].sum()), dtype=torch.float64))
    if N >= 2:
        assert float(gb[~c['dones'][T - 1]].abs().min()) > 0
    if gae and lam == 0.0:
        want = torch.cat([torch.zeros(1, N, dtype=torch.float64), gamma * nd[:-1] * c['G'][:-1]])
        assert torch.equal(gv, want)
        assert torch.equal(gb, gamma * nd[T - 1] * c['G'][T - 1])


def test_lambda_one_is_the_n_step_return():
    c = ref.to(ref.make_case(7, 513), torch.float64)
    a = ref.returns_spec(c['bootstrap'], c['rewards'], c['values'], c['dones'], 0.99, True, 1.0)
    b = ref.returns_spec(c['bootstrap'], c['rewards'], c['values'], c['dones'], 0.99)
    assert ref.rel_err(a, b) < 1e-14


@pytest.mark.parametrize('fn', [F.smooth_l1_loss, F.mse_loss])
@pytest.mark.parametrize('gae', [False, True])
def test_loss_specification_is_finite_and_normalised(gae, fn):
    c = ref.to(ref.make_case(5, 65), torch.float64)
    vl, pl, R = ref.loss_spec(c['bootstrap'], c['rewards'], c['values'], c['log_probs'], c['dones'], 0.99, gae,
                              0.95 if gae else None, True, fn)
    assert all(bool(torch.isfinite(x).all()) for x in (vl, pl, R))
    assert abs(float(R.mean())) < 1e-12 and abs(float(R.std()) - 1) < 1e-6


# ---------------------------------------------------------------- what the three entry points refuse before a launch
OK, INV = _lib.OK, _lib.ERR_INVALID_ARG
P = 0x10000   # a non-null pointer (never dereferenced: no row reaches a launch)
ROWS = []


def returns(bootstrap=P, rewards=P, values=P, dones=P, use_gae=0, out=P, t=2, n=8):
    return _lib.lib().wurm_a2c_returns(bootstrap, rewards, values, dones, 0.99, use_gae, 0.9405, out, t, n, None)


def backward(grad_returns=P, dones=P, use_gae=1, grad_values=P, grad_bootstrap=P, t=2, n=8):
    return _lib.lib().wurm_a2c_returns_backward(grad_returns, dones, 0.99, use_gae, 0.9405, grad_values, grad_bootstrap, t,
                                                n, None)


def stats(envs=P, reward=P, done=P, self_collision=P, edge_collision=P, accum=P, n=8, size=9):
    return _lib.lib().wurm_single_stats(envs, reward, done, self_collision, edge_collision, accum, n, size, None)


def row(want, fn, **kw):
    if want == OK:  # a row that passes its checks would launch on the address P, unless the batch is empty
        assert kw.get('n') == 0 or (fn is returns and kw.get('t') == 0), 'an accepted row with work to do'
    ROWS.append(pytest.param(want, fn, kw, id='%s(%s)' % (fn.__name__, ', '.join('%s=%s' % i for i in kw.items()))))


NULL_RETURNS = dict(bootstrap=None, rewards=None, values=None, dones=None, out=None)
NULL_BACKWARD = dict(grad_returns=None, dones=None, grad_values=None, grad_bootstrap=None)
NULL_STATS = dict(envs=None, reward=None, done=None, self_collision=None, edge_collision=None, accum=None)

for use_gae in (0, 1):
    for bad in (dict(t=-1), dict(n=-1), dict(t=-1, n=-1), dict(t=-1, n=0), dict(t=0, n=-1)):   # the sign first
        row(INV, returns, use_gae=use_gae, **bad)
        row(INV, returns, use_gae=use_gae, **NULL_RETURNS, **bad)
    for empty in (dict(t=0), dict(n=0), dict(t=0, n=0)):                                       # nothing to do, nothing read
        row(OK, returns, use_gae=use_gae, **empty)
        row(OK, returns, use_gae=use_gae, **NULL_RETURNS, **empty)
    for ptr in ('bootstrap', 'rewards', 'dones', 'out'):
        row(INV, returns, use_gae=use_gae, **{ptr: None})
row(INV, returns, use_gae=1, values=None)
row(INV, returns, use_gae=7, values=None)                                                      # any non-zero switch is GAE
row(OK, returns, use_gae=1, values=None, n=0)

for use_gae in (0, 1):
    for bad in (dict(t=-1), dict(n=-1), dict(t=-1, n=0), dict(t=0, n=-1)):
        row(INV, backward, use_gae=use_gae, **bad)
        row(INV, backward, use_gae=use_gae, **NULL_BACKWARD, **bad)
    for t in (0, 2):
        row(OK, backward, use_gae=use_gae, n=0, t=t)
        row(OK, backward, use_gae=use_gae, n=0, t=t, **NULL_BACKWARD)
    row(INV, backward, use_gae=use_gae, grad_returns=None)
    row(INV, backward, use_gae=use_gae, dones=None)
    row(INV, backward, use_gae=use_gae, grad_returns=None, t=0)                                # T == 0 still has work to do
    row(INV, backward, use_gae=use_gae, dones=None, t=0)

row(INV, stats, n=-1)
row(INV, stats, n=-1, **NULL_STATS)
for size in (2, 0, -9):
    row(INV, stats, size=size)
    row(INV, stats, size=size, n=0)                                                            # the size check comes first
    row(INV, stats, size=size, n=0, **NULL_STATS)
for size in (3, 9, 25):
    row(OK, stats, n=0, size=size)
    row(OK, stats, n=0, size=size, **NULL_STATS)
for ptr in NULL_STATS:
    row(INV, stats, **{ptr: None})


@pytest.mark.parametrize('want, fn, kw', ROWS)
def test_entry_point_returns_before_a_launch(want, fn, kw):
    n0 = _lib.lib().wurm_launch_count()
    assert fn(**kw) == want
    assert _lib.lib().wurm_launch_count() == n0, 'the row reached a launch'
