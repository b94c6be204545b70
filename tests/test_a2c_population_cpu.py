"""The population forms without a GPU: what FusedA2CPopulation's constructor takes and refuses, the re-homing of the
agents' parameters into the rows of one buffer, what the C ABI refuses before any HIP call, the workspace query, the
hyper-parameter table, and the argument errors of `policy_rollout(..., population=P)`."""
import ctypes

import numpy as np
import pytest
import torch

from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params
from wurm_amd.rl import FusedA2CPopulation

I64 = ctypes.c_int64
F32 = ctypes.c_float
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED


def _agents(P, E=75, **kw):
    cfg = dict(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)
    cfg.update(kw)
    return [FeedforwardAgent(**cfg) for _ in range(P)]


def test_scalars_and_sequences():
    pop = FusedA2CPopulation(_agents(3), lr=[1e-3, 3e-4, 1e-2], gamma=0.9, entropy_coef=(0.0, 0.01, 0.02))
    assert pop.lr == [1e-3, 3e-4, 1e-2] and pop.gamma == [0.9] * 3 and pop.entropy_coef == [0.0, 0.01, 0.02]
    assert pop.gae_lambda is None and pop.step == 0 and pop.num_members == 3
    assert pop.params.shape == (3, 64 * 75 + 4549) and pop.exp_avg.shape == pop.params.shape
    assert pop.exp_avg_sq.shape == pop.params.shape and not pop.exp_avg.any() and not pop.exp_avg_sq.any()
    # the table the kernels read: lr as the decimal written, the others the floats the single learner passes
    f32 = lambda x: float(np.float32(x))
    want = [[lr, f32(0.9), f32(e), 0.0] for lr, e in zip([1e-3, 3e-4, 1e-2], (0.0, 0.01, 0.02))]
    assert pop.hyper.dtype == torch.float64 and pop.hyper.tolist() == want
    gae = FusedA2CPopulation(_agents(2), gamma=[0.99, 0.9], use_gae=True, gae_lambda=0.95)
    assert gae.gae_lambda == [0.95, 0.95]
    assert gae.hyper[:, 3].tolist() == [f32(0.99 * 0.95), f32(0.9 * 0.95)]
    assert FusedA2CPopulation(_agents(2), lr=np.float32(0.5)).lr == [0.5, 0.5]


def test_constructor_refusals():
    for name in ('lr', 'gamma', 'entropy_coef'):
        with pytest.raises(ValueError):
            FusedA2CPopulation(_agents(3), **{name: [0.1, 0.2]})
    with pytest.raises(ValueError):
        FusedA2CPopulation(_agents(3), use_gae=True, gae_lambda=[0.9] * 4)
    with pytest.raises(ValueError):
        FusedA2CPopulation([])
    with pytest.raises(RuntimeError):
        FusedA2CPopulation(_agents(1, 75) + _agents(1, 27))
    with pytest.raises(NotImplementedError):
        FusedA2CPopulation(_agents(1) + _agents(1, num_layers=3))
    with pytest.raises(NotImplementedError):
        FusedA2CPopulation(_agents(1) + _agents(1, hidden_units=32))
    with pytest.raises(NotImplementedError):
        FusedA2CPopulation(_agents(2), use_gae=True)
    with pytest.raises(NotImplementedError):
        FusedA2CPopulation(_agents(2), value_loss='huber_2')
    with pytest.raises(TypeError):
        FusedA2CPopulation(_agents(2), normalise_returns=True)  # not offered
    with pytest.raises(RuntimeError):
        FusedA2CPopulation(_agents(2), lr=[1e-3, -1.0])         # the library refuses the table
    with pytest.raises(RuntimeError):
        FusedA2CPopulation(_agents(2), use_gae=True, gae_lambda=[0.9, float('nan')])


def test_agents_become_views_of_the_rows():
    torch.manual_seed(0)
    agents = _agents(3)
    x = torch.rand(7, 75)
    before = [a(x) for a in agents]
    packed = [pack_policy_params(a) for a in agents]
    pop = FusedA2CPopulation(agents)
    assert pop.params.is_contiguous() and pop.params.dtype == torch.float32
    for p, a in enumerate(agents):
        assert torch.equal(pop.params[p], packed[p]) and torch.equal(pack_policy_params(a), packed[p])
        assert all(torch.equal(u, v) for u, v in zip(a(x), before[p]))
        assert a.feedforward[0][0].weight.data_ptr() == pop.params[p].data_ptr()
    with torch.no_grad():
        pop.params[1, 0] = 5.0
        pop.params[2, -1] = -3.0
    assert agents[1].state_dict()['feedforward.0.0.weight'][0, 0] == 5.0
    assert agents[2].state_dict()['value_head.bias'][0] == -3.0 and agents[0].state_dict()['value_head.bias'][0] != -3.0
    sd = agents[1].state_dict()
    agents[1].load_state_dict({k: v.clone() + 1 for k, v in sd.items()})  # a round trip keeps the views attached
    assert pop.params[1, 0] == 6.0


def test_cpu_tensors_are_refused():
    pop = FusedA2CPopulation(_agents(2))
    out = {'observations': torch.zeros(1, 4, 75), 'actions': torch.zeros(1, 4).long(), 'rewards': torch.zeros(1, 4),
           'dones': torch.zeros(1, 4).bool()}
    with pytest.raises(_lib.WurmHipError):
        pop.grad(torch.zeros(4, 75), out)
    with pytest.raises(_lib.WurmHipError):
        pop.update(torch.zeros(4, 75), out)
    with pytest.raises(_lib.WurmHipError):
        pop.apply(torch.zeros_like(pop.params))


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    N, T, E, P = 8, 2, 27, 2
    nbytes = lib.wurm_a2c_ff_pop_workspace_bytes(N, T, E, P)
    assert nbytes > 0
    buf = (ctypes.c_float * 32)()
    p = (ctypes.addressof(buf) + 15) & ~15  # non-null and 16-byte aligned: every call below is refused before it is read

    def grad(fn=lib.wurm_a2c_ff_pop_grad, params=p, obs0=p, hyper=p, grad_=p, ws=p, ws_bytes=nbytes, n=N, t=T, e=E, kind=0,
             members=P, tail=()):
        return fn(params, obs0, p, p, p, p, hyper, kind, grad_, p, None, ws, I64(ws_bytes), I64(n), I64(t), e,
                  I64(members), None, *tail)

    def update(fn=lib.wurm_a2c_ff_pop_update, params=p, hyper=p, m=p, ws_bytes=nbytes, n=N, e=E, kind=0, step=1, members=P,
               beta1=0.9, tail=()):
        return fn(params, p, p, p, p, p, hyper, kind, p, p, None, p, I64(ws_bytes), I64(n), I64(T), e, I64(members), m,
                  p, None, I64(step), F32(beta1), F32(0.999), F32(1e-8), F32(0.5), None, *tail)

    def apply(params=p, g=p, m=p, hyper=p, step=1, n=1481, members=P, beta2=0.999):
        return lib.wurm_a2c_ff_pop_apply(params, g, m, p, None, hyper, I64(step), F32(0.9), F32(beta2), F32(1e-8),
                                         F32(0.5), I64(n), I64(members), None)

    for kw in (dict(), dict(fn=lib.wurm_a2c_ff_pop_grad_gae, tail=(None,))):
        assert grad(params=None, **kw) == INV and grad(obs0=None, **kw) == INV and grad(grad_=None, **kw) == INV
        assert grad(ws=None, **kw) == INV and grad(hyper=None, **kw) == INV
        assert grad(members=0, **kw) == INV and grad(members=-2, **kw) == INV and grad(members=3, **kw) == INV  # 8 % 3
        assert grad(n=-8, **kw) == INV and grad(n=0, **kw) == INV and grad(t=0, **kw) == INV
        assert grad(e=5, **kw) == UNS and grad(kind=7, **kw) == UNS
        assert grad(ws_bytes=nbytes - 1, **kw) == INV and grad(ws_bytes=0, **kw) == INV
        # enough for ONE member's update is not enough for two
        assert grad(ws_bytes=lib.wurm_a2c_ff_workspace_bytes(N // P, T, E), **kw) == INV
        assert grad(ws=p + 4, **kw) == INV                                       # misaligned
    for kw in (dict(), dict(fn=lib.wurm_a2c_ff_pop_update_gae, tail=(None,))):
        assert update(params=None, **kw) == INV and update(m=None, **kw) == INV and update(hyper=None, **kw) == INV
        assert update(step=0, **kw) == INV and update(members=0, **kw) == INV and update(members=3, **kw) == INV
        assert update(e=5, **kw) == UNS and update(kind=7, **kw) == UNS and update(ws_bytes=nbytes - 1, **kw) == INV
        assert update(beta1=1.0, **kw) == INV
    assert apply(params=None) == INV and apply(g=None) == INV and apply(m=None) == INV and apply(hyper=None) == INV
    assert apply(step=0) == INV and apply(n=0) == INV and apply(members=0) == INV and apply(beta2=1.5) == INV


def test_hyper_table():
    lib = _lib.lib()
    arr = lambda *v: (ctypes.c_float * len(v))(*v)
    table = (ctypes.c_double * 8)(*([-1.0] * 8))
    lr, gamma, ent, lam = arr(1e-3, 3e-4), arr(0.99, 0.9), arr(0.01, 0.0), arr(0.9405, 0.5)
    A = ctypes.addressof
    assert lib.wurm_a2c_ff_pop_hyper(A(lr), A(gamma), A(ent), A(lam), I64(2), A(table)) == _lib.OK
    f32 = lambda x: float(np.float32(x))
    assert list(table) == [1e-3, f32(0.99), f32(0.01), f32(0.9405), 3e-4, f32(0.9), 0.0, 0.5]
    assert lib.wurm_a2c_ff_pop_hyper(A(lr), A(gamma), A(ent), None, I64(2), A(table)) == _lib.OK  # n-step: no lambda
    assert table[3] == 0.0 and table[7] == 0.0
    for bad in (float('nan'), float('inf'), -0.5):      # a non-finite or negative gamma_lambda is refused, table untouched
        table[0] = -1.0
        assert lib.wurm_a2c_ff_pop_hyper(A(lr), A(gamma), A(ent), A(arr(0.9, bad)), I64(2), A(table)) == INV
        assert table[0] == -1.0
    assert lib.wurm_a2c_ff_pop_hyper(A(arr(1e-3, float('nan'))), A(gamma), A(ent), None, I64(2), A(table)) == INV
    assert lib.wurm_a2c_ff_pop_hyper(None, A(gamma), A(ent), None, I64(2), A(table)) == INV
    assert lib.wurm_a2c_ff_pop_hyper(A(lr), A(gamma), A(ent), None, I64(2), None) == INV
    assert lib.wurm_a2c_ff_pop_hyper(A(lr), A(gamma), A(ent), None, I64(0), A(table)) == INV


def test_workspace_query():
    lib = _lib.lib()
    for E in (4, 27, 75, 507):
        for P, M, T in ((1, 5, 5), (3, 2, 5), (2, 300, 20), (16, 512, 20)):
            one = lib.wurm_a2c_ff_workspace_bytes(M, T, E)
            got = lib.wurm_a2c_ff_pop_workspace_bytes(P * M, T, E, P)
            assert one > 0 and got >= P * one and got % 16 == 0
    assert lib.wurm_a2c_ff_pop_workspace_bytes(8, 5, 5, 2) == 0       # unsupported E
    assert lib.wurm_a2c_ff_pop_workspace_bytes(9, 5, 75, 2) == 0      # 9 % 2
    assert lib.wurm_a2c_ff_pop_workspace_bytes(8, 5, 75, 0) == 0 and lib.wurm_a2c_ff_pop_workspace_bytes(0, 5, 75, 2) == 0
    assert lib.wurm_a2c_ff_pop_workspace_bytes(8, 0, 75, 2) == 0


def test_policy_entry_points_refuse_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)

    def single(envs=p, params=p, status=p, mode=_lib.OBS_PARTIAL, n=2, num_envs=6, size=9, members=3):
        return lib.wurm_single_policy_rollout_pop(envs, p, params, p, p, p, p, p, p, p, p, status, mode, n, I64(num_envs),
                                                  size, I64(5), ctypes.c_uint64(1), ctypes.c_uint64(1), I64(0), None,
                                                  I64(members))

    def grid(envs=p, params=p, num_envs=6, size=5, start=(2, 2), members=3):
        return lib.wurm_grid_policy_rollout_pop(envs, p, params, p, p, p, p, p, p, p, p, I64(num_envs), size, I64(5),
                                                start[0], start[1], ctypes.c_uint64(1), ctypes.c_uint64(1), I64(0), None,
                                                I64(members))

    for fn in (single, grid):
        assert fn(envs=None) == INV and fn(params=None) == INV
        assert fn(members=0) == INV and fn(members=-1) == INV and fn(members=4) == INV  # 6 % 4
        assert fn(num_envs=-6) == INV
        assert fn(num_envs=0) == _lib.OK                                             # nothing to do, as the plain call
    for mode in (_lib.OBS_PARTIAL, _lib.OBS_POSITIONS):
        assert single(mode=mode, status=None) == INV
        assert single(mode=mode, size=8) == UNS and single(mode=mode, size=65) == UNS  # what the plain entry point returns
    assert single(n=7) == UNS and single(mode=_lib.OBS_DEFAULT) == UNS
    assert grid(size=4) == UNS and grid(size=65) == UNS and grid(start=(5, 0)) == UNS


def _stub(cls, num_envs, **attrs):
    """an env object without a device: what policy_rollout reads before it touches the library"""
    env = cls.__new__(cls)
    env.num_envs, env.device, env._mode_cache = num_envs, torch.device('cpu'), {}
    for k, v in attrs.items():
        setattr(env, k, v)
    return env


def test_policy_rollout_argument_errors_come_before_the_library(monkeypatch):
    from wurm_amd.envs import SimpleGridworld, SingleSnake

    def untouched(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', untouched)
    monkeypatch.setattr(_lib, 'call', untouched)
    snake = _stub(SingleSnake, 6, size=9, observation_mode='partial_2')
    grid = _stub(SimpleGridworld, 6, size=5, observation_mode='positions', start_location=(2, 2))
    for env, E in ((snake, 75), (grid, 4)):
        n, state = 64 * E + 4549, torch.zeros(6, E)
        for params, P in ((torch.zeros(3, n), 4), (torch.zeros(3, n), 0), (torch.zeros(3, n), -3),  # P must divide 6
                          (torch.zeros(2, n), 3), (torch.zeros(3 * n), 3), (torch.zeros(3, n + 1), 3),  # (P, num_params)
                          (torch.zeros(3, n, dtype=torch.float64), 3), (torch.zeros(n, 3).t(), 3)):    # fp32, contiguous
            with pytest.raises(RuntimeError):
                env.policy_rollout(params, state, 5, population=P)
    # without the keyword the errors are the ones raised before
    with pytest.raises(RuntimeError):
        snake.policy_rollout(torch.zeros(3, 64 * 75 + 4549), torch.zeros(6, 75), 5)
    with pytest.raises(NotImplementedError):
        _stub(SingleSnake, 6, size=9, observation_mode='default').policy_rollout(torch.zeros(2, 9), None, 5, population=2)
