"""Learning from a league window without a GPU: what `FusedA2CPopulation.grad / update / apply(..., plan=, learn=)` refuse
before anything is launched, what the C ABI of wurm_a2c_ff_league_* refuses before any HIP call, and the workspace query
against its formula (include/wurm_hip.h)."""
import ctypes
import types

import pytest
import torch

from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.envs._multi_league import league_plan
from wurm_amd.rl import FusedA2CPopulation

I64 = ctypes.c_int64
F32 = ctypes.c_float
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
E = 27


def _pop(P, **kw):
    return FusedA2CPopulation([FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)
                               for _ in range(P)], **kw)


def _window(T, R):
    out = {'observations': torch.zeros(T, R, E), 'actions': torch.zeros(T, R).long(), 'rewards': torch.zeros(T, R),
           'dones': torch.zeros(T, R).bool()}
    return torch.zeros(R, E), out


def _plan(K, N, A):
    env = types.SimpleNamespace(num_snakes=K, num_envs=N)  # (league_plan needs no more of an env)
    return league_plan(env, (torch.arange(K * N) % A).view(K, N), A)


def test_plan_and_members_must_agree():
    pop, (state, out) = _pop(3), _window(2, 8)
    for plan in (_plan(2, 4, 2), _plan(2, 4, 4)):
        for call in (lambda: pop.grad(state, out, plan=plan), lambda: pop.update(state, out, plan=plan),
                     lambda: pop.apply(torch.zeros_like(pop.params), plan=plan)):
            with pytest.raises(RuntimeError, match=f'the plan names {plan.num_policies} policies but the population has 3'):
                call()
    with pytest.raises(RuntimeError, match='plan must come from league_plan'):
        pop.update(state, out, plan=(1, 2, 3, 4))
    assert pop.step == 0


def test_learn_shape_and_dtype():
    pop, (state, out), plan = _pop(3), _window(2, 8), _plan(2, 4, 3)
    for learn in (torch.ones(2, dtype=torch.bool), torch.ones(3, 1, dtype=torch.bool), torch.ones(3), torch.ones(3).long(),
                  [1, 1, 0]):
        with pytest.raises(RuntimeError, match=r'learn must be a \(3,\) bool or uint8 tensor'):
            pop.update(state, out, plan=plan, learn=learn)
        with pytest.raises(RuntimeError, match=r'learn must be a \(3,\) bool or uint8 tensor'):
            pop.apply(torch.zeros_like(pop.params), plan=plan, learn=learn)
    with pytest.raises(RuntimeError, match='learn goes with a plan'):
        pop.update(state, out, learn=torch.ones(3, dtype=torch.bool))


def test_cpu_tensors_are_refused():
    pop, (state, out), plan = _pop(3), _window(2, 8), _plan(2, 4, 3)
    for learn in (None, torch.ones(3, dtype=torch.bool), torch.ones(3, dtype=torch.uint8)):
        with pytest.raises(_lib.WurmHipError):
            pop.grad(state, out, plan=plan, learn=learn)
        with pytest.raises(_lib.WurmHipError):
            pop.update(state, out, plan=plan, learn=learn)
        with pytest.raises(_lib.WurmHipError):
            pop.apply(torch.zeros_like(pop.params), plan=plan, learn=learn)
    assert pop.step == 0


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    R, T, A = 8, 2, 3
    nbytes = lib.wurm_a2c_ff_league_workspace_bytes(R, T, E, A)
    assert nbytes > 0
    buf = (ctypes.c_float * 32)()
    p = (ctypes.addressof(buf) + 15) & ~15  # non-null and 16-byte aligned: every call below is refused before it is read

    def grad(fn=lib.wurm_a2c_ff_league_grad, params=p, obs0=p, hyper=p, order=p, offsets=p, learn=None, grad_=p, ws=p,
             ws_bytes=nbytes, r=R, t=T, e=E, kind=0, members=A, tail=()):
        return fn(params, obs0, p, p, p, p, hyper, order, offsets, learn, kind, grad_, p, None, ws, I64(ws_bytes), I64(r),
                  I64(t), e, I64(members), None, *tail)

    def update(fn=lib.wurm_a2c_ff_league_update, params=p, hyper=p, order=p, offsets=p, m=p, ws_bytes=nbytes, r=R, e=E,
               kind=0, step=1, members=A, beta1=0.9, tail=()):
        return fn(params, p, p, p, p, p, hyper, order, offsets, None, kind, p, p, None, p, I64(ws_bytes), I64(r), I64(T), e,
                  I64(members), m, p, None, I64(step), F32(beta1), F32(0.999), F32(1e-8), F32(0.5), None, *tail)

    def apply(params=p, g=p, m=p, hyper=p, offsets=p, step=1, n=1481, r=R, members=A, beta2=0.999):
        return lib.wurm_a2c_ff_league_apply(params, g, m, p, None, hyper, offsets, None, I64(step), F32(0.9), F32(beta2),
                                            F32(1e-8), F32(0.5), I64(n), I64(r), I64(members), None)

    big = 1 << 31
    for kw in (dict(), dict(fn=lib.wurm_a2c_ff_league_grad_gae, tail=(None,))):
        assert grad(params=None, **kw) == INV and grad(obs0=None, **kw) == INV and grad(grad_=None, **kw) == INV
        assert grad(ws=None, **kw) == INV and grad(hyper=None, **kw) == INV
        assert grad(order=None, **kw) == INV and grad(offsets=None, **kw) == INV
        assert grad(members=0, **kw) == INV and grad(members=-2, **kw) == INV
        assert grad(r=-8, **kw) == INV and grad(r=0, **kw) == INV and grad(t=0, **kw) == INV
        assert grad(e=5, **kw) == UNS and grad(kind=7, **kw) == UNS
        assert grad(ws_bytes=nbytes - 1, **kw) == INV and grad(ws_bytes=0, **kw) == INV
        assert grad(ws=p + 4, **kw) == INV                                       # misaligned
        # more members than the grid's y has, more rows than an int32 names: with a workspace that would be large enough
        assert grad(members=65536, ws_bytes=1 << 62, **kw) == UNS and grad(r=big, ws_bytes=1 << 62, **kw) == UNS
    for kw in (dict(), dict(fn=lib.wurm_a2c_ff_league_update_gae, tail=(None,))):
        assert update(params=None, **kw) == INV and update(m=None, **kw) == INV and update(hyper=None, **kw) == INV
        assert update(order=None, **kw) == INV and update(offsets=None, **kw) == INV
        assert update(step=0, **kw) == INV and update(members=0, **kw) == INV and update(r=0, **kw) == INV
        assert update(e=5, **kw) == UNS and update(kind=7, **kw) == UNS and update(ws_bytes=nbytes - 1, **kw) == INV
        assert update(beta1=1.0, **kw) == INV
        assert update(members=65536, ws_bytes=1 << 62, **kw) == UNS and update(r=big, ws_bytes=1 << 62, **kw) == UNS
    assert apply(params=None) == INV and apply(g=None) == INV and apply(m=None) == INV and apply(hyper=None) == INV
    assert apply(offsets=None) == INV and apply(r=0) == INV and apply(r=-1) == INV
    assert apply(step=0) == INV and apply(n=0) == INV and apply(members=0) == INV and apply(beta2=1.5) == INV
    assert apply(members=65536) == UNS and apply(r=big) == UNS


def _formula(R, T, E, A):
    """include/wurm_hip.h: min(R, 256 A) partials of `stride` floats, then 8 floats for each of the R (T + 1) rows"""
    padded = (E + 15) // 16 * 16
    stride = (64 * padded + 64 + 4096 + 64 + 256 + 4 + 64 + 1 + 3 + 3) // 4 * 4
    return 4 * (min(R, 256 * A) * stride + R * (T + 1) * 8)


def test_workspace_query():
    lib = _lib.lib()
    query = lib.wurm_a2c_ff_league_workspace_bytes
    for e in (4, 27, 75, 507):
        # R < 256 A: a partial per row at most;  R = 256 A;  R > 256 A: 256 per member at most
        for R, T, A in ((1, 1, 1), (12, 5, 4), (511, 5, 2), (512, 5, 2), (513, 5, 2), (881, 2, 7), (40000, 20, 16),
                        (255, 3, 1), (256, 3, 1), (257, 3, 1)):
            got = query(R, T, e, A)
            assert got == _formula(R, T, e, A) and got % 16 == 0, (e, R, T, A)
    # one member with all the rows is the stand-alone workspace; a league never needs more than the population's
    assert query(300, 5, 75, 1) == lib.wurm_a2c_ff_workspace_bytes(300, 5, 75)
    assert query(1200, 5, 75, 4) <= lib.wurm_a2c_ff_pop_workspace_bytes(1200, 5, 75, 4)
    assert query(8, 5, 5, 2) == 0                                           # unsupported E
    assert query(8, 5, 75, 0) == 0 and query(0, 5, 75, 2) == 0 and query(8, 0, 75, 2) == 0
    assert query(8, 5, 75, 65536) == 0 and query(1 << 31, 5, 75, 2) == 0 and query((1 << 31) - 1, 5, 75, 2) > 0
