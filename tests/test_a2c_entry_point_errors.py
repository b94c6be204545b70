"""The return codes of the wurm_a2c_ff_* entry points for calls that must not reach a launch, and the ORDER of their
checks (no GPU): the eleven launching entry points — grad, grad_gae, apply, update, update_gae and the six _pop_ forms —
and the four that never launch (the two workspace queries, wurm_a2c_ff_pop_hyper, wurm_a2c_ff_hyper_parameter).  Every
row of a launching entry point breaks at least one rule, so it returns from the validation; the launch counter is
asserted unchanged for every row.

The expected codes are the ones the library returned BEFORE the host layer of wurm_amd/csrc/a2c_learner.hip was given one
copy of each path (docs/HISTORY.md: this table was run against a build of that revision, all rows equal); rows that
break two rules at once pin which check comes first.  Pointers that a row needs non-null are the address P (16-byte
aligned), which is never dereferenced."""
import ctypes

import pytest

from wurm_amd import _lib

OK, INV, UNS = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
P = 0x10000
NAN, INF = float('nan'), float('inf')
N, T, E, MEMBERS = 8, 2, 27, 2
FORMS = [(gae, pop) for pop in (False, True) for gae in (False, True)]
GRAD_PTRS = ('params', 'obs0', 'obs', 'actions', 'rewards', 'dones', 'grad', 'losses', 'ws')


def ws_bytes(pop, n=N, t=T, e=E, members=MEMBERS):
    """what the library asks for (the whole workspace of the form)"""
    if pop:
        return _lib.lib().wurm_a2c_ff_pop_workspace_bytes(n, t, e, members)
    return _lib.lib().wurm_a2c_ff_workspace_bytes(n, t, e)


def _args(pop, kw):
    """defaults that pass every check (so a row fails exactly where it says), then the row's own"""
    a = dict(params=P, obs0=P, obs=P, actions=P, rewards=P, dones=P, grad=P, losses=P, ws=P, hyper=P, exp_avg=P,
             exp_avg_sq=P, n=N, t=T, e=E, kind=0, members=MEMBERS, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             num_params=1481, gamma_lambda=0.9405)
    a.update(kw)
    if 'ws_bytes' not in a:
        a['ws_bytes'] = ws_bytes(pop, a['n'], a['t'], a['e'], a['members'])  # (0 for a shape the query refuses)
    return a


def _name(stem, gae, pop):
    return 'wurm_a2c_ff_%s%s%s' % ('pop_' if pop else '', stem, '_gae' if gae else '')


def _grad_head(a, pop):
    """the arguments grad and update share, up to num_inputs (values_out null)"""
    hyper = (a['hyper'],) if pop else (0.99, 0.0)
    return (a['params'], a['obs0'], a['obs'], a['actions'], a['rewards'], a['dones'], *hyper, a['kind'], a['grad'],
            a['losses'], None, a['ws'], a['ws_bytes'], a['n'], a['t'], a['e'], *((a['members'],) if pop else ()))


def _gae_tail(a, gae, pop):
    return () if not gae else (None,) if pop else (a['gamma_lambda'], None)


def grad(gae=False, pop=False, **kw):
    a = _args(pop, kw)
    return getattr(_lib.lib(), _name('grad', gae, pop))(*_grad_head(a, pop), None, *_gae_tail(a, gae, pop))


def update(gae=False, pop=False, **kw):
    a = _args(pop, kw)
    lr = () if pop else (a['lr'],)
    return getattr(_lib.lib(), _name('update', gae, pop))(
        *_grad_head(a, pop), a['exp_avg'], a['exp_avg_sq'], None, a['step'], *lr, a['beta1'], a['beta2'], a['eps'], 0.5,
        None, *_gae_tail(a, gae, pop))


def apply(pop=False, **kw):
    a = _args(pop, dict(dict(ws_bytes=0), **kw))
    if pop:
        return _lib.lib().wurm_a2c_ff_pop_apply(a['params'], a['grad'], a['exp_avg'], a['exp_avg_sq'], None, a['hyper'],
                                                a['step'], a['beta1'], a['beta2'], a['eps'], 0.5, a['num_params'],
                                                a['members'], None)
    return _lib.lib().wurm_a2c_ff_apply(a['params'], a['grad'], a['exp_avg'], a['exp_avg_sq'], None, a['step'], a['lr'],
                                        a['beta1'], a['beta2'], a['eps'], 0.5, a['num_params'], None)


def workspace(n=N, t=T, e=E):
    return _lib.lib().wurm_a2c_ff_workspace_bytes(n, t, e)


def pop_workspace(n=N, t=T, e=E, members=MEMBERS):
    return _lib.lib().wurm_a2c_ff_pop_workspace_bytes(n, t, e, members)


def pop_hyper(lr=(1e-3, 3e-4), gamma=(0.99, 0.9), entropy_coef=(0.01, 0.0), gamma_lambda=None, members=2, table=True):
    arr = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    cols = [arr(c) for c in (lr, gamma, entropy_coef, gamma_lambda)]
    out = (ctypes.c_double * 8)(*([-1.0] * 8))
    rc = _lib.lib().wurm_a2c_ff_pop_hyper(*[None if c is None else ctypes.addressof(c) for c in cols], members,
                                          ctypes.addressof(out) if table else None)
    assert rc == OK or list(out) == [-1.0] * 8, 'a refused table was written to'
    return rc


def hyper_parameter(x=1e-3, value=True):
    out = ctypes.c_double(-1.0)
    rc = _lib.lib().wurm_a2c_ff_hyper_parameter(x, ctypes.addressof(out) if value else None)
    assert (out.value == 1e-3) if rc == OK else (out.value == -1.0)
    return rc


NEVER_LAUNCH = (workspace, pop_workspace, pop_hyper, hyper_parameter)
ROWS = []


def row(want, fn, **kw):
    assert fn in NEVER_LAUNCH or want != OK, 'a row of a launching entry point that passes its checks would launch'
    name = '%s(%s)' % (fn.__name__, ', '.join('%s=%s' % (k, v) for k, v in kw.items()))
    ROWS.append(pytest.param(want, fn, kw, id=name))


def grad_rows(fn, gae, pop, **base):
    """check_grad's rules in their order; `base`: what makes the call fail BEHIND them in any case (update's rows: a rule
    of the apply half), so these rows also say that the grad half is checked first"""
    def r(want, **kw):
        row(want, fn, gae=gae, pop=pop, **dict(base, **kw))
    for ptr in GRAD_PTRS:
        r(INV, **{ptr: None})
    r(INV, n=0)
    r(INV, n=-N)
    r(INV, t=0)
    r(INV, t=-1)
    r(INV, e=0, ws_bytes=1 << 20)
    r(INV, e=-27, ws_bytes=1 << 20)
    r(INV, ws_bytes=-1)
    r(INV, ws=P + 4)                                             # 16-byte accesses
    r(INV, ws=P + 8)
    r(UNS, e=5, ws_bytes=1 << 20)
    r(UNS, e=26, ws_bytes=1 << 20)
    r(UNS, e=3 * 15 * 15, ws_bytes=1 << 30)                      # partial_7: one past the largest
    r(UNS, kind=2)
    r(UNS, kind=-1)
    r(INV, ws_bytes=0)
    r(INV, ws_bytes=ws_bytes(pop) - 1)
    # the order
    r(INV, e=5, params=None, ws_bytes=1 << 20)                   # the null test in front of the inputs
    r(INV, e=5, t=0, ws_bytes=1 << 20)                           # the sizes in front of the inputs
    r(INV, e=5, ws=P + 4, ws_bytes=1 << 20)                      # the alignment in front of the inputs
    r(INV, kind=7, losses=None)
    r(INV, kind=7, ws=P + 4)
    r(UNS, e=5, kind=7, ws_bytes=1 << 20)
    r(UNS, e=5, ws_bytes=0)                                      # unsupported E in front of a short workspace
    r(UNS, kind=7, ws_bytes=0)                                   # ... and the loss
    r(INV, kind=7, ws_bytes=-1)                                  # a NEGATIVE size belongs to the sizes, in front
    if gae and not pop:                                          # gamma_lambda in front of anything else
        for bad in (NAN, INF, -INF, -0.5):
            r(INV, gamma_lambda=bad)
            r(INV, gamma_lambda=bad, e=5, ws_bytes=1 << 20)      # (UNS without it)
            r(INV, gamma_lambda=bad, kind=7)
            r(INV, gamma_lambda=bad, params=None)
        r(UNS, gamma_lambda=0.0, kind=7)                         # zero is a gamma_lambda
    if pop:
        big = 65536                                              # more members than the grid's y has
        r(INV, hyper=None)
        r(INV, members=0)
        r(INV, members=-2)
        r(INV, members=3)                                        # 8 % 3
        r(INV, members=16)                                       # more members than envs: 8 % 16
        # the member rules in front of the stand-alone ones
        r(INV, members=3, params=None)
        r(INV, members=3, e=5, ws_bytes=1 << 20)                 # (UNS without the first)
        r(INV, members=3, kind=7)
        r(INV, hyper=None, e=5, ws_bytes=1 << 20)
        r(INV, hyper=None, kind=7)
        r(INV, members=0, kind=7)
        r(INV, n=0, kind=7)
        # the stand-alone rules are asked of N / members: enough for ONE member passes them and fails the whole
        r(INV, ws_bytes=ws_bytes(False, N // MEMBERS))
        r(INV, ws_bytes=ws_bytes(False, N // MEMBERS) - 1)
        r(INV, ws_bytes=ws_bytes(True) - 1)
        # members > 65535: behind the stand-alone rules, in front of the whole workspace
        r(UNS, members=big, n=2 * big)
        r(UNS, members=big, n=2 * big, ws_bytes=ws_bytes(False, 2))        # short for the population, enough for one
        r(INV, members=big, n=2 * big, ws_bytes=ws_bytes(False, 2) - 1)    # short for one member
        r(INV, members=big, n=2 * big, params=None)
        r(INV, members=big, n=2 * big, ws=P + 4)
        r(INV, members=big, n=2 * big + 1)
        r(INV, members=big, n=2 * big, hyper=None)
        r(UNS, members=big, n=2 * big, kind=7)
        r(UNS, members=65535 + 2, n=65537)
        r(INV, members=65535, n=65535, ws_bytes=ws_bytes(True, 65535, members=65535) - 1)   # the largest is supported


def apply_rows(fn, pop, **form):
    """check_apply's rules (every one of them INVALID_ARG)"""
    def r(want, **kw):
        row(want, fn, pop=pop, **dict(form, **kw))
    for ptr in ('params', 'grad', 'exp_avg', 'exp_avg_sq'):
        r(INV, **{ptr: None})
    r(INV, step=0)
    r(INV, step=-3)
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=NAN), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=-0.1),
                dict(beta2=NAN), dict(eps=-1e-8), dict(eps=NAN)):
        r(INV, **bad)
    if not pop:
        r(INV, lr=-1e-3)
        r(INV, lr=NAN)
    else:
        r(INV, hyper=None)
        r(INV, members=0)
        r(INV, members=-1)
    if fn is apply:
        r(INV, num_params=0)
        r(INV, num_params=-4)
        if pop:                                                  # members > 65535 behind everything else
            r(UNS, members=65536)
            r(UNS, members=1 << 40)
            for bad in (dict(params=None), dict(step=0), dict(beta1=1.0), dict(eps=-1.0), dict(num_params=0)):
                r(INV, members=65536, **bad)
            r(INV, members=65536, hyper=None)


for gae, pop in FORMS:
    grad_rows(grad, gae, pop)
    grad_rows(update, gae, pop, step=0)                          # every grad rule in front of a broken apply rule
    apply_rows(update, pop, gae=gae)
    # _update: all grad checks, then all apply checks
    for bad in (dict(step=0), dict(exp_avg=None), dict(exp_avg_sq=None), dict(beta1=1.0), dict(beta2=NAN), dict(eps=-1.0)):
        row(UNS, update, gae=gae, pop=pop, kind=7, **bad)
        row(UNS, update, gae=gae, pop=pop, e=5, ws_bytes=1 << 20, **bad)
        row(INV, update, gae=gae, pop=pop, ws_bytes=0, **bad)
    if not pop:
        row(UNS, update, gae=gae, pop=pop, kind=7, lr=-1.0)
    else:
        for bad in (dict(step=0), dict(exp_avg=None), dict(beta1=1.0)):
            row(UNS, update, gae=gae, pop=pop, members=65536, n=2 * 65536, **bad)   # the grad half's answer
    if gae and not pop:
        row(INV, update, gae=gae, pop=pop, gamma_lambda=NAN, step=0, kind=7)
for pop in (False, True):
    apply_rows(apply, pop)

# ---- the entry points that never launch
row(ws_bytes(False), workspace)
for bad in (dict(n=0), dict(n=-1), dict(t=0), dict(t=-5), dict(e=5), dict(e=0), dict(e=-27), dict(e=675), dict(n=0, e=5)):
    row(0, workspace, **bad)
    row(0, pop_workspace, **bad)
row(MEMBERS * ws_bytes(False, N // MEMBERS), pop_workspace)
row(65536 * ws_bytes(False, 2), pop_workspace, n=2 * 65536, members=65536)   # the query has no limit on the members
for bad in (dict(members=0), dict(members=-2), dict(members=3), dict(members=16)):
    row(0, pop_workspace, **bad)
row(OK, pop_hyper)
row(OK, pop_hyper, gamma_lambda=(0.9405, 0.0))
row(OK, pop_hyper, lr=(0.0, 1e-3))
row(OK, pop_hyper, gamma=(NAN, -1.0), entropy_coef=(INF, -1.0))              # only lr and gamma_lambda are judged
for bad in (dict(lr=None), dict(gamma=None), dict(entropy_coef=None), dict(table=False), dict(members=0), dict(members=-1),
            dict(lr=(1e-3, -1e-3)), dict(lr=(NAN, 1e-3)), dict(gamma_lambda=(0.9, NAN)), dict(gamma_lambda=(INF, 0.9)),
            dict(gamma_lambda=(0.9, -0.5)), dict(lr=(1e-3, -1.0), table=False)):
    row(INV, pop_hyper, **bad)
row(OK, hyper_parameter)
row(INV, hyper_parameter, value=False)


@pytest.mark.parametrize('want, fn, kw', ROWS)
def test_entry_point_returns_before_a_launch(want, fn, kw):
    n0 = _lib.lib().wurm_launch_count()
    assert fn(**kw) == want
    assert _lib.lib().wurm_launch_count() == n0, 'the row reached a launch'
