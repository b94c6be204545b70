"""The return codes of the wurm_single_* / wurm_grid_* entry points for calls that must not reach a launch, and the ORDER of
their checks (no GPU).  A row returns from the validation — a failing argument, num_steps == 0, the _resident forms at
num_envs == 0, a no-op flush — or, the OK rows of step / reset / observe / the plain rollout / step_reset / step_slot at
num_envs == 0, passes the validation and returns from `launch`'s own early-out in front of the first HIP call; the launch
counter is asserted unchanged for every row.

The expected codes are the ones the library returned BEFORE the host layer of wurm_amd/csrc/single_snake.hip was given one
copy of each entry path (docs/HISTORY.md: this table was run against a build of that revision, all rows equal); rows that
break two rules at once pin which check comes first.  Pointers that a row needs non-null are the address P, which is
never dereferenced."""
import ctypes

import pytest

from wurm_amd import _lib

OK, INV, UNS, DT = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_DTYPE
NONE, DEFAULT, RAW, ONE, POS, PART = (_lib.OBS_NONE, _lib.OBS_DEFAULT, _lib.OBS_RAW, _lib.OBS_ONE_CHANNEL, _lib.OBS_POSITIONS,
                                      _lib.OBS_PARTIAL)
P = 0x10000
FAMILIES = ('single', 'grid')


def _args(fam, kw):
    """defaults that pass every check (so a row fails exactly where it says), then the row's own"""
    a = dict(envs=P, actions=P, dtype=_lib.ACT_I64, reward=P, done=P, selfc=P, edgec=P, obs=None, mode=NONE, n=0, N=4,
             S=9, T=3, sy=4, sx=4)
    a.update(kw)
    return a


def _flags(fam, a):
    return (a['done'], a['selfc'], a['edgec']) if fam == 'single' else (a['done'], a['edgec'])


def _start(fam, a):
    return () if fam == 'single' else (a['sy'], a['sx'])


def step(fam, **kw):
    a = _args(fam, kw)
    fn = getattr(_lib.lib(), 'wurm_%s_step' % fam)
    return fn(a['envs'], a['actions'], a['dtype'], a['reward'], *_flags(fam, a), a['obs'], a['mode'], a['n'], a['N'], a['S'],
              0, 0, 0, None, None)


def reset(fam, **kw):
    a = _args(fam, kw)
    fn = getattr(_lib.lib(), 'wurm_%s_reset' % fam)
    return fn(a['envs'], a['done'], a['obs'], a['mode'], a['n'], a['N'], a['S'], *_start(fam, a), 0, 0, 0, None, None)


def observe(fam, **kw):
    a = _args(fam, dict(dict(mode=DEFAULT, obs=P), **kw))
    return getattr(_lib.lib(), 'wurm_%s_observe' % fam)(a['envs'], a['obs'], a['mode'], a['n'], a['N'], a['S'], None)


def rollout(fam, form='plain', **kw):
    """form: 'plain'; 'resident' (mirror and *resident_valid given); 'no_mirror' / 'no_valid' (the _resident entry point
    without one of them: it is the plain rollout)"""
    a = _args(fam, kw)
    head = (a['envs'], a['actions'], a['dtype'], a['reward'], *_flags(fam, a), a['obs'], a['mode'], a['n'], a['N'], a['S'],
            a['T'], *_start(fam, a), 0, 0, 0)
    if form == 'plain':
        return getattr(_lib.lib(), 'wurm_%s_rollout' % fam)(*head, None, None, None)
    valid = ctypes.c_int(1)
    rc = getattr(_lib.lib(), 'wurm_%s_rollout_resident' % fam)(
        *head, None if form == 'no_mirror' else P, None if form == 'no_valid' else ctypes.addressof(valid), 1, None)
    assert valid.value == 1, 'a call that launched nothing changed *resident_valid'
    return rc


ROLLOUT_FORMS = ('plain', 'resident', 'no_mirror', 'no_valid')


def block(fam, kw):
    a = _args(fam, kw)
    c = _lib.SingleCall()
    c.envs, c.actions, c.actions_dtype, c.reward, c.done = a['envs'], a['actions'], a['dtype'], a['reward'], a['done']
    c.self_collision, c.edge_collision, c.obs, c.obs_mode, c.obs_n = a['selfc'], a['edgec'], a['obs'], a['mode'], a['n']
    c.num_envs, c.size, c.start_y, c.start_x = a['N'], a['S'], a['sy'], a['sx']
    for k in ('post_reset', 'pre_done', 'obs_after', 'done_copy', 'resident', 'resident_valid', 'resident_lazy'):
        if k in a:
            setattr(c, k, a[k])
    return c


def step_reset(fam, **kw):
    fn = getattr(_lib.lib(), 'wurm_%s_step_reset' % fam)
    if kw.get('null_block'):
        return fn(None, None)
    c = block(fam, kw)
    return fn(ctypes.addressof(c), None)


def step_slot(fam, slot=0, slabs=True, apply_pending=0, act_dtype=_lib.ACT_I64, valid_after=None, **kw):
    """the block's output pointers come from the slabs: `reward`, `done` (the three flag rows) and `obs` of a row go there"""
    fn = getattr(_lib.lib(), 'wurm_%s_step_slot' % fam)
    a = _args(fam, kw)
    s = _lib.SingleSlabs()
    s.reward, s.flags, s.obs, s.steps = a['reward'], a['done'], a['obs'], 4
    if kw.get('null_block'):
        return fn(None, ctypes.addressof(s), slot, P, act_dtype, 0, apply_pending, 0, 0, None)
    c = block(fam, kw)
    rc = fn(ctypes.addressof(c), ctypes.addressof(s) if slabs else None, slot, P, act_dtype, 0, apply_pending, 0, 0, None)
    if valid_after is not None:
        assert c.resident_valid == valid_after
    return rc


def flush(fam, **kw):
    fn = getattr(_lib.lib(), 'wurm_%s_resident_flush' % fam)
    if kw.get('null_block'):
        return fn(None, None)
    c = block(fam, kw)
    return fn(ctypes.addressof(c), None)


def policy(**kw):
    a = dict(envs=P, obs0=P, params=P, actions=P, probs=P, values=P, reward=P, done=P, selfc=P, edgec=P, obs=P, status=P,
             n=2, N=4, S=9, T=3)
    a.update(kw)
    return _lib.lib().wurm_single_policy_rollout(a['envs'], a['obs0'], a['params'], a['actions'], a['probs'], a['values'],
                                                 a['reward'], a['done'], a['selfc'], a['edgec'], a['obs'], a['status'], a['n'],
                                                 a['N'], a['S'], a['T'], 0, 0, 0, None)


def check(envs=P, out=P, N=4, S=9):
    return _lib.lib().wurm_single_check(envs, out, N, S, None)


def orientations(envs=P, out=P, N=4, S=9):
    return _lib.lib().wurm_orientations(envs, out, N, S, None)


ROWS = []


def row(want, fn, *args, **kw):
    name = '%s(%s)' % (fn.__name__, ', '.join([str(x) for x in args] + ['%s=%s' % (k, v) for k, v in kw.items()]))
    ROWS.append(pytest.param(want, fn, args, kw, id=name))


def common_rows(fn, fam, **base):
    """the checks every validating entry point starts with (check_common), in their order; `base`: what makes the call
    fail behind them in any case, so that a row that passes them by mistake still launches nothing"""
    def r(want, **kw):
        row(want, fn, fam, **dict(base, **kw))
    r(INV, N=-1)
    r(INV, S=2)
    r(UNS, S=65)
    r(UNS, S=65, N=-1)                                           # (one test: the size decides its code)
    r(INV, envs=None)
    r(INV, mode=7 if fam == 'single' else ONE, obs=P)            # not an observation of the family
    r(INV, mode=PART, n=2 if fam == 'grid' else -1, obs=P)
    r(INV, mode=DEFAULT, obs=None)
    r(INV, S=2, envs=None, mode=7)


def dtype_rows(fn, fam, key='dtype', **base):
    row(DT, fn, fam, **dict(base, **{key: 7}))
    row(UNS, fn, fam, S=65, **dict(base, **{key: 7}))           # S > 64 in front of the dtype
    row(INV, fn, fam, envs=None, **dict(base, **{key: 7}))      # null envs in front of the dtype
    row(DT, fn, fam, mode=7, obs=P, **dict(base, **{key: 7}))   # the dtype in front of the mode
    row(DT, fn, fam, mode=DEFAULT, obs=None, **dict(base, **{key: 7}))


for fam in FAMILIES:
    small = 8 if fam == 'single' else 4                         # the largest size without a reset
    outs = ('actions', 'reward', 'done', 'edgec') + (('selfc',) if fam == 'single' else ())
    starts = () if fam == 'single' else (dict(sy=-1), dict(sx=-1), dict(sy=9), dict(sx=9))

    # ---- step
    common_rows(step, fam, reward=None)
    dtype_rows(step, fam, reward=None)
    for o in outs:
        row(INV, step, fam, **{o: None})
    row(OK, step, fam, N=0, actions=None, reward=None, done=None, selfc=None, edgec=None, envs=None)
    row(OK, step, fam, N=0, S=small)                            # (no reset in a step: no size limit beyond 3)

    # ---- reset
    common_rows(reset, fam, done=None)
    row(UNS, reset, fam, S=small)
    row(UNS, reset, fam, S=small, done=None)                    # the size limit in front of the null test
    row(INV, reset, fam, S=small, envs=None)                    # check_common in front of the size limit
    row(INV, reset, fam, done=None)
    row(OK, reset, fam, N=0, done=None, envs=None)
    for s in starts:
        row(UNS, reset, fam, **s)
        row(UNS, reset, fam, done=None, **s)                    # the start location in front of the null test
        row(UNS, reset, fam, N=0, **s)
        row(INV, reset, fam, envs=None, **s)

    # ---- observe
    common_rows(observe, fam)
    row(INV, observe, fam, mode=NONE)
    row(INV, observe, fam, mode=NONE, S=65)                     # "no observation" in front of check_common
    row(OK, observe, fam, N=0, S=small)
    row(OK, observe, fam, N=0, envs=None, obs=None)

    # ---- rollout, rollout_resident
    for form in ROLLOUT_FORMS:
        common_rows(rollout, fam, form=form, T=-1)
        dtype_rows(rollout, fam, form=form, T=-1)
        row(INV, rollout, fam, form=form, T=-1)
        row(UNS, rollout, fam, form=form, S=small)
        row(INV, rollout, fam, form=form, T=-1, S=small)        # num_steps < 0 in front of the size limit
        row(UNS, rollout, fam, form=form, T=-1, S=65)           # check_common in front of num_steps < 0
        row(UNS, rollout, fam, form=form, T=0, S=small)         # the size limit in front of "nothing to do"
        row(UNS, rollout, fam, form=form, S=small, reward=None)  # ... and of the null test
        for s in starts:
            row(UNS, rollout, fam, form=form, **s)
            row(UNS, rollout, fam, form=form, T=0, N=0, **s)
            row(UNS, rollout, fam, form=form, actions=None, reward=None, **s)   # the start location in front of the null test
            row(INV, rollout, fam, form=form, T=-1, **s)        # num_steps < 0 in front of the start location
        for o in outs:
            row(INV, rollout, fam, form=form, **{o: None})
            row(OK, rollout, fam, form=form, T=0, **{o: None})  # nothing is written in no steps
            row(OK, rollout, fam, form=form, N=0, **{o: None})
        row(OK, rollout, fam, form=form, T=0)
        row(OK, rollout, fam, form=form, N=0)
        row(OK, rollout, fam, form=form, N=0, T=0, envs=None)
        row(DT, rollout, fam, form=form, T=0, dtype=7)          # nothing to do is still validated

    # ---- step_reset and step_slot: a wurm_single_call block
    for fn in (step_reset, step_slot):
        row(INV, fn, fam, null_block=True)
        common_rows(fn, fam, reward=None)
        dtype_rows(fn, fam, key='dtype' if fn is step_reset else 'act_dtype', reward=None)
        for o in outs if fn is step_reset else ('reward', 'done'):   # (step_slot fills the block from its arguments and the slabs)
            row(INV, fn, fam, **{o: None})
        for resets in (dict(post_reset=1), dict(pre_done=P), dict(obs_after=P, obs=P, mode=DEFAULT)):
            if fn is step_slot and 'post_reset' not in resets:
                continue                                         # (step_slot sets pre_done / obs_after itself)
            row(UNS, fn, fam, S=small, **resets)
            row(UNS, fn, fam, S=small, N=0, **resets)
            row(INV, fn, fam, S=small, reward=None, **resets)    # the null test in front of the limits of a reset
            for s in starts:
                row(UNS, fn, fam, **dict(resets, **s))
                row(INV, fn, fam, reward=None, **dict(resets, **s))
        row(OK, fn, fam, N=0, S=small)                           # no reset asked for: no limit
        for s in starts:
            row(OK, fn, fam, N=0, **s)
        row(OK, fn, fam, N=0, post_reset=1)
        row(OK, fn, fam, N=0, resident=P, resident_valid=1, resident_lazy=1)   # a mirror of no envs is not looked at
        if fam == 'grid':
            row(UNS, fn, fam, selfc=None, post_reset=1, S=4)     # SimpleGridworld has no self collision to write
    row(INV, step_slot, fam, slabs=False)
    row(INV, step_slot, fam, slot=-1)
    row(INV, step_slot, fam, slot=4)
    row(INV, step_slot, fam, slot=4, act_dtype=7)                # the slot in front of everything in the block
    row(INV, step_slot, fam, apply_pending=1)                    # ... without done_copy
    row(INV, step_slot, fam, apply_pending=1, act_dtype=7)       # ... in front of the block's checks
    row(DT, step_slot, fam, apply_pending=1, done_copy=P, act_dtype=7)
    row(UNS, step_slot, fam, apply_pending=1, done_copy=P, S=small)   # a postponed reset is a reset
    row(OK, step_slot, fam, apply_pending=1, done_copy=P, N=0)
    # wurm_*_step_slot keeps resident_valid: untouched where nothing ran, stale (0) after a call that took no mirror
    row(INV, step_slot, fam, reward=None, resident=P, resident_valid=1, valid_after=1)
    row(OK, step_slot, fam, N=0, resident=P, resident_valid=1, valid_after=0)

    # ---- the flush of a lazy mirror
    mirror = dict(resident=P, resident_valid=1, resident_lazy=1)
    row(INV, flush, fam, null_block=True)
    row(OK, flush, fam)
    row(OK, flush, fam, envs=None)
    row(INV, flush, fam, envs=None, **mirror)
    row(OK, flush, fam, envs=None, **dict(mirror, resident=None))
    row(OK, flush, fam, envs=None, **dict(mirror, resident_lazy=0))
    row(OK, flush, fam, envs=None, **dict(mirror, resident_valid=0))
    row(OK, flush, fam, envs=None, N=0, **mirror)
    row(OK, flush, fam, envs=None, N=-1, **mirror)
    # resident_valid == 2 is SimpleGridworld's "refused" (nothing to write); SingleSnake knows valid or not
    row(OK if fam == 'grid' else INV, flush, fam, envs=None, **dict(mirror, resident_valid=2))
for S in (3, 8, 65):                                             # no SingleSnake mirror exists at these sizes
    row(INV, flush, 'single', S=S, resident=P, resident_valid=1, resident_lazy=1)

# ---- the fused actor
for bad, want in ((dict(N=-1), INV), (dict(T=-1), INV), (dict(S=2), INV), (dict(S=8), UNS), (dict(S=65), UNS), (dict(n=-1), UNS),
                  (dict(n=7), UNS), (dict(N=0), OK), (dict(T=0), OK)):
    row(want, policy, **bad)
    row(want, policy, envs=None, status=None, **bad)             # each of them in front of the null test
for ptr in ('envs', 'obs0', 'params', 'actions', 'probs', 'values', 'reward', 'done', 'selfc', 'edgec', 'obs', 'status'):
    row(INV, policy, **{ptr: None})
row(INV, policy, N=-1, S=8)
row(INV, policy, T=-1, n=7)
row(UNS, policy, N=0, S=8)
row(UNS, policy, T=0, n=7)

# ---- the consistency check and the orientations
for fn in (check, orientations):
    row(INV, fn, N=-1)
    row(INV, fn, S=2)
    row(INV, fn, N=-1, S=65)
    row(OK, fn, N=0)
    row(OK, fn, N=0, S=65, envs=None, out=None)                  # no envs: nothing to do, whatever the size
    row(INV, fn, envs=None)
    row(INV, fn, out=None)
    row(INV, fn, envs=None, S=65)                                # the null test in front of the size limit
    row(UNS, fn, S=65)


@pytest.mark.parametrize('want, fn, args, kw', ROWS)
def test_entry_point_returns_before_a_launch(want, fn, args, kw):
    n0 = _lib.lib().wurm_launch_count()
    assert fn(*args, **kw) == want
    assert _lib.lib().wurm_launch_count() == n0, 'the row reached a launch'
