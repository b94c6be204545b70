"""The choice of kernel of the MultiSnake entry points (wurm_amd/csrc/multi_snake.hip: multi_plan), one case per row:
which kernel instantiation serves a call is a function of (kind, K, S, N, T, observation, tapes, options) alone, read off
ONE table, and `wurm_multi_last_route()` names the row and how the kernel was driven.  Results never depend on the row:
every case is ONE launch through HipBackend, compared bit for bit (floats as uint32) with the oracle.
The expected names were read off multi_launch as it was before the table existed and confirmed by a kernel trace of that
build (tools/multi_routes.py, profiles/r10_multi_routes.txt), not by running the table.
The reference has one code path for every shape (/root/reference wurm/envs/multi_snake.py:462-731)."""
import numpy as np
import pytest

from oracle import oracle as _o
from tests import replay
from tests.backends import OracleBackend
from tests.test_hip_multi_vs_oracle import CFGS, _same

pytestmark = pytest.mark.gpu

GROUP, TWO = dict(WURM_MULTI_GROUP_MIN_ENVS=0), dict(WURM_MULTI_GROUP_MIN_ENVS=1 << 40)
GENERIC = dict(WURM_MULTI_SHAPE_KERNELS=0)


def _shape(code):
    return dict(GROUP, WURM_MULTI_GROUP_SHAPE=code)


# (kind, K, S, N, T, observation, tapes, options, expected wurm_multi_last_route())
CASES = [
    # grouped rollout: G consecutive envs per workgroup (N = 9: a last workgroup that is not full)
    ('rollout', 2, 12, 9, 3, 'full', False, GROUP, 'rollout_group_8215_rng'),
    ('rollout', 2, 12, 9, 3, 'full', True, GROUP, 'rollout_group_8215/tapes'),
    ('rollout', 4, 25, 5, 3, 'full', False, GROUP, 'rollout_group_4414_rng_k4_s25'),
    ('rollout', 4, 25, 5, 3, 'full', False, dict(GROUP, **GENERIC), 'rollout_group_8215_rng'),
    ('rollout', 6, 12, 5, 3, 'full', False, GROUP, 'rollout_group_5014_rng'),
    ('rollout', 2, 12, 9, 3, 'full', False, _shape(8215), 'rollout_group_8215_rng'),
    ('rollout', 2, 12, 9, 3, 'full', False, _shape(8416), 'rollout_group_8416_rng'),
    ('rollout', 2, 12, 9, 3, 'full', False, _shape(4414), 'rollout_group_4414_rng'),
    ('rollout', 4, 25, 5, 3, 'full', False, _shape(4414), 'rollout_group_4414_rng_k4_s25'),
    ('rollout', 2, 12, 9, 3, 'full', False, _shape(8424), 'rollout_group_8424'),   # (no instantiation that only draws)
    ('rollout', 6, 12, 5, 3, 'full', False, _shape(5014), 'rollout_group_5014_rng'),
    ('rollout', 6, 12, 5, 3, 'full', False, _shape(4514), 'rollout_group_4514'),
    ('rollout', 6, 12, 5, 3, 'full', False, _shape(3014), 'rollout_group_3014'),
    ('rollout', 2, 12, 9, 3, 'full', False, _shape(1111), 'rollout_two_rng'),       # no compiled shape: the two-wave kernel
    # two-wave rollout
    ('rollout', 2, 12, 9, 3, 'full', False, TWO, 'rollout_two_rng'),
    ('rollout', 2, 12, 9, 3, 'full', True, TWO, 'rollout_two/tapes'),
    # one-wave rollout
    ('rollout', 2, 12, 5, 1, 'full', False, {}, 'rollout_rng'),
    ('rollout', 11, 25, 3, 3, 'full', False, {}, 'rollout_rng'),                    # above SNAP_MAX_SNAKES
    ('rollout', 2, 12, 5, 3, 'partial_2', False, {}, 'rollout_rng_partial'),
    ('rollout', 2, 12, 5, 3, 'none', False, {}, 'rollout_rng_none'),
    ('rollout', 4, 25, 5, 3, 'partial_5', False, {}, 'rollout_rng_partial_k4_s25_n5'),
    ('rollout', 4, 25, 5, 3, 'partial_5', False, GENERIC, 'rollout_rng_partial'),
    ('rollout', 2, 12, 5, 1, 'full', True, {}, 'rollout/tapes'),
    # per-call step
    ('step', 3, 10, 5, 1, 'full', True, {}, 'step/tapes'),
    ('step', 4, 25, 5, 1, 'partial_5', False, {}, 'step_rng_partial_k4_s25_n5'),
    ('step', 4, 25, 5, 1, 'full', False, {}, 'step_rng_full_k4_s25'),
    ('step', 2, 12, 5, 1, 'full', False, {}, 'step_rng_full_k2_s12'),
    ('step', 3, 10, 5, 1, 'full', False, {}, 'step_rng_full'),
    ('step', 3, 10, 5, 1, 'partial_1', False, {}, 'step_rng_partial'),
    ('step', 3, 10, 5, 1, 'none', False, {}, 'step_rng_none'),
    # ... at or above the group threshold: 'full' observations through class codes, per wave or by the workgroup together
    ('step', 3, 10, 9, 1, 'full', False, dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=0), 'step_rng_full'),
    ('step', 3, 10, 9, 1, 'full', False, dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=1), 'step_rng_full+emit_wave'),
    ('step', 3, 10, 9, 1, 'full', False, dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=4), 'step_rng_full+emit_group'),
    ('step', 3, 10, 9, 1, 'full', False, dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=8), 'step_rng_full+emit_group'),
    # one env per workgroup
    ('step', 10, 36, 3, 1, 'full', False, {}, 'step_wg_rng_full_k10_s36'),
    ('step', 10, 36, 3, 1, 'full', False, GENERIC, 'step_wg_rng'),
    ('step', 10, 36, 3, 1, 'full', True, {}, 'step_wg/tapes'),
    ('reset', 10, 36, 3, 1, None, False, {}, 'reset_wg'),
    ('observe', 10, 36, 3, 1, 'full', False, {}, 'observe_wg'),
    # reset, observe, check on the one-wave kernels
    ('reset', 2, 12, 5, 1, None, False, {}, 'reset'),
    ('observe', 2, 12, 5, 1, 'full', False, {}, 'observe'),
    ('check', 2, 12, 5, 1, None, False, {}, 'check'),
]
IDS = ['-'.join(str(v) for v in c[:7]) + ''.join(f'-{k[5:].lower()}={v}' for k, v in c[7].items()) for c in CASES]


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _state(o, N, K, S, cfg):
    """fresh envs from the oracle alone (a case is ONE launch of the library), and a copy for the library"""
    so = _o.multi_empty_state(N, K, S)
    so['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
    o.call = 1
    o.multi_reset(so, np.ones(N), cfg)
    return so, {k: v.copy() for k, v in so.items()}


def _rollout_tapes(K, S, N, T):
    """the first T steps and N envs of the outcomes recorded from the reference for 2 snakes on 12 x 12 (tests/golden)"""
    fx = replay.load_multi('multi_k2_s12_default')
    assert (K, S) == (2, 12) and fx['mode'] == 'full'
    st = {k: v[:N * (1 if k == 'foods' else K)].copy() for k, v in replay.multi_state(fx, 'state0_').items()}
    per_env = lambda a: a[:T, :N]                      # noqa: E731
    per_agent = lambda a: a[:T, :N * K]                # noqa: E731
    inject = dict(death_a=per_env(fx['inj_death_a']), cost=per_agent(fx['inj_cost']), death_b=per_env(fx['inj_death_b']),
                  rate=per_env(fx['inj_rate']), food_cell=per_env(fx['inj_food_cell']))
    rinj = dict(create=per_env(fx['rinj_create']), create_food=per_env(fx['rinj_create_food']),
                colours=per_agent(fx['rinj_colours']), respawn=per_env(fx['rinj_respawn']))
    return st, {k: np.ascontiguousarray(v) for k, v in inject.items()}, {k: np.ascontiguousarray(v) for k, v in rinj.items()}, fx['cfg_dict']


def run_case(hip, case):
    """one case: ONE launch of the library.  Returns (what the library computed, what the oracle computed): two lists of
    (name, array) pairs, outputs first, then the state."""
    from wurm_amd._lib import knobs
    kind, K, S, N, T, mode, tapes, options, _ = case
    cfg = CFGS['default']
    rng = np.random.RandomState(1000 * K + 10 * S + N)
    o, h = OracleBackend(seed=21, env_offset=300), hip(seed=21, env_offset=300)
    inject = rinj = None
    if kind == 'rollout' and tapes:
        so, inject, rinj, cfg = _rollout_tapes(K, S, N, T)
        sh = {k: v.copy() for k, v in so.items()}
    else:
        so, sh = _state(o, N, K, S, cfg)
    if kind == 'step' and tapes:  # (no food from a death, no boost cost, the lone food respawns two cells from the corner)
        inject = dict(death_a=np.zeros((N, S, S), np.uint8), cost=np.zeros(N * K, np.uint8), death_b=np.zeros((N, S, S), np.uint8),
                      rate=np.zeros((N, S, S), np.uint8), food_cell=np.full(N, 2 * S + 2, np.int32))
    o.call = h.call = 7
    actions = rng.randint(0, 8, size=(T, K, N)).astype(np.int64)
    done_env = (np.arange(N) % 2 == 0).astype(np.uint8)
    if kind in ('observe', 'check'):  # (a state a few steps old rather than a fresh one)
        for t in range(3):
            o.multi_step(so, rng.randint(0, 8, size=(K, N)).astype(np.int64), cfg, 'none')
        sh = {k: v.copy() for k, v in so.items()}

    def call(b, st):
        if kind == 'rollout':
            return b.multi_rollout(st, actions.copy(), cfg, mode, inject=inject, reset_inject=rinj)
        if kind == 'step':
            return b.multi_step(st, actions[0].copy(), cfg, mode, inject=inject)
        if kind == 'reset':
            return dict(status=np.array(b.multi_reset(st, done_env, cfg)))
        if kind == 'observe':
            return dict(obs=b.multi_observe(st, mode))
        return dict(mask=b.multi_check(st))

    with knobs(**options):
        rh = call(h, sh)
    ro = call(o, so)
    pairs = lambda r, st: [(k, r[k]) for k in sorted(r) if r[k] is not None] + [('state ' + k, st[k]) for k in sorted(st)]   # noqa: E731
    return pairs(rh, sh), pairs(ro, so)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_row(hip, case):
    from wurm_amd import _lib
    n0 = _lib.lib().wurm_launch_count()
    got, want = run_case(hip, case)
    assert _lib.lib().wurm_launch_count() - n0 == 1
    assert _lib.lib().wurm_multi_last_route().decode() == case[-1]
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        _same(b, a, k)


def test_an_env_too_large_for_the_lds_is_unsupported_and_launches_nothing(hip):
    """19 snakes on 64 x 64: 2 K S^2 + 3 S^2 bytes and change are more than the 160 KB of a CU"""
    from wurm_amd import _lib
    h = hip(seed=1)
    st = _o.multi_empty_state(1, 19, 64)
    n0, route = _lib.lib().wurm_launch_count(), _lib.lib().wurm_multi_last_route()
    with pytest.raises(NotImplementedError):
        h.multi_step(st, np.zeros((19, 1), np.int64), CFGS['default'], 'full')
    assert _lib.lib().wurm_launch_count() == n0
    assert _lib.lib().wurm_multi_last_route() == route
