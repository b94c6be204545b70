"""GPU parity for the trio form of `rollout_s9_kernel` (RW = 2, wurm_amd/csrc/single_kernels.hpp): where the helper wave
would render the crops, batches of at most WURM_S9_TRIO_MAX_ENVS envs and launches of at least WURM_S9_TRIO_MIN_STEPS steps
run a workgroup of three waves per env.  Wave 0 steps, wave 1 does the per-chunk work and renders the first steps of each
chunk, wave 2 renders the others, on wave 1's barrier schedule and from the same record buffer.

Every case forces the form through the knobs (every launch length, every batch size), asserts through
wurm_single_last_waves_per_env() == 3 and wurm_single_last_crop_wave() == 1 that it ran in one launch, and compares bit for
bit with the CPU oracle, with the pair form whose helper renders alone and with the one-wave form: observations, rewards,
dones, both collision flags, the sanitised tape and the final state.

The shapes are those of tests/test_s9_crop_helper.py, whose tapes (and their checks on the oracle's own trajectory, made
before anything is compared) are used as they are: what can go wrong is the same — chunk edges, buffer parities, tails — plus
the split of a chunk, and of the lone last chunk, over two waves."""
import numpy as np
import pytest

from tests.backends import OracleBackend
from tests.test_s9_crop_helper import (OUTPUTS, S, _events_after_the_first_chunk, _fresh, _hunting_tape,
                                       _irregular_batch, _placed_tape, _same, _tape)

pytestmark = pytest.mark.gpu

KNOBS = {
    'trio': {'WURM_S9_PAIR_MAX_ENVS': 1 << 20, 'WURM_S9_CROP_HELPER_MIN_STEPS': 1, 'WURM_S9_TRIO_MAX_ENVS': 1 << 20, 'WURM_S9_TRIO_MIN_STEPS': 1},
    'helper': {'WURM_S9_PAIR_MAX_ENVS': 1 << 20, 'WURM_S9_CROP_HELPER_MIN_STEPS': 1, 'WURM_S9_TRIO_MAX_ENVS': 1 << 20, 'WURM_S9_TRIO_MIN_STEPS': -1},
    'one': {'WURM_S9_PAIR_MAX_ENVS': 0, 'WURM_S9_CROP_HELPER_MIN_STEPS': -1, 'WURM_S9_TRIO_MAX_ENVS': 1 << 20, 'WURM_S9_TRIO_MIN_STEPS': -1},
}
FORM = {'trio': (3, 1), 'helper': (2, 1), 'one': (1, 0)}   # (waves per env, the wave that renders)


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _form():
    from wurm_amd import _lib
    return _lib.lib().wurm_single_last_waves_per_env(), _lib.lib().wurm_single_last_crop_wave()


def _launch(backend, envs, actions, mode, form, **inject):
    """one rollout launch of `backend` in `form` (None: the oracle) on copies of envs / actions"""
    from wurm_amd import _lib
    e, a = envs.copy(), actions.copy()
    if form is None:
        return backend.single_rollout(e, a, mode, **inject), e, a
    with _lib.knobs(**KNOBS[form]):
        n0 = _lib.lib().wurm_launch_count()
        out = backend.single_rollout(e, a, mode, **inject)
        assert _lib.lib().wurm_launch_count() - n0 == 1
        assert _form() == FORM[form], f'{_form()} ran, {form} was meant to'
    return out, e, a


def _four_ways(hip, envs, actions, mode, seed=0, call=1, **inject):
    """oracle == trio form == helper-crop pair form == one-wave form on every output, the tape and the final state"""
    results = []
    for form in (None, 'trio', 'helper', 'one'):
        b = OracleBackend(seed=seed) if form is None else hip(seed=seed)
        b.call = call
        results.append(_launch(b, envs, actions, mode, form, **inject))
    (ro, eo, ao) = results[0]
    for name, (r, e, a) in zip(('trio form', 'helper-crop form', 'one-wave form'), results[1:]):
        for k in OUTPUTS:
            _same(ro[k], r[k], f'{name}: {k}')
        _same(ao, a, f'{name}: sanitised actions')
        _same(eo, e, f'{name}: final state')
    return ro, eo


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 127, 128, 129, 193, 257])
def test_chunk_edges_buffer_parities_and_tails(hip, T):
    """every chunk edge, both record-buffer parities, odd and even tails, the last chunk split over two waves (T = 1: the
    helper's share of it is empty; T = 2, 65, 129, 193, 257: so is all but wave 2's single pass)"""
    N = 3
    envs = _fresh(OracleBackend(seed=T), N)
    out, _ = _four_ways(hip, envs, _tape(T, T, N), 'partial_2', seed=T, call=7 + T)
    assert out['obs'].shape[:2] == (T, N)


@pytest.mark.parametrize('mode', ['partial_1', 'partial_2', 'partial_3'])
def test_observation_modes(hip, mode):
    """partial_3 has 49 window cells, more than half a wave: one step per pass"""
    N, T = 9, 129
    envs = _fresh(OracleBackend(seed=5), N)
    out, _ = _four_ways(hip, envs, _tape(31, T, N), mode, seed=5)
    _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'done'))


@pytest.mark.parametrize('N,seed', [(1, 1), (70, 70)])
def test_batch_sizes(hip, N, seed):
    """one workgroup alone; 70, which is no multiple of the XCD count, on the piloted tape of tests/test_s9_step_loop.py"""
    T = 129
    envs = _fresh(OracleBackend(seed=seed), N)
    tape = _hunting_tape(seed, envs, T) if N >= 6 else _tape(seed, T, N)
    out, _ = _four_ways(hip, envs, tape, 'partial_2', seed=seed)
    if N >= 6:
        _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'self_collision', 'done'))


def test_piloted_events_on_chunk_edges(hip):
    """eating steps and collisions with their resets on the last step of a chunk (63, 127) and on the first of the next (64,
    128), an eating step right after a reset — on the oracle's own trajectory, checked before anything is compared"""
    N, T, seed = 36, 130, 3
    envs = _fresh(OracleBackend(seed=seed), N)
    actions = _placed_tape(seed, envs, T)
    out, _ = _four_ways(hip, envs, actions, 'partial_2', seed=seed)
    first, last = np.arange(T) % 64 == 0, np.arange(T) % 64 == 63
    first[0] = False
    edge, selfc, ate, done = (np.asarray(out[k]).astype(bool) for k in ('edge_collision', 'self_collision', 'reward', 'done'))
    missing = [f'{kind} on the {name} step of a chunk' for name, when in (('first', first), ('last', last))
               for kind, ev in (('edge collision', edge), ('self collision', selfc), ('eating step', ate)) if not ev[when].any()]
    if not (ate[1:] & done[:-1]).any():
        missing.append('eating step right after a reset')
    assert not missing, f"the oracle's trajectory lacks: {missing}"


def test_edge_collision_on_every_step_with_injected_resets(hip):
    """injected resets put every new snake beside a side of the ring, heading for it: an edge collision and a reset on every
    step, the step right after a reset included, on each of the four sides and beside the corners, where the head code wraps
    (the INJ instantiation of the trio form)"""
    T, seed = 130, 2
    starts = [(2, 1, 0, 2), (2, 4, 0, 2), (2, 7, 0, 2), (6, 1, 2, 0), (6, 4, 2, 0), (6, 7, 2, 0),
              (1, 2, 3, 1), (4, 2, 3, 1), (7, 2, 3, 1), (1, 6, 1, 3), (4, 6, 1, 3), (7, 6, 1, 3)]
    N = len(starts)
    inject_reset = np.zeros((T, N, 4), np.int32)
    actions = np.zeros((T, N), np.int64)
    for i, (sy, sx, d, a) in enumerate(starts):
        inject_reset[:, i] = (sy, sx, d, 4 * S + 4)   # the food on the centre cell, which no such snake covers
        actions[:, i] = a
    inject_food = np.full((T, N), -1, np.int32)
    envs = np.zeros((N, 3, S, S), np.float32)
    OracleBackend(seed=seed).single_reset(envs, np.ones(N, np.uint8), 'none', inject_reset=inject_reset[0])
    out, _ = _four_ways(hip, envs, actions, 'partial_2', seed=seed, inject_food=inject_food, inject_reset=inject_reset)
    assert np.asarray(out['edge_collision']).astype(bool).all(), 'the oracle: not every step runs into the ring'
    from wurm_amd import _lib
    assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected'


def test_envs_outside_the_lean_domain_beside_running_trios(hip):
    """the steppers of envs 0, 4 and 8 take the generic path and both other waves of their workgroups leave after the first
    barrier; the six others run as trios in the same launch"""
    envs, actions = _irregular_batch()
    _four_ways(hip, envs, actions, 'partial_2', seed=21, call=50)


def test_chained_launches(hip):
    """two launches of 129 and 65 steps carry state and call counter on and equal the oracle's single launch of 194"""
    from wurm_amd import _lib
    N, seed, call = 9, 23, (1 << 40) + 3
    actions = _tape(4, 194, N)
    o = OracleBackend(seed=seed)
    o.call = call
    envs = _fresh(OracleBackend(seed=seed), N)
    eo, ao = envs.copy(), actions.copy()
    whole = o.single_rollout(eo, ao, 'partial_2')
    h = hip(seed=seed)
    h.call = call
    e, a = envs.copy(), actions.copy()
    with _lib.knobs(**KNOBS['trio']):
        first = h.single_rollout(e, a[:129], 'partial_2')
        assert _form() == FORM['trio']
        second = h.single_rollout(e, a[129:], 'partial_2')
        assert _form() == FORM['trio']
    for k in OUTPUTS:
        _same(whole[k], np.concatenate([first[k], second[k]]), k)
    _same(ao, a, 'sanitised actions')
    _same(eo, e, 'final state')


def test_the_bench_launch(hip):
    """512 envs x 1 024 steps, partial_2, RNG mode: the launch bench.py times, against the oracle"""
    from wurm_amd import _lib
    N, T, seed = 512, 1024, 0
    envs = _fresh(OracleBackend(seed=seed), N)
    actions = _tape(12, T, N)
    o, h = OracleBackend(seed=seed), hip(seed=seed)
    o.call = h.call = 1
    eo, ao, eh, ah = envs.copy(), actions.copy(), envs.copy(), actions.copy()
    ro = o.single_rollout(eo, ao, 'partial_2')
    with _lib.knobs(**KNOBS['trio']):
        n0 = _lib.lib().wurm_launch_count()
        rh = h.single_rollout(eh, ah, 'partial_2')
        assert _lib.lib().wurm_launch_count() - n0 == 1 and _form() == FORM['trio']
    for k in OUTPUTS:
        _same(ro[k], rh[k], k)
    _same(ao, ah, 'sanitised actions')
    _same(eo, eh, 'final state')


def test_the_knobs(hip):
    """batch size above the first knob or launch length below the second: the pair form whose helper renders alone; the
    second knob at -1: never; no observation: nothing to render"""
    from wurm_amd import _lib
    h = hip(seed=1)
    base = {'WURM_S9_PAIR_MAX_ENVS': 1 << 20, 'WURM_S9_CROP_HELPER_MIN_STEPS': 1}
    for trio_max, trio_min, N, T, mode, form in ((3, 65, 3, 65, 'partial_2', (3, 1)), (3, 65, 4, 65, 'partial_2', (2, 1)),
                                                  (3, 65, 3, 64, 'partial_2', (2, 1)), (3, -1, 3, 65, 'partial_2', (2, 1)),
                                                  (3, 65, 3, 65, 'none', (2, 0))):
        with _lib.knobs(WURM_S9_TRIO_MAX_ENVS=trio_max, WURM_S9_TRIO_MIN_STEPS=trio_min, **base):
            h.single_rollout(_fresh(h, N), _tape(1, T, N), mode)
            assert _form() == form, (trio_max, trio_min, N, T, mode)
    assert _lib.get_option('WURM_S9_TRIO_MIN_STEPS') == -1 or _lib.get_option('WURM_S9_TRIO_MIN_STEPS') >= 512
