"""GPU parity for the pair form of `rollout_s9_kernel` (wurm_amd/csrc/single_kernels.hpp): batches of at most
WURM_S9_PAIR_MAX_ENVS envs run a workgroup of two waves per env — a stepper, and a helper that prepares each 64-step chunk
(tape, move entries, Philox blocks or recorded outcomes) one chunk ahead and writes each chunk's step records one chunk
behind, both through double buffers in LDS with one barrier per chunk.

Every case is compared bit for bit with the CPU oracle AND with the one-wave form of the same library (knob at 0) on
observations, rewards, dones, both collision flags, the sanitised tape and the final state, and asserts through
wurm_single_last_waves_per_env() that the form it means to test ran.  The shapes are the smallest that reach every chunk
edge and both parities of both double buffers (2, 3 and 4 chunks), padding workgroups, the helper's exit beside running
pairs, and events (eat, edge collision, self collision, reset) in chunks after the first."""
import os
import re

import numpy as np
import pytest

from tests import replay
from tests.backends import OracleBackend
from tests.test_s9_step_loop import _pilot_tape

pytestmark = pytest.mark.gpu

S = 9
KNOB = 'WURM_S9_PAIR_MAX_ENVS'
OUTPUTS = ('obs', 'reward', 'done', 'self_collision', 'edge_collision')


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _same(a, b, what):
    if a is None and b is None:
        return
    a, b = np.asarray(a), np.asarray(b)
    x, y = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
    assert x.shape == y.shape, f'{what}: shape {x.shape} vs {y.shape}'
    bad = np.argwhere(x != y)
    assert len(bad) == 0, f'{what}: {len(bad)} mismatches, first at {bad[0].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}'


def _fresh(backend, N):
    envs = np.zeros((N, 3, S, S), np.float32)
    backend.single_reset(envs, np.ones(N, np.uint8), 'none')
    return envs


def _waves():
    from wurm_amd import _lib
    return _lib.lib().wurm_single_last_waves_per_env()


def _launch(backend, envs, actions, mode, waves, **inject):
    """one rollout launch of `backend` in the form `waves` (1 / 2 waves per env; None: the oracle) on copies of envs / actions"""
    from wurm_amd import _lib
    e, a = envs.copy(), actions.copy()
    if waves is None:
        return backend.single_rollout(e, a, mode, **inject), e, a
    with _lib.knobs(**{KNOB: 0 if waves == 1 else 1 << 20}):
        n0 = _lib.lib().wurm_launch_count()
        out = backend.single_rollout(e, a, mode, **inject)
        if actions.shape[0] > 0:  # (a tape of no steps launches nothing)
            assert _lib.lib().wurm_launch_count() - n0 == 1
            assert _waves() == waves, f'{_waves()} waves per env ran, {waves} were meant to'
        else:
            assert _lib.lib().wurm_launch_count() == n0
    return out, e, a


def _three_ways(hip, envs, actions, mode, seed=0, env_offset=0, call=1, **inject):
    """oracle == pair form == one-wave form on every output, the tape and the final state; returns the oracle's outputs"""
    results = []
    for waves in (None, 2, 1):
        b = OracleBackend(seed=seed, env_offset=env_offset) if waves is None else hip(seed=seed, env_offset=env_offset)
        b.call = call
        results.append(_launch(b, envs, actions, mode, waves, **inject))
    (ro, eo, ao) = results[0]
    for name, (r, e, a) in zip(('pair form', 'one-wave form'), results[1:]):
        for k in OUTPUTS:
            _same(ro[k], r[k], f'{name}: {k}')
        _same(ao, a, f'{name}: sanitised actions')
        _same(eo, e, f'{name}: final state')
    return ro, eo


def _tape(seed, T, N, dtype=np.int64):
    return np.random.RandomState(seed).randint(0, 4, size=(T, N)).astype(dtype)


def _events_after_the_first_chunk(out, names):
    late = {k: int(np.asarray(out[k][64:]).astype(bool).sum()) for k in names}
    assert all(late.values()), f"the oracle's trajectory lacks an event after step 64: {late}"


@pytest.mark.parametrize('T', [0, 1, 63, 64, 65, 128, 129, 193, 256])
def test_chunk_edges_and_buffer_parities(hip, T):
    N = 3
    envs = _fresh(OracleBackend(seed=T), N)
    # (T = 0 without observations: an empty observation tensor has no address, which the C ABI refuses before it looks at
    # the number of steps; a tape of no steps launches nothing in either form and leaves the state alone)
    out, eo = _three_ways(hip, envs, _tape(T, T, N), 'partial_2' if T else 'none', seed=T, call=7 + T)
    assert out['reward'].shape == (T, N)
    if T == 0:
        _same(eo, envs, 'the state after a tape of no steps')


@pytest.mark.parametrize('N', [1, 9, 70])
def test_batch_sizes_padding_and_xcd_blocks(hip, N):
    T = 129
    envs = _fresh(OracleBackend(seed=N), N)
    out, _ = _three_ways(hip, envs, _tape(N, T, N), 'partial_2', seed=N)
    if N >= 9:
        _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'done'))


@pytest.mark.parametrize('mode', ['partial_1', 'partial_2', 'partial_3', 'none'])
def test_observation_modes(hip, mode):
    N, T = 9, 129
    envs = _fresh(OracleBackend(seed=5), N)
    out, _ = _three_ways(hip, envs, _tape(31, T, N), mode, seed=5)
    _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'done'))


def test_env_offset_and_chained_launches(hip):
    """RNG mode with env ids and call counters beyond 32 bits; two launches of 129 and 65 steps carry the call counter on
    and equal the oracle's single launch of 194"""
    from wurm_amd import _lib
    N, seed, off, call = 9, 23, (1 << 33) + 5, (1 << 40) + 3
    actions = _tape(4, 194, N)
    o = OracleBackend(seed=seed, env_offset=off)
    o.call = call
    envs = _fresh(OracleBackend(seed=seed), N)
    eo, ao = envs.copy(), actions.copy()
    whole = o.single_rollout(eo, ao, 'partial_2')
    _events_after_the_first_chunk(whole, ('reward', 'edge_collision', 'done'))
    for waves in (2, 1):
        h = hip(seed=seed, env_offset=off)
        h.call = call
        e, a = envs.copy(), actions.copy()
        with _lib.knobs(**{KNOB: 0 if waves == 1 else 1 << 20}):
            first = h.single_rollout(e, a[:129], 'partial_2')
            assert _waves() == waves
            second = h.single_rollout(e, a[129:], 'partial_2')
            assert _waves() == waves
        for k in OUTPUTS:
            _same(whole[k], np.concatenate([first[k], second[k]]), f'{waves} waves per env: {k}')
        _same(ao, a, f'{waves} waves per env: sanitised actions')
        _same(eo, e, f'{waves} waves per env: final state')


def test_recorded_reference_tape_injected(hip):
    """tests/golden/single_s9_partial2.npz — 48 envs x 150 steps of the real reference, its random outcomes injected —
    through rollout_s9_kernel<partial, INJ> in both forms, against the reference's record"""
    from wurm_amd import _lib
    fx = replay.load('single_s9_partial2')
    assert int(fx['meta'][2]) > 128      # three chunks
    for waves in (2, 1):
        with _lib.knobs(**{KNOB: 0 if waves == 1 else 1 << 20}):
            replay.replay_single_rollout(hip(), fx)
            assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected' and _waves() == waves


def test_recorded_reference_tape_injected_without_observations(hip):
    """the same tape through rollout_s9_kernel<none, INJ>: the oracle, driven by the same injection, is the reference"""
    fx = replay.load('single_s9_partial2')
    out, _ = _three_ways(hip, fx['state0'].astype(np.float32), fx['actions_in'].copy(), 'none',
                         inject_food=fx['inject_food'], inject_reset=fx['inject_reset'])
    _same(out['done'], fx['done'], 'the oracle against the record: done')


@pytest.mark.parametrize('dtype', [np.int64, np.int32])
def test_action_dtypes_and_hostile_values(hip, dtype):
    """single_snake.py:221-222 only recognises a reversal for actions 0..3; anything else moves by action % 4 and the tape
    keeps the caller's value (negative actions wrap)"""
    N, T = 9, 129
    actions = np.random.RandomState(5).randint(-9, 13, size=(T, N)).astype(dtype)
    actions[::7] = np.iinfo(dtype).max
    actions[3::11] = np.iinfo(dtype).min + 1
    envs = _fresh(OracleBackend(seed=3), N)
    _three_ways(hip, envs, actions, 'partial_2', seed=3)


def _irregular_batch():
    """9 envs of which 0, 4 and 8 start where the stepper must take the generic path: the food under the body, a body cell on
    the border ring, two heads"""
    N = 9
    envs = _fresh(OracleBackend(seed=21), N)
    ys, xs = np.nonzero(envs[0, 2] == 1)
    envs[0, 0] = 0
    envs[0, 0, ys[0], xs[0]] = 1         # the food on the tail cell
    envs[4, 2, 0, 3] = 1                 # a body cell on the border ring
    free = np.argwhere((envs[8, 2, 1:-1, 1:-1] == 0) & (envs[8, 0, 1:-1, 1:-1] == 0) & (envs[8, 1, 1:-1, 1:-1] == 0))[0] + 1
    envs[8, 1, free[0], free[1]] = 1     # a second head
    assert (envs[0, 0] * envs[0, 2]).sum() > 0      # (a state the checker accepts, the lean loop does not)
    assert (OracleBackend(seed=21).single_check(envs)[[4, 8]] != 0).all()
    assert (OracleBackend(seed=21).single_check(envs)[[1, 2, 3, 5, 6, 7]] == 0).all()
    return envs, _tape(8, 129, N)


def test_envs_outside_the_lean_domain_beside_running_pairs(hip):
    """the steppers of envs 0, 4 and 8 take the generic path and their helpers leave after the first barrier; the six others
    run as pairs in the same launch.  Both forms of the library agree on every output of every env."""
    envs, actions = _irregular_batch()
    h2, h1 = hip(seed=21), hip(seed=21)
    h2.call = h1.call = 50
    (r2, e2, a2), (r1, e1, a1) = _launch(h2, envs, actions, 'partial_2', 2), _launch(h1, envs, actions, 'partial_2', 1)
    for k in OUTPUTS:
        _same(r1[k], r2[k], k)
    _same(a1, a2, 'sanitised actions')
    _same(e1, e2, 'final state')


def test_envs_outside_the_lean_domain_against_the_oracle(hip):
    """The same batch against the oracle, both forms, every output of every env.  The env with two heads is the one that
    asks something of the generic path: the reference moves the whole head channel, so both heads move until one of them
    leaves the interior, and the crop is centred on the first head in row-major order."""
    envs, actions = _irregular_batch()
    o = OracleBackend(seed=21)
    o.call = 50
    ro, eo, ao = _launch(o, envs, actions, 'partial_2', None)
    wrong = []
    for waves in (2, 1):
        h = hip(seed=21)
        h.call = 50
        r, e, a = _launch(h, envs, actions, 'partial_2', waves)
        pairs = [(k, ro[k], r[k], 1) for k in OUTPUTS] + [('sanitised actions', ao, a, 1), ('final state', eo, e, 0)]
        for name, want, got, env_axis in pairs:
            want, got = np.asarray(want), np.asarray(got)
            if want.dtype == np.float32:     # bit for bit
                want, got = want.view(np.uint32), np.ascontiguousarray(got, np.float32).view(np.uint32)
            bad = np.argwhere(want != got)
            if len(bad):
                wrong.append(f'{waves} waves per env: {name}: {len(bad)} elements, envs {sorted(set(bad[:, env_axis].tolist()))}'
                             + (f', steps {bad[:, 0].min()}-{bad[:, 0].max()}' if env_axis else ''))
    assert not wrong, '; '.join(wrong)


def test_long_snakes_events_after_the_first_chunk(hip):
    """a tape flown on the oracle that grows long snakes and then turns them into themselves or the wall late in every
    chunk: eating, edge collisions, self collisions and resets in the second and third chunk"""
    N, T, seed = 6, 192, 11
    envs = _fresh(OracleBackend(seed=seed), N)
    actions = _pilot_tape(seed, envs, T)
    out, eo = _three_ways(hip, envs, actions, 'partial_2', seed=seed)
    _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'self_collision', 'done'))
    assert (OracleBackend(seed=seed).single_check(eo) == 0).all()


def test_the_knob_and_its_default(hip):
    """N = 70 with the knob at 69 runs one wave per env, at 70 two; the default is what DESIGN.md states"""
    from wurm_amd import _lib
    N, T = 70, 3
    h = hip(seed=1)
    envs = _fresh(h, N)
    for knob, waves in ((69, 1), (70, 2)):
        with _lib.knobs(**{KNOB: knob}):
            h.single_rollout(envs.copy(), _tape(1, T, N), 'partial_2')
            assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9' and _waves() == waves
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'DESIGN.md')).read()
    stated = re.findall(KNOB + r'` \(default ([0-9]+)\)', design)
    assert stated, 'DESIGN.md states no default for ' + KNOB
    with _lib.knobs(**{KNOB: None}):
        assert {int(v) for v in stated} == {_lib.get_option(KNOB)}
