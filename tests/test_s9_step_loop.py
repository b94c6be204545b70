"""GPU parity for the step loop of `rollout_s9_kernel` (and of `rollout_lean_kernel`, which shares its statements) in
wurm_amd/csrc/single_kernels.hpp: the move entry taken from a 64-bit table by one shift, the per-step record written
into lane j, the clock advanced through the carry, and the reset nested behind the one event test.  Each case is
compared with the CPU oracle on every output of every step, like tests/test_hip_lean_rollout.py."""
import numpy as np
import pytest

from tests.backends import OracleBackend

pytestmark = pytest.mark.gpu

ACTION_VALUES = [-5, -1, 0, 1, 2, 3, 4, 7, 2 ** 31 - 1]


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    x, y = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
    assert x.shape == y.shape, f'{what}: shape {x.shape} vs {y.shape}'
    bad = np.argwhere(x != y)
    assert len(bad) == 0, f'{what}: {len(bad)} mismatches, first at {bad[0].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}'


def _fresh(backend, N, S):
    envs = np.zeros((N, 3, S, S), np.float32)
    backend.single_reset(envs, np.ones(N, np.uint8), 'none')
    return envs


def _compare_rollout(o, h, envs, actions, mode):
    eo, eh = envs.copy(), envs.copy()
    ao, ah = actions.copy(), actions.copy()
    ro, rh = o.single_rollout(eo, ao, mode), h.single_rollout(eh, ah, mode)
    for k in ro:
        if ro[k] is not None or rh[k] is not None:
            _same(ro[k], rh[k], k)
    _same(ao, ah, 'sanitised actions')
    _same(eo, eh, 'final state')
    assert (o.single_check(eo) == 0).all()
    return ro


def _pairs_seen(seed, envs, actions):
    """(orientation, action value) of every env-step, from the oracle stepped one call at a time with the rollout's
    call numbering (step t: call0 + 2 t, its reset: call0 + 2 t + 1)."""
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    seen = set()
    for t in range(actions.shape[0]):
        ori = o.orientations(e)
        seen.update(zip(ori.tolist(), actions[t].tolist()))
        a = actions[t].copy()
        done = o.single_step(e, a, 'none')[2]
        o.single_reset(e, done, 'none')
    return seen


@pytest.mark.parametrize('dtype', [np.int64, np.int32])
def test_move_table_every_orientation_and_action(hip, dtype):
    """Every (orientation, action value) pair occurs, so every 16-bit entry of the 64-bit move table is taken at every
    kind of action, and with T = 64 every one of the 64 lanes writes a record."""
    N, S, T, seed = 8, 9, 64, 41
    o, h = OracleBackend(seed=seed), hip(seed=seed)
    envs = _fresh(o, N, S)
    rng = np.random.RandomState(7)
    actions = np.asarray(ACTION_VALUES, np.int64)[rng.randint(0, len(ACTION_VALUES), size=(T, N))].astype(dtype)
    seen = _pairs_seen(seed, envs, actions)
    missing = [(ori, a) for ori in range(4) for a in ACTION_VALUES if (ori, a) not in seen]
    assert not missing, f'the tape does not reach (orientation, action) {missing}'
    o.call = h.call = 1
    _compare_rollout(o, h, envs, actions, 'partial_2')


@pytest.mark.parametrize('mode', ['partial_2', 'none'])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 5, 7, 61, 62, 63, 64, 65, 66, 67, 68, 130])
def test_tape_lengths(hip, T, mode):
    N, S = 3, 9
    rng = np.random.RandomState(1000 + T)
    o, h = OracleBackend(seed=T), hip(seed=T)
    envs = _fresh(o, N, S)
    o.call = h.call = 3 + T
    _compare_rollout(o, h, envs, rng.randint(0, 4, size=(T, N)).astype(np.int64), mode)


MOVES = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}  # action -> (row step, column step)


def _pilot_tape(seed, envs, T):
    """A tape flown on the oracle, one step at a time: every env hunts the food (so snakes grow long, the way the sweep of
    test_long_snakes_and_food_respawn grows them); late in each 64-step chunk envs 0-2 turn into their own body as
    soon as a body cell that will still be there is next to the head, and envs 3-5 run into the nearest wall."""
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    N, _, S, _ = e.shape
    last = np.zeros(N, np.int64)
    tape = np.zeros((T, N), np.int64)
    for t in range(T):
        phase = t % 64
        for i in range(N):
            hy, hx = np.argwhere(e[i, 1] > 0)[0]
            fy, fx = np.argwhere(e[i, 0] > 0)[0]
            body, L = e[i, 2], e[i, 2].max()
            cells = {a: (hy + dy, hx + dx) for a, (dy, dx) in MOVES.items()}
            inside = {a: 1 <= y <= S - 2 and 1 <= x <= S - 2 for a, (y, x) in cells.items()}
            neck = {a: body[cells[a]] == L - 1 for a in cells}          # a reversal: sanitised to "straight on"
            safe = [a for a in cells if inside[a] and body[cells[a]] <= 1]
            hits = [a for a in cells if inside[a] and body[cells[a]] >= 2 and not neck[a]]
            hunt = min(safe, key=lambda a: abs(cells[a][0] - fy) + abs(cells[a][1] - fx)) if safe else 0
            a = hunt
            if i < 3 and phase >= 40:
                turn = (last[i] + 1) % 4
                a = hits[0] if hits else turn if turn in safe else hunt
            elif i >= 3 and phase >= 56:
                free = [b for b in cells if not neck[b] and (not inside[b] or body[cells[b]] <= 1)]
                wall = lambda b: min(cells[b][0], S - 1 - cells[b][0], cells[b][1], S - 1 - cells[b][1])
                a = min(free, key=wall) if free else hunt
            tape[t, i] = last[i] = a
        done = o.single_step(e, tape[t].copy(), 'none')[2]
        o.single_reset(e, done, 'none')
    return tape


def test_eating_and_dying_in_every_chunk(hip):
    """Long snakes: the oracle's trajectory holds an eating step, a self collision and an edge collision in each of the
    three 64-step chunks (checked here, on the CPU, before anything is compared)."""
    N, S, T, seed = 6, 9, 192, 11
    o, h = OracleBackend(seed=seed), hip(seed=seed)
    envs = _fresh(o, N, S)
    actions = _pilot_tape(seed, envs, T)
    probe = OracleBackend(seed=seed)
    probe.call = 1
    exp = probe.single_rollout(envs.copy(), actions.copy(), 'none')
    for k in range(3):
        chunk = slice(64 * k, 64 * k + 64)
        counts = {name: int(np.asarray(exp[name][chunk]).astype(bool).sum())
                  for name in ('reward', 'self_collision', 'edge_collision')}
        assert all(counts.values()), f'the oracle trajectory lacks an event in chunk {k}: {counts}'
    assert envs.shape[0] == N and exp['reward'].sum() > 2 * N
    o.call = h.call = 1
    _compare_rollout(o, h, envs, actions, 'partial_2')


@pytest.mark.parametrize('S', [10, 11])
def test_lean_kernel_sizes(hip, S):
    N, T = 4, 70
    rng = np.random.RandomState(S)
    o, h = OracleBackend(seed=S), hip(seed=S)
    envs = _fresh(o, N, S)
    o.call = h.call = 1
    _compare_rollout(o, h, envs, rng.randint(0, 4, size=(T, N)).astype(np.int64), 'partial_1')


def test_chained_launches(hip):
    """Two launches of 100 steps == one launch of 200 steps."""
    N, S = 4, 9
    rng = np.random.RandomState(4)
    actions = rng.randint(0, 4, size=(200, N)).astype(np.int64)
    h1, h2 = hip(seed=6), hip(seed=6)
    e1, e2 = _fresh(h1, N, S), _fresh(h2, N, S)
    a1, a2 = actions.copy(), actions.copy()
    whole = h1.single_rollout(e1, a1, 'partial_2')
    first = h2.single_rollout(e2, a2[:100], 'partial_2')
    second = h2.single_rollout(e2, a2[100:], 'partial_2')
    for k in whole:
        _same(whole[k], np.concatenate([first[k], second[k]]), k)
    _same(e1, e2, 'final state')
    _same(a1, a2, 'actions')
