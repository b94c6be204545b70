"""GPU parity for the unrolled step loop of `rollout_s9_kernel` (wurm_amd/csrc/single_kernels.hpp): U steps per back
edge, the move entry whose low six bits are the next step's shift, the body mask taken before the move is known (the
clock carried as T + 1) and looked at again on a step that eats.  Each case is compared with the CPU oracle on every
output of every step, on the sanitised actions and on the final state; each test first asserts, on the CPU, that the
oracle's trajectory holds what it is about."""
import os
import re

import numpy as np
import pytest

from tests.backends import OracleBackend

pytestmark = pytest.mark.gpu

def _unroll_factor():
    """U as the kernel has it: the tape lengths and the residues below follow it."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'wurm_amd', 'csrc', 'single_kernels.hpp')
    found = re.findall(r'constexpr int U = (\d+);', open(src).read())
    assert len(found) == 1, f'the unroll factor of rollout_s9_kernel: {found}'
    return int(found[0])


U = _unroll_factor()
ACTION_VALUES = [-5, -1, 0, 1, 2, 3, 4, 7, 2 ** 31 - 1]
TAPE_LENGTHS = sorted(set(range(1, 2 * U + 2)) | set(range(64 - U, 64 + U + 2)) | {127, 128, 129, 192 + U - 1})
MOVES = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}  # action -> (row step, column step)
ACTION_OF = {v: k for k, v in MOVES.items()}


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


def _compare_rollout(o, h, envs, actions, mode, **inject):
    eo, eh = envs.copy(), envs.copy()
    ao, ah = actions.copy(), actions.copy()
    ro, rh = o.single_rollout(eo, ao, mode, **inject), h.single_rollout(eh, ah, mode, **inject)
    for k in ro:
        if ro[k] is not None or rh[k] is not None:
            _same(ro[k], rh[k], k)
    _same(ao, ah, 'sanitised actions')
    _same(eo, eh, 'final state')
    assert (o.single_check(eo) == 0).all()
    return ro


# ------------------------------------------------------------------------------------------------ tape lengths
@pytest.mark.parametrize('mode', ['partial_2', 'none'])
@pytest.mark.parametrize('T', TAPE_LENGTHS)
def test_tape_lengths(hip, T, mode):
    """Whole unrolled bodies only, a one-step tail only, both; chunks of 64 that end inside, at and past a body."""
    N, S = 3, 9
    rng = np.random.RandomState(2000 + T)
    o, h = OracleBackend(seed=T), hip(seed=T)
    envs = _fresh(o, N, S)
    o.call = h.call = 5 + T
    _compare_rollout(o, h, envs, rng.randint(0, 4, size=(T, N)).astype(np.int64), mode)


@pytest.mark.parametrize('S', [10, 11])
@pytest.mark.parametrize('T', TAPE_LENGTHS)
def test_tape_lengths_lean_kernel(hip, T, S):
    N = 3
    rng = np.random.RandomState(3000 + T + S)
    o, h = OracleBackend(seed=T + S), hip(seed=T + S)
    envs = _fresh(o, N, S)
    o.call = h.call = 1
    _compare_rollout(o, h, envs, rng.randint(0, 4, size=(T, N)).astype(np.int64), 'partial_1')


# ------------------------------------------------------------------------------------------------ entry layout
def _walk(seed, envs, actions, visit):
    """The oracle stepped one call at a time with the rollout's call numbering (step t: call0 + 2 t, its reset:
    call0 + 2 t + 1, call0 = 1); visit(t, oracle, state before, state after the step and before the reset, outputs,
    sanitised actions)."""
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    for t in range(actions.shape[0]):
        before = e.copy()
        a = actions[t].copy()
        out = o.single_step(e, a, 'none')
        visit(t, o, before, e.copy(), out, a)
        o.single_reset(e, out[2], 'none')


def _pairs_seen(seed, envs, actions):
    seen = set()
    _walk(seed, envs, actions,
          lambda t, o, before, after, out, a: seen.update(zip(o.orientations(before).tolist(), actions[t].tolist())))
    return seen


@pytest.mark.parametrize('dtype', [np.int64, np.int32])
def test_entry_layout_every_orientation_and_action(hip, dtype):
    """Every (orientation, action value) pair occurs: every entry of the table is taken at every kind of action, its
    low bits select the next one, and with T = 64 every lane writes a record the sanitised action is read back from."""
    N, S, T, seed = 8, 9, 64, 41
    o, h = OracleBackend(seed=seed), hip(seed=seed)
    envs = _fresh(o, N, S)
    rng = np.random.RandomState(7)
    actions = np.asarray(ACTION_VALUES, np.int64)[rng.randint(0, len(ACTION_VALUES), size=(T, N))].astype(dtype)
    seen = _pairs_seen(seed, envs, actions.astype(np.int64))
    missing = [(ori, a) for ori in range(4) for a in ACTION_VALUES if (ori, a) not in seen]
    assert not missing, f'the tape does not reach (orientation, action) {missing}'
    o.call = h.call = 1
    _compare_rollout(o, h, envs, actions, 'partial_2')


# ------------------------------------------------------------------------------------------------ piloted tapes
def _pilot_tape(seed, envs, T):
    """A tape flown on the oracle, one step at a time.  Every env hunts the food; on top of that, by env:
    0-1  turn into their own body late in a 64-step chunk, as soon as a body cell that will still be there is next to
         the head;
    2-3  run into the nearest wall late in a chunk (from different steps on, so that the collisions spread);
    4    with length 4, goes round the food so that it eats out of a turn and then turns on into the cell that is body
         only because the clock stood still: K -> H = K + d -> H + p -> F = K + p (eats) -> K (value 2 before the step);
    5    with length 4, goes round in a 2 x 2 square: the head enters the cell the tail leaves, step after step;
    6-7  hunt, and run into a wall at the very start / end of a chunk."""
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    N, _, S, _ = e.shape
    last = np.zeros(N, np.int64)
    script = [[] for _ in range(N)]
    tape = np.zeros((T, N), np.int64)
    inside_cell = lambda y, x: 1 <= y <= S - 2 and 1 <= x <= S - 2
    for t in range(T):
        phase = t % 64
        for i in range(N):
            hy, hx = np.argwhere(e[i, 1] > 0)[0]
            fy, fx = np.argwhere(e[i, 0] > 0)[0]
            body, L = e[i, 2], e[i, 2].max()
            cells = {a: (hy + dy, hx + dx) for a, (dy, dx) in MOVES.items()}
            inside = {a: inside_cell(*cells[a]) for a in cells}
            neck = {a: body[cells[a]] == L - 1 for a in cells}          # a reversal: sanitised to "straight on"
            safe = [a for a in cells if inside[a] and body[cells[a]] <= 1]
            hits = [a for a in cells if inside[a] and body[cells[a]] >= 2 and not neck[a]]
            towards = lambda ty, tx, allowed: min(allowed, key=lambda a: abs(cells[a][0] - ty) + abs(cells[a][1] - tx))
            hunt = towards(fy, fx, safe) if safe else 0
            free = [b for b in cells if not neck[b] and (not inside[b] or body[cells[b]] <= 1)]
            wall = lambda b: min(cells[b][0], S - 1 - cells[b][0], cells[b][1], S - 1 - cells[b][1])
            to_wall = min(free, key=wall) if free else hunt
            a = hunt
            if i < 2 and phase >= 40:
                turn = (last[i] + 1) % 4
                a = hits[0] if hits else turn if turn in safe else hunt
            elif i in (2, 3) and phase >= (50, 56)[i - 2]:
                a = to_wall
            elif i == 4:
                if script[i]:
                    a = script[i].pop(0)
                elif L == 4:
                    ny, nx = np.argwhere(body == L - 1)[0]
                    heading = (hy - ny, hx - nx)
                    plans = []                                          # (K, script) for every way round the food
                    for p in MOVES.values():
                        K = (fy - p[0], fx - p[1])
                        for d in MOVES.values():
                            if d[0] * p[0] + d[1] * p[1] != 0:
                                continue
                            H, Fd = (K[0] + d[0], K[1] + d[1]), (fy + d[0], fx + d[1])
                            if inside_cell(*K) and inside_cell(*H) and inside_cell(*Fd):
                                plans.append((K, d, [ACTION_OF[d], ACTION_OF[p], ACTION_OF[(-d[0], -d[1])],
                                                     ACTION_OF[(-p[0], -p[1])]]))
                    here = [pl for pl in plans if pl[0] == (hy, hx) and pl[1] != (-heading[0], -heading[1])
                            and body[hy + pl[1][0], hx + pl[1][1]] == 0 and body[fy + pl[1][0], fx + pl[1][1]] == 0]
                    no_food = [b for b in safe if cells[b] != (fy, fx)]
                    if here:
                        script[i] = list(here[0][2])
                        a = script[i].pop(0)
                    elif plans and no_food:
                        Ky, Kx = min((pl[0] for pl in plans), key=lambda K: abs(K[0] - hy) + abs(K[1] - hx))
                        a = towards(Ky, Kx, no_food)
                    elif no_food:
                        a = no_food[0]
            elif i == 5 and L == 4 and phase < 60:
                turn = (last[i] + 1) % 4
                a = turn if turn in safe and cells[turn] != (fy, fx) else hunt
            elif i == 5 and phase >= 60:
                a = to_wall
            elif i == 6 and phase >= 60:
                a = to_wall
            elif i == 7 and (phase >= 61 or phase < 2):
                a = to_wall
            tape[t, i] = last[i] = a
        done = o.single_step(e, tape[t].copy(), 'none')[2]
        if done[4]:
            script[4] = []
        o.single_reset(e, done, 'none')
    return tape


PILOT = dict(N=8, S=9, T=256, seed=11)
_pilot_cache = {}


def _piloted():
    """(start state, tape, what the oracle's trajectory holds per step): computed once, never changed."""
    if not _pilot_cache:
        o = OracleBackend(seed=PILOT['seed'])
        envs = _fresh(o, PILOT['N'], PILOT['S'])
        tape = _pilot_tape(PILOT['seed'], envs, PILOT['T'])
        T, N = tape.shape
        facts = {k: np.zeros((T, N), bool) for k in ('eat', 'selfc', 'edgec', 'tail_in_window', 'tail_chase',
                                                     'still_clock_collision')}

        def visit(t, o, before, after, out, moved):
            _, reward, done, sc, ec = out
            for i in range(N):
                body = before[i, 2]
                hy, hx = np.argwhere(before[i, 1] > 0)[0]
                ny, nx = hy + MOVES[int(moved[i])][0], hx + MOVES[int(moved[i])][1]
                eat = reward[i] > 0
                facts['eat'][t, i], facts['selfc'][t, i], facts['edgec'][t, i] = eat, sc[i] != 0, ec[i] != 0
                ty, tx = np.argwhere(body == 1)[0]
                facts['tail_in_window'][t, i] = eat and abs(ty - ny) <= 2 and abs(tx - nx) <= 2
                facts['tail_chase'][t, i] = (not eat) and (ny, nx) == (ty, tx) and not done[i]
                facts['still_clock_collision'][t, i] = (t > 0 and facts['eat'][t - 1, i] and sc[i] != 0
                                                        and body[ny, nx] == 2)

        _walk(PILOT['seed'], envs, tape, visit)
        envs.setflags(write=False)
        tape.setflags(write=False)
        _pilot_cache.update(envs=envs, tape=tape, facts=facts)
    return _pilot_cache['envs'], _pilot_cache['tape'], _pilot_cache['facts']


def test_event_at_every_position_of_the_unrolled_body(hip):
    envs, tape, facts = _piloted()
    t = np.arange(tape.shape[0])
    for r in range(U):
        at = {k: int(facts[k][t % U == r].sum()) for k in ('eat', 'selfc', 'edgec')}
        assert all(at.values()), f'the oracle trajectory lacks an event at steps with t % {U} == {r}: {at}'
    any_event = (facts['eat'] | facts['selfc'] | facts['edgec']).any(axis=1)
    assert any_event[t % 64 == 0].any() and any_event[t % 64 == 63].any(), 'no event on the first / last step of a chunk'
    o, h = OracleBackend(seed=PILOT['seed']), hip(seed=PILOT['seed'])
    o.call = h.call = 1
    _compare_rollout(o, h, np.array(envs), np.array(tape), 'partial_2')


def test_clock_that_stands_still(hip):
    """A step that eats leaves the clock alone: the tail cell stays body (and the crop shows it), and a cell that would
    have been free one step later is still a collision; a step that does not eat frees the tail's cell before the head
    enters it."""
    envs, tape, facts = _piloted()
    counts = {k: int(facts[k].sum()) for k in ('tail_in_window', 'tail_chase', 'still_clock_collision')}
    assert all(counts.values()), f'the oracle trajectory lacks: {counts}'
    for T in (tape.shape[0], tape.shape[0] - U + 1):
        o, h = OracleBackend(seed=PILOT['seed']), hip(seed=PILOT['seed'])
        o.call = h.call = 1
        _compare_rollout(o, h, np.array(envs), np.array(tape[:T]), 'partial_2')


# ------------------------------------------------------------------------------------------------ recorded outcomes
def _recorded_outcomes(seed, envs, actions):
    """inject_food (T, N) / inject_reset (T, N, 4) of the oracle's own RNG-mode run: the food cell after a step that
    ate, (seed row, seed column, direction, food cell) after a reset; -1 / a harmless centre seed where nothing happened."""
    T, N = actions.shape
    S = envs.shape[-1]
    food = np.full((T, N), -1, np.int32)
    reset = np.tile(np.asarray([4, 4, 0, -1], np.int32), (T, N, 1))
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    for t in range(T):
        _, reward, done, _, _ = o.single_step(e, actions[t].copy(), 'none')
        for i in np.flatnonzero(reward > 0):
            cell = np.argwhere(e[i, 0] > 0)
            food[t, i] = cell[0][0] * S + cell[0][1] if len(cell) else -1
        o.single_reset(e, done, 'none')
        for i in np.flatnonzero(done):
            (sy, sx), (hy, hx) = np.argwhere(e[i, 2] == 2)[0], np.argwhere(e[i, 2] == 3)[0]
            d = {(-1, 0): 0, (0, 1): 1, (1, 0): 2, (0, -1): 3}[(hy - sy, hx - sx)]
            fy, fx = np.argwhere(e[i, 0] > 0)[0]
            reset[t, i] = (sy, sx, d, fy * S + fx)
    return food, reset


def test_recorded_outcomes_through_the_injected_instantiation(hip):
    N, S, T, seed = 6, 9, 64 + U + 1, 23
    o = OracleBackend(seed=seed)
    envs = _fresh(o, N, S)
    actions = np.array(_pilot_tape(seed, envs, T)[:, :N])
    food, reset = _recorded_outcomes(seed, envs, actions)
    probe = OracleBackend(seed=seed)
    probe.call = 1
    exp = probe.single_rollout(envs.copy(), actions.copy(), 'partial_2')
    assert exp['reward'].sum() >= 3 and exp['done'].sum() >= 2, 'the tape neither eats nor dies'
    replay = OracleBackend(seed=seed + 1)                               # another stream: the outcomes come from the arrays
    replay.call = 1
    got = replay.single_rollout(envs.copy(), actions.copy(), 'partial_2', inject_food=food, inject_reset=reset)
    for k in exp:
        _same(exp[k], got[k], f'oracle with recorded outcomes: {k}')
    o, h = OracleBackend(seed=seed + 1), hip(seed=seed + 1)
    o.call = h.call = 1
    _compare_rollout(o, h, envs, actions, 'partial_2', inject_food=food, inject_reset=reset)


# ------------------------------------------------------------------------------------------------ chained launches
@pytest.mark.parametrize('split', [U + 1, 64 + U - 1, 2 * 64 + 1])
def test_chained_launches(hip, split):
    """Two launches of lengths that are no multiples of U == one launch of the sum == the oracle on the whole tape."""
    N, S, T = 4, 9, 2 * 64 + U + 2
    assert split % U and (T - split) % U
    rng = np.random.RandomState(split)
    actions = rng.randint(0, 4, size=(T, N)).astype(np.int64)
    o, h1, h2 = OracleBackend(seed=6), hip(seed=6), hip(seed=6)
    e0, e1, e2 = _fresh(o, N, S), _fresh(h1, N, S), _fresh(h2, N, S)
    _same(e0, e1, 'start state')
    a0, a1, a2 = actions.copy(), actions.copy(), actions.copy()
    ref = o.single_rollout(e0, a0, 'partial_2')
    whole = h1.single_rollout(e1, a1, 'partial_2')
    first = h2.single_rollout(e2, a2[:split], 'partial_2')
    second = h2.single_rollout(e2, a2[split:], 'partial_2')
    for k in ref:
        _same(ref[k], whole[k], f'one launch: {k}')
        _same(ref[k], np.concatenate([first[k], second[k]]), f'two launches: {k}')
    _same(e0, e1, 'final state, one launch')
    _same(e0, e2, 'final state, two launches')
    _same(a0, a1, 'sanitised actions, one launch')
    _same(a0, a2, 'sanitised actions, two launches')
    assert (o.single_check(e0) == 0).all()
