"""GPU parity for the trio form of `rollout_s9_kernel` once its render waves REBUILD what the stepper used to record
(wurm_amd/csrc/single_kernels.hpp, REBUILD; single_device.hpp, s9_rebuild_crop_words): the stepper keeps per step the move
entry and the body mask only, on an eating step also the food it drew, and hands over per chunk the head and food code it
entered the chunk with and the chunk's would-be reset words.  Each render wave works the head code (a prefix sum of the code
steps that restarts behind every reset) and the shown food code (whatever an eating step, a reset or the chunk start left
last) of all 64 steps out, one step per lane, before it draws.

Every case forces the forms through the knobs as tests/test_s9_trio_rollout.py does and compares the trio form bit for bit
with the CPU oracle and with the `helper` and `one` forms of the same library: observations, rewards, dones, both collision
flags, the sanitised tape and the final state.  Every case asserts on the ORACLE's outputs that the events it exists for did
happen, and how often, before anything is compared.

The piloted tapes walk a closed loop of interior cells and take every random outcome from injected arrays (the INJ
instantiation), so an event falls on exactly the step the schedule names: the perimeter of the interior (24 cells, always a
wall beside the head) for eating steps and edge collisions, a serpentine cycle of 38 cells for the long snakes."""
import numpy as np
import pytest

from tests import replay
from tests.backends import OracleBackend
from tests.test_s9_crop_helper import OUTPUTS, S, _fresh, _irregular_batch, _same, _tape
from tests.test_s9_step_loop import MOVES
from tests.test_s9_trio_rollout import FORM, KNOBS, _form, _four_ways

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _b(out, k):
    return np.asarray(out[k]).astype(bool)


# ---- random tapes

@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 128, 129, 257])
def test_chunk_edges_random_tape(hip, T):
    """every chunk edge and tail; from T = 65 on a chunk is rebuilt from a state the stepper handed over, from 129 on with
    both record-buffer parities"""
    N = 3
    envs = _fresh(OracleBackend(seed=40 + T), N)
    out, _ = _four_ways(hip, envs, _tape(40 + T, T, N), 'partial_2', seed=40 + T, call=3 + T)
    assert out['obs'].shape[:2] == (T, N)
    if T >= 128:
        done, ate = _b(out, 'done'), _b(out, 'reward')
        assert done.sum() >= 2 and ate.sum() >= 2, f"the oracle's trajectory: {done.sum()} resets, {ate.sum()} eating steps"


@pytest.mark.parametrize('mode', ['partial_1', 'partial_2', 'partial_3'])
def test_observation_modes(hip, mode):
    """two steps per pass (9 and 25 window cells) and one (49): the pass reads the rebuilt word of its own step"""
    N, T = 70, 129
    envs = _fresh(OracleBackend(seed=6), N)
    out, _ = _four_ways(hip, envs, _tape(32, T, N), mode, seed=6)
    late = {k: int(_b(out, k)[64:].sum()) for k in ('reward', 'edge_collision', 'done')}
    assert all(late.values()), f"the oracle's trajectory lacks an event after step 64: {late}"


def test_one_env(hip):
    N, T = 1, 129
    envs = _fresh(OracleBackend(seed=8), N)
    out, _ = _four_ways(hip, envs, _tape(8, T, N), 'partial_2', seed=8)
    assert _b(out, 'done').any(), 'the oracle: no reset'


# ---- piloted tapes with injected outcomes

PERIMETER = [(1, x) for x in range(1, 8)] + [(y, 7) for y in range(2, 8)] + [(7, x) for x in range(6, 0, -1)] + \
            [(y, 1) for y in range(6, 1, -1)]
# row 1 left to right, columns 7 .. 2 up and down over rows 2 .. 6, back through (2, 1); (3 .. 6, 1) and row 7 stay free
SERPENTINE = [(1, x) for x in range(1, 8)] + \
             [(y, x) for x in range(7, 1, -1) for y in (range(2, 7) if x % 2 else range(6, 1, -1))] + [(2, 1)]
PARK = {id(PERIMETER): (4, 4), id(SERPENTINE): (4, 1)}     # where the food waits when no eating step is scheduled
# injected resets whose head lies on the perimeter with the neck not on the way round: (seed row, seed column, direction)
STARTS = [(2, 4, 0), (4, 6, 1), (6, 4, 2), (4, 2, 3), (2, 1, 0), (1, 6, 1), (6, 7, 2), (7, 2, 3)]
TAP = {0: (-1, 0), 1: (0, 1), 2: (1, 0), 3: (0, -1)}       # direction of a reset -> (row step, column step)


def _assert_loops():
    for loop in (PERIMETER, SERPENTINE):
        assert len(set(loop)) == len(loop)
        for a, b in zip(loop, loop[1:] + loop[:1]):
            assert abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 and 1 <= a[0] <= 7 and 1 <= a[1] <= 7


def _fly(first, schedules, T, first_loop, seed=0):
    """Flies N envs on the oracle, one step at a time, and returns (envs, actions, inject_food, inject_reset).

    first[i]: (seed row, seed column, direction) of env i's first snake, whose head lies on first_loop; every later snake
    comes from STARTS in turn and walks PERIMETER.  schedules[i]: {step: 'eat' | 'edge' | 'self'}; 'self' means: from that step
    on, the first step on which the head can turn into its own body (not the neck).  On every other step the snake moves on
    along its loop.  The food always lies where the next eating step of the same life finds it, or is parked."""
    _assert_loops()
    N = len(first)
    inject_food = np.full((T, N), -1, np.int32)
    inject_reset = np.zeros((T, N, 4), np.int32)
    actions = np.zeros((T, N), np.int64)
    loops = [first_loop] * N
    nth_start = [i for i in range(N)]
    pending_self = [False] * N

    def food_for(i, head_after, t_now):
        """the cell the head reaches on env i's next eating step if that comes before any collision, as seen after step
        t_now with the head at head_after; else the parking cell"""
        loop = loops[i]
        coming = sorted(t for t in schedules[i] if t > t_now)
        if coming and schedules[i][coming[0]] == 'eat':
            d = coming[0] - t_now
            assert d <= 16, f'env {i}: the eating step {coming[0]} is {d} steps away'
            return loop[(loop.index(head_after) + d) % len(loop)]
        return PARK[id(loop)]

    def reset_row(i, t_now):
        sy, sx, d = STARTS[nth_start[i] % len(STARTS)]
        nth_start[i] += 1
        loops[i] = PERIMETER
        fy, fx = food_for(i, (sy + TAP[d][0], sx + TAP[d][1]), t_now)
        return (sy, sx, d, fy * S + fx)

    # the first snakes: an injected reset whose food is on the way to the first eating step
    envs = np.zeros((N, 3, S, S), np.float32)
    row0 = np.zeros((N, 4), np.int32)
    for i, (sy, sx, d) in enumerate(first):
        fy, fx = food_for(i, (sy + TAP[d][0], sx + TAP[d][1]), -1)
        row0[i] = (sy, sx, d, fy * S + fx)
    o = OracleBackend(seed=seed)
    o.single_reset(envs, np.ones(N, np.uint8), 'none', inject_reset=row0)
    e = envs.copy()
    for t in range(T):
        for i in range(N):
            loop = loops[i]
            hy, hx = (int(v) for v in np.argwhere(e[i, 1] > 0)[0])
            body, L = e[i, 2], e[i, 2].max()
            nxt = loop[(loop.index((hy, hx)) + 1) % len(loop)]
            cells = {a: (hy + dy, hx + dx) for a, (dy, dx) in MOVES.items()}
            want = schedules[i].get(t)
            pending_self[i] = pending_self[i] or want == 'self'
            a = next(a for a, c in cells.items() if c == nxt)
            if want == 'edge':
                a = next(a for a, (y, x) in cells.items() if not (1 <= y <= 7 and 1 <= x <= 7))
            elif pending_self[i]:
                hits = [a for a, c in cells.items() if 1 <= c[0] <= 7 and 1 <= c[1] <= 7 and 2 <= body[c] < L - 1]
                if hits:
                    a, pending_self[i] = hits[0], False
                    schedules[i][t] = 'self'
            actions[t, i] = a
            target = cells[a]
            ends = not (1 <= target[0] <= 7 and 1 <= target[1] <= 7) or body[target] >= 2
            if ends:
                inject_reset[t, i] = reset_row(i, t)
            elif e[i, 0][target] > 0:
                assert want == 'eat', f'env {i} eats on step {t}, which no schedule names'
                fy, fx = food_for(i, target, t)
                inject_food[t, i] = fy * S + fx
            else:
                assert want != 'eat', f'env {i}: no food where step {t} should eat'
        done = o.single_step(e, actions[t].copy(), 'none', inject_food=inject_food[t])[2]
        o.single_reset(e, done, 'none', inject_reset=inject_reset[t])
    return envs, actions, inject_food, inject_reset


def _injected(hip, mode, envs, actions, inject_food, inject_reset, seed=0):
    from wurm_amd import _lib
    out, _ = _four_ways(hip, envs, actions, mode, seed=seed, inject_food=inject_food, inject_reset=inject_reset)
    assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected'
    return out


@pytest.mark.parametrize('mode', ['partial_2', 'partial_3'])
def test_resets_and_eating_steps_around_a_chunk_boundary(hip, mode):
    """collisions on steps 63 and 64 (a reset word carried across the boundary, a segment that starts at lane 0), five resets
    inside one chunk, a reset on the last step of the launch; eating steps on steps 0, 63 and 64, right after a reset and on
    two consecutive steps"""
    T = 130
    schedules = [
        {0: 'eat', 1: 'eat', 10: 'edge', 11: 'eat', 25: 'eat', 40: 'eat', 50: 'edge', 63: 'eat', 64: 'eat', 70: 'edge',
         75: 'edge', 80: 'edge', 85: 'edge', 86: 'eat', 100: 'eat', 129: 'edge'},
        {5: 'edge', 6: 'eat', 20: 'edge', 30: 'edge', 40: 'edge', 63: 'edge', 64: 'edge', 65: 'eat', 66: 'eat', 127: 'edge',
         128: 'edge', 129: 'eat'},
        {0: 'edge', 1: 'eat', 2: 'eat', 62: 'edge', 63: 'eat', 64: 'edge', 65: 'eat', 66: 'edge', 67: 'edge', 68: 'edge',
         69: 'edge', 120: 'edge', 127: 'eat', 128: 'eat', 129: 'edge'},
    ]
    envs, actions, inject_food, inject_reset = _fly(STARTS[4:7], schedules, T, PERIMETER)
    out = _injected(hip, mode, envs, actions, inject_food, inject_reset)
    edge, ate, done = _b(out, 'edge_collision'), _b(out, 'reward'), _b(out, 'done')
    for i, sch in enumerate(schedules):      # the oracle's trajectory is the schedule, step for step
        assert np.flatnonzero(edge[:, i]).tolist() == sorted(t for t in sch if sch[t] == 'edge'), i
        assert np.flatnonzero(ate[:, i]).tolist() == sorted(t for t in sch if sch[t] == 'eat'), i
    assert (done == edge).all()
    assert edge[63, 1] and edge[64, 1] and edge[62, 2] and edge[64, 2]
    assert done[64:128, 0].sum() >= 4 and done[64:128, 2].sum() >= 4 and done[:64, 1].sum() >= 4
    assert done[T - 1, 0] and done[T - 1, 2]
    assert ate[0, 0] and ate[63, 0] and ate[64, 0] and ate[63, 2]
    assert (ate[1:] & done[:-1]).sum() >= 5, 'eating steps right after a reset'
    assert (ate[1:] & ate[:-1]).sum() >= 5, 'eating steps on two consecutive steps'


@pytest.mark.parametrize('mode', ['partial_2', 'partial_3'])
def test_edge_collisions_with_a_wrapped_head_code(hip, mode):
    """as test_edge_collision_on_every_step_with_injected_resets of tests/test_s9_trio_rollout.py: a new snake beside each
    of the four sides of the ring on every step, in the middle and beside both corners, walks into it at once; a head on
    row 8, column 0 or column 8 has a code that wrapped or aliases, and the crop needs the very integer the stepper had"""
    T = 129
    starts = [(2, 1, 0, 2), (2, 4, 0, 2), (2, 7, 0, 2), (6, 1, 2, 0), (6, 4, 2, 0), (6, 7, 2, 0),
              (1, 2, 3, 1), (4, 2, 3, 1), (7, 2, 3, 1), (1, 6, 1, 3), (4, 6, 1, 3), (7, 6, 1, 3)]
    N = 3
    inject_reset = np.zeros((T, N, 4), np.int32)
    actions = np.zeros((T, N), np.int64)
    first = np.zeros((N, 4), np.int32)
    # env i lives its step t as start (4 i + t) % 12: every life of an env has another seed and side than the one before
    for i in range(N):
        first[i] = (*starts[4 * i][:3], 4 * S + 4)   # the food on the centre cell, which no such snake covers
        for t in range(T):
            actions[t, i] = starts[(4 * i + t) % 12][3]
            inject_reset[t, i] = (*starts[(4 * i + t + 1) % 12][:3], 4 * S + 4)
    inject_food = np.full((T, N), -1, np.int32)
    envs = np.zeros((N, 3, S, S), np.float32)
    OracleBackend(seed=2).single_reset(envs, np.ones(N, np.uint8), 'none', inject_reset=first)
    out = _injected(hip, mode, envs, actions, inject_food, inject_reset, seed=2)
    assert _b(out, 'edge_collision').all(), 'the oracle: not every step runs into the ring'


def _long_snakes(T):
    """three snakes on the serpentine cycle that eat every second step until they have 21, 25 and 31 cells.  Env 0 walks on
    for more than 64 steps and then turns into its own body (from step 110 on); env 1 does so early in the second chunk
    (from step 66 on) and its three-cell successor lives through the rest of the launch; env 2 does so in the first chunk
    already (from step 60 on), its successor runs into the ring in the second and the next one eats at once."""
    grow = [18, 22, 28]
    schedules = [{2 * k: 'eat' for k in range(n)} for n in grow]
    schedules[0][110] = 'self'
    schedules[1][66] = 'self'
    schedules[2][60] = 'self'
    schedules[2][90] = 'edge'
    schedules[2][91] = 'eat'
    envs, actions, inject_food, inject_reset = _fly([(1, 2, 1)] * 3, schedules, T, SERPENTINE, seed=1)
    return schedules, grow, envs, actions, inject_food, inject_reset


@pytest.mark.parametrize('mode', ['partial_2', 'partial_3'])
def test_long_snakes_trail_and_snapshot_across_a_chunk_boundary(hip, mode):
    """the body a crop shows is partly the trail of the chunk's own steps, partly what the chunk started with, across the
    boundary at step 64 and, for the successors, at 128; each long life ends in a self collision, which shows body under the head"""
    T = 129
    schedules, grow, envs, actions, inject_food, inject_reset = _long_snakes(T)
    out = _injected(hip, mode, envs, actions, inject_food, inject_reset, seed=1)
    selfc, ate, done = _b(out, 'self_collision'), _b(out, 'reward'), _b(out, 'done')
    died = [np.flatnonzero(selfc[:, i]).tolist() for i in range(3)]
    assert all(len(d) == 1 for d in died) and (done[:, :2] == selfc[:, :2]).all(), died
    assert 110 <= died[0][0] < T and 66 <= died[1][0] < 80 and 60 <= died[2][0] < 64, died
    for i in range(3):
        assert ate[:died[i][0], i].sum() == grow[i] >= 17, 'a snake of at least 20 cells'
        assert died[i][0] - 2 * grow[i] > (64 if i == 0 else 0), 'walked on at full length'
    assert done[90, 2] and ate[91, 2] and ate[died[2][0]:, 2].sum() == 1


def test_chained_launches(hip):
    """3 x 129 steps: the state written back by one launch seeds the rebuild of the next one's first chunk"""
    from wurm_amd import _lib
    N, seed, call = 3, 29, (1 << 40) + 5
    actions = _tape(9, 3 * 129, N)
    o = OracleBackend(seed=seed)
    o.call = call
    envs = _fresh(OracleBackend(seed=seed), N)
    eo, ao = envs.copy(), actions.copy()
    whole = o.single_rollout(eo, ao, 'partial_2')
    for part in range(3):
        sl = slice(129 * part, 129 * part + 129)
        assert _b(whole, 'done')[sl].any() and _b(whole, 'reward')[sl].any(), f"the oracle: launch {part} lacks an event"
    h = hip(seed=seed)
    h.call = call
    e, a = envs.copy(), actions.copy()
    parts = []
    with _lib.knobs(**KNOBS['trio']):
        for part in range(3):
            parts.append(h.single_rollout(e, a[129 * part:129 * part + 129], 'partial_2'))
            assert _form() == FORM['trio']
    for k in OUTPUTS:
        _same(whole[k], np.concatenate([p[k] for p in parts]), k)
    _same(ao, a, 'sanitised actions')
    _same(eo, e, 'final state')


def test_envs_outside_the_lean_domain_beside_running_trios(hip):
    """envs 0, 4 and 8 take rollout_generic through the verdict and write their own crops; the others are rebuilt"""
    envs, actions = _irregular_batch()
    out, _ = _four_ways(hip, envs, actions, 'partial_2', seed=21, call=50)
    assert _b(out, 'done')[:, [1, 2, 3, 5, 6, 7]].any(), 'the oracle: no reset among the trios'


def test_recorded_reference_tape_injected(hip):
    """tests/golden/single_s9_partial2.npz, the real reference's 48 envs x 150 steps with its random outcomes injected,
    through rollout_s9_kernel<partial, INJ, PAIR, CROPH, 2>, against the reference's record"""
    from wurm_amd import _lib
    fx = replay.load('single_s9_partial2')
    assert int(fx['meta'][2]) > 128      # three chunks
    with _lib.knobs(**KNOBS['trio']):
        replay.replay_single_rollout(hip(), fx)
        assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected' and _form() == FORM['trio']
