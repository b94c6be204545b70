"""GPU parity for the trio form of `rollout_s9_kernel` once its render waves rebuild the BODY MASK of every step as well
(wurm_amd/csrc/single_kernels.hpp, REBUILD; single_device.hpp, s9_rebuild_body): the stepper records per step the move entry
alone and hands over per chunk the clocks, the length and the codes it entered the chunk with.  A render wave takes the body
of step j from the head's trail — the cells the head stood on during the last `length - 1` steps —, clipped at the last
reset's three seed cells, and before the chunk's first reset from the chunk-start clocks as well.

What can go wrong there is the length of the window (eating steps, also right after a reset and across a chunk edge), where it
is clipped (resets on the first and last steps of a chunk, resets closer together than a new snake is long) and what the chunk
started with (long snakes whose body reaches back across one or two chunk starts, a launch that starts from a long snake).

Every case forces the forms through the knobs as tests/test_s9_trio_rollout.py does and compares the trio form bit for bit
with the CPU oracle and with the `helper` and `one` forms of the same library: observations, rewards, dones, both collision
flags, the sanitised tape and the final state.  Every case asserts on the ORACLE's outputs that the events it exists for did
happen, and how often, before anything is compared.  The piloted tapes are those of tests/test_s9_record_rebuild.py: closed
loops of interior cells, every random outcome injected."""
import numpy as np
import pytest

from tests.backends import OracleBackend
from tests.test_s9_crop_helper import OUTPUTS, S, _fresh, _irregular_batch, _same, _tape
from tests.test_s9_record_rebuild import PARK, PERIMETER, SERPENTINE, STARTS, _b, _fly, _injected
from tests.test_s9_step_loop import MOVES
from tests.test_s9_trio_rollout import FORM, KNOBS, _form, _four_ways

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


# ---- random tapes

@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 128, 129, 257])
def test_chunk_edges_random_tape(hip, T):
    """every chunk edge and tail; from T = 65 on a chunk starts from clocks the stepper handed over, from 129 on in both
    record-buffer parities"""
    N = 5
    envs = _fresh(OracleBackend(seed=140 + T), N)
    out, _ = _four_ways(hip, envs, _tape(140 + T, T, N), 'partial_2', seed=140 + T, call=11 + T)
    assert out['obs'].shape[:2] == (T, N)
    if T >= 128:
        done, ate = _b(out, 'done'), _b(out, 'reward')
        assert done.sum() >= 2 and ate.sum() >= 2, f"the oracle's trajectory: {done.sum()} resets, {ate.sum()} eating steps"
        assert done[64:].any() and ate[64:].any(), 'the oracle: no event after the first chunk'


@pytest.mark.parametrize('mode', ['partial_1', 'partial_2', 'partial_3'])
def test_observation_modes(hip, mode):
    """two steps per pass (9 and 25 window cells) and one (49): the pass reads the rebuilt mask of its own step"""
    N, T = 70, 129
    envs = _fresh(OracleBackend(seed=16), N)
    out, _ = _four_ways(hip, envs, _tape(132, T, N), mode, seed=16)
    late = {k: int(_b(out, k)[64:].sum()) for k in ('reward', 'edge_collision', 'self_collision', 'done')}
    assert late['reward'] and late['edge_collision'] and late['done'], f"the oracle's trajectory lacks an event after step 64: {late}"


# ---- piloted tapes with injected outcomes

def _long_lives(T):
    """Env 0 grows to 36 of the serpentine's 38 cells (33 eating steps, every second step), walks on at full length across the
    chunk starts at 128 and 192 and turns into its own body from step 215 on.  Env 1 grows to 23 cells and runs into the
    ring on step 76 (its head is on row 1 then); its successors on the perimeter eat on steps 63 and 0 of a chunk, on
    consecutive steps and right after a reset, and die on steps 63, 0 and 1 of a chunk (three resets in a row), on steps 62
    and 63.  Env 2's lives end on steps 0 and 1 of a chunk, on step 62 and on step 63, in both record-buffer parities."""
    schedules = [
        {2 * k: 'eat' for k in range(33)},
        {2 * k: 'eat' for k in range(20)},
        {0: 'eat', 1: 'eat', 12: 'eat', 24: 'eat', 36: 'eat', 48: 'eat', 62: 'edge', 63: 'eat', 64: 'edge', 65: 'edge', 66: 'eat',
         67: 'eat', 80: 'eat', 94: 'eat', 108: 'eat', 120: 'eat', 126: 'edge', 127: 'edge', 128: 'eat', 129: 'eat', 130: 'edge',
         131: 'edge', 140: 'eat', 152: 'eat', 164: 'eat', 176: 'eat', 190: 'eat', 191: 'eat', 192: 'eat', 193: 'edge', 194: 'eat',
         254: 'edge', 255: 'eat', 256: 'eat'},
    ]
    schedules[0][215] = 'self'
    schedules[1].update({76: 'edge', 90: 'eat', 100: 'eat', 112: 'eat', 127: 'eat', 128: 'eat', 129: 'eat', 140: 'edge', 141: 'eat',
                         191: 'edge', 192: 'edge', 193: 'edge', 194: 'eat', 254: 'edge', 255: 'edge', 256: 'eat'})
    long = _fly([(1, 2, 1)] * 2, schedules[:2], T, SERPENTINE, seed=3)
    short = _fly(STARTS[4:5], schedules[2:], T, PERIMETER, seed=3)
    envs, actions, inject_food, inject_reset = (np.concatenate([a, b], axis=ax) for a, b, ax in zip(long, short, (0, 1, 1, 1)))
    return schedules, envs, actions, inject_food, inject_reset


@pytest.fixture(scope='module')
def long_lives():
    """flown once on the oracle and shared; the tests copy what they launch on"""
    return _long_lives(257)


def _assert_long_lives(out, schedules):
    selfc, edge, ate, done = _b(out, 'self_collision'), _b(out, 'edge_collision'), _b(out, 'reward'), _b(out, 'done')
    for i in (1, 2):                         # the oracle's trajectory is the schedule, step for step
        assert np.flatnonzero(edge[:, i]).tolist() == sorted(t for t in schedules[i] if schedules[i][t] == 'edge'), i
        assert np.flatnonzero(ate[:, i]).tolist() == sorted(t for t in schedules[i] if schedules[i][t] == 'eat'), i
    died0 = np.flatnonzero(selfc[:, 0]).tolist()
    assert len(died0) == 1 and 215 <= died0[0] < 257 and not edge[:, 0].any(), died0
    assert ate[:died0[0], 0].sum() == 33 and died0[0] - 66 > 128, 'a snake of 36 cells that crosses two chunk starts at full length'
    assert ate[:76, 1].sum() == 20 and edge[76, 1] and not done[:76, 1].any(), 'a snake of 23 cells runs into the ring'
    assert not selfc[:, 1:].any()
    # resets on steps 63, 0, 1 of a chunk (three in a row), 62 and 63, 0 and 1, 62 alone; in chunks of both parities
    assert done[[191, 192, 193, 254, 255], 1].all() and done[[62, 64, 65, 126, 127, 130, 131, 193, 254], 2].all()
    # eating steps on steps 63 and 0 of a chunk, on consecutive steps, right after a reset
    assert ate[[127, 128, 129], 1].all() and ate[[63, 128, 129, 191, 192, 255, 256], 2].all() and ate[[0, 64], 0].all()
    assert (ate[1:] & done[:-1]).sum() >= 6, 'eating steps right after a reset'
    assert (ate[1:] & ate[:-1]).sum() >= 8, 'eating steps on two consecutive steps'


@pytest.mark.parametrize('mode', ['partial_2', 'partial_3'])
def test_long_snakes_resets_and_eating_steps_on_chunk_edges(hip, long_lives, mode):
    schedules, envs, actions, inject_food, inject_reset = long_lives
    out = _injected(hip, mode, envs, actions, inject_food, inject_reset, seed=3)
    _assert_long_lives(out, schedules)


def test_chained_launches_of_long_snakes(hip, long_lives):
    """100 + 60 + 97 steps: the second and third launch start from a snake of 36 cells that the launch before wrote back, so
    the clocks of their first chunk come from the load; the chunk edges fall on other steps of every life than in one launch"""
    from wurm_amd import _lib
    schedules, envs, actions, inject_food, inject_reset = long_lives
    eo, ao = envs.copy(), actions.copy()
    whole = OracleBackend(seed=3).single_rollout(eo, ao, 'partial_2', inject_food=inject_food, inject_reset=inject_reset)
    _assert_long_lives(whole, schedules)
    h = hip(seed=3)
    e, a = envs.copy(), actions.copy()
    parts = []
    with _lib.knobs(**KNOBS['trio']):
        for lo, hi in ((0, 100), (100, 160), (160, 257)):
            parts.append(h.single_rollout(e, a[lo:hi], 'partial_2', inject_food=inject_food[lo:hi], inject_reset=inject_reset[lo:hi]))
            assert _form() == FORM['trio'] and _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected'
    for k in OUTPUTS:
        _same(whole[k], np.concatenate([p[k] for p in parts]), k)
    _same(ao, a, 'sanitised actions')
    _same(eo, e, 'final state')


def _placed(lengths, T, eat_at, turn_from):
    """Snakes laid by hand along the serpentine, env i with lengths[i] cells and its head on cell lengths[i] - 1 of the loop,
    the food on the cell its first eating step reaches.  They walk the loop, eat on the steps of eat_at[i] and, from step
    turn_from[i] on, turn into their own body as soon as they can; a successor walks the perimeter.  Flown on the oracle one
    step at a time; returns (envs, actions, inject_food, inject_reset, schedules as they came out)."""
    N = len(lengths)
    envs = np.zeros((N, 3, S, S), np.float32)
    inject_food = np.full((T, N), -1, np.int32)
    inject_reset = np.zeros((T, N, 4), np.int32)
    actions = np.zeros((T, N), np.int64)
    loops = [SERPENTINE] * N

    def food_for(i, head_after, t_now):
        coming = sorted(t for t in eat_at[i] if t > t_now)
        if loops[i] is SERPENTINE and coming:
            return SERPENTINE[(SERPENTINE.index(head_after) + coming[0] - t_now) % len(SERPENTINE)]
        return PARK[id(loops[i])]

    for i, L in enumerate(lengths):
        for k in range(L):
            envs[i, 2][SERPENTINE[k]] = k + 1
        envs[i, 1][SERPENTINE[L - 1]] = 1
        envs[i, 0][food_for(i, SERPENTINE[L - 1], -1)] = 1
    assert (envs[:, 0] * envs[:, 2]).sum() == 0 and (OracleBackend(seed=0).single_check(envs) == 0).all()
    o = OracleBackend(seed=5)
    e = envs.copy()
    died = [None] * N
    for t in range(T):
        for i in range(N):
            loop = loops[i]
            hy, hx = (int(v) for v in np.argwhere(e[i, 1] > 0)[0])
            body, L = e[i, 2], e[i, 2].max()
            nxt = loop[(loop.index((hy, hx)) + 1) % len(loop)]
            cells = {a: (hy + dy, hx + dx) for a, (dy, dx) in MOVES.items()}
            a = next(a for a, c in cells.items() if c == nxt)
            if died[i] is None and t >= turn_from[i]:
                hits = [a for a, c in cells.items() if 1 <= c[0] <= 7 and 1 <= c[1] <= 7 and 2 <= body[c] < L - 1]
                if hits:
                    a, died[i] = hits[0], t
            actions[t, i] = a
            target = cells[a]
            if body[target] >= 2:
                loops[i] = PERIMETER
                sy, sx, d = STARTS[i % len(STARTS)]
                inject_reset[t, i] = (sy, sx, d, PARK[id(PERIMETER)][0] * S + PARK[id(PERIMETER)][1])
            elif e[i, 0][target] > 0:
                assert t in eat_at[i], f'env {i} eats on step {t}'
                fy, fx = food_for(i, target, t)
                inject_food[t, i] = fy * S + fx
            else:
                assert t not in eat_at[i] or died[i] is not None, f'env {i}: no food where step {t} should eat'
        done = o.single_step(e, actions[t].copy(), 'none', inject_food=inject_food[t])[2]
        o.single_reset(e, done, 'none', inject_reset=inject_reset[t])
    return envs, actions, inject_food, inject_reset, died


@pytest.mark.parametrize('mode', ['partial_2', 'partial_3'])
def test_a_launch_that_starts_from_long_snakes_laid_by_hand(hip, mode):
    """no reset made these snakes: the clocks of chunk 0 are what the launch loaded.  30, 12 and 8 cells (the food of an
    eating step lies on the loop ahead of the head, on a cell the body has left free, so the first eating steps come early):
    the body of the first is partly what the launch began with for 30 steps, the second eats on steps 0 and 1, the third
    on steps 63 and 64 as well; all end in a self collision"""
    T = 129
    eat_at = [{2, 4}, {0, 1, 5}, {3, 30, 50, 63, 64}]
    envs, actions, inject_food, inject_reset, died = _placed([30, 12, 8], T, eat_at, [100, 30, 70])
    out = _injected(hip, mode, envs, actions, inject_food, inject_reset, seed=5)
    selfc, ate, done = _b(out, 'self_collision'), _b(out, 'reward'), _b(out, 'done')
    for i in range(3):
        assert died[i] is not None and np.flatnonzero(selfc[:, i]).tolist() == [died[i]] and (done[:, i] == selfc[:, i]).all(), died
        assert np.flatnonzero(ate[:, i]).tolist() == sorted(eat_at[i]), i
    assert died[0] >= 100 and died[1] >= 30 and died[2] >= 70, died


def test_envs_outside_the_lean_domain_beside_running_trios(hip):
    """envs 0, 4 and 8 take rollout_generic through the verdict and write their own crops (there is no record to rebuild
    from, and the render waves leave); the others are rebuilt"""
    envs, actions = _irregular_batch()
    out, _ = _four_ways(hip, envs, actions, 'partial_2', seed=21, call=50)
    done, ate = _b(out, 'done'), _b(out, 'reward')
    lean = [1, 2, 3, 5, 6, 7]
    assert done[:, lean].any() and ate[:, lean].any() and done[64:, lean].any(), 'the oracle: no reset among the trios'
