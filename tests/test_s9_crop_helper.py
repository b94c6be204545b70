"""GPU parity for the form of `rollout_s9_kernel`'s pair whose helper wave renders the crops (CROPH,
wurm_amd/csrc/single_kernels.hpp): launches of at least WURM_S9_CROP_HELPER_MIN_STEPS steps, `partial_n`, at most
WURM_S9_PAIR_MAX_ENVS envs.  The stepping wave records per step what the crop is a function of (move entry, head code, the
food code shown, the body mask without the head); the helper renders each 64-step chunk one chunk behind, and the last
chunk after the last barrier.

Every case forces the form through the knob (1: every launch), asserts through wurm_single_last_crop_wave() that it ran,
and compares bit for bit with the CPU oracle AND with the one-wave form on observations, rewards, dones, both collision
flags, the sanitised tape and the final state.

What a 9 x 9 game cannot show: a new snake has three cells and its head is at least two cells from the ring (the seed cell
is the centre), so with drawn resets no collision falls on the step right after a reset.  The edge collision right after a
reset is therefore built with injected resets (seed cells beside each of the four sides, through the INJ instantiation); a
self collision right after a reset does not exist."""
import numpy as np
import pytest

from tests import replay
from tests.backends import OracleBackend
from tests.test_s9_step_loop import MOVES, _pilot_tape

pytestmark = pytest.mark.gpu

S = 9
PAIR_KNOB, CROP_KNOB = 'WURM_S9_PAIR_MAX_ENVS', 'WURM_S9_CROP_HELPER_MIN_STEPS'
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


def _tape(seed, T, N):
    return np.random.RandomState(seed).randint(0, 4, size=(T, N)).astype(np.int64)


def _form():
    """(waves per env, the wave that rendered the crops) of the calling thread's last launch"""
    from wurm_amd import _lib
    return _lib.lib().wurm_single_last_waves_per_env(), _lib.lib().wurm_single_last_crop_wave()


def _knobs(form):
    """'helper': the pair form whose helper renders the crops, for every launch length; 'one': one wave per env"""
    from wurm_amd import _lib
    return _lib.knobs(**({PAIR_KNOB: 1 << 20, CROP_KNOB: 1} if form == 'helper' else {PAIR_KNOB: 0, CROP_KNOB: -1}))


def _launch(backend, envs, actions, mode, form, **inject):
    """one rollout launch of `backend` in `form` ('helper' / 'one'; None: the oracle) on copies of envs / actions"""
    from wurm_amd import _lib
    e, a = envs.copy(), actions.copy()
    if form is None:
        return backend.single_rollout(e, a, mode, **inject), e, a
    with _knobs(form):
        n0 = _lib.lib().wurm_launch_count()
        out = backend.single_rollout(e, a, mode, **inject)
        assert _lib.lib().wurm_launch_count() - n0 == 1
        assert _form() == ((2, 1) if form == 'helper' else (1, 0)), f'{_form()} ran, {form} was meant to'
    return out, e, a


def _three_ways(hip, envs, actions, mode, seed=0, call=1, **inject):
    """oracle == helper-crop form == one-wave form on every output, the tape and the final state; returns the oracle's"""
    results = []
    for form in (None, 'helper', 'one'):
        b = OracleBackend(seed=seed) if form is None else hip(seed=seed)
        b.call = call
        results.append(_launch(b, envs, actions, mode, form, **inject))
    (ro, eo, ao) = results[0]
    for name, (r, e, a) in zip(('helper-crop form', 'one-wave form'), results[1:]):
        for k in OUTPUTS:
            _same(ro[k], r[k], f'{name}: {k}')
        _same(ao, a, f'{name}: sanitised actions')
        _same(eo, e, f'{name}: final state')
    return ro, eo


def _events_after_the_first_chunk(out, names):
    late = {k: int(np.asarray(out[k][64:]).astype(bool).sum()) for k in names}
    assert all(late.values()), f"the oracle's trajectory lacks an event after step 64: {late}"


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 127, 128, 129, 193, 256])
def test_chunk_edges_buffer_parities_and_tails(hip, T):
    """every chunk edge, both record-buffer parities, odd and even tails of the two-steps-per-pass renderer, the lone last chunk"""
    N = 3
    envs = _fresh(OracleBackend(seed=T), N)
    out, _ = _three_ways(hip, envs, _tape(T, T, N), 'partial_2', seed=T, call=7 + T)
    assert out['obs'].shape[:2] == (T, N)


@pytest.mark.parametrize('mode', ['partial_1', 'partial_2', 'partial_3'])
def test_observation_modes(hip, mode):
    """partial_3 has 49 window cells, more than half a wave: one step per pass"""
    N, T = 9, 129
    envs = _fresh(OracleBackend(seed=5), N)
    out, _ = _three_ways(hip, envs, _tape(31, T, N), mode, seed=5)
    _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'done'))


@pytest.mark.parametrize('N,seed', [(9, 9), (70, 70)])
def test_events_after_the_first_chunk(hip, N, seed):
    """random tapes on which the oracle alone shows eat, edge collision, self collision and done after step 64"""
    T = 129
    envs = _fresh(OracleBackend(seed=seed), N)
    out, _ = _three_ways(hip, envs, _hunting_tape(seed, envs, T), 'partial_2', seed=seed)
    _events_after_the_first_chunk(out, ('reward', 'edge_collision', 'self_collision', 'done'))


def _hunting_tape(seed, envs, T):
    """the piloted tape of tests/test_s9_step_loop.py for the first six envs (long snakes that turn into themselves or the
    wall late in each chunk), random actions for the others"""
    tape = _tape(seed, T, envs.shape[0])
    tape[:, :6] = _pilot_tape(seed, envs[:6], T)
    return tape


# ---- piloted tapes: an event of each kind ON the first and the last step of a chunk, and the eating step right after a reset

def _placed_tape(seed, envs, T):
    """A tape flown on the oracle one step at a time.  Env i wants events of kind i % 3 (0: edge collision with side
    (i // 3) % 4 of the ring — top, left, bottom, right —, 1: self collision, 2: eating) on the steps t with t % 64 in
    (63, 0) and on the step after a reset; in between it gets into position: along the wanted side, long and curled up,
    or one step from the food on the right beat."""
    o = OracleBackend(seed=seed)
    o.call = 1
    e = envs.copy()
    N = e.shape[0]
    tape = np.zeros((T, N), np.int64)
    after_reset = np.zeros(N, bool)
    for t in range(T):
        phase = t % 64
        want = phase in (63, 0)
        to_go = min((63 - phase) % 64, (64 - phase) % 64)    # steps until the next wanted one
        for i in range(N):
            kind, side = i % 3, (i // 3) % 4
            hy, hx = np.argwhere(e[i, 1] > 0)[0]
            fy, fx = np.argwhere(e[i, 0] > 0)[0]
            body, L = e[i, 2], e[i, 2].max()
            cells = {a: (hy + dy, hx + dx) for a, (dy, dx) in MOVES.items()}
            inside = {a: 1 <= y <= S - 2 and 1 <= x <= S - 2 for a, (y, x) in cells.items()}
            neck = {a: body[cells[a]] == L - 1 for a in cells}          # a reversal: sanitised to "straight on"
            safe = [a for a in cells if inside[a] and body[cells[a]] <= 1 and not neck[a]]
            food_d = lambda a: abs(cells[a][0] - fy) + abs(cells[a][1] - fx)
            plain = [a for a in safe if food_d(a) > 0] or safe
            hunt = min(safe, key=food_d) if safe else 0
            if kind == 0:
                wall_d = lambda a: (cells[a][0], cells[a][1], S - 1 - cells[a][0], S - 1 - cells[a][1])[side]
                into = [a for a in cells if not neck[a] and not inside[a] and wall_d(a) == 0]
                a = into[0] if want and into else min(plain, key=wall_d) if plain else hunt
            elif kind == 1:
                hits = [a for a in cells if inside[a] and body[cells[a]] >= 2 and not neck[a]]
                near = lambda a: -sum(1 for dy, dx in MOVES.values() if body[cells[a][0] + dy, cells[a][1] + dx] >= 3 + to_go)
                a = hits[0] if want and hits else hunt if L < 12 or to_go > 6 else min(plain, key=near) if plain else hunt
            else:
                eats = [a for a in safe if food_d(a) == 0]
                if (want or after_reset[i]) and eats:
                    a = eats[0]
                elif to_go > 12:
                    a = hunt if not eats or len(safe) == 1 else min(plain, key=food_d)
                else:   # arrive beside the food with the beat: the distance after this move should be what is left to go
                    a = min(plain, key=lambda b: abs(food_d(b) - to_go)) if plain else hunt
            tape[t, i] = a
        done = o.single_step(e, tape[t].copy(), 'none')[2]
        o.single_reset(e, done, 'none')
        after_reset = np.asarray(done).astype(bool)
    return tape


def _heads_before(envs, actions, seed):
    """the head cell of every env before each step of the oracle's trajectory: (T, N, 2)"""
    o = OracleBackend(seed=seed)
    o.call = 1
    e, heads = envs.copy(), []
    for t in range(actions.shape[0]):
        heads.append([np.argwhere(e[i, 1] > 0)[0] for i in range(e.shape[0])])
        done = o.single_step(e, actions[t].copy(), 'none')[2]
        o.single_reset(e, done, 'none')
    return np.asarray(heads)


def test_piloted_events_on_chunk_edges(hip):
    """edge collisions with each of the four sides, self collisions and eating steps on the first and on the last step of a
    chunk, an eating step right after a reset — all on the oracle's own trajectory, checked before anything is compared"""
    N, T, seed = 36, 258, 3
    envs = _fresh(OracleBackend(seed=seed), N)
    actions = _placed_tape(seed, envs, T)
    out, _ = _three_ways(hip, envs, actions, 'partial_2', seed=seed)
    heads = _heads_before(envs, actions, seed)
    first, last = np.arange(T) % 64 == 0, np.arange(T) % 64 == 63
    first[0] = False                             # (chunk 0's first step follows no other chunk)
    edge, selfc, ate = (np.asarray(out[k]).astype(bool) for k in ('edge_collision', 'self_collision', 'reward'))
    done = np.asarray(out['done']).astype(bool)
    missing = []
    for name, when in (('first', first), ('last', last)):
        for kind, ev in (('self collision', selfc), ('eating step', ate)):
            if not ev[when].any():
                missing.append(f'{kind} on the {name} step of a chunk')
        for side in range(4):
            # the side the head ran into: it stood on the interior line beside it and the env is one that aims at that side
            line = (heads[..., 0] == 1, heads[..., 1] == 1, heads[..., 0] == S - 2, heads[..., 1] == S - 2)[side]
            aims = ((np.arange(N) // 3) % 4 == side) & (np.arange(N) % 3 == 0)
            if not (edge & line & aims[None, :])[when].any():
                missing.append(f'edge collision with side {side} on the {name} step of a chunk')
    if not (ate[1:] & done[:-1]).any():
        missing.append('eating step right after a reset')
    assert not missing, f"the oracle's trajectory lacks: {missing}"


def test_a_new_snake_can_collide_with_nothing_on_its_first_step():
    """what the docstring above rests on, on the oracle: a drawn reset gives three body cells and a head at least two cells
    from the ring, so neither collision can fall on the step right after a reset"""
    N = 512
    for seed in range(4):
        envs = _fresh(OracleBackend(seed=seed), N)
        assert ((envs[:, 2] > 0).sum(axis=(1, 2)) == 3).all()
        _, ys, xs = np.nonzero(envs[:, 1])
        assert len(ys) == N and min(ys.min(), xs.min(), S - 1 - ys.max(), S - 1 - xs.max()) >= 2


def test_edge_collision_on_every_step_with_injected_resets(hip):
    """Injected resets put every new snake beside a side of the ring, heading for it, and the tape walks it into the ring:
    an edge collision and a reset on EVERY step — the first and the last step of each chunk, the step right after a reset —
    with the head on each of the four sides and in both corners' neighbourhoods, where its code wraps."""
    T, seed = 130, 2
    # (seed row, seed column, direction, action that moves on in that direction): the head is seed + TAP[direction]
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
    out, _ = _three_ways(hip, envs, actions, 'partial_2', seed=seed, inject_food=inject_food, inject_reset=inject_reset)
    assert np.asarray(out['edge_collision']).astype(bool).all(), 'the oracle: not every step runs into the ring'
    from wurm_amd import _lib
    assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected'


def test_recorded_reference_tape_injected(hip):
    """tests/golden/single_s9_partial2.npz — 48 envs x 150 steps of the real reference, its random outcomes injected —
    through rollout_s9_kernel<partial, INJ, PAIR, CROPH>, against the reference's record"""
    from wurm_amd import _lib
    fx = replay.load('single_s9_partial2')
    assert int(fx['meta'][2]) > 128      # three chunks
    with _knobs('helper'):
        replay.replay_single_rollout(hip(), fx)
        assert _lib.lib().wurm_single_last_route().decode() == 'rollout_s9_injected' and _form() == (2, 1)


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
    return envs, _tape(8, 129, N)


def test_envs_outside_the_lean_domain_beside_running_pairs(hip):
    """the steppers of envs 0, 4 and 8 take the generic path (which writes its own crops) and their helpers leave after the
    first barrier; the six others run as pairs in the same launch, 9 workgroups being no multiple of the XCD count"""
    envs, actions = _irregular_batch()
    _three_ways(hip, envs, actions, 'partial_2', seed=21, call=50)


def test_chained_launches(hip):
    """two launches of 129 and 65 steps carry state and call counter on and equal the oracle's single launch of 194"""
    N, seed, call = 9, 23, (1 << 40) + 3
    actions = _tape(4, 194, N)
    o = OracleBackend(seed=seed)
    o.call = call
    envs = _fresh(OracleBackend(seed=seed), N)
    eo, ao = envs.copy(), actions.copy()
    whole = o.single_rollout(eo, ao, 'partial_2')
    _events_after_the_first_chunk(whole, ('reward', 'edge_collision', 'done'))
    for form in ('helper', 'one'):
        h = hip(seed=seed)
        h.call = call
        e, a = envs.copy(), actions.copy()
        with _knobs(form):
            first = h.single_rollout(e, a[:129], 'partial_2')
            assert _form() == ((2, 1) if form == 'helper' else (1, 0))
            second = h.single_rollout(e, a[129:], 'partial_2')
            assert _form() == ((2, 1) if form == 'helper' else (1, 0))
        for k in OUTPUTS:
            _same(whole[k], np.concatenate([first[k], second[k]]), f'{form}: {k}')
        _same(ao, a, f'{form}: sanitised actions')
        _same(eo, e, f'{form}: final state')


def test_the_knob_by_launch_length(hip):
    """T below the knob runs the pair form with the crop in the stepper, T at it the helper's; no observation: never"""
    from wurm_amd import _lib
    N = 3
    h = hip(seed=1)
    envs = _fresh(h, N)
    with _lib.knobs(**{PAIR_KNOB: 1 << 20, CROP_KNOB: 65}):
        for T, mode, form in ((64, 'partial_2', (2, 0)), (65, 'partial_2', (2, 1)), (65, 'none', (2, 0))):
            h.single_rollout(envs.copy(), _tape(1, T, N), mode)
            assert _form() == form, (T, mode)
    with _lib.knobs(**{PAIR_KNOB: 1 << 20, CROP_KNOB: -1}):
        h.single_rollout(envs.copy(), _tape(1, 65, N), 'partial_2')
        assert _form() == (2, 0)
