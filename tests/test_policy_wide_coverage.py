"""policy_wide_kernel over its whole launch space, bit for bit against the oracle (every output and the final state),
from start states in which the game happens (tests/policy_states.py).

tests/test_policy_rollout_wide.py compares the same way; what it leaves out is here:
  * all 16 instantiations policy_wide_kernel<CPL, SNAKE>: both edge sizes of each of the 8 cells-per-lane buckets
    (cpl_of: S 9-11 -> 2, 12-16 -> 4, 17-22 -> 8, 23-32 -> 16, 33-39 -> 24, 40-45 -> 32, 46-55 -> 48, 56-64 -> 64), for
    snake partial_n, snake positions and gridworld positions (EDGE_CASES);
  * every workgroup shape launch_policy_wide_cpl can choose: wpb = min(fit, most, ceil(N / 256)) waves, 1..8 below
    bucket 48 and 1..4 from there on, a partly empty last workgroup, and the launches in which the 160 KiB of LDS
    (fit) or the register bound (most) set wpb (SHAPE_CASES; the test cannot see wpb, the comments state the value
    each case is meant to give and profiles/r08_policy_wide_coverage.txt records what rocprofv3 saw);
  * the edges of the 64-step output chunks (T = 1, 63, 64, 65, 128, 129), Philox keys with non-zero high halves
    (call0 >= 2^33, crossing a 32-bit carry inside the launch; env_offset >= 2^40) and a second launch that continues
    from the first (CHUNK_CASES);
  * near-uniform (scale 0.05), saturated (scale 1 and 3: probabilities of exactly 0) and hand-built one-hot policies,
    and boards with 2 to 4 free cells (EVENT_CASES).
Every case first asserts on the ORACLE's outputs that the run is not empty (_floor): a condition on the inputs, met by
the choice of seeds and shares, never relaxed for a case — a case that cannot meet it does not belong in the list."""
import numpy as np
import pytest

from oracle import oracle as O
from wurm_amd import _lib
from tests import policy_states as PS
from tests.test_policy_rollout_wide import _same, hip_rollout, oracle_composed

EVENT_KEYS = ('self_collision', 'edge_collision', 'reward', 'done')


def _obs_size(mode):
    return 4 if mode == 'positions' else 3 * (2 * int(mode.split('_')[1]) + 1) ** 2


def make_case(family, S, mode, N, T, weights, seed, states='filled', call0=1, off=0, launches=1, floor='active'):
    """family 'snake' | 'grid'; weights: a scale for random normal parameters, or ('straight', action); states 'filled'
    (snake_states / grid_states) | 'crowded' | 'fresh' (a reset); floor 'active' | 'events' (+ '+uniform')"""
    return dict(family=family, S=S, mode=mode, N=N, T=T, weights=weights, seed=seed, states=states, call0=call0, off=off,
                launches=launches, floor=floor)


def case_id(c):
    w = c['weights'] if not isinstance(c['weights'], tuple) else 'straight%d' % c['weights'][1]
    return f"{c['family']}-S{c['S']}-{c['mode']}-N{c['N']}-T{c['T']}-{c['states']}-w{w}"


def build_inputs(c):
    """(envs, obs0, params, grid start or None) of a case, from its seed alone"""
    rng = np.random.RandomState(c['seed'])
    S, N, E = c['S'], c['N'], _obs_size(c['mode'])
    if c['family'] == 'snake':
        grid = None
        if c['states'] == 'fresh':
            envs = np.zeros((N, 3, S, S), np.float32)
            O.single_reset(envs, np.ones(N, np.uint8), 'none', c['seed'], 0, c['off'])
        elif c['states'] == 'crowded':
            envs = PS.crowded_snake_states(N, S, rng, near_food=0.7)
        else:
            envs = PS.snake_states(N, S, rng, fill=0.5, near_food=0.6)
        assert (O.single_check(envs) == 0).all()
        obs0 = O.single_observe(envs, c['mode'])
    else:
        grid = (int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1)))
        envs = PS.grid_states(N, S, rng, near_food=0.7)
        assert (PS.grid_check(envs) == 0).all()
        obs0 = O.grid_observe(envs, 'positions')
    if isinstance(c['weights'], tuple):
        params = PS.straight_params(E, c['weights'][1])
    else:
        params = (rng.randn(O.policy_param_count(E)) * c['weights']).astype(np.float32)
    return envs, np.asarray(obs0, np.float32).reshape(N, E), params, grid


def oracle_launches(c, envs, obs0, params, grid):
    """the case's launches on the oracle (envs updated in place): list of output dicts, launch k + 1 acting on the last
    observation of launch k with the call counter moved on by 2 T"""
    outs, x, call = [], obs0, c['call0']
    for _ in range(c['launches']):
        if c['family'] == 'snake' and c['mode'] != 'positions':
            ro = O.single_policy_rollout(envs, x, params, c['T'], obs_n=int(c['mode'].split('_')[1]), seed=c['seed'],
                                         call0=call, env_offset=c['off'])
        else:
            ro = oracle_composed(envs, x, params, c['T'], c['seed'], call, c['off'], c['mode'], grid)
        outs.append(ro)
        x, call = ro['obs'][-1], call + 2 * c['T']
    return outs


def count_events(c, start, outs):
    ev = {k: int(sum(o[k].sum() for o in outs if k in o)) for k in EVENT_KEYS}
    ev['actions'] = len(np.unique(np.concatenate([o['actions'].ravel() for o in outs])))
    ev['exact_zero_probs'] = int(sum((o['probs'] == 0).sum() for o in outs))
    if c['family'] == 'snake':
        ev['start_length'] = int(start[:, 2].max())
    return ev


def _floor(c, ev):
    """what the ORACLE's run must contain before it is worth comparing the GPU with it"""
    kind = c['floor'].split('+')
    assert ev['reward'] + ev['done'] >= 1, ev
    if 'events' in kind:
        assert ev['reward'] >= 1 and ev['edge_collision'] >= 1 and ev['done'] >= 1, ev
        if c['family'] == 'snake':
            assert ev['self_collision'] >= 1 and ev['start_length'] >= 20, ev
    if 'uniform' in kind:
        assert ev['actions'] == 4, ev
    if 'saturated' in kind:
        assert ev['exact_zero_probs'] >= 1, ev


def run_case(c):
    lib = _lib.lib()
    envs, obs0, params, grid = build_inputs(c)
    eo, eh = envs.copy(), envs.copy()
    outs = oracle_launches(c, eo, obs0, params, grid)
    ev = count_events(c, envs, outs)
    print(case_id(c), ev)
    _floor(c, ev)
    x, call = obs0, c['call0']
    for k, ro in enumerate(outs):
        rh = hip_rollout(eh, x, params, c['T'], c['seed'], call, c['off'], c['mode'], grid)
        assert lib.wurm_policy_last_route() == b'policy_wide'
        assert (rh.pop('status') == 0).all(), 'every generated state must be accepted'
        assert set(rh) == set(ro)
        for key in ro:
            _same(ro[key], rh[key], f'launch {k} {key}')
        x, call = ro['obs'][-1], call + 2 * c['T']
    _same(eo, eh, 'final state')


# ------------------------------------------------------------------------------------------- every instantiation
# Both edge sizes of each bucket.  The crops spread n over 0..6 so that each n meets a small bucket and a large one
# (n = 0: E = 3, EP = 16, 13 of 16 inputs padding; (9, 4) and (11, 6): the old kernels' sizes on this one).
# Weights alternate between near-uniform (0.05: all four actions must be drawn) and saturated.
EDGE_SIZES = [9, 11, 12, 16, 17, 22, 23, 32, 33, 39, 40, 45, 46, 55, 56, 64]
EDGE_N = {9: 4, 11: 6, 12: 0, 16: 2, 17: 5, 22: 1, 23: 3, 32: 6, 33: 0, 39: 4, 40: 6, 45: 5, 46: 2, 55: 3, 56: 1, 64: 6}
EDGE_CASES = []
for _i, _S in enumerate(EDGE_SIZES):
    _w, _fl = (0.05, 'events+uniform') if _i % 2 == 0 else (1.0, 'events')
    EDGE_CASES.append(make_case('snake', _S, f'partial_{EDGE_N[_S]}', 32, 65, _w, 300 + _S, floor=_fl))
    _w, _fl = (0.05, 'events+uniform') if _i % 2 == 1 else (0.3, 'events')
    EDGE_CASES.append(make_case('snake', _S, 'positions', 32, 65, _w, 400 + _S, floor=_fl))
for _i, _S in enumerate([5] + EDGE_SIZES):
    _w, _fl = (0.05, 'events+uniform') if _i % 2 == 0 else (0.3, 'events')
    EDGE_CASES.append(make_case('grid', _S, 'positions', 32, 65, _w, 500 + _S, floor=_fl))


@pytest.mark.gpu
@pytest.mark.parametrize('case', EDGE_CASES, ids=case_id)
def test_every_instantiation(case):
    run_case(case)


# ------------------------------------------------------------------------------------------- every workgroup shape
# wpb = min(fit, most, ceil(N / 256)); N is never a multiple of wpb, so the last workgroup has idle waves that leave
# after the W1 copy and the barrier.  T is small: the launch shape does not depend on it and the oracle is the cost.
SHAPE_CASES = [
    # bucket 8 (S 20), partial_2 (E 75, EP 80): fit 50, most 8              # wpb  block
    make_case('snake', 20, 'partial_2', 37, 5, 0.3, 601),                   #   1     64
    make_case('snake', 20, 'partial_2', 301, 5, 0.3, 602),                  #   2    128
    make_case('snake', 20, 'partial_2', 601, 5, 0.3, 603),                  #   3    192
    make_case('snake', 20, 'partial_2', 803, 5, 0.3, 604),                  #   4    256
    make_case('snake', 20, 'partial_2', 1101, 5, 0.3, 605),                 #   5    320
    make_case('snake', 20, 'partial_2', 1403, 5, 0.3, 606),                 #   6    384
    make_case('snake', 20, 'partial_2', 1601, 5, 0.3, 607),                 #   7    448
    make_case('snake', 20, 'partial_2', 1901, 5, 0.3, 608),                 #   8    512
    # gridworld, bucket 16 (S 30) and bucket 48 (S 50, most 4)
    make_case('grid', 30, 'positions', 301, 5, 0.05, 611),                  #   2    128
    make_case('grid', 30, 'positions', 803, 5, 0.05, 612),                  #   4    256
    make_case('grid', 30, 'positions', 1403, 5, 0.05, 613),                 #   6    384
    make_case('grid', 30, 'positions', 1901, 5, 0.05, 614),                 #   8    512
    make_case('grid', 50, 'positions', 601, 5, 0.05, 615),                  #   3    192
    make_case('grid', 50, 'positions', 1101, 5, 0.05, 616),                 #   4    256 (most)
    # snake, bucket 48 (S 50, partial_1) and bucket 64 (S 64, positions): most 4
    make_case('snake', 50, 'partial_1', 37, 5, 0.3, 621),                   #   1     64
    make_case('snake', 50, 'partial_1', 301, 5, 0.3, 622),                  #   2    128
    make_case('snake', 50, 'partial_1', 601, 5, 0.3, 623),                  #   3    192
    make_case('snake', 50, 'partial_1', 803, 5, 0.3, 624),                  #   4    256
    make_case('snake', 50, 'partial_1', 1101, 5, 0.3, 625),                 #   4    256 (most)
    make_case('snake', 64, 'positions', 301, 5, 0.05, 626),                 #   2    128
    make_case('snake', 64, 'positions', 601, 5, 0.05, 627),                 #   3    192
    make_case('snake', 64, 'positions', 1101, 5, 0.05, 628),                #   4    256 (most)
    # partial_6 (E 507, EP 512: W1 takes 131 072 of the 163 840 bytes of LDS)
    # S 45: 4 336 bytes per wave, fit 7 < ceil(1801 / 256) = 8: LDS sets wpb; 161 424 bytes
    make_case('snake', 45, 'partial_6', 1801, 8, 0.3, 631),                 #   7    448
    # S 40: 3 904 bytes per wave, fit 8: the largest launch, 162 304 bytes
    make_case('snake', 40, 'partial_6', 1795, 8, 0.3, 632),                 #   8    512
    # S 64: 6 400 bytes per wave, fit 5, most 4; 156 672 bytes
    make_case('snake', 64, 'partial_6', 771, 8, 0.3, 633),                  #   4    256
]


def expected_wpb(c):
    """launch_policy_wide_cpl's arithmetic, restated for the CPU test below"""
    S, E = c['S'], _obs_size(c['mode'])
    EP = (E + 15) & ~15
    wave_bytes = EP * 4 + 256 + ((S * S + 15) & ~15)
    fit = (160 * 1024 - EP * 256) // wave_bytes
    most = 4 if (S * S + 63) // 64 > 32 else 8
    wpb = max(1, min(fit, most, (c['N'] + 255) // 256))
    return wpb, EP * 256 + wpb * wave_bytes


def test_shape_cases_cover_every_wpb():
    """CPU: by the launcher's arithmetic the list reaches wpb 1..8 below bucket 48 and 1..4 from there on, every last
    workgroup is ragged, and the three partial_6 launches have the LDS sizes named above"""
    small = {expected_wpb(c)[0] for c in SHAPE_CASES if c['S'] <= 45}
    large = {expected_wpb(c)[0] for c in SHAPE_CASES if c['S'] >= 46}
    assert small == set(range(1, 9)) and large == set(range(1, 5))
    for fam in ('snake', 'grid'):
        assert {expected_wpb(c)[0] for c in SHAPE_CASES if c['family'] == fam} >= {2, 3, 4, 6, 8}
    assert all(c['N'] % expected_wpb(c)[0] for c in SHAPE_CASES if expected_wpb(c)[0] > 1)
    lds = {c['S']: expected_wpb(c) for c in SHAPE_CASES if c['mode'] == 'partial_6'}
    assert lds == {45: (7, 161424), 40: (8, 162304), 64: (4, 156672)}


@pytest.mark.gpu
@pytest.mark.parametrize('case', SHAPE_CASES, ids=case_id)
def test_every_workgroup_shape(case):
    run_case(case)


# ------------------------------------------------------------------------------------------- chunk edges and keys
# Two chained launches each.  call0 = 2^33 + 2^32 - 40: the high half of the call counter is non-zero and the low half
# wraps inside the first launch for T >= 21; env_offset = 2^40 + 3: the same for the env id.
BIG_CALL, BIG_OFF = (1 << 33) + (1 << 32) - 40, (1 << 40) + 3
CHUNK_CASES = [make_case('snake', 25, 'partial_3', 20, T, 0.3, 700 + T, call0=BIG_CALL, off=BIG_OFF, launches=2)
               for T in (1, 63, 64, 65, 128, 129)]
CHUNK_CASES += [make_case('snake', 41, 'positions', 20, T, 0.05, 720 + T, call0=BIG_CALL + 1, off=BIG_OFF, launches=2)
                for T in (64, 128, 129)]
CHUNK_CASES += [make_case('grid', 48, 'positions', 20, T, 0.05, 740 + T, call0=BIG_CALL, off=BIG_OFF + 1, launches=2)
                for T in (1, 63, 64, 65, 128, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CHUNK_CASES, ids=case_id)
def test_chunk_edges_and_keys(case):
    run_case(case)


# ------------------------------------------------------------------------------------------- weights and crowded boards
EVENT_CASES = [
    # one-hot policies (zero weights, one head bias of 100: probabilities exactly 0 and 1): every snake turns one way
    # and runs into the edge, eating what lies in its way — or into the row of its own body next to it
    make_case('snake', 12, 'partial_2', 64, 40, ('straight', 0), 801, floor='events+saturated'),
    make_case('snake', 33, 'partial_4', 64, 70, ('straight', 1), 802, floor='events+saturated'),
    make_case('snake', 46, 'positions', 64, 70, ('straight', 2), 803, floor='events+saturated'),
    make_case('snake', 64, 'partial_1', 64, 130, ('straight', 3), 804, floor='events+saturated'),
    make_case('grid', 40, 'positions', 64, 70, ('straight', 2), 805, floor='events+saturated'),
    # saturated random weights
    make_case('snake', 40, 'partial_5', 64, 65, 3.0, 811, floor='events+saturated'),
    make_case('snake', 56, 'partial_3', 64, 65, 3.0, 812, floor='events+saturated'),
    # 2 to 4 free cells: the respawn after a meal ranks 1 to 3 candidates; the crop is full of body cells
    make_case('snake', 9, 'partial_5', 64, 40, 0.05, 821, states='crowded', floor='events+uniform'),
    make_case('snake', 12, 'partial_2', 64, 40, 0.05, 822, states='crowded', floor='events+uniform'),
    make_case('snake', 23, 'partial_6', 64, 40, 0.05, 823, states='crowded', floor='events+uniform'),
    make_case('snake', 40, 'positions', 64, 40, 0.05, 824, states='crowded', floor='events+uniform'),
    make_case('snake', 47, 'partial_3', 64, 40, 0.05, 825, states='crowded', floor='events+uniform'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVENT_CASES, ids=case_id)
def test_weights_and_crowded_boards(case):
    run_case(case)


def test_event_floor_covers_the_cells():
    """CPU: each (bucket, family) cell has a case whose floor is 'events' — all 24 of them, where the bar is 90 % and
    every cell of buckets 32, 48 and 64"""
    def bucket(S):
        need = (S * S + 63) // 64
        return next(o for o in (2, 4, 8, 16, 24, 32, 48, 64) if need <= o)
    have = {(bucket(c['S']), c['family'], 'crop' if c['mode'] != 'positions' else 'positions')
            for c in EDGE_CASES + EVENT_CASES if 'events' in c['floor']}
    want = {(b, f, m) for b in (2, 4, 8, 16, 24, 32, 48, 64)
            for f, m in (('snake', 'crop'), ('snake', 'positions'), ('grid', 'positions'))}
    assert want <= have
