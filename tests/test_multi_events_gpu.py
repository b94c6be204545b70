"""The recorded snake-to-snake encounters (tests/golden/events_*.npz, see tests/test_multi_events_cpu.py) through the HIP
kernels: every fixture on every MultiSnake route that can serve its shape, bit for bit against what the reference did; the
instantiations that only draw (`_rng`), which tapes cannot reach, from the same start states and steered actions against the
oracle; and a loop in which every snake chases the nearest other head.  Every route is named by wurm_multi_last_route().

Census of the steered loop on the oracle's trajectory (seed 7, 60 steps; events of tests/multi_events_ref.py):
  cfg4 (N = 19, K = 4, S = 25, 'full', default): same_cell 22, swap 38, into_head 10, into_body 4, into_tail 5,
    into_dying 39, all_die 18, boost_gated 26, death_on_row_1 17, boost_first 2, boost_second 2
  dense (N = 9, K = 6, S = 14, 'full', dense): same_cell 72, same_food 10, swap 148, into_head 26, into_body 32,
    into_tail 41, into_tail_growing 3, into_tail_waiting 1, into_dying 157, own_tail 8, eat_and_die 22, all_die 23,
    boost_gated 77, death_on_row_1 49, respawn_blocked 271, boost_first 39, boost_second 41
Both hold at least 6 of the pairwise classes and both boost phases; test_steered_census_cpu checks that without a GPU.
"""
import numpy as np
import pytest

from oracle import oracle as _o
from tests import multi_events_ref as mer
from tests import replay
from tests.backends import OracleBackend
from tests.test_hip_multi_vs_oracle import CFGS, _same, _same_state
from tests.test_multi_events_cpu import NEW, PAIR_CLASSES, state_at

gpu = pytest.mark.gpu
GROUP, TWO, GENERIC = dict(WURM_MULTI_GROUP_MIN_ENVS=0), dict(WURM_MULTI_GROUP_MIN_ENVS=1 << 40), dict(WURM_MULTI_SHAPE_KERNELS=0)


@pytest.fixture(scope='module')
def hip():
    from tests.hip_backend import HipBackend
    return HipBackend


def _route():
    from wurm_amd import _lib
    return _lib.lib().wurm_multi_last_route().decode()


def _shape_of(name):
    fx = replay.load_multi(name)
    return fx, int(fx['meta'][1]), int(fx['meta'][2]), str(fx['mode'])


def step_routes(K, S, mode, tapes):
    """(options, route of the step launch) for every per-call route that serves the shape (multi_plan's table)"""
    t = '/tapes' if tapes else ''
    if K == 10:
        base = 'step_wg' if tapes else 'step_wg_rng_full_k10_s36'
        return [({}, base + t), (dict(WURM_MULTI_GROUP_VARIANT=1), base + t)] + \
            ([] if tapes else [(GENERIC, 'step_wg_rng')])
    if tapes:
        base = 'step'
    elif mode == 'full':
        base = {(4, 25): 'step_rng_full_k4_s25', (2, 12): 'step_rng_full_k2_s12'}.get((K, S), 'step_rng_full')
    else:
        base = 'step_rng_partial_k4_s25_n5' if (K, S, mode) == (4, 25, 'partial_5') else 'step_rng_partial'
    out = [({}, base + t)]
    if not tapes and base not in ('step_rng_full', 'step_rng_partial'):
        out.append((GENERIC, ('step_rng_full' if mode == 'full' else 'step_rng_partial')))
    if mode == 'full' and K <= 5:   # class codes: every wave its own env, or the workgroup's waves together
        out += [(dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=1), base + '+emit_wave' + t),
                (dict(GROUP, WURM_MULTI_GROUP_STEP_WPB=8), base + '+emit_group' + t)]
    return out


def rollout_routes(K, S, mode, tapes):
    t = '/tapes' if tapes else ''
    if mode != 'full':
        if tapes:
            return [({}, 'rollout/tapes')]
        if (K, S, mode) == (4, 25, 'partial_5'):
            return [({}, 'rollout_rng_partial_k4_s25_n5'), (GENERIC, 'rollout_rng_partial')]
        return [({}, 'rollout_rng_partial')]
    out = [(TWO, 'rollout_two' + (t if tapes else '_rng'))]
    has_rng = {8215: True, 8416: True, 4414: True, 8424: False, 5014: True, 4514: False, 3014: False}
    for code in ((8215, 8416, 4414, 8424) if K <= 5 else (5014, 4514, 3014)):
        name = f'rollout_group_{code}' + ('/tapes' if tapes else '_rng' if has_rng[code] else '')
        if not tapes and code == 4414 and (K, S) == (4, 25):
            out.append((dict(GROUP, WURM_MULTI_GROUP_SHAPE=code, **GENERIC), name))
            name += '_k4_s25'
        out.append((dict(GROUP, WURM_MULTI_GROUP_SHAPE=code), name))
    if tapes:
        out.append((dict(GROUP, **GENERIC), 'rollout_group_8215/tapes' if K <= 5 else 'rollout_group_5014/tapes'))
    return out


def _cases(kind, tapes):
    out = []
    for name in NEW:
        _, K, S, mode = _shape_of(name)
        for opts, route in (step_routes if kind == 'step' else rollout_routes)(K, S, mode, tapes):
            out.append(pytest.param(name, opts, route, id=f'{name}-{route}' + ''.join(f'-{k[11:].lower()}={v}' for k, v in opts.items())))
    return out


class _Named(object):
    """a backend whose step / rollout launches must take the named route"""

    def __init__(self, backend, route):
        self.b, self.route, self.seen = backend, route, 0

    def __getattr__(self, k):
        return getattr(self.b, k)

    def multi_step(self, *a, **kw):
        r = self.b.multi_step(*a, **kw)
        assert _route() == self.route, (_route(), self.route)
        self.seen += 1
        return r

    def multi_rollout(self, *a, **kw):
        r = self.b.multi_rollout(*a, **kw)
        assert _route() == self.route, (_route(), self.route)
        self.seen += 1
        return r


@gpu
@pytest.mark.parametrize('name,opts,route', _cases('step', True))
def test_recorded_encounters_per_call(hip, name, opts, route):
    from wurm_amd._lib import knobs
    with knobs(**opts):
        b = _Named(hip(), route)
        replay.replay_multi(b, replay.load_multi(name))
    assert b.seen == 6


@gpu
@pytest.mark.parametrize('name,opts,route', _cases('rollout', True))
def test_recorded_encounters_by_rollout(hip, name, opts, route):
    from wurm_amd._lib import knobs
    with knobs(**opts):
        b = _Named(hip(), route)
        replay.replay_multi_rollout(b, replay.load_multi(name))
    assert b.seen == 1


def _classes_at_step_0(fx, st):
    N, K = int(fx['meta'][0]), int(fx['meta'][1])
    for e in range(N):
        if int(fx['plan_step'][e]) == 0:
            evs = mer.classify_env(st, e, K, fx['actions'][0], fx['cfg_dict'])
            assert any(ev.cls == str(fx['plan_class'][e]) for ev in evs), (e, str(fx['plan_class'][e]), evs)


@gpu
@pytest.mark.parametrize('name,opts,route', _cases('step', False))
def test_steered_encounters_with_the_builds_rng_per_call(hip, name, opts, route, mode=None):
    """the start states and actions of the fixture, the build's own draws: oracle against library, step and reset"""
    from wurm_amd._lib import knobs
    fx = replay.load_multi(name)
    cfg, mode, T = fx['cfg_dict'], mode or str(fx['mode']), int(fx['meta'][3])
    o, h = OracleBackend(seed=5, env_offset=11), _Named(hip(seed=5, env_offset=11), route)
    so, sh = replay.multi_state(fx, 'state0_'), replay.multi_state(fx, 'state0_')
    _classes_at_step_0(fx, so)
    with knobs(**opts):
        for t in range(T):
            ro, rh = o.multi_step(so, fx['actions'][t], cfg, mode), h.multi_step(sh, fx['actions'][t], cfg, mode)
            _same_state(so, sh, f'state t={t}')
            for k in ro:
                _same(ro[k], rh[k], f'{k} t={t}')
            o.multi_reset(so, ro['all_done'], cfg)
            h.multi_reset(sh, rh['all_done'], cfg)
            _same_state(so, sh, f'reset state t={t}')


# the routes no fixture's own mode and length reach: no observation written, and a rollout of ONE step with 'full'
# observations (the one-wave kernel; longer ones double-buffer class codes between two waves)
OTHER_ROLLOUTS = [pytest.param(name, mode, T, route, id=f'{name}-{route}-T{T}')
                  for name in NEW if 'k10' not in name or name.endswith('_0')
                  for mode, T, route in (('none', 6, 'rollout_rng_none'), ('full', 1, 'rollout_rng'))]


@gpu
@pytest.mark.parametrize('name,mode,T,route', OTHER_ROLLOUTS)
def test_steered_encounters_on_the_one_wave_rollouts(hip, name, mode, T, route):
    test_steered_encounters_with_the_builds_rng_by_rollout(hip, name, {}, route, mode=mode, T=T)


@gpu
@pytest.mark.parametrize('name', [n for n in NEW if 'k10' not in n])
def test_steered_encounters_per_call_without_observations(hip, name):
    test_steered_encounters_with_the_builds_rng_per_call(hip, name, {}, 'step_rng_none', mode='none')


@gpu
@pytest.mark.parametrize('name', [n for n in NEW if '_full_' in n])
def test_recorded_encounters_by_a_rollout_of_one_step(hip, name):
    """the tapes' first step through the one-wave rollout kernel"""
    fx = replay.load_multi(name)
    N, K = int(fx['meta'][0]), int(fx['meta'][1])
    for k in list(fx):
        if k.startswith(('inj_', 'rinj_', 'step_', 'reset_', 'obs_')) or k in (
                'actions', 'rewards', 'dones_out', 'all_done', 'snake_collision', 'edge_collision', 'food', 'size', 'boost'):
            fx[k] = fx[k][:1]
    fx['meta'] = fx['meta'].copy()
    fx['meta'][3] = 1
    b = _Named(hip(), 'rollout/tapes')
    replay.replay_multi_rollout(b, fx)
    assert b.seen == 1


@gpu
@pytest.mark.parametrize('name,opts,route', _cases('rollout', False))
def test_steered_encounters_with_the_builds_rng_by_rollout(hip, name, opts, route, mode=None, T=None):
    from wurm_amd._lib import knobs
    fx = replay.load_multi(name)
    cfg, mode = fx['cfg_dict'], mode or str(fx['mode'])
    fx['actions'] = fx['actions'][:T]
    o, h = OracleBackend(seed=5, env_offset=11), _Named(hip(seed=5, env_offset=11), route)
    so, sh = replay.multi_state(fx, 'state0_'), replay.multi_state(fx, 'state0_')
    _classes_at_step_0(fx, so)
    with knobs(**opts):
        ro, rh = o.multi_rollout(so, fx['actions'], cfg, mode), h.multi_rollout(sh, fx['actions'], cfg, mode)
    for k in ro:
        _same(ro[k], rh[k], k)
    _same_state(so, sh, 'final state')


# ------------------------------------------------------------------ every snake chases the nearest other head

STEERED = {'cfg4': (19, 4, 25, 'default'), 'dense': (9, 6, 14, 'dense')}
STEERED_T, STEERED_SEED = 60, 7


def chase(st, N, K, S, rng):
    """(K, N) actions: towards the nearest other living head (the longer axis first), 20 % random, boosts at random"""
    a = rng.randint(0, 8, size=(K, N)).astype(np.int64)
    keep = rng.rand(K, N) < 0.2
    boost = rng.rand(K, N) < 0.3
    pos = {}
    for e in range(N):
        for s in range(K):
            if not st['dones'][e * K + s]:
                cell = int(np.argmax(st['heads'][e * K + s]))
                pos[e, s] = divmod(cell, S)
    for (e, s), (y, x) in pos.items():
        others = [(abs(y - v) + abs(x - u), v, u) for (f, q), (v, u) in pos.items() if f == e and q != s]
        if keep[s, e] or not others:
            continue
        _, v, u = min(others)
        dy, dx = v - y, u - x
        d = (0 if dy > 0 else 2) if abs(dy) >= abs(dx) else (3 if dx > 0 else 1)
        a[s, e] = d + 4 * int(boost[s, e])
    return a


def steered_run(which):
    """the oracle's trajectory under `chase` -> (start state, actions (T, K, N), census, [(outputs, state) per step], final state)"""
    N, K, S, cfg_name = STEERED[which]
    cfg = CFGS[cfg_name]
    rng = np.random.RandomState(STEERED_SEED)
    o = OracleBackend(seed=STEERED_SEED, env_offset=3)
    so = _o.multi_empty_state(N, K, S)
    so['colours'][...] = o.multi_colours(N, K, cfg['colour_mode'] == 'fixed', call=0)
    o.call = 1
    o.multi_reset(so, np.ones(N), cfg)
    start = {k: v.copy() for k, v in so.items()}
    acts, total, outs = [], {}, []
    for t in range(STEERED_T):
        a = chase(so, N, K, S, rng)
        mer.census([(t, e, ev) for e in range(N) for ev in mer.classify_env(so, e, K, a, cfg)], N, total)
        r = o.multi_step(so, a, cfg, 'full')
        acts.append(a)
        outs.append((r, {k: v.copy() for k, v in so.items()}))
        o.multi_reset(so, r['all_done'], cfg)
    return start, np.stack(acts), total, outs, so


def _steered_condition(total):
    assert sum(1 for c in PAIR_CLASSES if total.get(c, {}).get('n', 0) > 0) >= 6, total
    assert total.get('boost_first', {}).get('n', 0) > 0 and total.get('boost_second', {}).get('n', 0) > 0, total


@pytest.mark.parametrize('which', sorted(STEERED))
def test_steered_census_cpu(which):
    _steered_condition(steered_run(which)[2])


@gpu
@pytest.mark.parametrize('which', sorted(STEERED))
@pytest.mark.parametrize('how', ['per_call', 'rollout_two', 'rollout_group'])
def test_steered_loop(hip, which, how):
    from wurm_amd._lib import knobs
    N, K, S, cfg_name = STEERED[which]
    cfg = CFGS[cfg_name]
    start, acts, total, outs, final = steered_run(which)
    _steered_condition(total)
    h = hip(seed=STEERED_SEED, env_offset=3)
    h.call = 2
    sh = {k: v.copy() for k, v in start.items()}
    if how == 'per_call':
        for t in range(STEERED_T):
            rh = h.multi_step(sh, acts[t], cfg, 'full')
            assert _route() == ('step_rng_full_k4_s25' if K == 4 else 'step_rng_full')
            ro, so = outs[t]
            _same_state(so, sh, f'state t={t}')
            for k in ro:
                _same(ro[k], rh[k], f'{k} t={t}')
            h.multi_reset(sh, rh['all_done'], cfg)
        assert _route() == 'reset'
    else:
        with knobs(**(TWO if how == 'rollout_two' else GROUP)):
            rh = h.multi_rollout(sh, acts, cfg, 'full')
        want = {'rollout_two': 'rollout_two_rng', 'rollout_group': 'rollout_group_4414_rng_k4_s25' if K == 4 else 'rollout_group_5014_rng'}[how]
        assert _route() == want
        for k in outs[0][0]:
            if outs[0][0][k] is not None:
                _same(np.stack([r[k] for r, _ in outs]), rh[k], k)
    _same_state(final, sh, 'final state')


# ------------------------------------------------------------------ the class, with the resident mirror on and off

def _class_env(fx, mirror):
    import torch
    from wurm_amd.envs import MultiSnake
    N, K, S = (int(v) for v in fx['meta'][:3])
    cfg = fx['cfg_dict']
    env = MultiSnake(N, K, S, device='cuda:0', seed=13, env_offset=5, observation_mode=str(fx['mode']), manual_setup=True,
                     boost=cfg['boost'], food_on_death_prob=cfg['food_on_death_prob'], boost_cost_prob=cfg['boost_cost_prob'],
                     food_mode=cfg['food_mode'], food_rate=cfg['food_rate'], respawn_mode=cfg['respawn_mode'],
                     reward_on_death=cfg['reward_on_death'], agent_colours=cfg['colour_mode'], resident_mirror=mirror)
    st = replay.multi_state(fx, 'state0_')
    env.foods, env.heads, env.bodies = (torch.from_numpy(st[k]).cuda() for k in ('foods', 'heads', 'bodies'))
    env.dones = torch.from_numpy(st['dones']).bool().cuda()
    env.orientations = torch.from_numpy(st['orientations']).cuda()
    env.agent_colours = torch.from_numpy(st['colours']).cuda()
    return env


def _state_of(env):
    return dict(foods=env.foods.cpu().numpy(), heads=env.heads.cpu().numpy(), bodies=env.bodies.cpu().numpy(),
                dones=env.dones.cpu().numpy().astype(np.uint8), orientations=env.orientations.cpu().numpy())


def _raises(env):
    try:
        env.check_consistency()
        return False
    except RuntimeError:
        return True


CLASS_FIXTURES = ['events_k4_s25_full_0', 'events_k4_s25_full_1', 'events_k4_s25_partial_5_0', 'events_k10_s36_full_0',
                  'events_k10_s36_full_3']


@gpu
@pytest.mark.parametrize('name', CLASS_FIXTURES)
def test_class_steps_with_the_mirror_on_and_off(name):
    """the hand-made start states through MultiSnake objects, `step; reset(dones['__all__']); check_consistency()` as
    tests/test_multi_resident.py drives them: the object on the lazy resident mirror (its masks come out of the step launch)
    against the one without, and the masks against the oracle's checker on the state"""
    import torch
    from wurm_amd._lib import knobs
    fx = replay.load_multi(name)
    N, K, S, T = (int(v) for v in fx['meta'][:4])
    with knobs(WURM_RESIDENT_MIN_ENVS=0):
        on, off = _class_env(fx, 'lazy'), _class_env(fx, False)
        from_launch = 0
        for t in range(T):
            a = torch.from_numpy(fx['actions'][t]).cuda()
            outs = []
            for env in (on, off):
                obs, rew, dones, info = env.step({f'agent_{i}': a[i] for i in range(K)})
                env.reset(dones['__all__'], return_observations=False)
                outs.append((obs, rew, dones, info))
            for what, (x, y) in zip(('obs', 'rewards', 'dones'), zip(outs[0][:3], outs[1][:3])):
                assert sorted(x) == sorted(y)
                for k in x:
                    _same(x[k].cpu().numpy(), y[k].cpu().numpy(), f'{what} {k} t={t}')
            for k in outs[1][3]:
                _same(outs[0][3][k].cpu().numpy(), outs[1][3][k].cpu().numpy(), f'info {k} t={t}')
            m = on._step_check_mask()
            assert _raises(on) == _raises(off), t
            want = OracleBackend().multi_check({k: v for k, v in _state_of(off).items()}).astype(np.int64)
            if m is not None:
                got = m.cpu().numpy().astype(np.int64)
                known = got != -1
                _same(got[known], want[known], f'mask t={t}')
                from_launch += int(known.any())
            assert _raises(off) == bool((want != 0).any()), t
        assert from_launch > 0
        assert on._mirror is not None and off.mirror_state()['state'] == 'off'
        _same_state(_state_of(on), _state_of(off), 'final state')


@gpu
@pytest.mark.parametrize('name', CLASS_FIXTURES)
@pytest.mark.parametrize('group', [True, False])
def test_class_rollout_with_the_mirror_on_and_off(name, group):
    import torch
    from wurm_amd._lib import knobs
    fx = replay.load_multi(name)
    with knobs(WURM_RESIDENT_MIN_ENVS=0, WURM_MULTI_GROUP_MIN_ENVS=0 if group else 1 << 40):
        on, off = _class_env(fx, 'lazy'), _class_env(fx, False)
        a = torch.from_numpy(fx['actions']).cuda()
        x, y = on.rollout(a), off.rollout(a)
        for k in y:
            _same(x[k].cpu().numpy(), y[k].cpu().numpy(), k)
        assert _raises(on) == _raises(off)
        _same_state(_state_of(on), _state_of(off), 'final state')
