"""The cases of tests/test_stream_gate_gpu.py: every launching entry point of include/wurm_hip.h behind the stream gate
(tests/stream_gate.py), at the smallest shapes that take each route.  Importing this module needs no GPU: a case is a
few closures, and `covers` names the header's entry points its call reaches (tests/test_stream_inventory.py).

Class-level cases go through the host classes, so the way the host finds "the current stream" is under test as well
(`_lib.stream_ptr`, `PyStepper.get_stream`, the C Stepper with and without libwurm_torchinfo.so).  Entry points no class
method reaches without a host synchronisation are called through ctypes."""
import contextlib
import ctypes

import torch

from tests.stream_gate import Case
from wurm_amd import _lib

DEV = 'cuda:0'

# Class methods that synchronise with the host BY DESIGN, each with the line that says so.  They cannot be gated at class
# level (the host would wait for the gate before the launch is queued); the entry points behind them are gated through
# ctypes below ('abi ...' cases).
SYNCHRONISING = {
    'MultiSnake.league_plan': 'wurm_amd/envs/_multi_league.py: "One host synchronisation: the range check" — act_league and '
                              'league_window on a plan that exists do not synchronise',
    'SingleSnake.check_consistency': 'wurm_amd/envs/single_snake.py: `bool(err.any())` reads the masks back',
    'MultiSnake.check_consistency': 'wurm_amd/envs/multi_snake.py: `bool(err.any())` reads the masks back',
    'policy_rollout(check=True)': 'wurm_amd/envs/single_snake.py: "`check=True` synchronises once and raises if any env was '
                                  'outside the kernel\'s domain"',
    'SimpleGridworld: the launch that builds the mirror': 'include/wurm_hip.h (wurm_grid_resident_bytes): "reads that verdict '
                                                          'back synchronously (4 bytes, one stream synchronisation)"',
    'record_start(select) with a Python list': 'wurm_amd/envs/_fast_step.py, _multi_frames.py: `torch.as_tensor(select).to(device)` '
                                               'copies the list to the device; a device tensor is taken as it is',
    'MultiSnake.reset(done) that has to report no room': 'wurm_amd/envs/multi_snake.py: `int(status.item())` in _create_envs',
}

CASES = []


def _rand(seed, hi, *shape, dtype=torch.long):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(hi, shape, generator=g).to(dtype).to(DEV)


def _single_route():
    return _lib.lib().wurm_single_last_route().decode()


def _multi_route():
    return _lib.lib().wurm_multi_last_route().decode()


def _policy_route():
    return _lib.lib().wurm_policy_last_route().decode()


# ------------------------------------------------------------------------------------ SingleSnake / SimpleGridworld

def _snake(S=9, N=70, mode='partial_2', **kw):
    from wurm_amd.envs import SingleSnake
    return SingleSnake(num_envs=N, size=S, observation_mode=mode, device=DEV, seed=11, **kw)


def _gridworld(S=9, N=70, mode='default', **kw):
    from wurm_amd.envs import SimpleGridworld
    return SimpleGridworld(num_envs=N, size=S, observation_mode=mode, start_location=(S // 2, S // 2), device=DEV, seed=11, **kw)


def _envs_of(env):
    return {'envs': env.envs}


def _step_reset(want_obs):
    def call(env, inputs):
        obs, reward, done, info = env.step(inputs[0])
        after = env.reset(done, return_observations=want_obs)
        return dict(obs=obs, reward=reward, done=done, info=info, after=after)
    return call


@contextlib.contextmanager
def _patch(name, value):
    old = getattr(_lib, name)
    setattr(_lib, name, value)
    try:
        yield
    finally:
        setattr(_lib, name, old)


def _without_torchinfo():   # the C Stepper finds the stream through the Python accessor
    return _patch('torch_helpers', lambda: None)


def _python_stepper():      # no C address to hand to the C Stepper: PyStepper over the ctypes function
    return _patch('step_slot_fn', lambda name='wurm_single_step_slot': getattr(_lib.lib(), name))


STEPPERS = {'c_torchinfo': None, 'c_accessor': _without_torchinfo, 'python': _python_stepper}


def _stepper_check(kind, env):
    from wurm_amd.envs._fast_step import PyStepper
    assert isinstance(env._fs, PyStepper) == (kind == 'python'), type(env._fs)
    if kind == 'c_torchinfo':   # else the case would take the Python accessor a second time
        assert _lib.torch_helpers() is not None, 'libwurm_torchinfo.so is not built'
    return env


def _add_step_reset(family, maker, kind, lazy, want_obs, slot):
    N = 70
    CASES.append(Case(
        f'{family}.step+reset stepper={kind} lazy={int(lazy)} reset_obs={int(want_obs)}',
        lambda: _stepper_check(kind, maker(lazy_reset=lazy)), _step_reset(want_obs),
        lambda: (_rand(1, 4, N),), lambda: (_rand(2, 4, N),),
        (slot,) + (() if lazy and not want_obs else ('wurm_single_reset' if family == 'SingleSnake' else 'wurm_grid_reset',)),
        state=_envs_of, patch=STEPPERS[kind]))


for _kind in STEPPERS:
    for _lazy in (True, False):
        for _obs in (False, True):
            _add_step_reset('SingleSnake', _snake, _kind, _lazy, _obs, 'wurm_single_step_slot')
            _add_step_reset('SimpleGridworld', _gridworld, _kind, _lazy, _obs, 'wurm_grid_step_slot')


def _outside_grid_domain(call):
    """`call` with one env put outside the clock-grid kernels' domain (a second head) in front of it, on the current stream,
    every time: the kernel flags it and the generic kernel takes it in a second launch that has work to do"""
    def edited(env, inputs):
        # (the planes themselves: these cases keep no mirror and postpone no reset, so the tensor is the state)
        assert not env._fs.pending and not env._c.resident
        env._envs[3, 1, 0, 0].fill_(1.0)
        return call(env, inputs)
    return edited


def _flushed(call):
    """`call`, then the lazy mirror written out to the planes on the current stream (what reading `env.envs` does)"""
    def both(env, inputs):
        out = call(env, inputs)
        env._write_out()
        return dict(out=out, planes=env._envs)
    return both


STEP_ROUTES = [
    # (family, route, S, N, mode, knobs, mirror keyword, hand edit)
    ('SingleSnake', 'generic', 9, 70, 'partial_2', dict(WURM_LANE_STEP_MIN_ENVS=1 << 40, WURM_GRID_STEP_MIN_CELLS=1 << 40), False, False),
    ('SingleSnake', 'lane_step', 9, 70, 'partial_2', dict(WURM_LANE_STEP_MIN_ENVS=0, WURM_GRID_STEP_MIN_CELLS=1 << 40), False, False),
    ('SingleSnake', 'grid_step', 12, 40, 'partial_2', dict(WURM_LANE_STEP_MIN_ENVS=0, WURM_GRID_STEP_MIN_CELLS=0), False, False),
    # one env outside the clock grid's domain: the generic kernel takes it in a second launch (and names the route)
    ('SingleSnake', None, 12, 40, 'partial_2', dict(WURM_LANE_STEP_MIN_ENVS=0, WURM_GRID_STEP_MIN_CELLS=0), False, True),
    ('SingleSnake', 'lane_resident', 9, 70, 'partial_2', dict(WURM_RESIDENT_MIN_ENVS=0), 'lazy', False),
    ('SingleSnake', 'grid_step', 12, 40, 'partial_2', dict(WURM_RESIDENT_MIN_ENVS=0), 'lazy', False),
    ('SimpleGridworld', 'gridworld_lane_step', 9, 16, 'default', dict(WURM_RESIDENT_MIN_ENVS=0, WURM_LANE_STEP_MIN_ENVS=0), 'lazy', False),
]
for _family, _route, _S, _N, _mode, _knobs, _mirror, _edit in STEP_ROUTES:
    _maker = _snake if _family == 'SingleSnake' else _gridworld
    _pre = 'single' if _family == 'SingleSnake' else 'grid'
    CASES.append(Case(
        f'{_family}.step route={_route} S={_S}' + (' on its mirror, then written out' if _mirror else '') +
        (' + one env outside its domain' if _edit else ''),
        lambda m=_maker, S=_S, N=_N, mode=_mode, mirror=_mirror, edit=_edit:
            m(S, N, mode, resident_mirror=mirror, lazy_reset=not edit),
        _flushed(_step_reset(False)) if _mirror else _outside_grid_domain(_step_reset(False)) if _edit else _step_reset(False),
        lambda N=_N: (_rand(3, 4, N),), lambda N=_N: (_rand(4, 4, N),),
        (f'wurm_{_pre}_step_slot',) + ((f'wurm_{_pre}_resident_flush',) if _mirror else ()),
        state=_envs_of, knobs=_knobs, route=_route and (_single_route, _route),
        min_launches=3 if _edit else 1))   # (the hand edit: clock-grid step, the generic launch behind it, the eager reset)

ROLLOUT_ROUTES = [
    # (family, route, S, N, mode, lane threshold)
    ('SingleSnake', 'rollout_s9', 9, 70, 'partial_2', 1 << 40),
    ('SingleSnake', 'rollout_lean', 10, 70, 'partial_2', 1 << 40),
    ('SingleSnake', 'rollout_generic_partial', 9, 70, 'partial_4', 0),
    ('SingleSnake', 'generic', 9, 70, 'raw', 1 << 40),
    ('SingleSnake', 'lane_rollout', 9, 70, 'partial_2', 0),
    ('SingleSnake', 'lane_wide', 10, 70, 'partial_2', 0),
    ('SingleSnake', 'grid_rollout', 12, 40, 'partial_2', 0),
    ('SimpleGridworld', 'generic', 9, 16, 'default', 17),
    ('SimpleGridworld', 'gridworld_lane', 9, 16, 'default', 0),
]


def _rollout(env, inputs):
    return env.rollout(inputs[0])


for _family, _route, _S, _N, _mode, _min in ROLLOUT_ROUTES:
    _maker = _snake if _family == 'SingleSnake' else _gridworld
    CASES.append(Case(
        f'{_family}.rollout route={_route} S={_S}', lambda m=_maker, S=_S, N=_N, mode=_mode: m(S, N, mode), _rollout,
        lambda N=_N: (_rand(5, 4, 6, N),), lambda N=_N: (_rand(6, 4, 6, N),),
        ('wurm_single_rollout' if _family == 'SingleSnake' else 'wurm_grid_rollout',),
        state=_envs_of, knobs=dict(WURM_LANE_ROLLOUT_MIN_ENVS=_min), route=(_single_route, _route)))

# the clock-grid rollout with one env outside its domain: the second, generic launch over the envs it flagged
CASES.append(Case(
    'SingleSnake.rollout route=grid_rollout + one env outside its domain', lambda: _snake(12, 40, 'partial_2'),
    _outside_grid_domain(_rollout), lambda: (_rand(5, 4, 6, 40),), lambda: (_rand(6, 4, 6, 40),), ('wurm_single_rollout',),
    state=_envs_of, knobs=dict(WURM_LANE_ROLLOUT_MIN_ENVS=0), min_launches=2))

# rollouts that keep the mirror (wurm_*_rollout_resident): the lazy mirror is made by the warm call
CASES.append(Case(
    'SingleSnake.rollout with the mirror (12 x 12)', lambda: _snake(12, 40, 'partial_2', resident_mirror='lazy'), _flushed(_rollout),
    lambda: (_rand(5, 4, 6, 40),), lambda: (_rand(6, 4, 6, 40),), ('wurm_single_rollout_resident', 'wurm_single_resident_flush'),
    state=_envs_of, knobs=dict(WURM_LANE_ROLLOUT_MIN_ENVS=0, WURM_RESIDENT_MIN_ENVS=0), route=(_single_route, 'grid_rollout')))
CASES.append(Case(
    'SimpleGridworld.rollout with the mirror', lambda: _gridworld(9, 16, 'default', resident_mirror='lazy'), _flushed(_rollout),
    lambda: (_rand(5, 4, 6, 16),), lambda: (_rand(6, 4, 6, 16),), ('wurm_grid_rollout_resident', 'wurm_grid_resident_flush'),
    state=_envs_of, knobs=dict(WURM_LANE_ROLLOUT_MIN_ENVS=0, WURM_LANE_STEP_MIN_ENVS=0, WURM_RESIDENT_MIN_ENVS=0),
    route=(_single_route, 'gridworld_lane')))


def _policy_params(E, seed, rows=None):
    from wurm_amd.agents import FeedforwardAgent, pack_policy_params
    torch.manual_seed(seed)
    one = lambda: pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E))  # noqa: E731
    return (one() if rows is None else torch.stack([one() for _ in range(rows)])).to(DEV).contiguous()


def _policy_case(name, maker, E, covers, population=None, route=None, **kw):
    def make():
        env = maker()
        return env, env.reset()

    def call(x, inputs):
        env, state = x
        out = env.policy_rollout(inputs[0], state, 5, check=False, population=population)
        return out

    CASES.append(Case(name, make, call, lambda: (_policy_params(E, 1, population),), lambda: (_policy_params(E, 2, population),),
                      covers, state=lambda x: _envs_of(x[0]), route=route and (_policy_route, route), **kw))


_policy_case('SingleSnake.policy_rollout narrow (E = 75)', lambda: _snake(9, 70, 'partial_2'), 75,
             ('wurm_single_policy_rollout_mode',), route='policy_s9')
_policy_case('SingleSnake.policy_rollout wide (E = 507)', lambda: _snake(15, 33, 'partial_6'), 507,
             ('wurm_single_policy_rollout_mode',), route='policy_wide')
_policy_case('SingleSnake.policy_rollout population=2', lambda: _snake(9, 70, 'partial_2'), 75,
             ('wurm_single_policy_rollout_pop',), population=2)
_policy_case('SimpleGridworld.policy_rollout', lambda: _gridworld(5, 64, 'positions'), 4, ('wurm_grid_policy_rollout',))
_policy_case('SimpleGridworld.policy_rollout population=2', lambda: _gridworld(5, 64, 'positions'), 4,
             ('wurm_grid_policy_rollout_pop',), population=2)


class _Select(dict):
    """env indices as a device tensor, made once outside the gate (a Python list would be copied to the device inside
    record_start: SYNCHRONISING)"""
    def __missing__(self, N):
        self[N] = torch.tensor([0, N - 1, 3], device=DEV)
        torch.cuda.synchronize()
        return self[N]


_SELECT = _Select()


def _frames_case(family, maker, N, covers):
    def call(env, inputs):
        rec = env.record_start(_SELECT[N])
        out = env.rollout(inputs[0])
        return dict(rollout=out, frames=env.record_frames(rec, inputs[0]))
    CASES.append(Case(f'{family}.record_start + rollout + record_frames', maker, call,
                      lambda: (_rand(7, 4, 5, N),), lambda: (_rand(8, 4, 5, N),), covers, state=_envs_of))


_frames_case('SingleSnake', lambda: _snake(9, 70, 'partial_2'), 70, ('wurm_single_rollout_frames', 'wurm_single_rollout'))
_frames_case('SimpleGridworld', lambda: _gridworld(9, 16, 'default'), 16, ('wurm_grid_rollout_frames', 'wurm_grid_rollout'))


def _observe_case(family, maker, N, covers):
    def call(env, inputs):   # an eager reset (a `done` of the caller's own), then the observation of the state it left
        env.reset(inputs[0], return_observations=False)
        return dict(obs=env._observe(env.observation_mode))
    CASES.append(Case(f'{family}.reset(done) + _observe', maker, call, lambda: (_rand(9, 2, N, dtype=torch.bool),),
                      lambda: (_rand(10, 2, N, dtype=torch.bool),), covers, state=_envs_of))


_observe_case('SingleSnake', lambda: _snake(9, 70, 'one_channel'), 70, ('wurm_single_reset', 'wurm_single_observe'))
_observe_case('SimpleGridworld', lambda: _gridworld(9, 16, 'default'), 16, ('wurm_grid_reset', 'wurm_grid_observe'))


# ------------------------------------------------------------------------------------ MultiSnake

def _multi(K=3, N=17, n=2, **kw):
    from wurm_amd.envs import MultiSnake
    return MultiSnake(num_envs=N, num_snakes=K, size=12, observation_mode=f'partial_{n}', device=DEV, seed=7, boost=False,
                      food_mode='random_rate', food_rate=0.02, respawn_mode='any', **kw)


MULTI_STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours', 'boost_this_step')


def _multi_state(env):
    return {name: getattr(env, name) for name in MULTI_STATE}


def _multi_actions(t, K):
    return {f'agent_{k}': t[k] for k in range(K)}


_STEP_ROUTE = []


def _multi_step_route():
    """the kernel that served the last MultiSnake.step of a step case (the reset behind it names another)"""
    return _STEP_ROUTE[-1]


def _multi_step_case(name, K, N, knobs, route, covers, reset=True, make=None, **kw):
    def call(env, inputs):
        obs, rewards, dones, info = env.step(_multi_actions(inputs[0], K))
        _STEP_ROUTE[:] = [_multi_route() + ('|mirror ' + env.mirror_state()['state'] if kw.get('resident_mirror') else '')]
        if reset:
            env.reset(dones['__all__'], return_observations=False)
        return dict(obs=obs, rewards=rewards, dones=dones, info=info)
    CASES.append(Case(name, make or (lambda: _multi(K, N, **kw)), call, lambda: (_rand(11, 4, K, N),), lambda: (_rand(12, 4, K, N),),
                      covers, state=_multi_state, knobs=knobs, route=(_multi_step_route, route)))


_multi_step_case('MultiSnake.step + postponed reset, one wave per env', 3, 17, {}, 'step_rng_partial',
                 ('wurm_multi_step_slot',))
_multi_step_case('MultiSnake.step + eager reset(return_observations=False)', 3, 17, {}, 'step_rng_partial',
                 ('wurm_multi_step_slot', 'wurm_multi_reset'), lazy_reset=False)
_multi_step_case('MultiSnake.step with the mirror', 2, 9, dict(WURM_RESIDENT_MIN_ENVS=0), 'step_rng_partial|mirror lazy',
                 ('wurm_multi_step_slot', 'wurm_multi_resident_flush'), resident_mirror='lazy')


def _multi_wg():
    """10 snakes on 36 x 36, 'full': four envs' images do not fit the LDS of a workgroup, one env per workgroup
    (multi_step_wg_kernel; tests/test_multi_dispatch_table.py runs it at the same shape)"""
    from wurm_amd.envs import MultiSnake
    return MultiSnake(num_envs=3, num_snakes=10, size=36, observation_mode='full', device=DEV, seed=7)


_multi_step_case('MultiSnake.step, one env per workgroup', 10, 3, {}, 'step_wg_rng_full_k10_s36', ('wurm_multi_step_slot',),
                 make=_multi_wg)


def _multi_obs_after(env, inputs):
    obs, rewards, dones, info = env.step(_multi_actions(inputs[0], 3))
    after = env.reset(dones['__all__'])
    return dict(obs=obs, rewards=rewards, dones=dones, info=info, after={k: v + 0 for k, v in after.items()})


CASES.append(Case('MultiSnake.step with obs_after (reset whose observations are read)', lambda: _multi(3, 17), _multi_obs_after,
                  lambda: (_rand(11, 4, 3, 17),), lambda: (_rand(12, 4, 3, 17),), ('wurm_multi_step_slot', 'wurm_multi_reset'),
                  state=_multi_state))


def _multi_rollout(env, inputs):
    return env.rollout(inputs[0])


for _name, _knobs, _route, _kw, _covers in [
        ('one wave per env', {}, 'rollout_rng_partial', {}, ('wurm_multi_rollout',)),
        ('group kernel', dict(WURM_MULTI_GROUP_MIN_ENVS=0), 'rollout_group_8215_rng', dict(full=True), ('wurm_multi_rollout',)),
        ('with the mirror', dict(WURM_MULTI_GROUP_MIN_ENVS=0, WURM_RESIDENT_MIN_ENVS=0), None,
         dict(full=True, resident_mirror='lazy'), ('wurm_multi_rollout_resident', 'wurm_multi_resident_flush'))]:
    def _make(kw=_kw):
        from wurm_amd.envs import MultiSnake
        kw = dict(kw)
        if kw.pop('full', False):
            return MultiSnake(num_envs=9, num_snakes=2, size=12, observation_mode='full', device=DEV, seed=7, **kw)
        return _multi(2, 9, **kw)
    CASES.append(Case(f'MultiSnake.rollout {_name}', _make, _multi_rollout, lambda: (_rand(13, 8, 3, 2, 9),),
                      lambda: (_rand(14, 8, 3, 2, 9),), _covers, state=_multi_state, knobs=_knobs,
                      route=_route and (_multi_route, _route)))


def _multi_acting(name, method, covers, league=False):
    K, N, E, P = 4, 17, 75, 2

    def make():
        env = _multi(K, N)
        state = env.reset()
        plan = env.league_plan(_rand(15, P, K, N), P) if league else None   # (the one synchronisation, outside the gate)
        return env, state, plan

    def call(x, inputs):
        env, state, plan = x
        if method == 'act':
            return env.act(inputs[0], state, num_species=P)
        if method == 'act_league':
            return env.act_league(inputs[0], state, plan)
        if method == 'league_window':
            return env.league_window(inputs[0], state, 3, plan, info=True)
        return getattr(env, method)(inputs[0], state, 3, num_species=P, info=True)

    CASES.append(Case(name, make, call, lambda: (_policy_params(E, 3, P),), lambda: (_policy_params(E, 4, P),), covers,
                      state=lambda x: _multi_state(x[0])))


_multi_acting('MultiSnake.act', 'act', ('wurm_multi_act',))
_multi_acting('MultiSnake.act_window', 'act_window', ('wurm_multi_act', 'wurm_multi_step_slot'))
_multi_acting('MultiSnake.policy_window', 'policy_window', ('wurm_multi_policy_window',))
_multi_acting('MultiSnake.act_league on a plan that exists', 'act_league', ('wurm_multi_act_league',), league=True)
_multi_acting('MultiSnake.league_window', 'league_window', ('wurm_multi_act_league', 'wurm_multi_step_slot'), league=True)


def _multi_frames(env, inputs):
    rec = env.record_start(_SELECT[9])
    out = env.rollout(inputs[0])
    return dict(rollout=out, frames=env.record_frames(rec, inputs[0]))


CASES.append(Case('MultiSnake.record_start + rollout + record_frames', lambda: _multi(2, 9), _multi_frames,
                  lambda: (_rand(13, 8, 3, 2, 9),), lambda: (_rand(14, 8, 3, 2, 9),),
                  ('wurm_multi_rollout_frames', 'wurm_multi_rollout'), state=_multi_state))


def _multi_observe(env, inputs):
    env.reset(inputs[0], return_observations=False)
    return dict(obs=env._observe())


CASES.append(Case('MultiSnake.reset(done) + _observe', lambda: _multi(3, 17), _multi_observe,
                  lambda: (_rand(16, 2, 17, dtype=torch.bool),), lambda: (_rand(17, 2, 17, dtype=torch.bool),),
                  ('wurm_multi_reset', 'wurm_multi_observe'), state=_multi_state))


# ------------------------------------------------------------------------------------ learner side

E_, T_, N_ = 27, 5, 65
_FIXTURES = {}


def _fixture(seed, N=N_):
    from tests import a2c_learner_ref as ref
    if (seed, N) not in _FIXTURES:
        _FIXTURES[seed, N] = ref.make_fixture(E_, T_, N, seed=seed)
    return _FIXTURES[seed, N]


WINDOW = ('obs0', 'obs', 'actions', 'rewards', 'dones')


def _window(seed, N=N_):
    """the fixture's window, or its first N envs"""
    fx = _fixture(seed)
    return tuple((fx[k][:N] if k == 'obs0' else fx[k][:, :N]).contiguous().to(DEV) for k in WINDOW)


def _as_out(inputs):
    return inputs[0], dict(observations=inputs[1], actions=inputs[2], rewards=inputs[3], dones=inputs[4])


def _agents(n):
    from tests import a2c_learner_ref as ref
    return [ref.to_device(_fixture(10 + i), DEV)[0] for i in range(n)]


def _learner_state(learner):
    state = {k: getattr(learner, k) for k in ('params', 'exp_avg', 'exp_avg_sq')}
    if hasattr(learner, 'hyper'):
        state['hyper'] = learner.hyper
    return state


def _learner_call(what, extra=None):
    def call(learner, inputs):
        state, out = _as_out(inputs)
        kw = extra(learner) if extra else {}
        if what == 'update':
            return learner.update(state, out, **kw)
        grad, losses = learner.grad(state, out, **kw)
        if what == 'grad':
            return dict(grad=grad, losses=losses)
        return dict(grad=grad, losses=losses, norm=learner.apply(grad, **kw))
    return call


def _make_learner(gae):
    from wurm_amd.rl import FusedA2CLearner
    return FusedA2CLearner(_agents(1)[0], lr=1e-3, entropy_coef=0.01, use_gae=gae, gae_lambda=0.95 if gae else None)


def _make_population(gae, P=3):
    from wurm_amd.rl import FusedA2CPopulation
    return FusedA2CPopulation(_agents(P), lr=1e-3, entropy_coef=0.01, use_gae=gae, gae_lambda=0.95 if gae else None)


for _gae in (False, True):
    _g = '_gae' if _gae else ''
    for _what, _covers in (('grad', ('grad' + _g,)), ('grad+apply', ('grad' + _g, 'apply')), ('update', ('update' + _g,))):
        CASES.append(Case(f'FusedA2CLearner.{_what} gae={int(_gae)}', lambda gae=_gae: _make_learner(gae), _learner_call(_what),
                          lambda: _window(1), lambda: _window(2), tuple('wurm_a2c_ff_' + c for c in _covers),
                          state=_learner_state))
        # P = 3 members of M = 2 envs each
        CASES.append(Case(f'FusedA2CPopulation.{_what} gae={int(_gae)}', lambda gae=_gae: _make_population(gae),
                          _learner_call(_what), lambda: _window(1, 6), lambda: _window(2, 6),
                          tuple('wurm_a2c_ff_pop_' + c for c in _covers), state=_learner_state))

        def _league(learner):   # a league window: policy p learns from the columns the line-up gave it (an index list each)
            plan = getattr(learner, '_stream_case_plan', None)
            if plan is None:
                from wurm_amd.envs._multi_league import LeaguePlan
                lineup = torch.tensor([[0, 2, 1], [2, 2, 0]], device=DEV)
                flat = lineup.reshape(-1)
                offsets = torch.zeros(4, dtype=torch.long, device=DEV)
                torch.cumsum(torch.bincount(flat, minlength=3), 0, out=offsets[1:])
                plan = learner._stream_case_plan = LeaguePlan(lineup, torch.sort(flat, stable=True).indices.to(torch.int32),
                                                              offsets, 3)
            return dict(plan=plan)
        CASES.append(Case(f'FusedA2CPopulation.{_what} on a league window gae={int(_gae)}',
                          lambda gae=_gae: _make_population(gae), _learner_call(_what, _league), lambda: _window(1, 6),
                          lambda: _window(2, 6), tuple('wurm_a2c_ff_league_' + c for c in _covers), state=_learner_state))


def _exploit(pop, inputs):
    return dict(result=pop.exploit(inputs[0], num_replace=2, seed=5))


CASES.append(Case('FusedA2CPopulation.exploit (P = 5, k = 2)', lambda: _make_population(False, 5), _exploit,
                  lambda: (torch.tensor([3., 1., 4., 1.5, 9.], device=DEV),), lambda: (torch.tensor([2., 7., 1., 8., 2.5], device=DEV),),
                  ('wurm_a2c_ff_pop_exploit',), state=_learner_state))


def _returns(x, inputs):
    from wurm_amd.rl import a2c_returns
    bootstrap, rewards, values, dones = inputs
    values = values.clone().requires_grad_(True)
    bootstrap = bootstrap.clone().requires_grad_(True)
    returns = a2c_returns(bootstrap, rewards, values, dones, gamma=0.99, **x)
    loss = (returns * rewards).sum()
    loss.backward()     # (the backward launch asks for the stream on autograd's thread)
    return dict(returns=returns.detach(), grad_values=values.grad, grad_bootstrap=bootstrap.grad)


def _returns_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N_, generator=g).to(DEV), torch.randn(T_, N_, generator=g).to(DEV),
            torch.randn(T_, N_, generator=g).to(DEV), (torch.rand(T_, N_, generator=g) < 0.3).to(DEV))


for _gae in (False, True):
    CASES.append(Case(f'a2c_returns forward + backward gae={int(_gae)}',
                      lambda gae=_gae: dict(use_gae=True, gae_lambda=0.95) if gae else {}, _returns,
                      lambda: _returns_inputs(1), lambda: _returns_inputs(2), ('wurm_a2c_returns', 'wurm_a2c_returns_backward')))


def _stats_windows(family):
    """two chained windows of a real env under a fixed policy, made once"""
    key = ('stats', family)
    if key not in _FIXTURES:
        env = _snake(9, 64, 'partial_2') if family == 'snake' else _gridworld(5, 64, 'positions')
        params = _policy_params(75 if family == 'snake' else 4, 5)
        state, windows = env.reset(), []
        for _ in range(2):
            out = env.policy_rollout(params, state, 8, check=False)
            state = out['state']
            keys = ('rewards', 'dones', 'edge_collision') + (('self_collision',) if family == 'snake' else ()) + ('probs',)
            windows.append(tuple(out[k].clone() for k in keys) + (keys,))
        torch.cuda.synchronize()
        _FIXTURES[key] = windows
    return _FIXTURES[key]


def _rollout_stats(family):
    def make():
        from wurm_amd.rl import RolloutStats
        _stats_windows(family)
        return RolloutStats(_snake(9, 64, 'partial_2') if family == 'snake' else _gridworld(5, 64, 'positions'))

    def call(stats, inputs):
        keys = _stats_windows(family)[0][-1]
        return dict(table=stats.update(dict(zip(keys, inputs)), per_step=True))

    CASES.append(Case(f'RolloutStats.update, two chained windows ({family})', make, call,
                      lambda: _stats_windows(family)[0][:-1], lambda: _stats_windows(family)[1][:-1], ('wurm_rollout_stats',),
                      state=lambda s: dict(carry=s.carry, accum=s.accum, smooth=s.smooth)))


_rollout_stats('snake')
_rollout_stats('gridworld')

MULTI_STATS_KEYS = ('rewards', 'dones', 'all_done', 'food', 'size', 'boost', 'snake_collision', 'edge_collision', 'probs')


def _multi_windows():
    if 'multi_stats' not in _FIXTURES:
        env = _multi(4, 17)
        params, state, windows = _policy_params(75, 6, 2), env.reset(), []
        for _ in range(2):
            out = env.act_window(params, state, 6, num_species=2, info=True)
            state = out['state']
            windows.append({k: out[k].clone() for k in out if isinstance(out[k], torch.Tensor) and k != 'state'})
        torch.cuda.synchronize()
        _FIXTURES['multi_stats'] = windows
    return _FIXTURES['multi_stats']


def _multi_stats_inputs(i):
    w = _multi_windows()[i]
    return tuple(w[k] for k in sorted(w))


def _multi_stats_make():
    from wurm_amd.rl import MultiRolloutStats
    _multi_windows()
    return MultiRolloutStats(_multi(4, 17))


def _multi_stats_call(stats, inputs):
    return dict(table=stats.update(dict(zip(sorted(_multi_windows()[0]), inputs)), per_step=True))


CASES.append(Case('MultiRolloutStats.update, two chained windows', _multi_stats_make, _multi_stats_call,
                  lambda: _multi_stats_inputs(0), lambda: _multi_stats_inputs(1), ('wurm_multi_rollout_stats',),
                  state=lambda s: {k: v for k, v in vars(s).items() if isinstance(v, torch.Tensor)}))


def _league_table_make():
    from wurm_amd.rl import LeagueTable
    _multi_windows()
    env = _multi(4, 17)
    return LeagueTable(3, DEV), env.league_plan(_rand(18, 3, 4, 17), 3)


def _league_table_call(x, inputs):
    table, plan = x
    table.update(plan, dict(zip(sorted(_multi_windows()[0]), inputs)))
    return {k: v for k, v in vars(table).items() if isinstance(v, torch.Tensor)}


CASES.append(Case('LeagueTable.update', _league_table_make, _league_table_call, lambda: _multi_stats_inputs(0),
                  lambda: _multi_stats_inputs(1), ('wurm_multi_league_scores',),
                  state=lambda x: {k: v for k, v in vars(x[0]).items() if isinstance(v, torch.Tensor)}))


# ------------------------------------------------------------------------------------ the C ABI through ctypes
# Entry points behind class methods that synchronise by design (SYNCHRONISING), and those no class method calls: one call
# each with the arguments under the header's parameter names (`_lib.call_named`), on the stream current at the call.

def _abi(name, covers, make, a, b, inputs, fn=None, block=None, ok=(0,), route=None):
    """make() -> dict of values under the parameter names of `fn` (tensors as they are);  inputs: the names the gate
    rewrites;  block: None, or (ctypes struct type, parameter name): the tensors and numbers go into a host struct"""
    fn = fn or covers[0]

    def call(values, bufs):
        values = dict(values, **dict(zip(inputs, bufs)))
        raw = {k: (_lib.ptr(v) if isinstance(v, torch.Tensor) else v) for k, v in values.items()}
        raw['stream'] = _lib.stream_ptr()
        keep = None
        if block is not None:
            keep = block[0]()
            for field, _ in keep._fields_:
                if field in raw:
                    setattr(keep, field, raw[field])
            raw[block[1]] = ctypes.addressof(keep)
        rc = _lib.call_named(0, getattr(_lib.lib(), fn), raw)
        assert rc in ok, f'{fn} returned {rc}'
        return {k: v for k, v in values.items() if isinstance(v, torch.Tensor) and k not in inputs}

    CASES.append(Case(f'abi {name}', make, call, a, b, covers, route=route))


def _snake_planes(S=9, N=70):
    env = _snake(S, N, 'partial_2')
    return env.envs.clone()


def _outs(N, *names, dtype=torch.uint8):
    return {n: torch.zeros(N, dtype=dtype, device=DEV) for n in names}


def _single_common(S=9, N=70):
    return dict(envs=_snake_planes(S, N), num_envs=N, size=S, seed=11, env_offset=0, actions_dtype=_lib.ACT_I64,
                obs_mode=_lib.OBS_PARTIAL, obs_n=2, inject_food=None, inject_reset=None,
                reward=torch.zeros(N, device=DEV), obs=torch.zeros((N, 75), device=DEV),
                **_outs(N, 'done', 'self_collision', 'edge_collision'))


_abi('wurm_single_step', ('wurm_single_step',), lambda: dict(_single_common(), call=100),
     lambda: (_rand(21, 4, 70),), lambda: (_rand(22, 4, 70),), ('actions',))
_abi('wurm_single_step_reset (post_reset, obs_after)', ('wurm_single_step_reset',),
     lambda: dict(_single_common(), call=100, pre_call=0, post_reset=1, obs_after=torch.zeros((70, 75), device=DEV),
                  start_y=-1, start_x=-1, c=None, **_outs(70, 'done_copy')),
     lambda: (_rand(21, 4, 70),), lambda: (_rand(22, 4, 70),), ('actions',), block=(_lib.SingleCall, 'c'))
_abi('wurm_single_check', ('wurm_single_check',),
     lambda: dict(num_envs=70, size=9, err=torch.zeros(70, dtype=torch.int32, device=DEV)),
     lambda: (_snake_planes(),), lambda: (_snake_planes().flip(0).contiguous().index_fill_(2, torch.tensor([4], device=DEV), 1.0),),
     ('envs',))
_abi('wurm_orientations', ('wurm_orientations',),
     lambda: dict(n=70, size=9, out=torch.zeros(70, dtype=torch.long, device=DEV)),
     lambda: (_snake_planes(),), lambda: (_snake_planes().flip(0).contiguous(),), ('envs',))


def _tapes_abi():
    """wurm_single_rollout with both tapes on 9 x 9: the injected form of rollout_s9_kernel.  Every rebuilt snake starts at
    (4, 4) — the only seed cell of a 9 x 9 grid — heading up with its food at (2, 2); food eaten respawns at (6, 6)."""
    T, N = 6, 70
    st = _single_common()
    flags = {k: torch.zeros((T, N), dtype=torch.uint8, device=DEV) for k in ('done', 'self_collision', 'edge_collision')}
    st.update(flags, reward=torch.zeros((T, N), device=DEV), obs=torch.zeros((T, N, 75), device=DEV), num_steps=T, call0=100,
              inject_food=torch.full((T, N), 6 * 9 + 6, dtype=torch.int32, device=DEV),
              inject_reset=torch.tensor([4, 4, 0, 2 * 9 + 2], dtype=torch.int32, device=DEV).repeat(T, N, 1).contiguous())
    return st


_abi('wurm_single_rollout with both tapes (rollout_s9_injected)', ('wurm_single_rollout',), _tapes_abi,
     lambda: (_rand(27, 4, 6, 70),), lambda: (_rand(28, 4, 6, 70),), ('actions',), route=(_single_route, 'rollout_s9_injected'))


def _policy_abi():
    env = _snake(9, 70, 'partial_2')
    obs0 = env.reset().reshape(70, 75).clone()
    T, N = 5, 70
    return dict(envs=env.envs.clone(), obs0=obs0, actions=torch.zeros((T, N), dtype=torch.long, device=DEV),
                probs=torch.zeros((T, N, 4), device=DEV), values=torch.zeros((T, N), device=DEV),
                reward=torch.zeros((T, N), device=DEV), obs=torch.zeros((T, N, 75), device=DEV),
                status=torch.zeros(N, dtype=torch.uint8, device=DEV), obs_n=2, num_envs=N, size=9, num_steps=T, seed=11,
                call0=50, env_offset=0, **{k: torch.zeros((T, N), dtype=torch.uint8, device=DEV)
                                           for k in ('done', 'self_collision', 'edge_collision')})


_abi('wurm_single_policy_rollout (what check=True launches)', ('wurm_single_policy_rollout',), _policy_abi,
     lambda: (_policy_params(75, 1),), lambda: (_policy_params(75, 2),), ('params',))


def _single_stats_abi():
    N = 70
    return dict(envs=_snake_planes(), accum=torch.zeros(8, dtype=torch.float64, device=DEV), num_envs=N, size=9)


def _single_stats_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    flag = lambda: (torch.rand(70, generator=g) < 0.4).to(torch.uint8).to(DEV)   # noqa: E731
    return torch.randn(70, generator=g).to(DEV), flag(), flag(), flag()


_abi('wurm_single_stats', ('wurm_single_stats',), _single_stats_abi, lambda: _single_stats_inputs(1),
     lambda: _single_stats_inputs(2), ('reward', 'done', 'self_collision', 'edge_collision'))


def _grid_planes(N=16, S=9):
    return _gridworld(S, N, 'default').envs.clone()


_abi('wurm_grid_step', ('wurm_grid_step',),
     lambda: dict(envs=_grid_planes(), num_envs=16, size=9, seed=11, env_offset=0, call=100, actions_dtype=_lib.ACT_I64,
                  obs_mode=_lib.OBS_DEFAULT, obs_n=0, inject_food=None, reward=torch.zeros(16, device=DEV),
                  obs=torch.zeros((16, 3, 9, 9), device=DEV), **_outs(16, 'done', 'edge_collision')),
     lambda: (_rand(23, 4, 16),), lambda: (_rand(24, 4, 16),), ('actions',))
_abi('wurm_grid_step_reset (post_reset)', ('wurm_grid_step_reset',),
     lambda: dict(envs=_grid_planes(), num_envs=16, size=9, seed=11, env_offset=0, call=100, pre_call=0, post_reset=1,
                  actions_dtype=_lib.ACT_I64, obs_mode=_lib.OBS_DEFAULT, obs_n=0, start_y=4, start_x=4, c=None,
                  reward=torch.zeros(16, device=DEV), obs=torch.zeros((16, 3, 9, 9), device=DEV),
                  **_outs(16, 'done', 'edge_collision', 'done_copy')),
     lambda: (_rand(23, 4, 16),), lambda: (_rand(24, 4, 16),), ('actions',), block=(_lib.SingleCall, 'c'))


def _multi_planes(K=3, N=17):
    env = _multi(K, N)
    foods, heads, bodies, dones, orientations, colours, boost = [t.clone() for t in env._state()]
    cfg = _lib.MultiConfig.from_buffer_copy(env._cfg())
    return dict(foods=foods, heads=heads, bodies=bodies, dones=dones, orientations=orientations, colours=colours,
                boost_this_step=boost, num_envs=N, num_snakes=K, size=12, _cfg=cfg, seed=7, env_offset=0)


def _multi_step_abi(K=3, N=17):
    st = _multi_planes(K, N)
    f = lambda: torch.zeros(N * K, device=DEV)                          # noqa: E731
    u = lambda n=N * K: torch.zeros(n, dtype=torch.uint8, device=DEV)   # noqa: E731
    st.update(rewards=f(), food_consumed=f(), sizes=f(), snake_collision=u(), edge_collision=u(), all_done=u(N),
              obs=torch.zeros((K, N, 75), device=DEV), obs_mode=_lib.OBS_PARTIAL, obs_n=2, call=100, inject=None,
              agent_major_f32=torch.zeros((3, K, N), device=DEV), agent_major_u8=torch.zeros((4, K, N), dtype=torch.uint8, device=DEV))
    st['cfg'] = ctypes.addressof(st['_cfg'])
    return st


_abi('wurm_multi_step', ('wurm_multi_step',), _multi_step_abi, lambda: (_rand(25, 4, 3, 17),), lambda: (_rand(26, 4, 3, 17),),
     ('actions',))


def _multi_call_abi():
    st = _multi_step_abi()
    st['cfg'] = st['_cfg']      # (the block holds the configuration by value)
    st.update(pre_call=0, c=None, all_done_copy=torch.zeros(17, dtype=torch.uint8, device=DEV))
    return st


_abi('wurm_multi_step_reset', ('wurm_multi_step_reset',), _multi_call_abi, lambda: (_rand(25, 4, 3, 17),),
     lambda: (_rand(26, 4, 3, 17),), ('actions',), block=(_lib.MultiCall, 'c'))


def _multi_packed_abi():
    st = _multi_call_abi()
    K, N = 3, 17
    st.update(out_f32=torch.zeros(6 * K * N, device=DEV), out_u8=torch.zeros(7 * K * N + N, dtype=torch.uint8, device=DEV),
              obs_after=None, apply_pending=0)
    return st


_abi('wurm_multi_step_packed', ('wurm_multi_step_packed',), _multi_packed_abi, lambda: (_rand(25, 4, 3, 17),),
     lambda: (_rand(26, 4, 3, 17),), ('actions',), block=(_lib.MultiCall, 'c'))


def _multi_check_abi():
    return dict(err=torch.zeros(17, dtype=torch.int32, device=DEV), num_envs=17, num_snakes=3, size=12)


def _multi_check_inputs(flip):
    st = _multi_planes()
    t = [st[k] for k in ('foods', 'heads', 'bodies', 'dones')]
    if flip:   # envs in another order, and a second head in every env's first snake: masks that are not all zero
        t[1][::3, 0, 0, 0] = 1.0
    return tuple(t)


_abi('wurm_multi_check (what check_consistency launches)', ('wurm_multi_check',), _multi_check_abi,
     lambda: _multi_check_inputs(False), lambda: _multi_check_inputs(True), ('foods', 'heads', 'bodies', 'dones'))


def _colours_call(x, inputs):
    # (no tensor input: the two calls differ in the counter, which the first input carries on the host side)
    x['colours'].zero_()   # (on the current stream: a launch that went elsewhere wrote before this, and is wiped)
    rc = _lib.lib().wurm_multi_colours(_lib.ptr(x['colours']), 17, 3, 0, 7, int(x['calls'].pop(0)), 0, _lib.stream_ptr())
    assert rc == 0
    torch.add(inputs[0], 1, out=x['echo'])   # something that depends on the gated inputs rides along
    return dict(colours=x['colours'], echo=x['echo'])


CASES.append(Case('abi wurm_multi_colours', lambda: dict(colours=torch.zeros((51, 3), dtype=torch.int16, device=DEV),
                                                         echo=torch.zeros(4, device=DEV), calls=[1, 2, 3, 4]),
                  _colours_call, lambda: (torch.zeros(4, device=DEV),), lambda: (torch.ones(4, device=DEV),),
                  ('wurm_multi_colours',)))

def _learner_abi(stem, members):
    """wurm_a2c_ff_[pop_]<stem> with the arguments of tests/a2c_learner_ref.build_entry_point; the gate rewrites the window"""
    from tests import a2c_learner_ref as ref
    N = 6 if members else 13

    def make():
        return ref.build_entry_point(stem, True, DEV, E_, T_, N, members=members, lrs=(1e-3,) * max(members, 1))

    def call(x, inputs):
        launch, t, window, optional = x
        for k, v in zip(('obs0', 'obs', 'rewards'), inputs):
            window[k].copy_(v)
        assert launch(_lib.stream_ptr()) == _lib.OK
        return dict(t=t, optional={k: v for k, v in optional.items() if k != 'workspace'})

    def inputs(seed):
        g = torch.Generator().manual_seed(seed)
        return tuple(torch.rand(shape, generator=g).to(DEV) for shape in ((N, E_), (T_, N, E_), (T_, N)))

    CASES.append(Case(f'abi wurm_a2c_ff_{"pop_" if members else ""}{stem}', make, call, lambda: inputs(1), lambda: inputs(2),
                      (f'wurm_a2c_ff_{"pop_" if members else ""}{stem}',)))


for _stem, _members in (('update', 0), ('update_gae', 0), ('update', 3), ('grad_gae', 3)):
    _learner_abi(_stem, _members)

# Entry points with a `stream` parameter that no case reaches, each with the reason (tests/test_stream_inventory.py)
NOT_COVERED = {}
