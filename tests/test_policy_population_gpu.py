"""`policy_rollout(..., population=P)`: P policies acting in one launch (include/wurm_hip.h:
wurm_single_policy_rollout_pop, wurm_grid_policy_rollout_pop).  Member p of a population env must equal, bit for bit,
a stand-alone env of its M envs (`env_offset` moved by p M, the same seed, the same number of calls) acting with its own
weights through the call without the keyword — on every route, for M = 1, a prime M and an M beyond one workgroup's waves,
across the 64-step chunk boundary, and with the state and call counter carried into a second rollout."""
import pytest
import torch

from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED, BASE = 77, 1000

# (class name, constructor keywords, route)
CONFIGS = {
    's9_partial2': ('SingleSnake', dict(size=9, observation_mode='partial_2'), b'policy_s9'),
    's10_partial1': ('SingleSnake', dict(size=10, observation_mode='partial_1'), b'policy_generic'),
    's12_partial2': ('SingleSnake', dict(size=12, observation_mode='partial_2'), b'policy_wide'),
    's12_positions': ('SingleSnake', dict(size=12, observation_mode='positions'), b'policy_wide'),
    's20_partial5': ('SingleSnake', dict(size=20, observation_mode='partial_5'), b'policy_wide'),  # E = 363
    'grid5_positions': ('SimpleGridworld', dict(size=5, observation_mode='positions', start_location=(2, 2)), b'policy_wide'),
    'grid9_positions': ('SimpleGridworld', dict(size=9, observation_mode='positions', start_location=(4, 4)), b'policy_wide'),
}
SHAPES = [(1, 5), (2, 1), (3, 5), (2, 67)]


def _make(config, num_envs, offset):
    import wurm_amd.envs as envs
    name, kw, _ = CONFIGS[config]
    env = getattr(envs, name)(num_envs=num_envs, env_offset=offset, seed=SEED, device=DEV, **kw)
    return env, env.reset()


def _member_params(P, E):
    rows = []
    for p in range(P):  # another torch seed per member: different weights
        torch.manual_seed(100 + p)
        rows.append(pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)))
    return torch.stack(rows).to(DEV).contiguous()


def _compare_member(res, ref, sl, what):
    assert set(res) == set(ref)
    for k in ref:
        got = res[k][sl] if k in ('state', 'status') else res[k][:, sl]
        assert got.shape == ref[k].shape, (what, k)
        assert torch.equal(got, ref[k]), (what, k)


@pytest.mark.parametrize('T', [7, 70])
@pytest.mark.parametrize('P,M', SHAPES)
@pytest.mark.parametrize('config', list(CONFIGS))
def test_member_equals_stand_alone_run(config, P, M, T):
    route = CONFIGS[config][2]
    lib = _lib.lib()
    env, state = _make(config, P * M, BASE)
    E = state[0].numel()
    params = _member_params(P, E)
    start = env.envs.clone()
    first = env.policy_rollout(params, state, T, population=P)
    assert lib.wurm_policy_last_route() == route
    second = env.policy_rollout(params, first['state'], T, population=P)  # the state and the call counter carried over
    assert lib.wurm_policy_last_route() == route
    assert not first['status'].any() and not second['status'].any()
    assert first['observations'].shape == (T, P * M) + tuple(state.shape[1:]) and first['actions'].shape == (T, P * M)
    for p in range(P):
        sl = slice(p * M, (p + 1) * M)
        ref_env, ref_state = _make(config, M, BASE + p * M)
        # every draw is keyed by the global env id: the stand-alone env starts from the member's slice of the state
        assert torch.equal(ref_env.envs, start[sl]) and torch.equal(ref_state, state[sl])
        r1 = ref_env.policy_rollout(params[p], ref_state, T)
        assert lib.wurm_policy_last_route() == route
        r2 = ref_env.policy_rollout(params[p], r1['state'], T)
        _compare_member(first, r1, sl, (p, 'first'))
        _compare_member(second, r2, sl, (p, 'second'))
        assert torch.equal(env.envs[sl], ref_env.envs), (p, 'final state')
    if P > 1:  # the members really acted with different weights
        assert not torch.equal(first['probs'][0, 0], first['probs'][0, M]) or \
            not torch.equal(first['values'][:, :M], first['values'][:, M:2 * M])


@pytest.mark.parametrize('config', ['s9_partial2', 's10_partial1', 's20_partial5', 'grid5_positions'])
def test_population_of_one_is_the_plain_call(config):
    a, state_a = _make(config, 6, BASE)
    b, state_b = _make(config, 6, BASE)
    params = _member_params(1, state_a[0].numel())
    ra = a.policy_rollout(params, state_a, 70, population=1)
    rb = b.policy_rollout(params[0], state_b, 70)
    assert set(ra) == set(rb)
    for k in rb:
        assert torch.equal(ra[k], rb[k]), k
    assert torch.equal(a.envs, b.envs)


def _raw_population_rollout(env, params, state, T, P, sentinel=7):
    """the population entry point on outputs the caller filled with `sentinel`, as the class calls it"""
    N, dev = env.num_envs, env.device
    shape = tuple(state.shape[1:])
    out = dict(actions=torch.full((T, N), sentinel, dtype=torch.long, device=dev),
               probs=torch.full((T, N, 4), float(sentinel), device=dev), values=torch.full((T, N), float(sentinel), device=dev),
               rewards=torch.full((T, N), float(sentinel), device=dev))
    flags = [torch.full((T, N), sentinel, dtype=torch.uint8, device=dev) for _ in env._FLAG_KEYS]
    out['observations'] = torch.full((T, N) + shape, float(sentinel), device=dev)
    out['status'] = torch.full((N,), sentinel, dtype=torch.uint8, device=dev)
    mode_args = env._mode_info(env.observation_mode)[:2] if env._NAME == 'SingleSnake' else ()
    rc = _lib.call(dev.index, getattr(_lib.lib(), env._POLICY_POP_FN), _lib.ptr(env._state()), _lib.ptr(state),
                   _lib.ptr(params), _lib.ptr(out['actions']), _lib.ptr(out['probs']), _lib.ptr(out['values']),
                   _lib.ptr(out['rewards']), *[_lib.ptr(f) for f in flags], _lib.ptr(out['observations']),
                   _lib.ptr(out['status']), *mode_args, _lib.i64(N), env.size, _lib.i64(T), *env._start_args(),
                   _lib.u64(env.seed), _lib.u64(env._next_call(2 * T)), _lib.i64(env.env_offset),
                   _lib.stream_ptr(dev.index), _lib.i64(P))
    assert rc == _lib.OK
    out.update(zip(env._FLAG_KEYS, flags))
    return out


@pytest.mark.parametrize('config', ['s9_partial2', 's10_partial1', 's12_partial2', 'grid5_positions'])
def test_env_outside_the_domain_is_left_alone(config):
    """An env of member 1 that is not a well-formed state: status != 0, its outputs unwritten, its state untouched;
    the rest of member 1 and the other members as if nothing had happened."""
    P, M, T, bad = 3, 5, 7, 5 + 2
    clean, state = _make(config, P * M, BASE)
    env, _ = _make(config, P * M, BASE)
    params = _member_params(P, state[0].numel())
    env.envs[bad, 2 if CONFIGS[config][0] == 'SingleSnake' else 0] = 0.0  # a snake without a body / a grid with a plane empty
    broken = env.envs[bad].clone()
    want = clean.policy_rollout(params, state, T, population=P)
    got = _raw_population_rollout(env, params, state, T, P)
    assert got['status'][bad] != 0 and int((got['status'] != 0).sum()) == 1
    assert torch.equal(env.envs[bad], broken)
    keep = torch.ones(P * M, dtype=torch.bool, device=DEV)
    keep[bad] = False
    for k, v in got.items():
        if k == 'status':
            continue
        assert bool((v[:, bad] == 7).all()), (k, 'written for the env outside the domain')
        assert torch.equal(v[:, keep], want[k][:, keep].to(v.dtype)), k
    assert torch.equal(env.envs[keep], clean.envs[keep])
    with pytest.raises(RuntimeError):
        env.policy_rollout(params, state, T, population=P)  # check=True reports it


def test_argument_errors():
    env, state = _make('s9_partial2', 6, BASE)
    params = _member_params(3, 75)
    with pytest.raises(RuntimeError):
        env.policy_rollout(params, state, 3, population=4)       # 6 % 4
    with pytest.raises(RuntimeError):
        env.policy_rollout(params, state, 3, population=2)       # 3 rows for 2 members
    with pytest.raises(RuntimeError):
        env.policy_rollout(params.t().contiguous().t(), state, 3, population=3)  # not contiguous
    with pytest.raises(RuntimeError):
        env.policy_rollout(params.double(), state, 3, population=3)
    with pytest.raises(RuntimeError):
        env.policy_rollout(params, state, 3)                     # without the keyword: one row only, as before
    out = env.policy_rollout(params, state, 3, population=3)
    assert out['actions'].shape == (3, 6)
