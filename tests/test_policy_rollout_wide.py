"""The fused acting loop beyond policy_rollout.hpp's domain (policy_wide.hpp; include/wurm_hip.h:
wurm_single_policy_rollout for 9 <= size <= 64 and obs_n <= 6, wurm_single_policy_rollout_mode, wurm_grid_policy_rollout,
wurm_policy_last_route).

CPU part: the entry points exist and refuse what they do not serve before any launch; the arithmetic spec of
oracle/policy.c against the REAL reference agent on 4, 363 and 507 inputs (tests/golden/make_golden_policy_wide.py).
GPU part: bit for bit against the oracle on every output and the final state — partial_n through
oracle.single_policy_rollout, 'positions' (SingleSnake and SimpleGridworld) against a composition of the oracle's policy
forward, sampler, step and reset; sharding; status flags; the old shapes' routes and WURM_POLICY_WIDE; the Python API."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from wurm_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ['wurm_single_policy_rollout_mode', 'wurm_grid_policy_rollout', 'wurm_policy_last_route']


def _params(E, seed=0, scale=0.3):
    rng = np.random.RandomState(seed)
    return (rng.randn(O.policy_param_count(E)) * scale).astype(np.float32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    x, y = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
    assert x.shape == y.shape, f'{what}: shape {x.shape} vs {y.shape}'
    bad = np.argwhere(x != y)
    assert len(bad) == 0, f'{what}: {len(bad)} mismatches, first at {bad[0].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}'


# ------------------------------------------------------------------------------------------------------- CPU

def test_new_entry_points_are_declared_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name), f'{name} missing from libwurm_hip.so'
    assert _lib.lib().wurm_get_option(b'WURM_POLICY_WIDE') == 0


def _single(lib, obs_mode, obs_n, size, N=4, T=3, ptr=None):
    return lib.wurm_single_policy_rollout_mode(*([ptr] * 12), obs_mode, obs_n, ctypes.c_int64(N), size, ctypes.c_int64(T),
                                               ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int64(0), None)


def _grid(lib, size, start=(2, 2), N=4, T=3, ptr=None):
    return lib.wurm_grid_policy_rollout(*([ptr] * 11), ctypes.c_int64(N), size, ctypes.c_int64(T), start[0], start[1],
                                        ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int64(0), None)


def test_refusals_before_any_launch():
    """Out of the domain: ERR_UNSUPPORTED (n = 7, size 65, the image modes, no observation); null pointers inside it:
    ERR_INVALID_ARG.  Both before a launch, so no device is needed."""
    lib = _lib.lib()
    UNS, INV = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG
    fake = ctypes.c_void_p(16)  # never dereferenced: the refusals come first
    for mode in (_lib.OBS_DEFAULT, _lib.OBS_RAW, _lib.OBS_ONE_CHANNEL, _lib.OBS_NONE):
        assert _single(lib, mode, 0, 12, ptr=fake) == UNS
    assert _single(lib, _lib.OBS_PARTIAL, 7, 20, ptr=fake) == UNS
    assert _single(lib, _lib.OBS_PARTIAL, 2, 65, ptr=fake) == UNS
    assert _single(lib, _lib.OBS_POSITIONS, 0, 65, ptr=fake) == UNS
    assert _single(lib, _lib.OBS_POSITIONS, 0, 8, ptr=fake) == UNS
    assert _grid(lib, 65, ptr=fake) == UNS
    assert _grid(lib, 4, ptr=fake) == UNS
    assert _grid(lib, 9, start=(9, 2), ptr=fake) == UNS
    assert _single(lib, _lib.OBS_PARTIAL, 4, 20) == INV
    assert _single(lib, _lib.OBS_PARTIAL, 6, 64) == INV
    assert _single(lib, _lib.OBS_POSITIONS, 0, 36) == INV
    assert _grid(lib, 9) == INV
    assert _grid(lib, 64, start=(1, 62)) == INV
    # the original entry point: its domain widened, its signature kept
    args = [None] * 12 + [4, ctypes.c_int64(4), 20, ctypes.c_int64(3), ctypes.c_uint64(0), ctypes.c_uint64(0),
                          ctypes.c_int64(0), None]
    assert lib.wurm_single_policy_rollout(*args) == INV
    args[12], args[14] = 7, 20
    assert lib.wurm_single_policy_rollout(*args) == UNS
    assert _single(lib, _lib.OBS_POSITIONS, 0, 12, N=0) == _lib.OK
    assert _grid(lib, 9, T=0) == _lib.OK


WIDE_FIXTURES = ['policy_ff_positions_snake_s12', 'policy_ff_positions_grid_s9', 'policy_ff_n5_s25', 'policy_ff_n6_s36']
# The tolerance of tests/test_policy_rollout.py.  Measured on these fixtures when they were recorded:
# at most 9e-8 on probabilities and 3e-7 on values, so 2e-6 still holds at 507 inputs.
PROB_ATOL, VALUE_RTOL = 2e-6, 1e-5


def _load(name):
    z = np.load(os.path.join(HERE, 'golden', name + '.npz'))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name', WIDE_FIXTURES)
def test_spec_forward_matches_the_reference_agent_wide(name):
    fx = _load(name)
    p, v = O.policy_forward(fx['params'], fx['obs'])
    assert np.abs(p - fx['probs']).max() < PROB_ATOL
    assert np.abs(v - fx['values'][:, 0]).max() < VALUE_RTOL * max(1.0, np.abs(fx['values']).max())
    assert (p.argmax(1) == fx['probs'].argmax(1)).all()


# ------------------------------------------------------------------------------------------------------- GPU

DEV = 'cuda:0'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(shape, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full(shape, float('nan'), dtype=dtype, device=DEV)
    return torch.full(shape, 77, dtype=dtype, device=DEV)


def hip_rollout(envs, obs0, params, T, seed, call0, env_offset=0, mode='partial_2', grid=None):
    """one launch of wurm_single_policy_rollout_mode (grid None) or wurm_grid_policy_rollout (grid = start location);
    envs (numpy) updated in place"""
    lib = _lib.lib()
    N, _, S, _ = envs.shape
    m, n = _lib.parse_obs_mode(mode)
    E = 4 if m == _lib.OBS_POSITIONS else 3 * (2 * n + 1) ** 2
    e, x0, w = _t(envs), _t(np.asarray(obs0, np.float32).reshape(N, E)), _t(np.asarray(params, np.float32))
    actions, probs = _nan((T, N), torch.int64), _nan((T, N, 4))
    values, reward = _nan((T, N)), _nan((T, N))
    done, sc, ec = (_nan((T, N), torch.uint8) for _ in range(3))
    obs, status = _nan((T, N, E)), _nan((N,), torch.uint8)
    P = _lib.ptr
    if grid is None:
        rc = lib.wurm_single_policy_rollout_mode(P(e), P(x0), P(w), P(actions), P(probs), P(values), P(reward), P(done),
                                                 P(sc), P(ec), P(obs), P(status), m, n, _lib.i64(N), S, _lib.i64(T),
                                                 _lib.u64(seed), _lib.u64(call0), _lib.i64(env_offset), None)
    else:
        rc = lib.wurm_grid_policy_rollout(P(e), P(x0), P(w), P(actions), P(probs), P(values), P(reward), P(done), P(ec),
                                          P(obs), P(status), _lib.i64(N), S, _lib.i64(T), int(grid[0]), int(grid[1]),
                                          _lib.u64(seed), _lib.u64(call0), _lib.i64(env_offset), None)
    _lib.check(rc, 'policy rollout')
    torch.cuda.synchronize()
    envs[...] = e.cpu().numpy()
    out = dict(actions=actions, probs=probs, values=values, reward=reward, done=done, edge_collision=ec, obs=obs,
               status=status)
    if grid is None:
        out['self_collision'] = sc
    return {k: v.cpu().numpy() for k, v in out.items()}


def oracle_composed(envs, obs0, params, T, seed, call0, env_offset=0, mode='positions', grid=None):
    """the acting loop composed from the oracle's pieces: policy_forward, oracle_policy_sample (RNG_POLICY draw of
    call0 + 2t), single_step / grid_step at call0 + 2t, single_reset / grid_reset at call0 + 2t + 1"""
    sample = O.lib().oracle_policy_sample
    N = envs.shape[0]
    x = np.asarray(obs0, np.float32).reshape(N, -1)
    keys = ['actions', 'probs', 'values', 'reward', 'done', 'edge_collision', 'obs'] + ([] if grid else ['self_collision'])
    out = {k: [] for k in keys}
    for t in range(T):
        call = call0 + 2 * t
        probs, values = O.policy_forward(params, x)
        acts = np.asarray([sample(probs[i].ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(seed), ctypes.c_uint64(call),
                                  ctypes.c_uint64(env_offset + i)) for i in range(N)], np.int64)
        if grid is None:
            obs, r, d, sc, ec = O.single_step(envs, acts, mode, seed, call, env_offset)
            O.single_reset(envs, d, 'none', seed, call + 1, env_offset)
            out['self_collision'].append(sc)
        else:
            obs, r, d, ec = O.grid_step(envs, acts, mode, seed, call, env_offset)
            O.grid_reset(envs, d, grid, 'none', seed, call + 1, env_offset)
        for k, v in zip(['actions', 'probs', 'values', 'reward', 'done', 'edge_collision', 'obs'],
                        [acts, probs, values, r, d, ec, obs.reshape(N, -1)]):
            out[k].append(v)
        x = obs
    return {k: np.stack(v) for k, v in out.items()}


def _snake_start(N, S, mode, seed):
    envs = np.zeros((N, 3, S, S), np.float32)
    obs = O.single_reset(envs, np.ones(N, np.uint8), mode, seed, 0)
    return envs, obs


def _grid_start(N, S, start, seed):
    envs = np.zeros((N, 2, S, S), np.float32)
    obs = O.grid_reset(envs, np.ones(N, np.uint8), start, 'positions', seed, 0)
    return envs, obs


def _compare(ro, rh, eo, eh):
    assert (rh['status'] == 0).all()
    for k in ro:
        _same(ro[k], rh[k], k)
    _same(eo, eh, 'final state')


@pytest.mark.gpu
@pytest.mark.parametrize('S,n,N,T', [(12, 2, 29, 65), (16, 3, 37, 130), (20, 4, 29, 65), (25, 5, 37, 65), (36, 6, 29, 65),
                                     (64, 3, 29, 65), (64, 6, 37, 130), (9, 4, 29, 130), (11, 6, 37, 65),
                                     (20, 4, 700, 40)])
def test_partial_equals_oracle(S, n, N, T):
    """(700 envs: several waves per workgroup and several hundred workgroups)"""
    mode, seed = f'partial_{n}', 40 + S + n
    E = 3 * (2 * n + 1) ** 2
    params = _params(E, seed=S * 10 + n, scale=0.5)
    envs, obs0 = _snake_start(N, S, mode, seed)
    eo, eh = envs.copy(), envs.copy()
    ro = O.single_policy_rollout(eo, obs0, params, T, obs_n=n, seed=seed, call0=1, env_offset=5)
    rh = hip_rollout(eh, obs0, params, T, seed, 1, 5, mode)
    assert _lib.lib().wurm_policy_last_route() == b'policy_wide'
    assert (rh.pop('status') == 0).all()
    for k in ro:
        _same(ro[k], rh[k], k)
    _same(eo, eh, 'final state')
    assert len(np.unique(ro['actions'])) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize('S', [9, 12, 36, 64])
def test_snake_positions_equals_oracle(S):
    N, T, seed = 29, 65 if S > 12 else 130, 70 + S
    params = _params(4, seed=S, scale=0.6)
    envs, obs0 = _snake_start(N, S, 'positions', seed)
    eo, eh = envs.copy(), envs.copy()
    ro = oracle_composed(eo, obs0, params, T, seed, 1, 3)
    rh = hip_rollout(eh, obs0, params, T, seed, 1, 3, 'positions')
    _compare(ro, rh, eo, eh)
    assert len(np.unique(ro['actions'])) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize('S', [5, 9, 17, 64])
@pytest.mark.parametrize('corner', [False, True])
def test_grid_positions_equals_oracle(S, corner):
    N, T, seed = 37, 65, 90 + S
    start = (1, S - 2) if corner else (S // 2, S // 2)
    params = _params(4, seed=S + 1, scale=0.6)
    envs, obs0 = _grid_start(N, S, start, seed)
    eo, eh = envs.copy(), envs.copy()
    ro = oracle_composed(eo, obs0, params, T, seed, 1, 2, grid=start)
    rh = hip_rollout(eh, obs0, params, T, seed, 1, 2, 'positions', grid=start)
    _compare(ro, rh, eo, eh)
    assert _lib.lib().wurm_policy_last_route() == b'policy_wide'
    if S <= 9:
        assert ro['done'].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['snake', 'grid'])
def test_sharding_invariance_wide(family):
    """draws keyed by the global env id: two shards (env_offset 0 / 16) == one batch"""
    N, T, seed = 32, 70, 9
    if family == 'snake':
        S, mode, grid, E = 20, 'partial_4', None, 243
        envs, obs0 = _snake_start(N, S, mode, seed)
    else:
        S, mode, grid, E = 9, 'positions', (4, 4), 4
        envs, obs0 = _grid_start(N, S, grid, seed)
    params = _params(E, seed=4)
    obs0 = np.asarray(obs0, np.float32).reshape(N, E)
    full = envs.copy()
    out = hip_rollout(full, obs0, params, T, seed, 1, 0, mode, grid)
    for lo in (0, 16):
        es = np.ascontiguousarray(envs[lo:lo + 16])
        rs = hip_rollout(es, obs0[lo:lo + 16], params, T, seed, 1, lo, mode, grid)
        for k in ('actions', 'probs', 'values', 'reward', 'done', 'obs'):
            _same(rs[k], out[k][:, lo:lo + 16], f'shard {lo} {k}')
        _same(es, full[lo:lo + 16], f'shard {lo} final state')


@pytest.mark.gpu
def test_status_flags_wide():
    N, T, seed = 12, 30, 1
    # SingleSnake 20 x 20 partial_4: two foods; no body
    envs, obs0 = _snake_start(N, 20, 'partial_4', seed)
    envs[4, 0] = 0
    envs[4, 0, 3, 3] = envs[4, 0, 15, 15] = 1
    envs[9, 2] = 0
    before, eh = envs.copy(), envs.copy()
    params = _params(243, seed=3)
    rh = hip_rollout(eh, obs0, params, T, seed, 1, 0, 'partial_4')
    assert rh['status'].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    _same(eh[[4, 9]], before[[4, 9]], 'flagged snakes untouched')
    assert np.isnan(rh['probs'][:, [4, 9]]).all() and (rh['actions'][:, [4, 9]] == 77).all()
    keep = [i for i in range(N) if i not in (4, 9)]
    for i in keep:  # env ids are global: compare one by one
        ei = envs[i:i + 1].copy()
        ri = O.single_policy_rollout(ei, obs0[i:i + 1], params, T, obs_n=4, seed=seed, call0=1, env_offset=i)
        _same(ri['actions'][:, 0], rh['actions'][:, i], f'actions env {i}')
        _same(ri['obs'][:, 0], rh['obs'][:, i], f'obs env {i}')
        _same(ei[0], eh[i], f'state env {i}')
    # SimpleGridworld 17 x 17 positions: two agents; no food
    genvs, gobs0 = _grid_start(N, 17, (8, 8), seed)
    genvs[2, 1, 3, 3] = 1
    genvs[7, 0] = 0
    gbefore, gh = genvs.copy(), genvs.copy()
    gp = _params(4, seed=5)
    rg = hip_rollout(gh, gobs0, gp, T, seed, 1, 0, 'positions', grid=(8, 8))
    assert rg['status'].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    _same(gh[[2, 7]], gbefore[[2, 7]], 'flagged gridworlds untouched')
    for i in (0, 5, 11):
        gi = genvs[i:i + 1].copy()
        ro = oracle_composed(gi, gobs0[i:i + 1], gp, T, seed, 1, i, grid=(8, 8))
        _same(ro['actions'][:, 0], rg['actions'][:, i], f'grid actions env {i}')
        _same(gi[0], gh[i], f'grid state env {i}')


@pytest.mark.gpu
@pytest.mark.parametrize('S,n', [(9, 2), (9, 0), (10, 1), (11, 3)])
def test_old_domain_routes_and_forced_wide(S, n):
    """S 9-11 with n <= 3 stay on policy_rollout.hpp's kernels; WURM_POLICY_WIDE = 1 moves them to policy_wide_kernel,
    which gives the same bits"""
    lib = _lib.lib()
    N, T, seed, mode = 37, 130, 12, f'partial_{n}'
    E = 3 * (2 * n + 1) ** 2
    params = _params(E, seed=S + n, scale=0.5)
    envs, obs0 = _snake_start(N, S, mode, seed)
    e_old, e_new = envs.copy(), envs.copy()
    r_old = hip_rollout(e_old, obs0, params, T, seed, 1, 0, mode)
    assert lib.wurm_policy_last_route() == (b'policy_s9' if S == 9 else b'policy_generic')
    assert lib.wurm_set_option(b'WURM_POLICY_WIDE', 1) == 0
    try:
        r_new = hip_rollout(e_new, obs0, params, T, seed, 1, 0, mode)
        assert lib.wurm_policy_last_route() == b'policy_wide'
    finally:
        lib.wurm_reset_option(b'WURM_POLICY_WIDE')
    for k in r_old:
        _same(r_old[k], r_new[k], k)
    _same(e_old, e_new, 'final state')
    hip_rollout(envs.copy(), obs0, params, 3, seed, 1, 0, mode)
    assert lib.wurm_policy_last_route() == (b'policy_s9' if S == 9 else b'policy_generic')


@pytest.mark.gpu
@pytest.mark.parametrize('name', WIDE_FIXTURES)
def test_hip_policy_matches_the_reference_agent_wide(name):
    """step 0 (the policy applied to obs0) against the reference's forward"""
    fx = _load(name)
    M, E, n, S = (int(x) for x in fx['meta'])
    if 'grid' in name:
        envs, _ = _grid_start(M, S, (4, 4), 3)
        out = hip_rollout(envs, fx['obs'], fx['params'], 1, 3, 1, 0, 'positions', grid=(4, 4))
    else:
        envs, _ = _snake_start(M, S, 'none', 3)
        out = hip_rollout(envs, fx['obs'], fx['params'], 1, 3, 1, 0, 'positions' if E == 4 else f'partial_{n}')
    assert (out['status'] == 0).all()
    assert np.abs(out['probs'][0] - fx['probs']).max() < PROB_ATOL
    assert np.abs(out['values'][0] - fx['values'][:, 0]).max() < VALUE_RTOL * max(1.0, np.abs(fx['values']).max())


# ------------------------------------------------------------------------------------------------ Python API

def _agent(E, seed):
    from wurm_amd.agents import FeedforwardAgent
    torch.manual_seed(seed)
    return FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV)


def _check_learner_recompute(agent, state, out):
    inputs = torch.cat([state.reshape(1, state.shape[0], -1), out['observations'][:-1].flatten(2)])
    with torch.no_grad():
        probs, values = agent(inputs)
    assert (probs - out['probs']).abs().max().item() < 2e-6
    assert (values.squeeze(-1) - out['values']).abs().max().item() < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize('size,mode', [(20, 'partial_4'), (12, 'positions'), (36, 'partial_5')])
def test_python_api_single_snake(size, mode):
    from wurm_amd.agents import pack_policy_params
    from wurm_amd.envs import SingleSnake
    N, T, seed = 24, 40, 11
    env = SingleSnake(num_envs=N, size=size, observation_mode=mode, device=DEV, seed=seed)
    E = 4 if mode == 'positions' else 3 * (2 * int(mode.split('_')[1]) + 1) ** 2
    agent = _agent(E, size)
    params = pack_policy_params(agent)
    state = env.reset()
    start = env.envs.cpu().numpy().copy()
    call0 = env._call
    out = env.policy_rollout(params, state, T)
    assert env._call == call0 + 2 * T
    assert out['observations'].shape == (T,) + tuple(state.shape)
    if mode == 'positions':
        ref = oracle_composed(start, state.cpu().numpy(), params.cpu().numpy(), T, seed, call0)
    else:
        ref = O.single_policy_rollout(start, state.cpu().numpy(), params.cpu().numpy(), T,
                                      obs_n=int(mode.split('_')[1]), seed=seed, call0=call0)
    _same(out['actions'].cpu().numpy(), ref['actions'], 'actions')
    _same(out['probs'].cpu().numpy(), ref['probs'], 'probs')
    _same(out['values'].cpu().numpy(), ref['values'], 'values')
    _same(out['dones'].cpu().numpy().astype(np.uint8), ref['done'], 'dones')
    _same(out['observations'].cpu().numpy().reshape(T, N, E), ref['obs'].reshape(T, N, E), 'observations')
    _same(env.envs.cpu().numpy(), start, 'final state')
    _check_learner_recompute(agent, state, out)


@pytest.mark.gpu
def test_python_api_gridworld():
    from wurm_amd.agents import pack_policy_params
    from wurm_amd.envs import SimpleGridworld
    N, T, seed, S, start_loc = 24, 50, 13, 9, (3, 5)
    env = SimpleGridworld(num_envs=N, size=S, observation_mode='positions', device=DEV, seed=seed,
                          start_location=start_loc)
    agent = _agent(4, 5)
    params = pack_policy_params(agent)
    state = env.reset()
    start = env.envs.cpu().numpy().copy()
    call0 = env._call
    out = env.policy_rollout(params, state, T)
    assert env._call == call0 + 2 * T
    assert 'self_collision' not in out
    ref = oracle_composed(start, state.cpu().numpy(), params.cpu().numpy(), T, seed, call0, grid=start_loc)
    _same(out['actions'].cpu().numpy(), ref['actions'], 'actions')
    _same(out['probs'].cpu().numpy(), ref['probs'], 'probs')
    _same(out['values'].cpu().numpy(), ref['values'], 'values')
    _same(out['rewards'].cpu().numpy(), ref['reward'], 'rewards')
    _same(out['dones'].cpu().numpy().astype(np.uint8), ref['done'], 'dones')
    _same(out['observations'].cpu().numpy(), ref['obs'], 'observations')
    _same(env.envs.cpu().numpy(), start, 'final state')
    assert ref['done'].sum() > 0
    _check_learner_recompute(agent, state, out)
    for bad in ('default', 'raw'):
        with pytest.raises(NotImplementedError, match='image'):
            SimpleGridworld(num_envs=2, size=S, observation_mode=bad, device=DEV, start_location=start_loc
                            ).policy_rollout(params, state[:2], 3)


@pytest.mark.gpu
def test_python_refusals_say_why():
    from wurm_amd.envs import SingleSnake
    p = torch.zeros(10, device=DEV)
    for mode in ('default', 'raw', 'one_channel'):
        env = SingleSnake(num_envs=2, size=12, observation_mode=mode, device=DEV, seed=1)
        with pytest.raises(NotImplementedError, match='image'):
            env.policy_rollout(p, env.reset(), 3)
    env = SingleSnake(num_envs=2, size=20, observation_mode='partial_7', device=DEV, seed=1)
    with pytest.raises(NotImplementedError, match='n <= 6'):
        env.policy_rollout(p, env.reset(), 3)


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['snake', 'grid'])
@pytest.mark.parametrize('mirror', [True, False])
def test_step_lazy_reset_policy_rollout_step(family, mirror):
    """step -> reset(done) (postponed by the lazy reset) -> policy_rollout -> step equals the oracle composition, with
    the resident mirror on and off"""
    from wurm_amd.agents import pack_policy_params
    from wurm_amd.envs import SimpleGridworld, SingleSnake
    N, T, seed = 64, 20, 21
    if family == 'snake':
        S, mode, grid, E = 20, 'partial_4', None, 243
        env = SingleSnake(num_envs=N, size=S, observation_mode=mode, device=DEV, seed=seed, resident_mirror=mirror)
        ref = np.zeros((N, 3, S, S), np.float32)
        O.single_reset(ref, np.ones(N, np.uint8), 'none', seed, 0)
    else:
        S, mode, grid, E = 9, 'positions', (4, 4), 4
        env = SimpleGridworld(num_envs=N, size=S, observation_mode=mode, device=DEV, seed=seed, start_location=grid,
                              resident_mirror=mirror)
        ref = np.zeros((N, 2, S, S), np.float32)
        O.grid_reset(ref, np.ones(N, np.uint8), grid, 'none', seed, 0)
    assert np.array_equal(env.envs.cpu().numpy(), ref)
    params = pack_policy_params(_agent(E, 7))
    p_np = params.cpu().numpy()
    g = torch.Generator().manual_seed(1)
    call = 1

    def step_both(a):
        nonlocal call
        a_dev, a_ref = a.to(DEV), a.numpy().copy()
        obs, _, done, _ = env.step(a_dev)
        if grid is None:
            o_ref, _, d_ref, _, _ = O.single_step(ref, a_ref, mode, seed, call, 0)
        else:
            o_ref, _, d_ref, _ = O.grid_step(ref, a_ref, mode, seed, call, 0)
        _same(obs.cpu().numpy(), o_ref, f'step obs at call {call}')
        _same(done.squeeze(-1).cpu().numpy().astype(np.uint8), d_ref, f'step done at call {call}')
        call += 1
        return obs, done, d_ref

    obs = None
    for _ in range(40):   # until some env is done, so that the reset below has work to postpone
        obs, done, d_ref = step_both(torch.randint(4, (N,), generator=g))
        state = env.reset(done)
        if grid is None:
            O.single_reset(ref, d_ref, 'none', seed, call, 0)
        else:
            O.grid_reset(ref, d_ref, grid, 'none', seed, call, 0)
        call += 1
        if d_ref.any():
            break
    assert d_ref.any()
    out = env.policy_rollout(params, state, T)
    if grid is None:
        ro = O.single_policy_rollout(ref, state.cpu().numpy(), p_np, T, obs_n=4, seed=seed, call0=call)
    else:
        ro = oracle_composed(ref, state.cpu().numpy(), p_np, T, seed, call, grid=grid)
    call += 2 * T
    _same(out['actions'].cpu().numpy(), ro['actions'], 'rollout actions')
    _same(out['probs'].cpu().numpy(), ro['probs'], 'rollout probs')
    _same(out['observations'].cpu().numpy().reshape(T, N, E), ro['obs'].reshape(T, N, E), 'rollout observations')
    step_both(torch.randint(4, (N,), generator=g))
    _same(env.envs.cpu().numpy(), ref, 'final state')
