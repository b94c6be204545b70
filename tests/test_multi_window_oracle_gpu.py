"""`MultiSnake.policy_window` and `MultiSnake.act_window` against a whole policy-driven window on the CPU oracle
(tests/multi_window_ref.py: oracle_policy_window), bit for bit.

The twin tests (tests/test_multi_policy_window_gpu.py) say that the two agree with each other; they share the step, reset,
crop and policy code and the host counters, so an error of composition made by both — a counter off by one, the crop of
the reset env fed to the policy, `env_offset` left out of the policy draw's stream — is only visible here.  Every key of the
returned dict, the state tensors and the counters afterwards are compared with np.array_equal, floats through their uint32
views: no tolerance anywhere (oracle/policy.c is the bit-exact policy spec both kernels implement).

Cases and what their trajectories contain: tests/test_multi_window_oracle_cpu.py (module docstring), which checks it without
a device.  Routes: `act_window`; `policy_window` RESIDENT with one, two and four heads, the envs per workgroup chosen by
batch size and forced to 1, 2 and 4; RELOAD; each entered fresh, and behind a postponed reset(done) in the RELOAD form, the
four-head form and under respawn_mode 'any' (where that reset respawns single snakes in front of step 0)."""
import numpy as np
import pytest
import torch

from tests import multi_window_ref as W
from wurm_amd import _lib
from wurm_amd.envs import MultiSnake, _multi_policy_window

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RESIDENT, RELOAD = 1, 2


def launches():
    return int(_lib.lib().wurm_launch_count())


def bits(a):
    """a numpy array under a view in which equal means the same bits"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if not np.array_equal(g, w):
        where = np.argwhere(g != w)
        raise AssertionError(f'{what}: {len(where)} of {g.size} elements differ, first at {where[0].tolist()}: '
                             f'{np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)[tuple(where[0])]!r} != '
                             f'{np.asarray(want)[tuple(where[0])]!r}')


def make_env(case):
    # manual_setup + reset: the constructor's own two calls (colours: counter 0, the reset of every env: 1) without its
    # RuntimeError for a snake that found no room, which four snakes on 8 x 8 do run into
    env = MultiSnake(num_envs=case.N, num_snakes=case.K, size=case.S, observation_mode=case.mode, device=DEV, seed=case.seed,
                     env_offset=case.env_offset, manual_setup=True, **case.options)
    env.reset(torch.ones(case.N, dtype=torch.bool, device=DEV), return_observations=False)
    return env


def enter(env, case, win):
    """the policy input of step 0: the env's observations, or (entry cases) those of one hand-made step whose reset(done) is
    left postponed"""
    if case.entry is None:
        return env._observe()
    a = torch.from_numpy(W.entry_actions(case)).to(DEV)
    obs, _, dones, _ = env.step({f'agent_{k}': a[k] for k in range(case.K)})
    env.reset(dones['__all__'], return_observations=False)
    assert env._fs.pending   # the scenario: that reset is still owed
    same(dones['__all__'], win.entry['all_done'], 'all_done of the hand-made step')
    return obs


def check_out(out, want, case, info, rows=slice(None)):
    """every key of a window's dict against the oracle's rows `rows`"""
    keys = ('observations', 'actions', 'probs', 'values', 'rewards', 'dones', 'all_done') + (W.INFO if info else ())
    assert set(out) == set(keys) | {'state'}
    for k in keys:   # (in the order in which an error would spread: what the policy saw and did first)
        same(out[k], want[k][rows], k)
    assert list(out['state']) == [f'agent_{k}' for k in range(case.K)]
    w = 2 * int(case.mode.split('_')[1]) + 1
    last = want['state'] if rows == slice(None) else want['observations'][rows][-1]
    for k, o in enumerate(out['state'].values()):
        assert tuple(o.shape) == (case.N, 3, w, w)
        same(o.reshape(case.N, -1), last.reshape(case.K, case.N, -1)[k], f'state agent_{k}')


def check_env(env, win, call=None, policy_calls=None):
    """the env after the window: the counters, then the state (reading it applies the reset `act_window` leaves postponed)"""
    assert int(env._fs.call) == (win.call if call is None else call)
    assert env.policy_calls == (win.policy_calls if policy_calls is None else policy_calls)
    f = win.final
    same(env.rewards, f['rewards'], 'env.rewards')
    for attr, key in (('foods', 'foods'), ('heads', 'heads'), ('bodies', 'bodies'), ('dones', 'dones'),
                      ('orientations', 'orientations'), ('agent_colours', 'colours'), ('boost_this_step', 'boost_this_step')):
        same(getattr(env, attr), f[key], 'env.' + attr)


def form_of(case):
    return RELOAD if (case.P > 4 or (case.P == 4 and case.mode == 'partial_3')) else RESIDENT


# (case, route, envs per workgroup): act_window once; policy_window by batch size and, RESIDENT, forced to 1, 2 and 4
RUNS = []
for _c in W.CASES.values():
    RUNS.append((_c.name, 'act_window', 0))
    RUNS += [(_c.name, 'policy_window', w) for w in ((0, 1, 2, 4) if form_of(_c) == RESIDENT and _c.T else (0,))]


@pytest.mark.parametrize('name,route,wpb', RUNS, ids=[f'{n}-{r}-wpb{w}' for n, r, w in RUNS])
def test_window_equals_the_oracle(name, route, wpb):
    case, win = W.CASES[name], W.window_of(name)
    env = make_env(case)
    params = torch.from_numpy(W.make_params(case)).to(DEV)
    assert _multi_policy_window.plan(env, case.P) == form_of(case) and env.policy_window_fused(case.P)
    state = enter(env, case, win)
    if case.entry is None:
        same(torch.stack(list(state.values())).reshape(case.K, case.N, -1), W.window_of(name, 0).out['state'], 'inputs of step 0')
    env._policy_window_wpb = wpb
    n0 = launches()
    out = getattr(env, route)(params, state, case.T, num_species=case.P, info=case.info)
    n = launches() - n0
    assert n == ((1 if case.T else 0) if route == 'policy_window' else 2 * case.T)
    check_out(out, win.out, case, case.info)
    check_env(env, win)


@pytest.mark.parametrize('route', ['policy_window', 'act_window'])
def test_two_chained_windows(route):
    """the second window starts at the first's counters and on its last observations: one oracle window of twice the length"""
    case, win = W.CASES[W.CHAINED], W.window_of(W.CHAINED)
    half = case.T // 2
    env = make_env(case)
    params = torch.from_numpy(W.make_params(case)).to(DEV)
    state = env._observe()
    for w in range(2):
        n0 = launches()
        out = getattr(env, route)(params, state, half, num_species=case.P, info=True)
        assert launches() - n0 == (1 if route == 'policy_window' else 2 * half)
        assert (int(env._fs.call), env.policy_calls) == (2 + 2 * half * (w + 1), half * (w + 1))
        check_out(out, win.out, case, True, slice(w * half, (w + 1) * half))
        state = out['state']
    check_env(env, win)


def test_record_frames_of_a_fused_window():
    """the frames replayed from the fused window's `actions` are the pictures of the oracle's per-step states"""
    case, win = W.CASES[W.FRAMES], W.window_of(W.FRAMES)
    select = W.frames_select(case)
    env = make_env(case)
    params = torch.from_numpy(W.make_params(case)).to(DEV)
    state = env._observe()
    want = W.oracle_frames(win.pre + [win.final], select)
    same(env._get_env_images()[select], want[0], 'the env\'s own picture of the start')
    rec = env.record_start(select)
    out = env.policy_window(params, state, case.T, num_species=case.P)
    same(out['actions'], win.out['actions'], 'actions')
    res = env.record_frames(rec, out['actions'])
    assert not res['status'].any()
    same(res['frames'], want, 'frames')
    idx = np.asarray(select)
    aidx = (idx[:, None] * case.K + np.arange(case.K)).reshape(-1)
    for name, key in (('foods', 'foods'), ('heads', 'heads'), ('bodies', 'bodies'), ('dones', 'dones'),
                      ('orientations', 'orientations'), ('agent_colours', 'colours'), ('boost_this_step', 'boost_this_step')):
        same(res['final'][name], win.final[key][idx if name == 'foods' else aidx], 'final ' + name)
