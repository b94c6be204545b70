"""MultiSnake.record_start / record_frames against the project's own per-call path.

The reference of every comparison is a `copy.deepcopy` twin of the env, made before the window and stepped by hand with the
window's actions — `step`, then `reset(dones['__all__'], return_observations=False)` — whose `_get_env_images()[select]` is
read before every step and after the last reset.  Everything is `torch.equal`: no tolerance anywhere.

Windows: `rollout` on a tape uniform in 0 .. 7 (boost actions, and the stored orientation itself, which the sanitiser
turns around) and `act_window` with one and two species, on the four shapes of tests/multi_frames_cases.py, T in
{0, 1, 3} everywhere and {70, 130} (one and two 64-step chunks of the action prefetch) on the two small shapes.

Event coverage (a quiet window must not pass for a correct one) is asserted on the twin's outputs, over the selected envs.
Seeds found with the CPU oracle (tests/test_multi_frames_cpu.py runs the same count without a device); observed:
    crowded (seed 4102, tape seed 12), T = 130:  4 rebuilds, 9 meals, 10 boosted steps, 16 snake-to-snake collisions
                                                 (no single respawn: respawn_mode is 'all' there)
    respawn (seed 4203, tape seed 13), T = 130:  1 rebuild, 91 single respawns, 80 meals, 151 boosted steps, 29 collisions
"""
import copy

import numpy as np
import pytest
import torch

from tests import multi_frames_cases as C
from wurm_amd import _lib
from wurm_amd.envs import _multi_act, _multi_frames

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUT_KEYS = ('rewards', 'dones', 'food', 'size', 'boost', 'snake_collision', 'edge_collision')


def launches():
    return int(_lib.lib().wurm_launch_count())


def state_at(env, select):
    """the seven state tensors of the envs `select`, in the layout of record_frames' `final`"""
    N, K = env.num_envs, env.num_snakes
    idx = torch.as_tensor(select, dtype=torch.long, device=env.device)
    aidx = (idx[:, None] * K + torch.arange(K, device=env.device)).reshape(-1)
    per_agent = (env.heads, env.bodies, env.dones, env.orientations, env.agent_colours, env.boost_this_step)
    vals = (env.foods.index_select(0, idx),) + tuple(t.index_select(0, aidx) for t in per_agent)
    return dict(zip(_multi_frames.STATE_NAMES, vals))


def by_hand(twin, actions, select):
    """The window on the twin, one call at a time.  actions: (T, K, N) on the device.  Returns the (T + 1, k, 3, S, S) images
    and the per-step records under `rollout`'s names, agent-major (T, K, N), plus dones_after (after each reset)."""
    T, K, N = actions.shape
    idx = torch.as_tensor(select, dtype=torch.long, device=twin.device)
    imgs, rec = [], {k: [] for k in OUT_KEYS + ('all_done', 'observations', 'dones_after')}
    info_key = dict(food='food_', size='size_', boost='boost_', snake_collision='snake_collision_',
                    edge_collision='edge_collision_')
    for t in range(T):
        imgs.append(twin._get_env_images().index_select(0, idx))
        obs, rewards, dones, info = twin.step({f'agent_{k}': actions[t, k] for k in range(K)})
        rec['observations'].append(torch.stack([obs[f'agent_{k}'] for k in range(K)]))
        rec['rewards'].append(torch.stack([rewards[f'agent_{k}'] for k in range(K)]))
        rec['dones'].append(torch.stack([dones[f'agent_{k}'] for k in range(K)]))
        rec['all_done'].append(dones['__all__'].clone())
        for name, prefix in info_key.items():
            rec[name].append(torch.stack([info[f'{prefix}{k}'] for k in range(K)]))
        twin.reset(dones['__all__'], return_observations=False)
        rec['dones_after'].append(twin.dones.view(N, K).t().clone())
    imgs.append(twin._get_env_images().index_select(0, idx))
    return torch.stack(imgs), {k: (torch.stack(v) if v else None) for k, v in rec.items()}


def check_replay(env, res, imgs, select, twin=None):
    valid = [j for j, s in enumerate(select) if 0 <= s < env.num_envs]
    k, S = len(select), env.size
    assert res['frames'].dtype == torch.int16 and tuple(res['frames'].shape) == (imgs.shape[0], k, 3, S, S)
    assert res['status'].dtype == torch.uint8
    assert res['status'].tolist() == [0 if j in valid else 1 for j in range(k)]
    assert torch.equal(res['frames'][:, valid], imgs)
    own = state_at(env, [select[j] for j in valid])
    K = env.num_snakes
    rows = torch.as_tensor([j * K + i for j in valid for i in range(K)], device=env.device)
    for name in _multi_frames.STATE_NAMES:
        got = res['final'][name]
        got = got[valid] if name == 'foods' else got.index_select(0, rows)
        assert got.dtype == own[name].dtype and torch.equal(got, own[name]), name
    if twin is not None:
        theirs = state_at(twin, [select[j] for j in valid])
        for name in _multi_frames.STATE_NAMES:
            assert torch.equal(own[name], theirs[name]), name
        assert int(env._fs.call) == int(twin._fs.call) and env.policy_calls == twin.policy_calls


ROLLOUT_WINDOWS = [(name, T) for name in C.CASES for T in C.TS[name]]


@pytest.mark.parametrize('name,T', ROLLOUT_WINDOWS, ids=[f'{n}-T{t}' for n, t in ROLLOUT_WINDOWS])
def test_rollout_window(name, T):
    case = C.CASES[name]
    env = C.make_env(case, DEV)
    twin = copy.deepcopy(env)
    select = C.select_of(case)
    actions = torch.from_numpy(C.tape(case, T)).to(DEV)
    calls0, policy0 = int(env._fs.call), env.policy_calls
    rec = env.record_start(select)
    assert int(env._fs.call) == calls0 and env.policy_calls == policy0  # nothing consumed
    out = env.rollout(actions, return_observations=T > 0)  # (an empty window has no observation buffer to hand over)
    n0 = launches()
    res = env.record_frames(rec, actions)
    assert launches() == n0 + 1
    again = env.record_frames(rec, actions)
    assert launches() == n0 + 2
    assert torch.equal(res['frames'], again['frames']) and torch.equal(res['status'], again['status'])
    for k in _multi_frames.STATE_NAMES:
        assert torch.equal(res['final'][k], again['final'][k])
    imgs, ref = by_hand(twin, actions, select)
    check_replay(env, res, imgs, select, twin)
    if T > 0:  # the window itself is what it was without a record: bit-equal to the twin's per-call outputs
        for k in OUT_KEYS + ('all_done', 'observations'):
            assert torch.equal(out[k], ref[k].view(out[k].shape)), k
    assert int(env._fs.call) == calls0 + 2 * T


ACT_WINDOWS = [('k2_s12', 1, 0), ('k2_s12', 1, 3), ('k2_s12', 2, 1), ('k2_s12', 2, 70), ('crowded', 2, 3),
               ('crowded', 1, 130), ('respawn', 2, 3), ('respawn', 1, 1)]


@pytest.mark.parametrize('name,species,T', ACT_WINDOWS, ids=[f'{n}-P{p}-T{t}' for n, p, t in ACT_WINDOWS])
def test_act_window(name, species, T):
    case = C.CASES[name]
    env = C.make_env(case, DEV)
    K, N = case.K, case.N
    n = int(case.mode.split('_')[1])
    E = 3 * (2 * n + 1) ** 2
    g = torch.Generator().manual_seed(case.seed + species)
    params = (torch.randn((species, _multi_act.num_policy_params(E)), generator=g) * 0.3).to(DEV)
    state0 = env._observe()
    hand, free = copy.deepcopy(env), copy.deepcopy(env)
    select = C.select_of(case)
    calls0 = int(env._fs.call)
    rec = env.record_start(select)
    out = env.act_window(params, state0, T, num_species=species, info=True)
    assert env.policy_calls == T and int(env._fs.call) == calls0 + 2 * T
    n0 = launches()
    res = env.record_frames(rec, out['actions'])
    assert launches() == n0 + 1
    # a twin that never recorded: the same window, the same counters
    out_free = free.act_window(params, state0, T, num_species=species, info=True)
    for k, v in out.items():
        if k == 'state':
            for a in v:
                assert torch.equal(v[a], out_free[k][a]), (k, a)
        else:
            assert torch.equal(v, out_free[k]), k
    assert free.policy_calls == env.policy_calls and int(free._fs.call) == int(env._fs.call)
    imgs, ref = by_hand(hand, out['actions'].view(T, K, N), select)
    check_replay(env, res, imgs, select)
    theirs, own = state_at(hand, select), state_at(env, select)
    for k in _multi_frames.STATE_NAMES:
        assert torch.equal(own[k], theirs[k]), k
    if T > 0:
        assert torch.equal(out['rewards'], ref['rewards'].view(T, K * N))
        assert torch.equal(out['dones'], ref['dones'].view(T, K * N))


@pytest.mark.parametrize('name,T', [('k2_s12', 3), ('k10_s36', 1)])
def test_select_outside_the_batch(name, T):
    case = C.CASES[name]
    env = C.make_env(case, DEV)
    twin = copy.deepcopy(env)
    select = C.select_of(case, extra=(-1, case.N))
    select = select[:2] + [case.N + 7] + select[2:]   # (and one in the middle: its neighbours are unaffected)
    actions = torch.from_numpy(C.tape(case, T)).to(DEV)
    rec = env.record_start(select)
    env.rollout(actions)
    res = env.record_frames(rec, actions)
    bad = [j for j, s in enumerate(select) if not 0 <= s < case.N]
    assert len(bad) == 3
    assert not res['frames'][:, bad].any()
    K = case.K
    for name_, t in res['final'].items():
        rows = bad if name_ == 'foods' else [j * K + i for j in bad for i in range(K)]
        assert not t[rows].any(), name_
    imgs, _ = by_hand(twin, actions, [s for s in select if 0 <= s < case.N])
    check_replay(env, res, imgs, select, twin)


def test_reset_postponed_before_record_start():
    case = C.CASES['k2_s12']
    env = C.make_env(case, DEV)
    twin = copy.deepcopy(env)
    select = C.select_of(case)
    tape = torch.from_numpy(C.tape(case, 4)).to(DEV)
    for e in (env, twin):
        for t in range(1):
            _, _, dones, _ = e.step({f'agent_{k}': tape[t, k] for k in range(case.K)})
            e.reset(dones['__all__'], return_observations=False)
    assert env._fs.pending           # the scenario: that reset is still owed
    calls0 = int(env._fs.call)
    rec = env.record_start(select)
    assert not env._fs.pending and int(env._fs.call) == calls0
    out = env.rollout(tape[1:].contiguous())
    res = env.record_frames(rec, tape[1:].contiguous())
    imgs, ref = by_hand(twin, tape[1:], select)
    check_replay(env, res, imgs, select, twin)
    for k in OUT_KEYS + ('all_done', 'observations'):
        assert torch.equal(out[k], ref[k].view(out[k].shape)), k


def test_stale_records_are_refused():
    case = C.CASES['k2_s12']
    env, other = C.make_env(case, DEV), C.make_env(case, DEV)
    select = C.select_of(case)
    tape = torch.from_numpy(C.tape(case, 3)).to(DEV)
    step = lambda: env.step({f'agent_{k}': tape[0, k] for k in range(case.K)})
    # a step in between
    rec = env.record_start(select)
    env.rollout(tape)
    step()
    with pytest.raises(RuntimeError, match='stale record'):
        env.record_frames(rec, tape)
    # a second window
    rec = env.record_start(select)
    env.rollout(tape)
    env.rollout(tape)
    with pytest.raises(RuntimeError, match='stale record'):
        env.record_frames(rec, tape)
    # an annealed food_rate between the two calls
    rec = env.record_start(select)
    env.rollout(tape)
    env.food_rate = 2 * env.food_rate
    with pytest.raises(RuntimeError, match='stale record'):
        env.record_frames(rec, tape)
    # a record of another object
    rec_other = other.record_start(select)
    other.rollout(tape)
    rec = env.record_start(select)
    env.rollout(tape)
    with pytest.raises(RuntimeError, match='another env object'):
        env.record_frames(rec_other, tape)
    n0 = launches()
    assert env.record_frames(rec, tape)['status'].tolist() == [0] * len(select)  # (the env's own record still serves)
    assert launches() == n0 + 1
    with pytest.raises(RuntimeError, match='empty'):
        env.record_start([])


@pytest.mark.parametrize('name,T', C.EVENT_WINDOWS)
def test_event_windows(name, T):
    """the condition on the twin's outputs (module docstring), and the frames of the very windows it is put on"""
    case = C.CASES[name]
    env = C.make_env(case, DEV)
    twin = copy.deepcopy(env)
    select = C.select_of(case)
    actions = torch.from_numpy(C.tape(case, T)).to(DEV)
    rec = env.record_start(select)
    env.rollout(actions, return_observations=False)
    res = env.record_frames(rec, actions)
    imgs, ref = by_hand(twin, actions, select)
    ev = C.events({k: ref[k].cpu().numpy() for k in ('dones', 'dones_after', 'all_done', 'food', 'boost',
                                                     'snake_collision')}, select)
    print(name, T, ev)
    for n in C.EVENT_NAMES:
        if n == 'respawn' and case.options.get('respawn_mode', 'all') != 'any':
            continue
        assert ev[n] >= 1, (n, ev)
    check_replay(env, res, imgs, select, twin)
    assert len(torch.unique(res['frames'])) > 4   # (pictures, not a constant)


def test_half_env_is_served():
    case = C.CASES['k2_s12']._replace(options=dict(dtype=torch.half))
    env = C.make_env(case, DEV)
    twin = copy.deepcopy(env)
    select = C.select_of(case)
    actions = torch.from_numpy(C.tape(case, 3)).to(DEV)
    rec = env.record_start(select)
    env.rollout(actions)
    res = env.record_frames(rec, actions)
    imgs, _ = by_hand(twin, actions, select)
    check_replay(env, res, imgs, select, twin)


def test_multi_species_example_saves_video(tmp_path):
    """examples/a2c_multi_species.py --save-video: every second window of four is recorded, three envs on a 2 x 2 grid of
    tiles; the two recorded windows are not neighbours, so both keep their first frame"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import a2c_multi_species
    path = str(tmp_path / 'snakes.npy')
    a2c_multi_species.main(['--num-envs', '8', '--n-agents', '2', '--n-species', '2', '--size', '12', '--total-steps', '640',
                            '--save-video', path, '--video-envs', '3', '--video-interval', '2', '--device', DEV])
    clip = np.load(path)
    assert clip.dtype == np.uint8 and clip.shape == (2 * 21, 256, 256, 3)
    assert (clip[:, 128:, 128:] == 0).all() and len(np.unique(clip[:, :128, :128])) > 2
