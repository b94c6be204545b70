"""record_start / record_frames (wurm_amd/csrc/rollout_frames.hpp) against the unfused loop, bit for bit.

The yardstick is a twin object with the same seed, num_envs and env_offset that is stepped call by call:

    for t in range(T): expected[t] = twin._get_rgb(); twin.step(actions[t]); twin.reset(done)
    expected[T] = twin._get_rgb()

The windows, their seeds and the selected envs come from tests/rollout_frames_cases.py (vetted against the CPU oracle in
tests/test_rollout_frames_cpu.py); every parametrised window of T >= 5 asserts from the launch's own `dones` / `rewards`
that a selected env finished an episode and that one ate inside it.  One window serves its k values: several records may
be started in front of the same window."""
import numpy as np
import pytest
import torch

from tests import rollout_frames_cases as C
from wurm_amd import _lib
from wurm_amd.agents import pack_policy_params
from wurm_amd.envs import SimpleGridworld, SingleSnake

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def make_env(w, **kw):
    if w.family == 'grid':
        return SimpleGridworld(num_envs=w.N, size=w.S, observation_mode='positions', device=DEV, seed=w.seed,
                               env_offset=w.env_offset, start_location=C.START[w.S], **kw)
    return SingleSnake(num_envs=w.N, size=w.S, observation_mode=C.mode_of(w), device=DEV, seed=w.seed,
                       env_offset=w.env_offset, **kw)


class Actor(object):
    """what produces a window on an env object: policy_rollout with the window's agent, or rollout() on its tape"""

    def __init__(self, w, env, population=None, wild=False):
        self.w, self.env, self.population, self.t, self.wild = w, env, population, 0, wild
        if w.family != 'tape':
            self.params = pack_policy_params(C.make_agent(w)).to(DEV)
            if population:
                self.params = torch.stack([self.params * (1.0 + 0.25 * p) for p in range(population)]).contiguous()
            self.state = env._observe(C.mode_of(w))  # (consumes no call counter: the twin must see the same ones)

    def window(self, T):
        if self.w.family == 'tape':
            tape = torch.from_numpy(C.tape_of(self.w, self.t + T, self.wild)[self.t:]).to(DEV).contiguous()
            self.t += T
            raw = tape.clone()
            out = self.env.rollout(tape, return_observations=False)
            out['actions'], out['raw'] = tape, raw  # (sanitised in place)
            return out
        out = self.env.policy_rollout(self.params, self.state, T, population=self.population)
        self.state = out['state']
        return out


def unfused(twin, actions):
    """(T + 1, N, 3, S, S) uint8: what `_get_rgb()` shows at the top of every iteration of the per-call loop, and after it"""
    shots = []
    for a in actions:
        shots.append(twin._get_rgb())
        _, _, done, _ = twin.step(a.clone())
        twin.reset(done)
    shots.append(twin._get_rgb())
    shots = torch.stack(shots)
    assert int(shots.min()) >= 0 and int(shots.max()) <= 255
    return shots.to(torch.uint8)


def check_clip(clip, sel, expected, twin, env):
    idx = torch.tensor(sel, device=DEV)
    assert clip['frames'].dtype == torch.uint8 and clip['frames'].shape == (expected.shape[0], len(sel)) + expected.shape[2:]
    assert not bool(clip['status'].any())
    assert torch.equal(clip['frames'], expected[:, idx])
    assert torch.equal(clip['final'], twin.envs[idx])
    assert torch.equal(clip['final'], env.envs[idx])


WINDOW_CASES = [(i, T) for i in range(len(C.WINDOWS)) for T in C.STEPS]


@pytest.mark.parametrize('i,T', WINDOW_CASES, ids=[f'{C.WINDOWS[i].family}-S{C.WINDOWS[i].S}-N{C.WINDOWS[i].N}-'
                                                   f'off{C.WINDOWS[i].env_offset}-T{T}' for i, T in WINDOW_CASES])
def test_frames_equal_the_unfused_loop(i, T):
    w = C.WINDOWS[i]
    env, twin = make_env(w), make_env(w)
    actor = Actor(w, env)
    sels = [C.select_of(w, k) for k in C.KS]
    assert all(s[0] == w.N - 1 for s in sels) and all(s != sorted(s) for s in sels if len(s) > 1)
    recs = [env.record_start(s) for s in sels]
    out = actor.window(T)
    assert out['actions'].shape == (T, w.N)
    clips = [env.record_frames(r, out['actions']) for r in recs]
    expected = unfused(twin, out['actions'])
    for sel, clip in zip(sels, clips):
        check_clip(clip, sel, expected, twin, env)
        if T >= 5:  # the window must have something to show: an episode's end (and the reset behind it) and a meal
            idx = torch.tensor(sel, device=DEV)
            assert bool(out['dones'][:, idx].any()), 'no selected env finished an episode'
            assert bool((out['rewards'][:, idx] > 0).any()), 'no selected env ate'


def _window(family, S, N):
    return next(w for w in C.WINDOWS if (w.family, w.S, w.N, w.env_offset) == (family, S, N, 0))


@pytest.mark.parametrize('family,S', [('snake', 9), ('snake', 12), ('grid', 9)])
def test_population_of_five(family, S):
    """indices are the object's whatever the population: member p's envs replay with their own global ids"""
    w = _window(family, S, 130)
    env, twin = make_env(w), make_env(w)
    actor = Actor(w, env, population=5)
    sel = [129, 26, 0, 52, 103, 77]  # the last env, the first of members 1, 0, 2, and two more
    rec = env.record_start(torch.tensor(sel))
    out = actor.window(70)
    clip = env.record_frames(rec, out['actions'])
    check_clip(clip, sel, unfused(twin, out['actions']), twin, env)


@pytest.mark.parametrize('family,S', [('snake', 9), ('snake', 36), ('grid', 5), ('tape', 12)])
def test_three_chained_windows_and_no_effect_on_results(family, S):
    """each window with its own record_start; the recording object and a twin that never records return the same"""
    w = _window(family, S, 65)
    env, plain, twin = make_env(w), make_env(w), make_env(w)
    actor, plain_actor = Actor(w, env), Actor(w, plain)
    sel = C.select_of(w, 4)
    for T in (5, 70, 1):
        rec = env.record_start(sel)
        out, out_plain = actor.window(T), plain_actor.window(T)
        clip = env.record_frames(rec, out['actions'])
        assert out.keys() == out_plain.keys()
        for key in out:
            if out[key] is not None:
                assert torch.equal(out[key], out_plain[key]), key
        assert torch.equal(env.envs, plain.envs)
        check_clip(clip, sel, unfused(twin, out['actions']), twin, env)
    assert env._call == plain._call == twin._call


@pytest.mark.parametrize('family,S', [('snake', 9), ('snake', 11), ('grid', 9)])
def test_window_after_a_postponed_reset(family, S):
    """steps with `reset(done)` postponed (lazy_reset) until some env has finished: record_start applies the pending reset"""
    w = _window(family, S, 65)
    env, twin = make_env(w), make_env(w)
    g = torch.Generator().manual_seed(3)
    for _ in range(40):
        a = torch.randint(4, (w.N,), generator=g).to(DEV)
        _, _, done, _ = env.step(a.clone())
        env.reset(done, return_observations=False)
        _, _, done2, _ = twin.step(a.clone())
        twin.reset(done2, return_observations=False)
        if bool(done.any()) and env._pending:
            break
    assert env._pending and bool(done.any())
    sel = C.select_of(w, 4) + [int(done.view(-1).nonzero()[0])]
    rec = env.record_start(sel)
    assert not env._pending
    out = Actor(w, env).window(20)
    clip = env.record_frames(rec, out['actions'])
    check_clip(clip, sel, unfused(twin, out['actions']), twin, env)


def test_tape_with_actions_outside_0_3():
    """A tape with values the sanitiser maps (negative, 4 and above: 4 + orientation leaves it AS the orientation).  The twin
    steps on the tape as rollout() was given it; the replay reads the sanitised one and must not sanitise again."""
    w = _window('tape', 9, 65)
    env, twin = make_env(w), make_env(w)
    sel = C.select_of(w, 65)
    rec = env.record_start(sel)
    out = Actor(w, env, wild=True).window(70)
    assert bool(((out['raw'] < 0) | (out['raw'] > 3)).any()) and not torch.equal(out['raw'], out['actions'])
    clip = env.record_frames(rec, out['actions'])
    check_clip(clip, sel, unfused(twin, out['raw']), twin, env)


def test_refusals():
    w = _window('snake', 9, 65)
    env, other = make_env(w), make_env(w)
    actor = Actor(w, env)
    sel = C.select_of(w, 4)
    rec = env.record_start(sel)
    out = actor.window(5)
    acts = out['actions']
    with pytest.raises(RuntimeError, match='another env object'):
        other.record_frames(rec, acts)
    for bad in (acts.to(torch.int32), acts[:, :-1].contiguous(), acts[0], acts.cpu(), acts.t().contiguous().t()):
        with pytest.raises(RuntimeError, match='actions must be'):
            env.record_frames(rec, bad)
    with pytest.raises(RuntimeError, match='stale'):
        env.record_frames(rec, acts[:4].contiguous())             # another window length than the counter shows
    before = env.envs.clone()
    clip = env.record_frames(rec, acts)                           # the refusals consumed nothing
    assert torch.equal(clip['final'], before[torch.tensor(sel, device=DEV)])
    # a step between record_start and the window
    rec = env.record_start(sel)
    _, _, done, _ = env.step(torch.zeros(w.N, dtype=torch.long, device=DEV))
    env.reset(done)
    actor.state = env._observe('partial_2')
    out = actor.window(5)
    with pytest.raises(RuntimeError, match='stale'):
        env.record_frames(rec, out['actions'])
    # a record that is used after the next window
    rec = env.record_start(sel)
    out = actor.window(5)
    actor.window(5)
    with pytest.raises(RuntimeError, match='stale'):
        env.record_frames(rec, out['actions'])
    with pytest.raises(RuntimeError):
        env.record_start([])


@pytest.mark.parametrize('family,S', [('snake', 9), ('grid', 5)])
def test_out_of_range_select(family, S):
    """status set, that env's frames and planes zero, the other envs' frames and the env object undisturbed"""
    w = _window(family, S, 65)
    env, twin = make_env(w), make_env(w)
    actor = Actor(w, env)
    sel = [64, 65, 3, -1, 1 << 40, 17]
    rec = env.record_start(sel)
    out = actor.window(70)
    state, call = env.envs.clone(), env._call
    clip = env.record_frames(rec, out['actions'])
    assert clip['status'].tolist() == [0, 1, 0, 1, 1, 0]
    good, bad = torch.tensor([0, 2, 5], device=DEV), torch.tensor([1, 3, 4], device=DEV)
    assert int(clip['frames'][:, bad].max()) == 0 and float(clip['final'][bad].abs().max()) == 0.0
    expected = unfused(twin, out['actions'])
    idx = torch.tensor([64, 3, 17], device=DEV)
    assert torch.equal(clip['frames'][:, good], expected[:, idx])
    assert torch.equal(clip['final'][good], twin.envs[idx])
    assert torch.equal(env.envs, state) and env._call == call and torch.equal(env.envs, twin.envs)


@pytest.mark.parametrize('family,S,T', [('snake', 9, 70), ('snake', 36, 5), ('grid', 9, 0)])
def test_one_launch_per_record_frames(family, S, T):
    w = _window(family, S, 65)
    env = make_env(w)
    actor = Actor(w, env)
    rec = env.record_start(C.select_of(w, 65))
    out = actor.window(T)
    count = _lib.lib().wurm_launch_count
    before = count()
    env.record_frames(rec, out['actions'])
    assert count() - before == 1


# ---------------------------------------------------------------------------------------------- the examples' --save-video

def _examples():
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    if path not in sys.path:
        sys.path.insert(0, path)


def _same_rows(a, b):
    drop = ('env_steps_per_s',)
    return [{k: v for k, v in r.items() if k not in drop} for r in a] == [{k: v for k, v in r.items() if k not in drop} for r in b]


def test_fused_learner_example_records_and_trains_the_same(tmp_path):
    _examples()
    import a2c_fused_learner
    kw = dict(num_envs=64, size=9, observation='partial_2', steps=40, update_steps=5, log_interval=20, verbose=False)
    path = str(tmp_path / 'clip.npy')
    plain = a2c_fused_learner.run(**kw)
    filmed = a2c_fused_learner.run(save_video=path, video_envs=3, video_interval=2, **kw)
    assert _same_rows(plain, filmed)
    clip = np.load(path)   # windows 0, 2, 4, 6 of 8: T + 1 = 6 frames each, 3 envs on 2 x 2 tiles of 128 pixels
    assert clip.dtype == np.uint8 and clip.shape == (24, 256, 256, 3)
    assert (clip[:, 192:, 192:] == 0).all() and clip[:, :128, :128].max() == 255
    # the first frame is the constructor's reset of envs 0, 1, 2 (and a black tile), tiled as render('rgb_array') tiles
    env = SingleSnake(num_envs=64, size=9, observation_mode='partial_2', device=DEV, seed=0)
    from wurm_amd._render import tile_frames
    first = env._get_rgb()[:4].to(torch.uint8)
    first[3] = 0
    assert np.array_equal(clip[0], tile_frames(first, {'num_rows': 2, 'num_cols': 2, 'size': 128}))


def test_pbt_example_records_the_first_env_of_each_member(tmp_path):
    _examples()
    import a2c_pbt
    kw = dict(num_envs=32, size=9, observation='partial_2', steps=30, update_steps=5, lrs=(1e-4, 1e-3, 3e-3),
              pbt_interval=2, log_interval=15, verbose=False)
    path = str(tmp_path / 'members.npy')
    plain = a2c_pbt.run(**kw)
    filmed = a2c_pbt.run(save_video=path, **kw)
    assert len(plain) == len(filmed) == 3 and all(_same_rows(a, b) for a, b in zip(plain, filmed))
    clip = np.load(path)   # 6 consecutive windows: 6 frames, then 5 each (a window's last frame is the next one's first)
    assert clip.shape == (6 + 5 * 5, 256, 256, 3)
    env = SingleSnake(num_envs=96, size=9, observation_mode='partial_2', device=DEV, seed=0)
    from wurm_amd._render import tile_frames
    first = env._get_rgb()[torch.tensor([0, 32, 64, 0], device=DEV)].to(torch.uint8)
    first[3] = 0
    assert np.array_equal(clip[0], tile_frames(first, {'num_rows': 2, 'num_cols': 2, 'size': 128}))


def test_start_location_changed_since_record_start_is_refused():
    w = _window('grid', 9, 65)
    env = make_env(w)
    actor = Actor(w, env)
    rec = env.record_start([64, 3])
    env.start_location = (5, 3)
    out = actor.window(5)
    with pytest.raises(RuntimeError, match='start_location'):
        env.record_frames(rec, out['actions'])


def test_record_start_between_step_and_reset_keeps_the_reset_postponed():
    """record_start only reads: the `reset(done)` that follows a step directly is still put off into the next launch"""
    w = _window('snake', 9, 65)
    env, twin = make_env(w), make_env(w)
    a = torch.ones(w.N, dtype=torch.long, device=DEV)
    for e in (env, twin):
        _, _, done, _ = e.step(a.clone())
        if e is env:
            env.record_start([0])       # (a record nobody uses)
        e.reset(done, return_observations=False)
        assert e._pending
    assert torch.equal(env.envs, twin.envs)
