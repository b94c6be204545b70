"""The windows tests/test_rollout_frames_gpu.py replays and tests/test_rollout_frames_cpu.py vets without a GPU.

A WINDOW is (family, S, N, T) plus what makes it reproducible: the env seed, the agent seed (policy windows) or the tape
seed (tape windows) and env_offset.  Families:
    'snake'  SingleSnake 'partial_2', actions from policy_rollout with a seeded FeedforwardAgent
    'grid'   SimpleGridworld 'positions' with a start location off the origin, actions from policy_rollout
    'tape'   SingleSnake in a mode policy_rollout refuses ('default'), actions from rollout() on a random tape
Every window starts from the constructor's reset (call counter 0), so its first counter is 1.

The frames of k envs are asked for: `select_of` puts the LAST env first (so the list is unsorted and holds it), then the
two ANCHORS of the window — the first env that eats and the first that finishes an episode inside the first five steps —
then the rest in a seeded shuffle.  With k = 1 only the last env is left, so every window's seed is one at which the LAST
ENV BY ITSELF eats and finishes an episode within the first five steps (`find_window`: the first such seed; at 36 x 36 that
is one seed in several thousand).  So every (window, T in STEPS, k in KS) runs, and every one with T >= 5 shows both events.
tests/test_rollout_frames_cpu.py recomputes every window with the oracle and asserts all of this.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from oracle import oracle as O
from wurm_amd.agents import FeedforwardAgent, pack_policy_params

STEPS = (0, 1, 5, 70)          # 70 crosses the 64-step chunk of the kernels' action prefetch
KS = (1, 4, 65)                # 65: more selected envs than a wave has lanes
START = {5: (2, 2), 9: (3, 5)}  # SimpleGridworld start locations (row, column)

Window = namedtuple('Window', 'family S N seed env_offset a b')

# family, S, N, seed, env_offset, eater, dier           (made by find_window, below)
WINDOWS = [
    Window('snake', 9, 65, 4, 0, 9, 2),
    Window('snake', 9, 130, 24, 0, 14, 4),
    Window('snake', 11, 65, 90, 0, 1, 1),
    Window('snake', 11, 130, 17, 0, 14, 5),
    Window('snake', 12, 65, 20, 0, 9, 1),
    Window('snake', 12, 130, 292, 0, 5, 5),
    Window('snake', 36, 65, 5613, 0, 64, 13),
    Window('snake', 36, 130, 10021, 0, 52, 35),
    Window('grid', 5, 65, 3, 0, 2, 1),
    Window('grid', 5, 130, 9, 0, 2, 0),
    Window('grid', 9, 65, 110, 0, 15, 5),
    Window('grid', 9, 130, 9, 0, 34, 4),
    Window('tape', 9, 65, 18, 0, 13, 3),
    Window('tape', 12, 65, 95, 0, 0, 3),
    Window('snake', 9, 65, 5, 1000, 9, 0),
]


def mode_of(w):
    return {'snake': 'partial_2', 'grid': 'positions', 'tape': 'default'}[w.family]


def make_agent(w):
    """the seeded agent of a policy window (on the CPU; the GPU test moves it)"""
    torch.manual_seed(1000 + w.seed)
    return FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75 if w.family == 'snake' else 4)


def tape_of(w, T, wild=False):
    """(T, N) int64 actions of a tape window, in 0..3 (wild: in -3..7, values the sanitiser maps among them)"""
    lo, hi = (-3, 8) if wild else (0, 4)
    return np.random.RandomState(w.seed).randint(lo, hi, size=(T, w.N)).astype(np.int64)


def select_of(w, k):
    rest = [int(i) for i in np.random.RandomState(w.seed + 7).permutation(w.N)]
    sel = []
    for i in [w.N - 1, w.a, w.b] + rest:
        if i not in sel:
            sel.append(i)
    return sel[:k]


def oracle_window(w, T):
    """The window on the CPU oracle: dict of (T, N) `actions` (sanitised), `done`, `reward` and the final planes `envs`."""
    N, S, seed, off = w.N, w.S, w.seed, w.env_offset
    mode = mode_of(w)
    if w.family == 'grid':
        envs = np.zeros((N, 2, S, S), np.float32)
        x = O.grid_reset(envs, np.ones(N, np.uint8), START[S], mode, seed, 0, off).reshape(N, -1)
        params = pack_policy_params(make_agent(w)).numpy()
        sample = O.lib().oracle_policy_sample
        acts, dones, rewards = [], [], []
        for t in range(T):  # policy_forward, the RNG_POLICY draw of call 1 + 2t, step at 1 + 2t, reset at 2 + 2t
            call = 1 + 2 * t
            probs, _ = O.policy_forward(params, x)
            a = np.asarray([sample(probs[i].ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(seed), ctypes.c_uint64(call),
                                   ctypes.c_uint64(off + i)) for i in range(N)], np.int64)
            obs, r, d, _ = O.grid_step(envs, a, mode, seed, call, off)
            O.grid_reset(envs, d, START[S], 'none', seed, call + 1, off)
            acts.append(a), dones.append(d), rewards.append(r)
            x = obs.reshape(N, -1)
        stack = lambda v, dt: np.stack(v) if v else np.zeros((0, N), dt)
        return dict(actions=stack(acts, np.int64), done=stack(dones, np.uint8), reward=stack(rewards, np.float32), envs=envs)
    envs = np.zeros((N, 3, S, S), np.float32)
    obs0 = O.single_reset(envs, np.ones(N, np.uint8), mode, seed, 0, off)
    if w.family == 'snake':
        params = pack_policy_params(make_agent(w)).numpy()
        r = O.single_policy_rollout(envs, obs0, params, T, obs_n=2, seed=seed, call0=1, env_offset=off)
        return dict(actions=r['actions'], done=r['done'], reward=r['reward'], envs=envs)
    actions = tape_of(w, T)
    r = O.single_rollout(envs, actions, mode, seed, 1, off)
    return dict(actions=actions, done=r['done'], reward=r['reward'], envs=envs)


def events(win, sel, T):
    """(some selected env finished an episode, some selected env ate) within the first T steps"""
    return bool(win['done'][:T][:, sel].any()), bool((win['reward'][:T][:, sel] > 0).any())


def find_window(family, S, N, env_offset=0, seeds=range(1, 20000)):
    """How a row of WINDOWS was made: the first seed at which the last env eats and finishes an episode within five steps
    (an env's window depends on its id alone, so that env is tried by itself: one env at env_offset + N - 1; a tape is
    drawn for the whole batch, so tape windows are tried whole), then the first eater and the first dier of its window."""
    for seed in seeds:
        if family == 'tape':
            win, last = oracle_window(Window(family, S, N, seed, env_offset, 0, 0), 5), N - 1
        else:
            win, last = oracle_window(Window(family, S, 1, seed, env_offset + N - 1, 0, 0), 5), 0
        if all(events(win, [last], 5)):
            w = Window(family, S, N, seed, env_offset, 0, 0)
            win = oracle_window(w, 5)
            eat, die = np.flatnonzero((win['reward'] > 0).any(0)), np.flatnonzero(win['done'].any(0))
            return w._replace(a=int(eat[0]), b=int(die[0]))
    return None
