"""The windows tests/test_multi_frames_gpu.py replays, and what says that they are not quiet ones.

A case is an env configuration, a seed and a tape seed.  `tape(case, T)` is the (T, K, N) action tape of its `rollout`
window: uniform in 0 .. 7, so half the actions boost (4-7) and a quarter are the stored orientation itself, which the
step's sanitiser turns around.  `oracle_window(case, T)` runs that window on the CPU oracle (oracle/oracle.py draws the
same Philox stream as the kernels): the constructor's colours (call 0) and reset (call 1), then T iterations of step
(call 2 + 2 t) and reset(all_done) (3 + 2 t) — and `events(...)` counts, over chosen envs, what the issue wants to see:
whole-env rebuilds, respawns of a single snake, meals, boosted steps, snake-to-snake collisions.  The GPU test counts
the same five on the twin it steps by hand (`events` takes either); tests/test_multi_frames_cpu.py checks here, without a
device, that the seeds below deliver them."""
from collections import namedtuple

import numpy as np

Case = namedtuple('Case', 'name K S N mode options env_offset seed tape_seed')

CASES = {c.name: c for c in (
    # the reference's own test shape (tests/test_multi_snake_env.py:340)
    Case('k2_s12', 2, 12, 64, 'partial_2', dict(), 0, 4101, 11),
    # crowded: six snakes on 10 x 10, an event every few steps; fixed colours, a shard's env_offset
    Case('crowded', 6, 10, 65, 'partial_2', dict(agent_colours='fixed'), 1000, 4102, 12),
    # the reference's training defaults (experiments/multiagent.py:79-86)
    Case('respawn', 4, 25, 33, 'partial_5', dict(food_mode='random_rate', respawn_mode='any'), 0, 4203, 13),
    # the largest LDS footprint (experiments/speeds.py); no boost
    Case('k10_s36', 10, 36, 5, 'full', dict(boost=False), 1000, 4104, 14),
)}

# T of the windows: 70 and 130 cross one and two 64-step chunks of the action prefetch (the two small shapes only)
TS = {'k2_s12': (0, 1, 3, 70, 130), 'crowded': (0, 1, 3, 70, 130), 'respawn': (0, 1, 3), 'k10_s36': (0, 1, 3)}
# the windows whose events are counted: the crowded case's longest, and one of 130 steps on the respawn case that is run
# for this count (three steps of four snakes on 25 x 25 show nothing)
EVENT_WINDOWS = (('crowded', 130), ('respawn', 130))
EVENT_NAMES = ('rebuild', 'respawn', 'food', 'boost', 'collision')


def select_of(case, extra=()):
    """env 0 and env N - 1, unsorted, one duplicate"""
    N = case.N
    return [N - 1, N // 2, 0, 1, N // 2] + list(extra)


def tape(case, T):
    rs = np.random.RandomState(case.tape_seed)
    return rs.randint(0, 8, size=(T, case.K, case.N)).astype(np.int64)


def make_env(case, device='cuda:0'):
    import torch
    from wurm_amd.envs import MultiSnake
    # manual_setup + reset: the constructor's own two calls (colours: counter 0, the reset of every env: 1) without its
    # RuntimeError for a snake that found no room, which six snakes on 10 x 10 do run into
    env = MultiSnake(num_envs=case.N, num_snakes=case.K, size=case.S, observation_mode=case.mode, device=device,
                     seed=case.seed, env_offset=case.env_offset, manual_setup=True, **case.options)
    env.reset(torch.ones(case.N, dtype=torch.bool, device=device), return_observations=False)
    return env


def oracle_window(case, T):
    """the per-step records of the case's `rollout` window on the CPU oracle, agent-major (T, K, N) like `rollout`'s"""
    from oracle import oracle
    K, S, N, o = case.K, case.S, case.N, case.options
    cfg = oracle.multi_cfg(K, boost=o.get('boost', True), food_mode=o.get('food_mode', 'only_one'),
                           respawn_mode=o.get('respawn_mode', 'all'),
                           colour_mode='fixed' if o.get('agent_colours') == 'fixed' else 'random')
    st = oracle.multi_empty_state(N, K, S)
    st['colours'] = oracle.multi_colours(N, K, fixed=o.get('agent_colours') == 'fixed', seed=case.seed, call=0,
                                         env_offset=case.env_offset)
    # (a snake that finds no room on a crowded board stays dead: make_env does not go through the constructor's check)
    oracle.multi_reset(st, np.ones(N, np.uint8), cfg, seed=case.seed, call=1, env_offset=case.env_offset)
    acts = tape(case, T)
    rec = dict(dones=[], dones_after=[], all_done=[], food=[], boost=[], snake_collision=[])
    am = lambda a: np.asarray(a).reshape(N, K).T.copy()  # env-major (N K) -> agent-major (K, N)
    for t in range(T):
        r = oracle.multi_step(st, acts[t], cfg, mode=None, seed=case.seed, call=2 + 2 * t, env_offset=case.env_offset)
        rec['dones'].append(am(st['dones']))
        rec['all_done'].append(r['all_done'].copy())
        rec['food'].append(am(r['food']))
        rec['boost'].append(am(st['boost_this_step']))
        rec['snake_collision'].append(am(r['snake_collision']))
        oracle.multi_reset(st, r['all_done'], cfg, seed=case.seed, call=3 + 2 * t, env_offset=case.env_offset)
        rec['dones_after'].append(am(st['dones']))
    return {k: np.stack(v) if v else np.zeros((0,)) for k, v in rec.items()}


def events(win, select):
    """{name: count} over the envs `select` of a window's records: dones, all_done, food, boost, snake_collision as
    `rollout` returns them ((T, K, N) / (T, N)), and dones_after (T, K, N), the flags after each step's reset"""
    sel = sorted(set(int(i) for i in select))
    g = lambda k: np.asarray(win[k])[..., sel]
    dones, after, all_done = g('dones') != 0, g('dones_after') != 0, g('all_done') != 0
    return dict(rebuild=int(all_done.sum()),
                # a snake that was dead after the step and lives after the reset of an env that was not rebuilt
                respawn=int((dones & ~after & ~all_done[:, None, :]).sum()),
                food=int((g('food') > 0).sum()), boost=int((g('boost') != 0).sum()),
                collision=int((g('snake_collision') != 0).sum()))
