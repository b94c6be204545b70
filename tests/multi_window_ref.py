"""A whole policy-driven MultiSnake window on the CPU oracle: what tests/test_multi_window_oracle_*.py share.  Not a test
module.

`oracle_policy_window` restates the contract of `MultiSnake.act_window` (and therefore of `policy_window`) with oracle/ alone,
in numpy: it imports nothing of wurm_amd/envs.  The cases below are the smallest shapes that reach each form of the fused
kernel (one, two and four policy heads resident on chip; weights reloaded per species), and `events`, `census` and
`oracle_frames` say what such a window contains and what it looks like.

Counters, as read from the host code (not from a run):
  * wurm_amd/envs/multi_snake.py: the constructor draws the colours with `_next_call()` = 0; the first `reset` of every env
    (tests build envs with manual_setup=True and reset them once) goes through `_reset_kernel` and takes `_next_call()` = 1.
    A fresh env therefore enters its first window with the env counter c = 2 and `policy_calls` = 0.
  * wurm_amd/envs/_multi_act.py: `act` draws from `policy_calls` and adds one to it; it leaves the env counter alone.  The
    stream of a row is (env_offset + env) * K + k.  `act_window` is T times act / step / reset(dones['__all__']).
  * wurm_amd/envs/_fast_step.py: `launch_multi` steps with `call` and adds one; `reset_lazy` notes `pend_call = call` and adds
    one (an eager `reset` takes `_next_call()`: the same number).  So step t of a window that starts at c draws from c + 2 t,
    its reset from c + 2 t + 1, its policy from p + t; afterwards the counters are c + 2 T and p + T.
  * wurm_amd/envs/_multi_policy_window.py hands the fused launch call0 = `fs.call`, policy_call0 = `policy_calls` and, for a
    reset postponed in front of the window, pre_call = `fs.pend_call`, and then does `_next_call(2 T)`, `policy_calls += T`.
  * an entry (one hand-made step and its reset(done) in front of the window): the step draws from 2, its reset is called at 3
    (applied later, in front of step 0 of the window, with that 3), the window starts at c = 4, p = 0, and its step-0 inputs
    are the observations that hand-made step returned (of the stepped envs, before their reset).
"""
import functools
from collections import namedtuple

import numpy as np

from tests import multi_act_ref
from tests import multi_events_ref as mer

# options: keywords of MultiSnake beyond the shape; scale: factor on the torch-initialised action head and hidden layers
# (multi_act_ref.sharp_params; 1.0 = as torch initialises them); entry: seed of the hand-made step in front, or None
Case = namedtuple('Case', 'name K S N mode P T seed env_offset options scale info events entry')

ANY = dict(food_mode='random_rate', respawn_mode='any')
CASES = {c.name: c for c in (
    # one head resident; the reference's respawning rules
    Case('one_head_any', 2, 10, 65, 'partial_1', 1, 70, 5109, 0, ANY, 1.0, True, True, None),
    # two heads
    Case('two_heads', 4, 8, 65, 'partial_2', 2, 70, 5202, 0, {}, 1.0, True, True, None),
    # four heads (three species take the four-head form), a shard's env_offset, fixed colours, sharpened policies
    Case('four_heads_shard', 3, 9, 130, 'partial_3', 3, 70, 5303, 1000, dict(agent_colours='fixed'), 4.0, True, True, None),
    # weights reloaded per species: 4 species at partial_3
    Case('reload', 4, 9, 9, 'partial_3', 4, 70, 5401, 0, {}, 1.0, True, True, None),
    # species of unequal size
    Case('uneven_species', 3, 10, 5, 'partial_2', 2, 5, 5501, 0, {}, 1.0, False, False, None),
    Case('no_steps', 2, 10, 3, 'partial_1', 1, 0, 5601, 0, ANY, 1.0, True, False, None),
    Case('one_step', 4, 9, 9, 'partial_3', 4, 1, 5701, 7, {}, 1.0, False, False, None),
    # windows entered behind a postponed reset
    # (nine envs of four snakes seldom lose a whole env in one step: seeds 5800 .. 5829 were tried, 5829 is the one that does)
    Case('entry_reload', 4, 9, 9, 'partial_3', 4, 5, 5829, 0, {}, 1.0, True, False, 101),
    Case('entry_four_heads', 3, 9, 130, 'partial_3', 3, 5, 5901, 1000, dict(agent_colours='fixed'), 1.0, False, False, 102),
    Case('entry_one_head_any', 2, 10, 65, 'partial_1', 1, 5, 6001, 0, ANY, 1.0, True, False, 103),
)}
EVENT_CASES = tuple(c.name for c in CASES.values() if c.events)
ENTRY_CASES = tuple(c.name for c in CASES.values() if c.entry is not None)
CHAINED = 'two_heads'     # run as two windows of T // 2 against the one oracle window of T
FRAMES = 'four_heads_shard'

STATE = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'colours', 'boost_this_step')
INFO = ('food', 'size', 'boost', 'snake_collision', 'edge_collision')

Window = namedtuple('Window', 'out final pre dones_after call policy_calls entry')


def num_inputs(case):
    return 3 * (2 * int(case.mode.split('_')[1]) + 1) ** 2


def make_params(case):
    """(P, num_params) numpy: torch-initialised FeedforwardAgents in `pack_policy_params` order"""
    return multi_act_ref.sharp_params(case.P, num_inputs(case), scale=case.scale, seed=case.seed)


def entry_actions(case):
    """the (K, N) actions of the hand-made step in front of an entry case: uniform in 0 .. 7"""
    return np.random.RandomState(case.entry).randint(0, 8, size=(case.K, case.N)).astype(np.int64)


def event_cfg(case):
    """what multi_events_ref.classify reads of the configuration"""
    return dict(boost=case.options.get('boost', True), respawn_mode=case.options.get('respawn_mode', 'all'))


def _copy(st):
    return {k: v.copy() for k, v in st.items()}


def oracle_policy_window(case, params, T, info, entry=None, wrong=None):
    """`act_window(params, state, T, num_species=case.P, info=info)` of a fresh env of `case` on the CPU oracle.

    Set-up: colours at counter 0, the reset of every env at 1 (seed and env_offset of the case).  Without `entry` the step-0
    inputs are `oracle.multi_observe` of that state and the window starts at the counters c = 2, p = 0.  With `entry` (the
    (K, N) actions of one hand-made step) that step runs at 2, its reset(all_done) at 3, the window starts at c = 4, p = 0
    on the observations the hand-made step returned.  Step t: the policy of species k * P // K on the current inputs, sampled
    at (seed, p + t, (env_offset + env) * K + k); `oracle.multi_step` at c + 2 t with the sampled actions, whose observations
    are the next inputs; `oracle.multi_reset(all_done)` at c + 2 t + 1.

    Returns Window(out, final, pre, dones_after, call, policy_calls, entry): `out` has act_window's keys with columns
    k * N + env ('state': the last inputs, (K, N, E)); `final` the state planes after the window, plus 'rewards', the
    env-major rewards of the last step; `pre[t]` the state before step t; `dones_after[t]` the (K, N) flags after step t's
    reset; `call` / `policy_calls` the counters afterwards; `entry` None or dict(all_done, dones) of the hand-made step.

    `wrong` makes one of the composition errors this reference exists to catch, so that a test can say that it would show:
    'policy_counter' (the policy draws from p + t + 1), 'policy_stream' (env_offset left out of the policy draw's stream),
    'reset_crop' (the policy of step t + 1 sees the crops of the reset env instead of the stepped one)."""
    from oracle import oracle
    K, S, N, o = case.K, case.S, case.N, case.options
    E = num_inputs(case)
    seed, off = case.seed, case.env_offset
    fixed = o.get('agent_colours') == 'fixed'
    cfg = oracle.multi_cfg(K, boost=o.get('boost', True), food_mode=o.get('food_mode', 'only_one'),
                           respawn_mode=o.get('respawn_mode', 'all'), colour_mode='fixed' if fixed else 'random')
    st = oracle.multi_empty_state(N, K, S)
    st['colours'] = oracle.multi_colours(N, K, fixed=fixed, seed=seed, call=0, env_offset=off)
    oracle.multi_reset(st, np.ones(N, np.uint8), cfg, seed=seed, call=1, env_offset=off)
    am = lambda a: np.ascontiguousarray(np.asarray(a).reshape(N, K).T).reshape(K * N)  # env-major (N K) -> column k N + env
    call, policy_call, entered, last_rewards = 2, 0, None, np.zeros(N * K, np.float32)
    if entry is None:
        x = oracle.multi_observe(st, case.mode)
    else:
        r = oracle.multi_step(st, entry, cfg, mode=case.mode, seed=seed, call=2, env_offset=off)
        entered = dict(all_done=r['all_done'].copy(), dones=st['dones'].reshape(N, K).copy())
        oracle.multi_reset(st, r['all_done'], cfg, seed=seed, call=3, env_offset=off)
        x, call, last_rewards = r['obs'], 4, r['rewards']
    x = x.reshape(K, N, E)
    keys = ('observations', 'actions', 'probs', 'values', 'rewards', 'dones', 'all_done') + INFO
    rows = {k: [] for k in keys}
    pre, dones_after = [], []
    for t in range(T):
        probs, values, actions = multi_act_ref.expected_rows(params, x, case.P, seed,
                                                             policy_call + t + (wrong == 'policy_counter'),
                                                             0 if wrong == 'policy_stream' else off)
        pre.append(_copy(st))
        r = oracle.multi_step(st, actions, cfg, mode=case.mode, seed=seed, call=call + 2 * t, env_offset=off)
        x = r['obs'].reshape(K, N, E)
        rows['observations'].append(x.reshape(K * N, E))
        rows['actions'].append(actions.reshape(K * N))
        rows['probs'].append(probs.reshape(K * N, 4))
        rows['values'].append(values.reshape(K * N))
        rows['rewards'].append(am(r['rewards']))
        rows['dones'].append(am(st['dones']))
        rows['all_done'].append(r['all_done'].copy())
        rows['food'].append(am(r['food']))
        rows['size'].append(am(r['size']))
        rows['boost'].append(am(st['boost_this_step']))
        rows['snake_collision'].append(am(r['snake_collision']))
        rows['edge_collision'].append(am(r['edge_collision']))
        last_rewards = r['rewards']
        oracle.multi_reset(st, r['all_done'], cfg, seed=seed, call=call + 2 * t + 1, env_offset=off)
        dones_after.append(st['dones'].reshape(N, K).T.copy())
        if wrong == 'reset_crop':
            x = oracle.multi_observe(st, case.mode).reshape(K, N, E)
    empty = dict(observations=((0, K * N, E), np.float32), actions=((0, K * N), np.int64), probs=((0, K * N, 4), np.float32),
                 values=((0, K * N), np.float32), rewards=((0, K * N), np.float32), dones=((0, K * N), np.uint8),
                 all_done=((0, N), np.uint8), food=((0, K * N), np.float32), size=((0, K * N), np.float32),
                 boost=((0, K * N), np.uint8), snake_collision=((0, K * N), np.uint8), edge_collision=((0, K * N), np.uint8))
    out = {k: np.stack(rows[k]) if T else np.zeros(*empty[k]) for k in keys if info or k not in INFO}
    out['state'] = x.copy()
    final = _copy(st)
    final['rewards'] = np.asarray(last_rewards, np.float32).copy()
    return Window(out, final, pre, dones_after, call + 2 * T, policy_call + T, entered)


@functools.lru_cache(maxsize=None)
def window_of(name, T=None):
    """the oracle's window of a case of the table, computed once per process (read only: nobody writes into it)"""
    case = CASES[name]
    entry = entry_actions(case) if case.entry is not None else None
    return oracle_policy_window(case, make_params(case), case.T if T is None else T, True, entry)


def events(win):
    """dict(deaths, rebuilds, meals, respawns) of a window: snakes that died in a step, all_done rebuilds, meals, and single
    respawns — a snake dead after a step and alive after that step's reset in an env that was not rebuilt"""
    d = win.out['dones'] != 0
    if d.shape[0] == 0:
        return dict(deaths=0, rebuilds=0, meals=0, respawns=0)
    T = d.shape[0]
    K, N = win.dones_after[0].shape
    after = np.stack(win.dones_after) != 0                       # (T, K, N)
    before = np.concatenate([(win.pre[0]['dones'].reshape(N, K).T != 0)[None], after[:-1]])
    d3, all_done = d.reshape(T, K, N), win.out['all_done'] != 0
    return dict(deaths=int((d3 & ~before).sum()), rebuilds=int(all_done.sum()), meals=int((win.out['food'] > 0).sum()),
                respawns=int((d3 & ~after & ~all_done[:, None, :]).sum()))


def census(case, win):
    """class -> count of multi_events_ref.classify_env over every pre-step state of the window and the actions sampled"""
    cfg, out = event_cfg(case), {}
    for t, st in enumerate(win.pre):
        actions = win.out['actions'][t].reshape(case.K, case.N)
        for e in range(case.N):
            for ev in mer.classify_env(st, e, case.K, actions, cfg):
                for key in mer.census_keys(ev):
                    out[key] = out.get(key, 0) + 1
    return out


def frames_select(case):
    """the envs whose frames are compared: env 0, env N - 1 and a middle one"""
    return [0, case.N - 1, case.N // 2]


def oracle_frames(states, select):
    """(len(states), len(select), 3, S, S) int16: the reference's env images (wurm/envs/multi_snake.py:194-227) of the envs
    `select` of every state dict, restated in numpy fp32: a body cell shows a third of its snake's colour, the head two
    thirds, half as much again while boosting; food adds 255 of red; an empty cell is white and the edge black"""
    f32 = np.float32
    frames = []
    for st in states:
        N, _, S, _ = st['foods'].shape
        K = st['heads'].shape[0] // N
        edge = np.ones((S, S), np.int16)
        edge[1:-1, 1:-1] = 0
        out = np.zeros((len(select), 3, S, S), np.int16)
        for j, e in enumerate(select):
            img = np.zeros((3, S, S), f32)
            for k in range(K):
                a = e * K + k
                inten = (st['bodies'][a, 0] > 1e-6).astype(f32) * f32(1) / f32(3) + \
                    (st['heads'][a, 0] > 1e-6).astype(f32) * f32(1) / f32(3)
                inten = inten * (f32(1) + f32(0.5) * f32(st['boost_this_step'][a] != 0))
                img = img + inten[None] * st['colours'][a].astype(f32)[:, None, None]
            img = img.astype(np.int16)
            img[0] += (st['foods'][e, 0] > 1e-6).astype(np.int16) * 255
            black = (img == 0).all(axis=0, keepdims=True)
            img = np.where(black, np.int16(255), img)
            out[j] = img * (1 - edge)
        frames.append(out)
    return np.stack(frames)
