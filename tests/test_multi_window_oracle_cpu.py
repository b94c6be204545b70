"""Conditions on the inputs of tests/test_multi_window_oracle_gpu.py, on the CPU oracle alone: the windows the GPU module
compares bit for bit (tests/multi_window_ref.py) are not quiet ones.  No device, nothing of wurm_amd/envs.

What the oracle's trajectories contain (printed by these tests; events: snakes that died, all_done rebuilds, meals, respawns
of a single snake in an env that was not rebuilt; census: multi_events_ref.classify_env over every pre-step state):
  one_head_any (seed 5109; K 2, S 10, N 65, partial_1, 1 species, random_rate food, respawn 'any', T 70):
    1344 deaths, 141 rebuilds, 487 meals, 1062 single respawns
    same_cell 94, same_food 4, swap 24, into_head 29, into_body 52, into_tail 83, into_tail_growing 5, into_dying 33,
    own_tail 44, eat_and_die 4, all_die 140, death_on_row_1 350, respawn_blocked 18
  two_heads (seed 5202; K 4, S 8, N 65, partial_2, 2 species, T 70):
    280 deaths, 24 rebuilds, 42 meals
    same_cell 10, same_food 2, into_head 18, into_body 22, into_tail 21, into_dying 5, own_tail 11, eat_and_die 2,
    all_die 88, death_on_row_1 84
  four_heads_shard (seed 5303; K 3, S 9, N 130, partial_3, 3 species, env_offset 1000, fixed colours, weights x 4, T 70):
    3264 deaths, 1031 rebuilds, 507 meals; smallest probability 1.1e-9
    same_cell 204, same_food 4, swap 80, into_head 137, into_body 182, into_tail 271, into_tail_growing 5, into_dying 152,
    own_tail 26, eat_and_die 4, all_die 1039, death_on_row_1 794
  reload (seed 5401; K 4, S 9, N 9, partial_3, 4 species, T 70):
    135 deaths, 29 rebuilds, 33 meals
    same_cell 10, swap 2, into_head 10, into_body 4, into_tail 5, into_tail_growing 2, into_dying 3, own_tail 5, all_die 35,
    death_on_row_1 32
(all_die counts the snakes that are on the board: on 8 x 8 and 9 x 9 a fourth snake often finds no room at creation and stays
off it without a done flag, so such an env is not rebuilt when the others die.)  Every class the issue names is reached: the
seeds are the first ones tried.  No boost_* class occurs: the policy head has four actions.
Entries (one hand-made step of actions uniform in 0 .. 7 and its reset(done) in front of the window):
  entry_reload (seed 5829, the one of 5800 .. 5829 that loses a whole env in that step): 1 env all done, 6 partly dead
  entry_four_heads (seed 5901): 2 envs all done, 59 partly dead
  entry_one_head_any (seed 6001): 1 env all done, 9 with a living and a dead snake
"""
import numpy as np
import pytest

from tests import multi_events_ref as mer
from tests import multi_window_ref as W

NAMED = {'same_cell', 'into_body', 'into_tail', 'into_dying', 'all_die'}


def test_table_reaches_every_form():
    cs = W.CASES
    shape = lambda c: (c.mode, c.K, c.P, c.S)
    assert shape(cs['one_head_any']) == ('partial_1', 2, 1, 10) and cs['one_head_any'].options == W.ANY
    assert shape(cs['two_heads']) == ('partial_2', 4, 2, 8) and cs['two_heads'].N == 65
    c = cs['four_heads_shard']
    assert shape(c) == ('partial_3', 3, 3, 9) and (c.N, c.env_offset) == (130, 1000) and c.options == dict(agent_colours='fixed')
    assert shape(cs['reload']) == ('partial_3', 4, 4, 9) and cs['reload'].N == 9
    assert (cs['uneven_species'].K, cs['uneven_species'].P) == (3, 2)
    assert {c.T for c in cs.values()} == {0, 1, 5, 70} and all(c.T == 70 for c in cs.values() if c.events)
    assert set(W.EVENT_CASES) == {'one_head_any', 'two_heads', 'four_heads_shard', 'reload'}
    assert any(c.scale > 1 for c in cs.values()) and any(c.scale == 1.0 for c in cs.values())
    # the entries: RELOAD, four heads, and respawn_mode 'any' with one head
    assert {shape(cs[n]) + (cs[n].options.get('respawn_mode', 'all'),) for n in W.ENTRY_CASES} == {
        ('partial_3', 4, 4, 9, 'all'), ('partial_3', 3, 3, 9, 'all'), ('partial_1', 2, 1, 10, 'any')}
    assert W.CHAINED in cs and cs[W.CHAINED].T % 2 == 0 and W.FRAMES in W.EVENT_CASES
    for c in cs.values():
        assert W.make_params(c).shape == (c.P, 64 * W.num_inputs(c) + 64 + 4096 + 64 + 256 + 4 + 64 + 1)


@pytest.mark.parametrize('name', sorted(W.CASES))
def test_counters_shapes_and_sampler(name):
    case, win = W.CASES[name], W.window_of(name)
    T, KN, E = case.T, case.K * case.N, W.num_inputs(case)
    c0 = 2 if case.entry is None else 4
    assert (win.call, win.policy_calls) == (c0 + 2 * T, T)
    shapes = dict(observations=(T, KN, E), actions=(T, KN), probs=(T, KN, 4), values=(T, KN), rewards=(T, KN),
                  dones=(T, KN), all_done=(T, case.N), state=(case.K, case.N, E))
    shapes.update({k: (T, KN) for k in W.INFO})
    assert {k: v.shape for k, v in win.out.items()} == shapes
    assert len(win.pre) == len(win.dones_after) == T
    if T:
        a, p = win.out['actions'], win.out['probs']
        print(f'{name}: actions {np.bincount(a.ravel(), minlength=4).tolist()}, smallest probability {p.min():.3e}')
        assert set(a.ravel().tolist()) == {0, 1, 2, 3}
        assert bool(np.isfinite(p).all()) and np.allclose(p.sum(-1), 1.0, atol=1e-5)
        assert (p.min() < 1e-3) == (case.scale > 1)
        assert np.array_equal(win.out['state'].reshape(KN, E), win.out['observations'][-1])
        # the policy never boosts
        assert not win.out['boost'].any() and not win.final['boost_this_step'].any()


@pytest.mark.parametrize('name', W.EVENT_CASES)
def test_event_windows_are_not_quiet(name):
    case, win = W.CASES[name], W.window_of(name)
    ev = W.events(win)
    print(name, ev)
    assert ev['deaths'] >= 1 and ev['rebuilds'] >= 1 and ev['meals'] >= 1
    if case.options.get('respawn_mode', 'all') == 'any':
        assert ev['respawns'] >= 1
    else:
        assert ev['respawns'] == 0


def test_respawn_any_is_among_the_event_cases():
    assert any(W.CASES[n].options.get('respawn_mode') == 'any' for n in W.EVENT_CASES)


def test_encounter_classes():
    union = set()
    for name in W.EVENT_CASES:
        cen = W.census(W.CASES[name], W.window_of(name))
        print(name, dict(sorted(cen.items())))
        assert not any(k.startswith('boost_') for k in cen), name
        assert len(set(cen) & set(mer.PAIRWISE)) >= 3, name
        union |= set(cen)
    assert NAMED <= union
    assert {'swap', 'into_head'} & union


@pytest.mark.parametrize('wrong,first', [('policy_counter', 0), ('policy_stream', 0), ('reset_crop', 1)])
def test_composition_errors_would_show(wrong, first):
    """The errors a twin comparison cannot see change the window on these inputs: made on purpose in the reference
    (`wrong=`), each gives other bits from step `first` on, in the keys the GPU module compares.  On entry_four_heads: a
    shard's env_offset, and envs rebuilt at every step (48 all_done rebuilds in its 5 steps)."""
    case, win = W.CASES['entry_four_heads'], W.window_of('entry_four_heads')
    assert case.env_offset != 0 and (win.out['all_done'][:-1] != 0).any(axis=1).all()
    bad = W.oracle_policy_window(case, W.make_params(case), case.T, True, W.entry_actions(case), wrong=wrong)
    differs = lambda k: [bool((win.out[k][t] != bad.out[k][t]).any()) for t in range(case.T)]
    print(wrong, {k: differs(k) for k in ('probs', 'actions', 'observations', 'dones')})
    assert differs('probs') == [False] + [True] * (case.T - 1)
    if wrong == 'reset_crop':   # the inputs of step 1 are other crops where an env was rebuilt: other probabilities, and
        assert not any(differs('actions')[:first]) and any(differs('actions')[first:])   # sooner or later another action
    else:                       # the same probabilities at step 0, other uniforms: other actions at once
        assert differs('actions')[first] and all(differs('observations')[first:])
    assert not np.array_equal(win.final['bodies'], bad.final['bodies'])


def test_frames_of_the_recorded_window_move():
    """the pictures the GPU module compares: of env 0, env N - 1 and a middle env, every one changes at every step and each env
    is rebuilt within the window (observed: 7, 12 and 11 times)"""
    case, win = W.CASES[W.FRAMES], W.window_of(W.FRAMES)
    select = W.frames_select(case)
    assert select == [0, case.N - 1, case.N // 2]
    frames = W.oracle_frames(win.pre + [win.final], select)
    assert frames.shape == (case.T + 1, 3, 3, case.S, case.S) and frames.dtype == np.int16
    assert (frames[1:] != frames[:-1]).any(axis=(2, 3, 4)).all()
    assert (win.out['all_done'][:, select] != 0).any(axis=0).all()
    # the edge is black, an empty cell white, food red, and a snake shows its colour: a head twice as bright as its body
    assert not frames[:, :, :, 0, :].any() and not frames[:, :, :, :, -1].any()
    st, e = win.pre[0], select[0]
    pic = frames[0, 0]
    for k in range(case.K):
        colour = st['colours'][e * case.K + k].astype(np.int64)
        (hy,), (hx,) = np.nonzero(st['heads'][e * case.K + k, 0])
        assert np.abs(pic[:, hy, hx] - 2 * colour // 3).max() <= 1
        (by, bx) = [v[0] for v in np.nonzero((st['bodies'][e * case.K + k, 0] > 0) & (st['heads'][e * case.K + k, 0] == 0))]
        assert np.abs(pic[:, by, bx] - colour // 3).max() <= 1
    free = (st['foods'][e, 0] == 0) & (st['bodies'][e * case.K:(e + 1) * case.K, 0].sum(0) == 0)
    free[0], free[-1], free[:, 0], free[:, -1] = False, False, False, False
    assert (pic[:, free] == 255).all()
    fy, fx = [v[0] for v in np.nonzero(st['foods'][e, 0])]
    assert pic[:, fy, fx].tolist() == [255, 0, 0]


@pytest.mark.parametrize('name', W.ENTRY_CASES)
def test_entries_owe_a_reset(name):
    case, win = W.CASES[name], W.window_of(name)
    a = W.entry_actions(case)
    assert a.shape == (case.K, case.N) and a.min() == 0 and a.max() == 7
    all_done, d = win.entry['all_done'] != 0, win.entry['dones'] != 0
    mixed = d.any(axis=1) & ~d.all(axis=1)
    print(f'{name}: {int(all_done.sum())} envs all done at entry, {int(mixed.sum())} with a living and a dead snake')
    assert all_done.sum() >= 1
    if case.options.get('respawn_mode') == 'any':
        assert mixed.sum() >= 1
        # ... which the reset in front of step 0 respawns: nobody is dead when the window starts, unless it found no room
        assert (win.pre[0]['dones'] != 0).sum() < d[~all_done].sum()
