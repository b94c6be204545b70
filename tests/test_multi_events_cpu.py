"""Snake-to-snake encounters of MultiSnake, recorded from the reference on hand-made states (tests/golden/events_*.npz,
made by tests/golden/make_golden_multi_events.py) and named by the plain classifier tests/multi_events_ref.py.

Census (a condition on the fixtures, checked again when they are recorded).  Classes of the issue's table that are split or
left out, and why:
* `into_tail_waiting` is split off `into_tail`: a booster that enters, in its FIRST cell, the tail of a snake that does not
  boost dies, because only boosters decay in the boost phase (multi_snake.py:523-526); it exists in the first phase only.
* `death_over_food` is recorded with 'full' observations only: the crops' image adds the colours of a body and the food
  under it (:203-209) to a red of 280 / 255, which the fixtures' uint8 colour codes cannot hold.
* `respawn_blocked`, `death_on_row_1`, `all_die`, `eat_and_die`, `boost_gated`, `own_tail` involve one snake (or all), so
  they have no index order; `boost_gated`, `all_die`, `respawn_blocked`, `death_on_row_1` are not met in a boost phase by
  construction.  `death_on_row_1` needs row 1, so its second placement is the top-RIGHT corner.
Uniformity: within a class the reference's outcome for the pair is one function of the class, stated in OUTCOME below as
printed by the recording script.  One class has a second argument: a booster that enters its own tail in its SECOND cell
eats it if and only if it paid the boost cost, because the cost turns the tail cell into food between the two phases
(:579-592).
"""
import glob
import os

import numpy as np
import pytest

from tests import multi_events_ref as mer
from tests import replay
from tests.backends import OracleBackend

NEW = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN, 'events_*.npz')))
OLD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(replay.GOLDEN, '*multi_*.npz')))

PAIR_CLASSES = ('same_cell', 'same_food', 'swap', 'into_head', 'into_body', 'into_tail', 'into_tail_growing', 'into_dying',
                'death_over_food')
BOTH_PHASES = PAIR_CLASSES + ('own_tail',)
ALL_CLASSES = BOTH_PHASES + ('into_tail_waiting', 'eat_and_die', 'all_die', 'boost_first', 'boost_second', 'boost_gated',
                             'death_on_row_1', 'respawn_blocked')

# (dead, snake_collision, edge_collision, ate) of the attacker, then of the victim, at the step of the encounter; the same
# for every variant (no boost, first cell, second cell, the victim boosting), order of indices, placement, shape and mode
OUTCOME = {
    'same_cell': (1, 1, 0, 0, 1, 1, 0, 0),
    'same_food': (1, 1, 0, 1, 1, 1, 0, 1),          # both eat the one food, both die
    'swap': (1, 1, 0, 0, 1, 1, 0, 0),
    'into_head': (1, 1, 0, 0, 0, 0, 0, 0),
    'into_body': (1, 1, 0, 0, 0, 0, 0, 0),
    'into_tail': (0, 0, 0, 0, 0, 0, 0, 0),          # the tail leaves in the same phase
    'into_tail_growing': (1, 1, 0, 0, 0, 0, 0, 1),
    'into_tail_waiting': (1, 1, 0, 0, 0, 0, 0, 0),
    'own_tail': (0, 0, 0, 'cost', 0, 0, 0, 0),      # (the 'victim' is a bystander; 'cost': second cell of a booster that paid)
    'into_dying': (1, 1, 0, 0, 1, 0, 1, 0),         # the victim's body still kills in the step in which it dies
    'death_over_food': (1, 1, 0, 1, 1, 0, 1, 0),    # ... and the food under it is eaten first
    'all_die': (1, 1, 0, 0, 1, 1, 0, 0),
    'boost_gated': (1, 1, 0, 0, 0, 0, 0, 0),
    'death_on_row_1': (1, 0, 1, 0, 0, 0, 0, 0),
    'respawn_blocked': (1, 0, 0, 0, 1, 0, 0, 0),    # dead before, dead after: no seed cell
}


def state_at(fx, t):
    return replay.multi_state(fx, 'state0_') if t == 0 else replay.multi_state(fx, 'reset_', t - 1)


@pytest.fixture(scope='module')
def loaded():
    return {name: replay.load_multi(name) for name in NEW}


@pytest.fixture(scope='module')
def events(loaded):
    return {name: mer.fixture_events(fx, state_at) for name, fx in loaded.items()}


def check_census(total):
    for cls in ALL_CLASSES:
        c = total.get(cls)
        assert c is not None and c['n'] >= 4, (cls, c)
        assert c['env0'] > 0 and c['envN'] > 0, (cls, c)
    for cls in PAIR_CLASSES + ('into_tail_waiting',):
        assert total[cls]['lt'] > 0 and total[cls]['gt'] > 0, (cls, total[cls])
    for cls in BOTH_PHASES:
        assert total[cls]['first'] > 0 and total[cls]['second'] > 0, (cls, total[cls])


def test_there_are_19_fixtures():
    assert len(NEW) == 19


def test_census_of_the_new_fixtures(loaded, events):
    total = {}
    for name, fx in loaded.items():
        mer.census(events[name], int(fx['meta'][0]), total)
    check_census(total)


def test_every_env_holds_the_class_it_was_built_for(loaded, events):
    for name, fx in loaded.items():
        found = {}
        for t, e, ev in events[name]:
            found.setdefault((t, e), []).append(ev)
        for e in range(int(fx['meta'][0])):
            cls, t, (i, j) = str(fx['plan_class'][e]), int(fx['plan_step'][e]), (int(v) for v in fx['plan_pair'][e])
            evs = found.get((t, e), [])
            if cls in ('all_die', 'death_on_row_1', 'respawn_blocked', 'own_tail'):
                assert any(ev.cls == cls for ev in evs), (name, e, cls, evs)
            else:
                assert any(ev.cls == cls and (ev.i, ev.j) == (i, j) for ev in evs), (name, e, cls, (i, j), evs)
            variant = str(fx['plan_variant'][e])
            if fx['cfg_dict']['boost'] and variant in ('first', 'second', 'victim_first', 'victim_second'):
                assert any(ev.cls == cls and ev.boost == variant.split('_')[-1] for ev in evs), (name, e, cls, variant, evs)


def test_outcomes_are_one_function_of_the_class(loaded):
    for name, fx in loaded.items():
        K = int(fx['meta'][1])
        for e in range(int(fx['meta'][0])):
            cls, t, (i, j) = str(fx['plan_class'][e]), int(fx['plan_step'][e]), (int(v) for v in fx['plan_pair'][e])
            got = []
            for s in (i, j):
                a = e * K + s
                got += [int(fx['dones_out'][t, a]), int(fx['snake_collision'][t, a]), int(fx['edge_collision'][t, a]),
                        int(fx['food'][t, a] > 0)]
            paid = int(fx['inj_cost'][t, e * K + i]) if str(fx['plan_variant'][e]) == 'second' else 0
            want = tuple(paid if v == 'cost' else v for v in OUTCOME[cls])
            assert tuple(got) == want, (name, e, cls, str(fx['plan_variant'][e]), got, want)


def test_a_fatal_move_is_fatal_wherever_it_is_found(loaded, events):
    """every event of a fatal class in every step (the random ones included): the attacker is dead after the step.  Env-steps
    in which some snake boosts are left to the steered envs above: whether a booster pays the cost, and so loses one more
    cell between the phases, is a draw the classifier cannot see"""
    n = 0
    for name, fx in loaded.items():
        K = int(fx['meta'][1])
        for t, e, ev in events[name]:
            if ev.cls in mer.FATAL and not (fx['cfg_dict']['boost'] and fx['boost'][t, e * K:(e + 1) * K].any()):
                assert fx['dones_out'][t, e * K + ev.i] == 1 and fx['snake_collision'][t, e * K + ev.i] == 1, (name, t, e, ev)
                n += 1
    assert n > 500, n


@pytest.mark.parametrize('name', NEW)
def test_oracle_matches_the_reference_per_call(name):
    replay.replay_multi(OracleBackend(), replay.load_multi(name))


@pytest.mark.parametrize('name', NEW)
def test_oracle_matches_the_reference_by_rollout(name):
    replay.replay_multi_rollout(OracleBackend(), replay.load_multi(name))


def format_census(total):
    rows = [f'{"class":20s} {"n":>6s} {"i<j":>5s} {"i>j":>5s} {"env0":>5s} {"envN":>5s} {"1st":>5s} {"2nd":>5s}']
    for cls in ALL_CLASSES:
        c = total.get(cls, dict(n=0, lt=0, gt=0, env0=0, envN=0, first=0, second=0))
        rows.append(f'{cls:20s} {c["n"]:6d} {c["lt"]:5d} {c["gt"]:5d} {c["env0"]:5d} {c["envN"]:5d} {c["first"]:5d} {c["second"]:5d}')
    return '\n'.join(rows)


def test_print_the_census_of_the_old_and_new_fixtures(loaded, events):
    """`pytest -s`: what the 16 fixtures of uniformly random actions held (printed, not asserted), next to the new ones"""
    assert len(OLD) == 16
    old = {}
    for name in OLD:
        fx = replay.load_multi(name)
        mer.census(mer.fixture_events(fx, state_at), int(fx['meta'][0]), old)
    new = {}
    for name, fx in loaded.items():
        mer.census(events[name], int(fx['meta'][0]), new)
    print('\nold fixtures (%d):\n%s\nnew fixtures (%d):\n%s' % (len(OLD), format_census(old), len(NEW), format_census(new)))
