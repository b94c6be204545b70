"""A plain classifier of snake-to-snake encounters in ONE MultiSnake env, judged from the pre-step planes and the K actions.

Numpy integers and loops only; shares no code with oracle/ or wurm_amd/.  It names what a step is ABOUT to contain (who
enters which cell of whom, in which of the two movement phases); what the reference then does with it is recorded, not
computed here (tests/golden/make_golden_multi_events.py prints the outcomes, tests/test_multi_events_cpu.py states them).

The reference's rules used (wurm/envs/multi_snake.py):
* directions: ORIENTATION_FILTERS (wurm/_filters.py:7-28) under conv2d move a head 0: row + 1, 1: col - 1, 2: row - 1,
  3: col + 1;
* an action is direction = a % 4 and boost = a > 3 (:483-484); a move equal to the stored orientation is a reversal and is
  replaced by its opposite (:336-339), the stored orientation becomes (move + 2) % 4 (:355-357);
* a snake boosts when it asks to and its size is >= 4 (:497-498); the boost phase runs only with cfg['boost'] (:503);
* boost phase (:509-605): only boosters move, eat (:514-518), decay unless they ate (:523-526), collide with every other
  head and every body as they are then (:534-547), grow their new head cell (:553), die on the edge (:560-562), and the
  dead are deleted (:595-596); regular phase (:613-677): every living snake does the same.
So a cell of value v is still filled for a head that enters it in a phase when v minus the owner's decays up to and
including that phase is >= 1: a value-1 tail is fatal when its owner does not move in that phase (a non-booster during the
boost phase) or eats in it, and free otherwise.

Classes (i = attacker, j = victim; `boost` says in which cell of a booster the encounter lies):
  same_cell / same_food   i and j move into one free / food cell in the same phase
  swap                    i moves into j's head cell and j into i's, same phase
  into_head               i moves into j's head cell, j moves elsewhere or not at all in that phase
  into_body               the cell holds a value >= 2 of j (after j's earlier decays)
  into_tail               ... value 1, j moves in this phase and does not eat: the tail leaves
  into_tail_growing       ... value 1, j eats in this phase: the tail stays
  into_tail_waiting       ... value 1, j does not move in this phase (i boosts, j does not): the tail stays
  own_tail                i moves into its own value-1 cell
  into_dying              i moves into a head / body cell of j while j's own move of this phase is fatal
  death_over_food         ... and that cell also holds food (only hand-made states have food under a body)
  eat_and_die             i eats in a phase it reaches and makes a fatal move in that or a later phase
  all_die                 every snake alive at the start makes a fatal move
  boost_gated             i asks to boost below size 4 and its one cell is an encounter
  death_on_row_1          a snake that makes a fatal move has cells in row 1 (`dead[:, :, 1, :] = 0`, :418)
  respawn_blocked         respawn_mode 'any', a snake is dead at the start, no seed cell passes the 3 x 3 rule (:848-858)

One class has two outcomes that no geometry tells apart: `own_tail` in a booster's SECOND cell.  Whether the booster pays the
boost cost is a draw (:579); if it does, its tail cell becomes food between the phases (:583-586) and the head eats it.  The
classifier does not split the class on a draw it cannot see; tests/test_multi_events_cpu.py keys the expected outcome of this
one class on the recorded cost bit instead.  For the same reason every class is judged as if no booster paid: in a step of
random actions a cell that a paying booster gives up one phase early may be named into_body / into_tail and be free.
"""
from collections import namedtuple

import numpy as np

Event = namedtuple('Event', 'cls i j boost')   # boost: None | 'first' | 'second'

DELTA = ((1, 0), (0, -1), (-1, 0), (0, 1))
PAIRWISE = ('same_cell', 'same_food', 'swap', 'into_head', 'into_body', 'into_tail', 'into_tail_growing',
            'into_tail_waiting', 'into_dying', 'death_over_food')
FATAL = ('same_cell', 'same_food', 'swap', 'into_head', 'into_body', 'into_tail_growing', 'into_tail_waiting')


def sanitised(action, orientation):
    d = int(action) % 4
    return (d + 2) % 4 if d == int(orientation) else d


def classify(foods, heads, bodies, orientations, dones, actions, cfg):
    """foods (S,S), heads / bodies (K,S,S), orientations / dones / actions (K,) -> list of Event"""
    foods = np.rint(np.asarray(foods, np.float64)).astype(np.int64).copy()
    K, S = heads.shape[0], foods.shape[-1]
    foods = foods.reshape(S, S)
    val = [np.rint(np.asarray(bodies[s], np.float64)).astype(np.int64).reshape(S, S).copy() for s in range(K)]
    alive = [not bool(dones[s]) and val[s].max() > 0 for s in range(K)]
    head, size, move, asks, boosts = [None] * K, [0] * K, [0] * K, [False] * K, [False] * K
    for s in range(K):
        if not alive[s]:
            continue
        (y,), (x,) = np.nonzero(np.asarray(heads[s]).reshape(S, S) > 0.5)
        head[s], size[s] = (int(y), int(x)), int(val[s].max())
        move[s] = sanitised(actions[s], orientations[s])
        asks[s] = int(actions[s]) > 3
        boosts[s] = asks[s] and size[s] >= 4 and bool(cfg['boost'])
    started = [s for s in range(K) if alive[s]]
    events, fatal, ate = [], set(), set()
    first_cell = {s: (head[s][0] + DELTA[move[s]][0], head[s][1] + DELTA[move[s]][1]) for s in started if boosts[s]}

    # respawn_blocked, on the planes as they are now
    dead = [s for s in range(K) if not alive[s]]
    if cfg['respawn_mode'] == 'any' and dead:
        filled = foods > 0
        for s in started:
            filled = filled | (val[s] > 0)
        free = False
        for y in range(2, S - 2):
            for x in range(2, S - 2):
                free = free or not filled[y - 1:y + 2, x - 1:x + 2].any()
        if not free:
            events.append(Event('respawn_blocked', dead[0], dead[0], None))

    for phase in ('first', 'second'):
        movers = [s for s in started if alive[s] and (boosts[s] or phase == 'second')]
        if phase == 'first' and not movers:
            continue
        tgt = {s: (head[s][0] + DELTA[move[s]][0], head[s][1] + DELTA[move[s]][1]) for s in movers}
        wall = {s: not (0 < tgt[s][0] < S - 1 and 0 < tgt[s][1] < S - 1) for s in movers}
        eats = {s: (not wall[s]) and foods[tgt[s]] > 0 for s in movers}
        found, dying = [], set(s for s in movers if wall[s])
        for i in movers:
            if wall[i]:
                continue
            t = tgt[i]
            for j in started:
                if not alive[j]:
                    continue
                if j == i:
                    if val[i][t] == 1 and not eats[i]:
                        found.append(('own_tail', i, i))
                    elif val[i][t] >= 1:
                        dying.add(i)
                    continue
                cls = None
                if j in movers and tgt[j] == t and val[j][t] == 0:
                    occupied = any(val[s][t] > 0 for s in started if alive[s])
                    cls = None if occupied else ('same_food' if foods[t] > 0 else 'same_cell')
                elif head[j] == t:
                    cls = 'swap' if (j in movers and tgt[j] == head[i]) else 'into_head'
                elif val[j][t] >= 2:
                    cls = 'into_body'
                elif val[j][t] == 1:
                    cls = 'into_tail_waiting' if j not in movers else 'into_tail_growing' if eats[j] else 'into_tail'
                if cls is not None:
                    found.append((cls, i, j))
                    if cls in FATAL:
                        dying.add(i)

        def tag(i, j, t):
            if boosts[i]:
                return phase
            if j != i and boosts[j]:
                if first_cell[j] == t:
                    return 'first'
                if phase == 'second' and tgt.get(j) == t:
                    return 'second'
            return None

        for cls, i, j in found:
            b = tag(i, j, tgt[i])
            events.append(Event(cls, i, j, b))
            if cls in ('into_head', 'into_body', 'into_tail_growing', 'into_tail_waiting', 'swap') and j in dying:
                events.append(Event('into_dying', i, j, b))
                if foods[tgt[i]] > 0:
                    events.append(Event('death_over_food', i, j, b))
            if asks[i] and not boosts[i] and cfg['boost'] and size[i] < 4 and j != i:
                events.append(Event('boost_gated', i, j, None))
        for s in movers:
            if eats[s]:
                ate.add(s)
        # what the phase leaves behind: decay, new head cells, eaten food, the dead deleted
        for s in movers:
            if not eats[s]:
                val[s] = np.maximum(val[s] - 1, 0)
        for s in movers:
            if s in dying:
                cells = val[s] > 0
                if not wall[s]:
                    cells[tgt[s]] = True
                if cells[1, :].any():
                    events.append(Event('death_on_row_1', s, s, phase if boosts[s] else None))
        for s in movers:
            if eats[s]:
                foods[tgt[s]] = 0
        for s in movers:
            if s in dying:
                fatal.add(s)
                alive[s] = False
                val[s][...] = 0
            else:
                size[s] += int(eats[s])
                val[s][tgt[s]] = size[s]
                head[s] = tgt[s]
    for s in sorted(fatal & ate):
        events.append(Event('eat_and_die', s, s, 'first' if boosts[s] else None))
    if started and all(s in fatal for s in started):
        events.append(Event('all_die', started[0], started[-1], None))
    return events


def classify_env(st, e, K, actions, cfg):
    """env e of a batched state dict (foods (N,1,S,S), heads / bodies (N*K,1,S,S), ...), actions (K, N)"""
    S = st['foods'].shape[-1]
    sl = slice(e * K, (e + 1) * K)
    return classify(st['foods'][e, 0], st['heads'][sl].reshape(K, S, S), st['bodies'][sl].reshape(K, S, S),
                    st['orientations'][sl], st['dones'][sl], np.asarray(actions)[:, e], cfg)


def census_keys(ev):
    """the census classes one event counts towards"""
    keys = [ev.cls]
    if ev.boost is not None and ev.cls not in ('eat_and_die',):
        keys.append('boost_' + ev.boost)
    return keys


def fixture_events(fx, state_at):
    """every event of every env-step of a loaded fixture: (t, env, Event).  state_at(fx, t) -> the state dict before step t"""
    N, K, _, T = (int(v) for v in fx['meta'][:4])
    out = []
    for t in range(T):
        st = state_at(fx, t)
        for e in range(N):
            out += [(t, e, ev) for ev in classify_env(st, e, K, fx['actions'][t], fx['cfg_dict'])]
    return out


def census(events, N, into=None):
    """class -> dict(n, lt (i < j), gt (i > j), env0, envN): counts over (t, env, Event) triples of one fixture"""
    into = {} if into is None else into
    for t, e, ev in events:
        for key in census_keys(ev):
            c = into.setdefault(key, dict(n=0, lt=0, gt=0, env0=0, envN=0, first=0, second=0))
            c['n'] += 1
            c['lt'] += ev.i < ev.j
            c['gt'] += ev.i > ev.j
            c['env0'] += e == 0
            c['envN'] += e == N - 1
            c['first'] += ev.boost == 'first'
            c['second'] += ev.boost == 'second'
    return into
