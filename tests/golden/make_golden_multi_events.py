"""Hand-made snake-to-snake encounters, recorded from the REAL reference (see make_golden.py: runs where the reference is,
records data only, holds none of its text).

Every env of a fixture is one encounter class of tests/multi_events_ref.py, set up by hand the way the reference's own
tests/test_multi_snake_env.py does: the planes are written into a `manual_setup` object, `check_consistency()` must pass,
and the snakes are then driven into the encounter with chosen actions: at step 0 ('copy' 0) or, started two cells further
back along their paths, at step 2.  Three more steps of seeded random actions follow.  Everything is recorded through
make_golden_multi.Recorder, so every random outcome is injected on replay and `reset(dones['__all__'])` follows every step.

Layout of an env, in local coordinates (row, col) of the board's interior: the attacker A comes up a column, the victim B
along row 1, the encounter cell is (1, c); local (0, 0) is the interior's top-left cell (1, 1) for placement 0 and, turned by
180 degrees, its bottom-right cell for placement 1 (on 25 x 25 and 36 x 36 that is the last group of 64 cells).  The other
K - 2 snakes walk along rows 8 and below.  A and B are snakes (0, K - 1) or (K - 1, 0).

Re-running this script reproduces every array of the committed files exactly (fixed seeds, no other source of randomness);
the files themselves differ in the time stamps that np.savez_compressed writes into the zip entries, and in nothing else.
It asserts the census condition of tests/test_multi_events_cpu.py on what the reference did, and prints the census and the
outcome table that docs/HISTORY.md and that test quote.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_multi as mgm  # noqa: E402
import multi_events_ref as mer  # noqa: E402

MultiSnake = mgm.MultiSnake
D, L, U, R = 0, 1, 2, 3
DELTA = mer.DELTA
T = 6
ROWS, COLS = 8, 10     # the part of the local frame A and B live in


def back_path(head, heading, n):
    """n cells ending at `head`, walked with `heading` at the end; bends (down / right) where the frame ends"""
    path, (y, x), d = [head], head, (heading + 2) % 4
    while len(path) < n:
        ny, nx = y + DELTA[d][0], x + DELTA[d][1]
        if not (0 <= ny < ROWS and 0 <= nx < COLS) or (ny, nx) in path:
            d = D if d in (L, R) else R
            ny, nx = y + DELTA[d][0], x + DELTA[d][1]
        assert 0 <= ny < ROWS + 2 and 0 <= nx < COLS and (ny, nx) not in path, (head, heading, n)
        path.append((ny, nx))
        y, x = ny, nx
    return path[::-1]


def direction(a, b):
    return DELTA.index((b[0] - a[0], b[1] - a[1]))


class Snake(object):
    """a path (cells in the order they are walked) whose last `length` cells are the snake when the encounter happens,
    and the action that makes it"""

    def __init__(self, length, act, boost=False, head=None, heading=None, path=None):
        self.length, self.act, self.boost = length, act, boost
        self.path = path if path is not None else back_path(head, heading, length + 2)
        assert len(self.path) == length + 2

    def cells(self, copy):                       # tail first
        return self.path[2 - copy:len(self.path) - copy]

    def actions(self, copy):
        p = self.path
        walk = [direction(p[k - 1], p[k]) for k in range(len(p) - copy, len(p))]
        return walk + [self.act + (4 if self.boost else 0)]


def scenario(name, variant):
    """-> dict(A=Snake, B=Snake, food=[cells]) in local coordinates"""
    c = 5
    first, second = variant == 'first', variant == 'second'
    la = 4 if variant in ('first', 'second') else 3
    A = Snake(la, U, boost=first or second, head=(3 if second else 2, c), heading=U)
    E = (1, c)
    food = []
    if name in ('same_cell', 'same_food'):
        vb = variant in ('first', 'victim_second')
        hb = (1, c - 2) if variant == 'victim_second' else (1, c - 1)
        B = Snake(4 if vb else 3, R, boost=vb, head=hb, heading=R)
        food = [E] if name == 'same_food' else []
    elif name == 'swap':
        # (second: A's first cell is (2, c), its second B's head; B moves down into the cell A's head is in by then)
        n = 4 if first else 3
        B = Snake(n, D, boost=first, path=[(0, c + k) for k in range(n, 0, -1)] + [(0, c), E])
    elif name == 'into_head':
        if variant == 'victim_first':     # B boosts along row 1 through E; A (no boost) enters E in the regular phase,
            A = Snake(3, U, head=(2, c), heading=U)                     # when B's head is there and about to leave
            B = Snake(4, R, boost=True, head=(1, c - 1), heading=R)
        else:
            B = Snake(3, R, head=E, heading=R)
    elif name == 'into_body':
        B = Snake(3, R, head=(1, c + 1), heading=R)
    elif name in ('into_tail', 'into_tail_growing', 'into_tail_waiting'):
        c = 4
        A = Snake(la, U, boost=first or second, head=(3 if second else 2, c), heading=U)
        E = (1, c)
        if first and name != 'into_tail_waiting':
            B = Snake(4, R, boost=True, head=(1, c + 3), heading=R)
        else:
            B = Snake(3, R, head=(1, c + 2), heading=R)
        if name == 'into_tail_growing':
            hy, hx = B.path[-1]
            food = [(hy, hx + 1)]
    elif name == 'own_tail':
        B = Snake(3, R, head=(5, 5), heading=R)      # (a bystander)
        if second:   # the cell holds 2 now and 1 when A gets there
            A = Snake(6, U, boost=True, path=[(0, c - 2), (0, c - 1), (1, c - 1), (1, c), (1, c + 1), (2, c + 1), (3, c + 1), (3, c)])
        elif first:
            A = Snake(4, U, boost=True, path=[(0, c + 1), (0, c), (1, c), (1, c + 1), (2, c + 1), (2, c)])
        else:
            A = Snake(4, U, path=[(0, c + 1), (0, c), (1, c), (1, c + 1), (2, c + 1), (2, c)])
    elif name == 'death_over_food':
        # as into_dying, with food under E; B is long enough to lie over E already two steps earlier (a head never walks
        # over food without eating it), turns up into row 0 two cells further on and then into the wall
        B = Snake(5, U, boost=first, path=[(1, c + 3), (1, c + 2), (1, c + 1), E, (1, c - 1), (1, c - 2), (0, c - 2)])
        food = [E]
    elif name == 'into_dying':
        # B walks along row 1, turns up into row 0 and then into the wall; E is its value-2 cell
        # (first: B boosts as well, so that it dies in the phase in which A arrives)
        n = 4 if first else 3
        B = Snake(n, U, boost=first, path=[(1, c + k) for k in range(n, 0, -1)] + [E, (0, c)])
    elif name == 'all_die':
        B = Snake(3, R, head=(1, c - 1), heading=R)
    elif name == 'boost_gated':
        A = Snake(3, U, boost=True, head=(2, c), heading=U)
        B = Snake(3, R, head=(1, c + 1), heading=R)
    elif name == 'death_on_row_1':
        A = Snake(3, L, path=[(0, 4), (0, 3), (0, 2), (0, 1), (0, 0)])
        B = Snake(3, R, head=(3, 5), heading=R)
    else:
        raise KeyError(name)
    return dict(A=A, B=B, food=food)


GROUPS = [(n, v) for n in ('same_cell', 'same_food') for v in ('plain', 'first', 'second', 'victim_second')] + \
         [(n, v) for n in ('swap', 'into_head', 'into_body', 'into_tail', 'into_tail_growing', 'own_tail', 'into_dying',
                           'death_over_food') for v in ('plain', 'first', 'second')] + \
         [('into_head', 'victim_first'), ('into_tail_waiting', 'first'), ('all_die', 'plain'), ('boost_gated', 'plain'),
          ('death_on_row_1', 'plain'), ('respawn_blocked', 'plain')]
LEADS = [('respawn_blocked', 'plain'), ('death_over_food', 'plain'), ('same_cell', 'first'), ('same_food', 'plain'),
         ('swap', 'second'), ('into_head', 'plain'), ('into_body', 'plain'), ('into_tail', 'plain'),
         ('into_tail_growing', 'plain'), ('into_tail_waiting', 'first'), ('own_tail', 'plain'), ('into_dying', 'plain'),
         ('all_die', 'plain'), ('boost_gated', 'plain'), ('death_on_row_1', 'plain')]
# (order of A and B, placement, copy): HALF of the 2 x 2 x 2 cross, chosen so that both orders, both placements and both
# copies occur within every group of four envs and every pair of the three occurs in both combinations but one.  The full
# cross would double every file: the six K = 10 files (306 .. 367 KiB for 6 groups each) would have to become twelve to
# stay below the largest older fixture, and the GPU replay of every route doubles with them.
LATIN = [(0, 0, 0), (1, 1, 0), (1, 0, 2), (0, 1, 2)]


def place(cell, S, placement, mirror=False):
    y, x = cell[0] + 1, cell[1] + 1
    if placement == 0:
        return y, x
    return (y, S - 1 - x) if mirror else (S - 1 - y, S - 1 - x)


def turn(d, placement, mirror=False):
    if placement == 0:
        return d
    return ({L: R, R: L}.get(d, d)) if mirror else (d + 2) % 4


def build_env(name, variant, K, S, order, placement, copy, any_mode):
    """-> dict(snakes={index: [global cells, tail first]}, food=[global cells], actions=[steered steps][K], pair=(i, j),
    dead=[indices])"""
    ia, ib = (0, K - 1) if order == 0 else (K - 1, 0)
    mirror = name == 'death_on_row_1'
    snakes, acts, food, dead = {}, {}, [], []
    if name == 'respawn_blocked':
        # snake ia is dead; food on a grid of pitch 3 leaves no seed cell; the living walk between the rows of food
        dead = [ia]
        food = [(y, x) for y in range(3, S - 1, 3) for x in range(3, S - 1, 3)]
        rows = [r for r in range(4, S - 1) if r % 3 != 0]
        for n, s in enumerate(s for s in range(K) if s != ia):
            cells = [(rows[n], 1), (rows[n], 2), (rows[n], 3)]
            snakes[s] = [place((y - 1, x - 1), S, placement) for (y, x) in cells]
            acts[s] = [turn(R, placement)] * (copy + 1)
        food = [place((y - 1, x - 1), S, placement) for (y, x) in food]
        acts[ia] = [0] * (copy + 1)
        steered = [[acts[s][t] for s in range(K)] for t in range(copy + 1)]
        return dict(snakes=snakes, food=food, actions=steered, pair=(ia, ia), dead=dead)
    sc = scenario(name, variant)
    local = {ia: sc['A']}
    if sc['B'] is not None and K > 1:
        local[ib] = sc['B']
    fillers = [s for s in range(K) if s not in local]
    for n, s in enumerate(fillers):
        if name == 'all_die':     # the others walk into the left wall in the same step
            local[s] = Snake(3, L, path=[(3 + n, 4), (3 + n, 3), (3 + n, 2), (3 + n, 1), (3 + n, 0)])
        else:                     # the others start on rows 8 and below in both copies and keep walking right
            snakes[s] = [place((8 + n // 2, 4 * (n % 2) + k), S, placement, mirror) for k in range(3)]
            acts[s] = [turn(R, placement, mirror)] * (copy + 1)
    for s, sn in local.items():
        snakes[s] = [place(cell, S, placement, mirror) for cell in sn.cells(copy)]
        acts[s] = [turn(a % 4, placement, mirror) + (a // 4) * 4 for a in sn.actions(copy)]
    food = [place(cell, S, placement, mirror) for cell in sc['food']] + [place((6, 9), S, placement, mirror)]
    steered = [[acts[s][t] for s in range(K)] for t in range(copy + 1)]
    return dict(snakes=snakes, food=food, actions=steered, pair=(ia, ib if sc['B'] is not None else ia), dead=dead)


def write_env(env, e, K, built):
    for s in range(K):
        a = e * K + s
        env.heads[a].zero_()
        env.bodies[a].zero_()
        if s in built['dead']:
            env.dones[a] = 1
            continue
        cells = built['snakes'][s]
        for v, (y, x) in enumerate(cells, start=1):
            assert env.bodies[e * K:(e + 1) * K, 0, y, x].sum() == 0, ('overlap', e, s, (y, x))
            env.bodies[a, 0, y, x] = v
        hy, hx = cells[-1]
        env.heads[a, 0, hy, hx] = 1
        py, px = cells[-2]
        env.orientations[a] = (mer.DELTA.index((hy - py, hx - px)) + 2) % 4
    env.foods[e].zero_()
    for (y, x) in built['food']:
        env.foods[e, 0, y, x] = 1


def record_events(name, K, S, seed, groups, lead, mode='full', write=True, **kwargs):
    """groups: list of (class, variant); lead: the group whose envs come first and last"""
    any_mode = kwargs.get('respawn_mode', 'all') == 'any'
    plan = []
    for g in groups:
        if g[0] == 'respawn_blocked' and not any_mode:
            continue
        if g[0] == 'death_over_food' and mode != 'full':
            # food under a body is drawn as the SUM of the two colours by the crops' image (:203-209): a red of 280 / 255,
            # which the fixtures' uint8 colour codes cannot hold.  The 'full' files carry the class.
            continue
        envs = [(g, o, p, cp) for (o, p, cp) in LATIN]
        plan.append(envs)
    plan.sort(key=lambda envs: envs[0][0] != lead)          # (stable: the lead group first)
    flat = [x for envs in plan for x in envs]
    # the lead group opens and closes the batch; one more env of it makes N % 4 == 1 (a last workgroup that is not full)
    flat = [flat[0]] + flat[4:] + [flat[1], flat[2], (lead, 0, 0, 2), flat[3]]
    N = len(flat)
    torch.manual_seed(seed)
    env = MultiSnake(num_envs=N, num_snakes=K, size=S, device='cpu', manual_setup=True, observation_mode=mode, **kwargs)
    built = []
    for e, (g, o, p, cp) in enumerate(flat):
        b = build_env(g[0], g[1], K, S, o, p, cp, any_mode)
        write_env(env, e, K, b)
        built.append(b)
    env.check_consistency()
    rng = np.random.RandomState(seed)
    all_actions = rng.randint(0, 8, size=(T, K, N)).astype(np.int64)
    for e, b in enumerate(built):
        for t, row in enumerate(b['actions']):
            all_actions[t, :, e] = row
    rec = mgm.Recorder(env)
    out = {'state0_' + k: v for k, v in mgm.state_of(env).items()}
    out['actions'] = all_actions.copy()
    cols = {}

    def put(key, val):
        cols.setdefault(key, []).append(val)

    acts_t = torch.from_numpy(all_actions)
    for t in range(T):
        actions = {f'agent_{i}': acts_t[t, i].clone() for i in range(K)}
        obs, rewards, dones, info, inj = rec.step(actions)
        for k, v in mgm.state_of(env).items():
            put('step_' + k, v)
        put('obs_step', mgm.obs_to_u8(obs, K))
        put('rewards', mgm.per_agent(rewards, 'agent_', K, np.float32))
        put('dones_out', mgm.per_agent(dones, 'agent_', K, np.uint8))
        put('all_done', dones['__all__'].numpy().astype(np.uint8))
        put('snake_collision', mgm.per_agent(info, 'snake_collision_', K, np.uint8))
        put('edge_collision', mgm.per_agent(info, 'edge_collision_', K, np.uint8))
        put('food', mgm.per_agent(info, 'food_', K, np.float32))
        put('size', mgm.per_agent(info, 'size_', K, np.float32))
        put('boost', mgm.per_agent(info, 'boost_', K, np.uint8))
        for k, v in inj.items():
            put('inj_' + k, np.packbits(v, axis=None) if k in ('death_a', 'death_b', 'rate') else v)
        obs_r, rinj = rec.reset(dones['__all__'], return_observations=True)
        for k, v in mgm.state_of(env).items():
            put('reset_' + k, v)
        put('obs_reset', mgm.obs_to_u8(obs_r, K))
        for k, v in rinj.items():
            put('rinj_' + k, v)
        env.check_consistency()
    out.update({k: np.stack(v) for k, v in cols.items()})
    out['meta'] = np.array([N, K, S, T, seed], np.int64)
    out['mode'] = np.array(env.observation_mode)
    cfgd = dict(boost=env.boost, food_on_death_prob=env.food_on_death_prob, boost_cost_prob=env.boost_cost_prob,
                food_mode=env.food_mode, food_rate=env.food_rate, reward_on_death=env.reward_on_death,
                respawn_mode=env.respawn_mode, colour_mode=env.colour_mode)
    out['cfg'] = np.array(repr(cfgd))
    # which env was built for what: class, variant, attacker, victim, step of the encounter (read by the tests)
    out['plan_class'] = np.array([g[0] for (g, o, p, cp) in flat])
    out['plan_variant'] = np.array([g[1] for (g, o, p, cp) in flat])
    out['plan_pair'] = np.array([b['pair'] for b in built], np.int64)
    out['plan_step'] = np.array([cp for (g, o, p, cp) in flat], np.int64)
    out['plan_placement'] = np.array([p for (g, o, p, cp) in flat], np.int64)
    if write:
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print(f'{name}: N={N} {os.path.getsize(path) / 1024:.0f} KiB; deaths {int(out["dones_out"].sum())}')
    return out


def split(groups, parts):
    return [groups[k::parts] for k in range(parts)]


ANY = dict(respawn_mode='any')


def files():
    """name -> (K, S, seed, groups, lead, mode, kwargs); the lead groups walk through GROUPS so that every class opens and
    closes some file"""
    spec = []
    for K, S, part_mode, parts in ((2, 12, 'partial_2', 2), (4, 25, 'partial_5', 2), (6, 12, 'partial_2', 2), (10, 36, None, 6)):
        for k, g in enumerate(split(GROUPS, parts)):
            spec.append((f'events_k{K}_s{S}_full_{k}', K, S, g, 'full', {}))
        if part_mode:
            for k, g in enumerate(split(GROUPS, parts)):
                spec.append((f'events_k{K}_s{S}_{part_mode}_{k}', K, S, g, part_mode, ANY))
    plain = [g for g in GROUPS if g[1] == 'plain' and g[0] != 'boost_gated']
    spec.append(('events_k2_s12_noboost', 2, 12, plain, 'full', dict(boost=False)))
    def usable(g, mode, kw):
        return [x for x in g if (x[0] != 'respawn_blocked' or kw.get('respawn_mode') == 'any') and
                (x[0] != 'death_over_food' or mode == 'full')]

    # every class opens and closes one file: the most constrained leads choose first, the narrow files are taken first
    lead = {}
    order = sorted(range(len(spec)), key=lambda n: len(spec[n][3]))
    for want in LEADS:
        n = next(n for n in order if n not in lead and want in usable(spec[n][3], spec[n][4], spec[n][5]))
        lead[n] = want
    out = {}
    for n, (name, K, S, g, mode, kw) in enumerate(spec):
        out[name] = (K, S, 900 + n, g, lead.get(n, usable(g, mode, kw)[0]), mode, kw)
    return out


def outcome_rows(fx):
    """one row per env: what the reference did at the steered step with the pair the env was built for"""
    N, K = int(fx['meta'][0]), int(fx['meta'][1])
    rows = []
    for e in range(N):
        t, (i, j) = int(fx['plan_step'][e]), (int(v) for v in fx['plan_pair'][e])
        bits = []
        for s in (i, j):
            a = e * K + s
            bits += [int(fx['dones_out'][t, a]), int(fx['snake_collision'][t, a]), int(fx['edge_collision'][t, a]),
                     int(fx['food'][t, a] > 0)]
        rows.append((str(fx['plan_class'][e]), str(fx['plan_variant'][e]), i < j or i == j, tuple(bits),
                     float(fx['rewards'][t, e * K + i]), float(fx['rewards'][t, e * K + j]),
                     float(fx['size'][t, e * K + i]), float(fx['size'][t, e * K + j]),
                     int(fx['step_foods'][t, e].sum())))
    return rows


def print_table(names):
    """per class / variant / boost off: the outcome bits, rewards, sizes after the step and cells of food left in the env"""
    table = {}
    for name in names:
        z = np.load(os.path.join(HERE, name + '.npz'))
        fx = {k: z[k] for k in z.files}
        for row in outcome_rows(fx):
            key = (row[0], row[1], "'boost': False" in str(fx['cfg']))
            t = table.setdefault(key, [set(), set(), set(), set(), set(), set()])
            for k, v in enumerate((row[3], row[4], row[5], row[6], row[7], row[8])):
                t[k].add(v)
    print('class / variant / boost off: (dead, snake_collision, edge_collision, ate) of attacker then victim | rewards of '
          'attacker | of victim | sizes of attacker | of victim | cells of food left (min..max)')
    for key in sorted(table):
        bits, ra, rb, sa, sb, fl = table[key]
        print(key, sorted(bits), '|', sorted(ra), '|', sorted(rb), '|', sorted(sa), '|', sorted(sb), '|', f'{min(fl)}..{max(fl)}')


if __name__ == '__main__':
    todo = files()
    args = [a for a in sys.argv[1:] if a != '--table']
    if '--table' not in sys.argv[1:]:          # (--table: print the table of the files as they are, record nothing)
        for name in (args or list(todo)):
            K, S, seed, groups, lead, mode, kw = todo[name]
            record_events(name, K, S, seed, groups, lead, mode=mode, **kw)
    if not args:      # the census condition of tests/test_multi_events_cpu.py, on what the reference did
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from tests import test_multi_events_cpu as cpu
        total = {}
        for name in todo:
            fx = cpu.replay.load_multi(name)
            mer.census(mer.fixture_events(fx, cpu.state_at), int(fx['meta'][0]), total)
        cpu.check_census(total)
        print(cpu.format_census(total))
    print_table(args or list(todo))
