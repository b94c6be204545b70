"""Start states for the fused acting loop's tests (tests/test_policy_wide_coverage.py, tools/fuzz_parity.py:
fuzz_policy_wide) in which the game happens: long snakes, food next to the head, boards with a handful of free cells.
A fresh reset gives a snake of length 3 on an empty board, and a random policy then dies at an edge long before it
meets its own body or eats twice; the states here start where those events are a few steps away.

Plain numpy, no GPU and no test in this module.  Every state passes the oracle's consistency check
(oracle.single_check; grid_check below for SimpleGridworld): tests/test_policy_states.py."""
import numpy as np


def interior_path(S):
    """the interior cells (1 .. S-2)^2 as one boustrophedon path: consecutive entries are 4-neighbours"""
    cells = []
    for i, y in enumerate(range(1, S - 1)):
        xs = range(1, S - 1) if i % 2 == 0 else range(S - 2, 0, -1)
        cells.extend(y * S + x for x in xs)
    return np.asarray(cells, np.int64)


def _free_neighbours(env, S, cell):
    """free interior 4-neighbours of a cell (no body, no food)"""
    y, x = divmod(int(cell), S)
    out = []
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        yy, xx = y + dy, x + dx
        if 1 <= yy <= S - 2 and 1 <= xx <= S - 2 and env[2, yy, xx] == 0 and env[0, yy, xx] == 0:
            out.append(yy * S + xx)
    return out


def _lay_snakes(N, S, rng, lengths, near_food):
    by_rows = interior_path(S)
    by_columns = (by_rows % S) * S + by_rows // S
    M = len(by_rows)
    envs = np.zeros((N, 3, S, S), np.float32)
    for i in range(N):
        L = int(lengths[i])
        assert 3 <= L < M, (L, M)   # at least one free cell for the food
        path = by_rows if rng.rand() < 0.5 else by_columns
        start = int(rng.randint(0, M - L + 1))
        cells = path[start:start + L]
        if rng.rand() < 0.5:
            cells = cells[::-1]
        body = envs[i, 2].reshape(-1)
        body[cells] = np.arange(1, L + 1, dtype=np.float32)   # tail 1 .. head L
        envs[i, 1].reshape(-1)[cells[-1]] = 1
        near = _free_neighbours(envs[i], S, cells[-1]) if rng.rand() < near_food else []
        if near:
            food = near[rng.randint(len(near))]
        else:
            free = path[body[path] == 0]
            food = free[rng.randint(len(free))]
        envs[i, 0].reshape(-1)[food] = 1
    return envs


def snake_states(N, S, rng, fill=0.5, near_food=0.5):
    """(N, 3, S, S) SingleSnake states (food, head, body): the snake lies along interior_path(S) or its transpose (rows or
    columns of body next to each other) from a random start in a random direction, body values 1 .. L with the head at L; L is drawn per env from 3 .. max(3, fill * (S-2)^2).
    One food: for a share `near_food` of the envs on a free neighbour of the head (where the head has one), else on a
    random free interior cell."""
    M = (S - 2) ** 2
    top = min(M - 1, max(3, int(fill * M)))
    return _lay_snakes(N, S, rng, rng.randint(3, top + 1, N), near_food)


def crowded_snake_states(N, S, rng, near_food=0.5):
    """snake_states with 2 to 4 free interior cells (the food on one of them), so that the food respawn after a meal
    ranks 1 to 3 candidates.  (For S > 47 the length passes 2047 and oracle.single_check's float32 square root of
    8 * sum(body) + 1 is no longer exact: the check, not the state, sets that limit.)"""
    M = (S - 2) ** 2
    return _lay_snakes(N, S, rng, M - rng.randint(2, 5, N), near_food)


def grid_states(N, S, rng, near_food=0.5, reach=2):
    """(N, 2, S, S) SimpleGridworld states (food, agent): one agent on a random interior cell and one food, for a
    share `near_food` of the envs within `reach` cells of the agent (Chebyshev distance), else anywhere in the
    interior."""
    envs = np.zeros((N, 2, S, S), np.float32)
    for i in range(N):
        ay, ax = (int(v) for v in rng.randint(1, S - 1, 2))
        envs[i, 1, ay, ax] = 1
        close = rng.rand() < near_food
        while True:
            if close:
                fy, fx = ay + int(rng.randint(-reach, reach + 1)), ax + int(rng.randint(-reach, reach + 1))
            else:
                fy, fx = (int(v) for v in rng.randint(1, S - 1, 2))
            if 1 <= fy <= S - 2 and 1 <= fx <= S - 2 and (fy, fx) != (ay, ax):
                break
        envs[i, 0, fy, fx] = 1
    return envs


GRID_FOOD_VALUE, GRID_ONE_AGENT, GRID_ONE_FOOD, GRID_AGENT_ON_FOOD, GRID_ON_EDGE = 1, 2, 4, 8, 16


def grid_check(envs):
    """per-env error bitmask of a SimpleGridworld state, 0 = consistent: both channels in {0, 1}, exactly one agent and
    one food, on different cells, both in the interior (what the env's own reset and step leave behind)"""
    N, _, S, _ = envs.shape
    err = np.zeros(N, np.uint32)
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    for i in range(N):
        food, agent = envs[i, 0], envs[i, 1]
        e = 0
        if not np.isin(envs[i], (0.0, 1.0)).all():
            e |= GRID_FOOD_VALUE
        if agent.sum() != 1:
            e |= GRID_ONE_AGENT
        if food.sum() != 1:
            e |= GRID_ONE_FOOD
        if (agent * food).sum() != 0:
            e |= GRID_AGENT_ON_FOOD
        if (agent[~inner] != 0).any() or (food[~inner] != 0).any():
            e |= GRID_ON_EDGE
        err[i] = e
    return err


def straight_params(E, action, bias=100.0):
    """zero weights and one head bias: the policy's probabilities are exactly (.., 1, ..) for `action` whatever the
    observation, so every snake turns that way (or keeps going, if that is straight back) and runs into the edge"""
    from oracle import oracle as O
    p = np.zeros(O.policy_param_count(E), np.float32)
    bp = 64 * E + 64 + 64 * 64 + 64 + 4 * 64
    p[bp + action] = bias
    return p
