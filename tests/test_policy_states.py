"""tests/policy_states.py: every generated start state passes the env's consistency check and has what its docstring
promises (long snakes, food next to the head for the stated share, 2 to 4 free cells on the crowded boards)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import policy_states as PS

SIZES = [9, 11, 12, 16, 17, 22, 23, 32, 33, 39, 40, 45, 46, 55, 56, 64]


def _head_food_adjacent(envs):
    N, _, S, _ = envs.shape
    h = envs[:, 1].reshape(N, -1).argmax(1)
    f = envs[:, 0].reshape(N, -1).argmax(1)
    return np.abs(h // S - f // S) + np.abs(h % S - f % S) == 1


@pytest.mark.parametrize('S', SIZES)
def test_snake_states_are_consistent(S):
    rng = np.random.RandomState(S)
    N, fill = 48, 0.5
    envs = PS.snake_states(N, S, rng, fill=fill, near_food=0.5)
    assert envs.shape == (N, 3, S, S) and envs.dtype == np.float32
    assert (O.single_check(envs) == 0).all()
    L = envs[:, 2].reshape(N, -1).max(1)
    assert L.min() >= 3 and L.max() <= fill * (S - 2) ** 2 and L.max() > 0.3 * (S - 2) ** 2
    edge = np.ones((S, S), bool)
    edge[1:-1, 1:-1] = False
    assert (envs[:, :, edge] == 0).all()
    for i in range(N):   # the body is a path: value k + 1 lies next to value k
        ys, xs = np.nonzero(envs[i, 2])
        order = np.argsort(envs[i, 2][ys, xs])
        assert (np.abs(np.diff(ys[order])) + np.abs(np.diff(xs[order])) == 1).all()
    near = _head_food_adjacent(envs).mean()
    assert 0.25 <= near <= 0.8   # the stated share is 0.5 (a head in a dead end has no free neighbour; chance adds some)


@pytest.mark.parametrize('S', [9, 11, 12, 17, 23, 33, 40, 45, 47])
def test_crowded_snake_states_are_consistent(S):
    """(up to S = 47: see crowded_snake_states on the check's own float32 limit)"""
    rng = np.random.RandomState(100 + S)
    N = 32
    envs = PS.crowded_snake_states(N, S, rng)
    assert (O.single_check(envs) == 0).all()
    free = (S - 2) ** 2 - (envs[:, 2] > 0).reshape(N, -1).sum(1)
    assert free.min() >= 2 and free.max() <= 4 and len(np.unique(free)) == 3
    assert _head_food_adjacent(envs).any()


@pytest.mark.parametrize('S', [5, 9, 17, 32, 45, 55, 64])
def test_grid_states_are_consistent(S):
    rng = np.random.RandomState(200 + S)
    N = 64
    envs = PS.grid_states(N, S, rng, near_food=0.5)
    assert envs.shape == (N, 2, S, S)
    assert (PS.grid_check(envs) == 0).all()
    a = envs[:, 1].reshape(N, -1).argmax(1)
    f = envs[:, 0].reshape(N, -1).argmax(1)
    cheb = np.maximum(np.abs(a // S - f // S), np.abs(a % S - f % S))
    assert (cheb >= 1).all()
    if S >= 17:
        assert 0.3 <= (cheb <= 2).mean() <= 0.75


def test_grid_check_flags_what_it_names():
    envs = PS.grid_states(6, 9, np.random.RandomState(0))
    envs[1, 1, 4, 4] = envs[1, 1, 5, 5] = 1          # a second agent (or a third)
    envs[2, 0] = 0                                   # no food
    envs[3, 0] = envs[3, 1]                          # food under the agent
    envs[4, 0] = 0
    envs[4, 0, 0, 3] = 1                             # food on the edge
    envs[5, 0][envs[5, 0] == 1] = 0.5
    err = PS.grid_check(envs)
    assert err[0] == 0
    assert err[1] & PS.GRID_ONE_AGENT and err[2] & PS.GRID_ONE_FOOD and err[3] & PS.GRID_AGENT_ON_FOOD
    assert err[4] & PS.GRID_ON_EDGE and err[5] & PS.GRID_FOOD_VALUE


def test_straight_params_give_one_hot_probabilities():
    rng = np.random.RandomState(1)
    for E in (3, 4, 243):
        for a in range(4):
            p, v = O.policy_forward(PS.straight_params(E, a), rng.rand(5, E).astype(np.float32) * 60)
            assert (p == np.eye(4, dtype=np.float32)[a]).all() and (v == 0).all()
