"""Cross-check of the CPU oracle against the REAL reference on random configurations — beyond the scenario fixtures.
tests/golden/make_golden_random.py drew each configuration from a seeded RandomState, drove the reference with the
recorder of tests/golden/ (capturing its random outcomes) and stored the record as tests/golden/random_*.npz; the tape
is replayed into the oracle with those outcomes injected: bit-equality on every output."""
import pytest

from tests import replay
from tests.backends import OracleBackend


@pytest.mark.parametrize('seed', range(6))
def test_single_snake_random_config(seed):
    fx = replay.load(f'random_single_{seed}')
    replay.replay_single(OracleBackend(), fx)
    if int(fx['meta'][4]) == 1:  # reset_every
        replay.replay_single_rollout(OracleBackend(), fx)


@pytest.mark.parametrize('seed', range(2))
def test_gridworld_random_config(seed):
    fx = replay.load(f'random_grid_{seed}')
    replay.replay_grid(OracleBackend(), fx)
    replay.replay_grid_rollout(OracleBackend(), fx)


@pytest.mark.parametrize('seed', range(11))
def test_multi_snake_random_config(seed):
    fx = replay.load_multi(f'random_multi_{seed}')
    replay.replay_multi(OracleBackend(), fx)
    replay.replay_multi_rollout(OracleBackend(), fx)
