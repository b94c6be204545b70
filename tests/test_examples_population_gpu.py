"""examples/a2c_population.py runs end to end on the GPU: three members with their own learning rates in one env object."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))


def test_population_example_runs():
    import a2c_population
    lrs = (3e-4, 1e-3, 3e-3)
    hist = a2c_population.run(num_envs=16, size=9, observation='partial_2', steps=40, update_steps=5, lrs=lrs,
                              log_interval=20, verbose=False)
    assert len(hist) == 3
    for p, rows in enumerate(hist):
        assert len(rows) == 2 and rows[-1]['step'] == 40
        for row in rows:
            assert row['member'] == p and row['lr'] == lrs[p]
            assert all(math.isfinite(v) for v in row.values())
            assert 0 <= row['done_rate'] <= 1 and 0 <= row['reward_rate'] <= 1
    assert len({rows[-1]['loss'] for rows in hist}) == 3  # three different agents
