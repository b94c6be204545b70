"""Records the random configurations of tests/test_oracle_vs_live_reference.py from the REAL reference into
tests/golden/random_<family>_<seed>.npz (same recorders and file format as make_golden.py / make_golden_multi.py).

Run only in the build container (where the reference exists):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_random.py

Each configuration is drawn from np.random.RandomState(<base> + seed), so a fixture can be re-made bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
import make_golden_multi  # noqa: E402

SINGLE_SEEDS, GRID_SEEDS, MULTI_SEEDS = range(6), range(2), range(11)


def single(seed):
    rng = np.random.RandomState(500 + seed)
    S = int(rng.choice([9, 10, 12, 15, 20]))
    mode = ['default', 'raw', 'one_channel', 'positions', f'partial_{rng.randint(1, 5)}'][rng.randint(5)]
    reset_every = 1 if mode.startswith('partial') else int(rng.choice([1, 1, 3]))
    make_golden.record_single(f'random_single_{seed}', N=int(rng.randint(2, 24)), S=S, T=int(rng.randint(20, 70)),
                              mode=mode, seed=1000 + seed, reset_every=reset_every)


def grid(seed):
    rng = np.random.RandomState(600 + seed)
    S = int(rng.choice([5, 7, 9, 13]))
    make_golden.record_grid(f'random_grid_{seed}', N=int(rng.randint(2, 30)), S=S, T=int(rng.randint(20, 60)),
                            mode=['default', 'raw'][rng.randint(2)], seed=2000 + seed,
                            start=(int(rng.randint(1, S - 1)), int(rng.randint(1, S - 1))))


def multi(seed):
    rng = np.random.RandomState(700 + seed)
    K = int(rng.choice([1, 2, 3, 4, 6]))
    S = int(rng.choice([10, 12, 14, 18, 25]))
    if seed >= 8:  # the smallest grids the reference can populate
        K, S = 1, int(rng.choice([5, 6, 7]))
    kw = dict(boost=bool(rng.rand() < 0.8), food_on_death_prob=float(rng.choice([0.0, 0.3, 0.5, 1.0])),
              boost_cost_prob=float(rng.choice([0.0, 0.25, 0.5, 1.0])),
              food_mode=['only_one', 'random_rate'][rng.randint(2)], food_rate=float(rng.choice([5e-4, 5e-3, 3e-2])),
              respawn_mode=['all', 'any'][rng.randint(2)], agent_colours=['random', 'fixed'][rng.randint(2)],
              observation_mode=['full', f'partial_{rng.randint(1, 5)}'][rng.randint(2)],
              reward_on_death=int(rng.choice([-1, -2, 0])))
    make_golden_multi.record_multi(f'random_multi_{seed}', N=int(rng.randint(2, 10)), K=K, S=S,
                                   T=int(rng.randint(15, 50)), seed=3000 + seed, **kw)


if __name__ == '__main__':
    for s in SINGLE_SEEDS:
        single(s)
    for s in GRID_SEEDS:
        grid(s)
    for s in MULTI_SEEDS:
        multi(s)
