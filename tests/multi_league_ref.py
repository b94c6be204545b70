"""What tests/test_multi_league_*.py share: the plan of a line-up by brute force, the expected rows of wurm_multi_act_league
from the CPU oracle (oracle.policy_forward with the policy of each row; oracle_policy_sample with the row's own stream, as
tests/multi_act_ref.py has it for `act`), and the score table of wurm_multi_league_scores in numpy float64.  Not a test
module."""
import ctypes

import numpy as np

COLUMNS = ('steps', 'reward', 'deaths', 'food', 'snake_collisions', 'edge_collisions', 'boost', 'size_sum')
# column of the table <- key of the window (None: the count of row-steps)
SOURCES = (None, 'rewards', 'dones', 'food', 'snake_collision', 'edge_collision', 'boost', 'size')


def brute_plan(lineup, num_policies):
    """lineup (K, N) of ints -> (order, offsets) as lists: for a = 0, 1, ... every row r = k N + i with lineup[k][i] == a,
    rows ascending"""
    lineup = np.asarray(lineup)
    K, N = lineup.shape
    order, offsets = [], [0]
    for a in range(num_policies):
        for r in range(K * N):
            if int(lineup[r // N][r % N]) == a:
                order.append(r)
        offsets.append(len(order))
    return order, offsets


def expected_rows(params, obs, lineup, seed, call, env_offset=0):
    """params (A, num_params), obs (K, N, E), lineup (K, N) numpy -> probs (K, N, 4), values (K, N), actions (K, N) of the
    oracle, row by row: the forward of the row's policy on the row alone, the draw of stream (env_offset + i) K + k"""
    from oracle import oracle as O
    K, N, E = obs.shape
    params = np.ascontiguousarray(params, np.float32).reshape(-1, O.policy_param_count(E))
    sample = O.lib().oracle_policy_sample
    sample.restype = ctypes.c_int
    sample.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    probs, values = np.empty((K, N, 4), np.float32), np.empty((K, N), np.float32)
    actions = np.empty((K, N), np.int64)
    for k in range(K):
        for i in range(N):
            p, v = O.policy_forward(params[int(lineup[k, i])], np.ascontiguousarray(obs[k, i:i + 1]))
            probs[k, i], values[k, i] = p[0], v[0]
            row = np.ascontiguousarray(probs[k, i])
            actions[k, i] = sample(row.ctypes.data, seed, call, (env_offset + i) * K + k)
    return probs, values, actions


def score_table(lineup, num_policies, windows):
    """(A, 8) float64: for every window (a dict of (T, K N) numpy arrays) and policy, the sums over the policy's columns"""
    flat = np.asarray(lineup).reshape(-1)
    table = np.zeros((num_policies, len(COLUMNS)), np.float64)
    for out in windows:
        T = out['rewards'].shape[0]
        for a in range(num_policies):
            cols = np.nonzero(flat == a)[0]
            for c, key in enumerate(SOURCES):
                if key is None:
                    table[a, c] += float(T * len(cols))
                elif key in out:
                    table[a, c] += out[key][:, cols].astype(np.float64).sum()
    return table
