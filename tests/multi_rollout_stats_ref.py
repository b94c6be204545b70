"""Numpy restatement of wurm_multi_rollout_stats (include/wurm_hip.h): the expected values of
tests/test_multi_rollout_stats_*.py.  Written from the header's description for ONE agent (a window of K agents is one of
these per block of N columns): integers for the flag and size columns, float64 for reward, food and entropy, the smoother
with its skip rule, the life carry.  Vectorised over envs, a loop over steps."""
import numpy as np

from tests.rollout_stats_ref import entropy64

SUMS = 10   # alive, done, reward alive, H alive, food alive, boost alive, size alive, edge, snake, size done
COLS = 9    # reward, policy_entropy, food, edge_collisions, snake_collisions, boost, size, done, return
ACC = 16
# the smoother's columns as (numerator, mask) among the ten sums; mask None: all N envs
RATIOS = ((2, 0), (3, 0), (4, 0), (7, None), (8, None), (5, 0), (6, 0), (1, None), (9, 1))


class RefMultiStats(object):
    """One agent's statistics over chained windows."""

    def __init__(self, num_envs, alpha=0.025):
        self.ret = np.zeros(num_envs, np.float64)
        self.length = np.zeros(num_envs, np.int64)
        self.alpha = alpha
        self.accum = np.zeros(ACC, np.float64)
        self.accum[13:15] = -np.inf
        self.smooth = np.full(COLS, np.nan)

    def update(self, rewards, food, size, dones, boost, snake, edge, probs=None, all_done=None):
        """(T, N) arrays of this agent (probs (T, N, 4); all_done (T, N) of the envs); returns the (T, 10) table"""
        T, N = rewards.shape
        table = np.zeros((T, SUMS), np.float64)
        for t in range(T):
            d = dones[t].astype(bool)
            a = ~d
            r, sz = rewards[t].astype(np.float64), size[t].astype(np.int64)
            self.ret += r
            self.length += 1
            if d.any():
                self.accum[11] += self.ret[d].sum()
                self.accum[12] += self.length[d].sum()
                self.accum[13] = max(self.accum[13], sz[d].max())
                self.accum[14] = max(self.accum[14], self.ret[d].max())
            self.ret[d] = 0
            self.length[d] = 0
            h = entropy64(probs[t]) if probs is not None else np.zeros(N)
            table[t] = [int(a.sum()), int(d.sum()), r[a].sum(), h[a].sum(), food[t].astype(np.float64)[a].sum(),
                        int((boost[t].astype(bool) & a).sum()), int(sz[a].sum()), int(edge[t].astype(bool).sum()),
                        int(snake[t].astype(bool).sum()), int(sz[d].sum())]
            for c, (num, den) in enumerate(RATIOS):
                mask = N if den is None else table[t, den]
                if mask == 0:
                    continue  # the skip rule: an empty mask leaves the smoother as it was
                x = table[t, num] / mask
                self.smooth[c] = x if np.isnan(self.smooth[c]) else self.alpha * x + (1 - self.alpha) * self.smooth[c]
        self.accum[0] += T * N
        self.accum[1:11] += table.sum(0)
        if all_done is not None:
            self.accum[15] += int(all_done.astype(bool).sum())
        return table

    def reset(self):
        self.accum[:] = 0
        self.accum[13:15] = -np.inf
