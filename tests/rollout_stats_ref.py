"""Numpy restatement of wurm_rollout_stats (include/wurm_hip.h) in float64 / integers: the expected values of
tests/test_rollout_stats_*.py.  Written from the header's description, vectorised over envs, a loop over steps."""
import numpy as np

COLS = 6   # done, reward, edge collision, self collision, size, entropy
ACC = 12
EPS32 = np.float32(1.1920928955078125e-07)
HI32 = np.float32(1.0) - EPS32


def entropy64(probs):
    """-sum_k p_k log(clamp(p_k, eps32, 1 - eps32)) in float64 on fp32 probabilities (..., 4)"""
    p = probs.astype(np.float64)
    return -(p * np.log(np.clip(p, np.float64(EPS32), np.float64(HI32)))).sum(-1)


class RefStats(object):
    """One member's statistics over chained windows (a population is one of these per block of columns)."""

    def __init__(self, size0, initial_size=3, alpha=0.025):
        n = len(size0)
        self.ret = np.zeros(n, np.float64)
        self.length = np.zeros(n, np.int64)
        self.size = np.asarray(size0, np.int64).copy()
        self.initial_size, self.alpha = initial_size, alpha
        self.accum = np.zeros(ACC, np.float64)
        self.accum[10:] = -np.inf
        self.smooth = np.full(COLS, np.nan)

    def update(self, rewards, dones, edge, selfc=None, probs=None):
        """(T, N) arrays (probs (T, N, 4)); returns the (T, 6) table of batch sums"""
        T, N = rewards.shape
        table = np.zeros((T, COLS), np.float64)
        for t in range(T):
            r, d = rewards[t].astype(np.float64), dones[t].astype(bool)
            grown = self.size + ((rewards[t] == 1) if self.initial_size > 0 else 0)  # initial_size 0: no snake
            self.ret += r
            self.length += 1
            if d.any():
                self.accum[7] += self.ret[d].sum()
                self.accum[8] += self.length[d].sum()
                self.accum[9] += grown[d].sum()
                self.accum[10] = max(self.accum[10], self.ret[d].max())
                self.accum[11] = max(self.accum[11], grown[d].max())
            self.ret[d] = 0
            self.length[d] = 0
            self.size = np.where(d, self.initial_size, grown)
            table[t] = [d.sum(), r.sum(), edge[t].astype(bool).sum(),
                        selfc[t].astype(bool).sum() if selfc is not None else 0, self.size.sum(),
                        entropy64(probs[t]).sum() if probs is not None else 0.0]
            for k in range(COLS):
                x = table[t, k] / N
                self.smooth[k] = x if np.isnan(self.smooth[k]) else self.alpha * x + (1 - self.alpha) * self.smooth[k]
        self.accum[0] += T * N
        self.accum[1:7] += table.sum(0)
        return table

    def reset(self):
        self.accum[:10] = 0
        self.accum[10:] = -np.inf
