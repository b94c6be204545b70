"""Pure-Python restatement of the league's matchmaking (include/wurm_hip.h: wurm_multi_league_draw, wurm_multi_league_plan;
wurm_amd/csrc/multi_matchmaking.hpp), written from the specification, for the tests: the draw of a line-up per env from
integer tickets in Python ints — Philox4x32-10 and the counter layout of `rng_words` from tests/a2c_pbt_ref.py — and the
sort rule of a plan, dropped rows included."""
import numpy as np

from tests.a2c_pbt_ref import rng_words

RNG_LEAGUE = 10


def mulhi64(x, n):
    return (x * n) >> 64


def draw_env(env_id, K, A, seed, call, tickets=None, replacement=False, pinned=None):
    """the K seats of the env with global id `env_id` (= env_offset + i), a list of ints"""
    pinned = [-1] * K if pinned is None else [int(p) for p in pinned]
    t = [1] * A if tickets is None else [max(int(x), 0) for x in tickets]
    seats = list(pinned)
    for k in range(K):
        if pinned[k] >= 0:
            continue
        if replacement:
            pool = list(range(A))
        else:  # every pinned policy is out from the start, and so is whoever sits already
            taken = set(p for p in pinned if p >= 0) | set(seats[j] for j in range(k) if pinned[j] < 0)
            pool = [a for a in range(A) if a not in taken]
        weights = [t[a] for a in pool]
        total = sum(weights)
        if total == 0:
            weights, total = [1] * len(pool), len(pool)
        w = rng_words(seed, call, env_id, RNG_LEAGUE, k)
        r = mulhi64((w[0] << 32) | w[1], total)
        run = 0
        for a, wa in zip(pool, weights):
            run += wa
            if run > r:
                seats[k] = a
                break
    return seats


def draw(K, N, A, seed, call, env_offset=0, tickets=None, replacement=False, pinned=None):
    """(K, N) int64 numpy line-up: column i is `draw_env(env_offset + i, ...)`"""
    out = np.empty((K, N), np.int64)
    for i in range(N):
        out[:, i] = draw_env(env_offset + i, K, A, seed, call, tickets, replacement, pinned)
    return out


def plan(lineup, A):
    """(order, offsets, dropped) of a (K, N) line-up: the rows r = k N + i whose entry lies in [0, A) sorted by policy,
    ascending within a policy; order keeps its K N entries, -1 behind offsets[A]; dropped = the rows left out"""
    flat = [int(v) for v in np.asarray(lineup).reshape(-1)]
    lists = [[] for _ in range(A)]
    for r, v in enumerate(flat):
        if 0 <= v < A:
            lists[v].append(r)
    order = [r for rows in lists for r in rows]
    offsets = [0]
    for rows in lists:
        offsets.append(offsets[-1] + len(rows))
    dropped = len(flat) - len(order)
    return order + [-1] * dropped, offsets, dropped
