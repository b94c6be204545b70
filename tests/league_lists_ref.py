"""What tests/test_league_plan_contract_*.py share: the two documented rules that turn a league plan's `order` and `offsets`
into per-policy lists WHATEVER the two arrays hold, restated in plain Python, a fixed list of malformed plans, and guarded
buffers.  Not a test module.

The acting and scores kernels (wurm_amd/csrc/multi_league.hpp) clamp the two offsets of a policy to [0, R] each on its
own and skip an entry of `order` outside [0, R): `act_lists`.  The learner (wurm_amd/csrc/a2c_learner.hpp: league_member)
clamps to [0, R] and takes a running maximum, and an entry outside [0, R) stays in the list as an inert row that still
counts in M: `learner_lists`.  On offsets that decrease somewhere the two rules give different lists.

Every malformed value lies inside an envelope of G = GUARD entries or rows around the arrays the kernels index with it:
offsets in [-G, R + G], entries of `order` in [-G, R + G).  The GPU tests place `order`, the observations, the outputs and
the (T, R, .) inputs in the middle of larger allocations (`embed`) whose margins hold a sentinel, so a kernel whose clamp or
skip were broken would write into, or read from, memory the test owns: a wrong value or a touched guard, never a fault.
"""
from collections import namedtuple

import numpy as np
import torch

from tests.multi_league_ref import COLUMNS, SOURCES

GUARD = 8


# ---------------------------------------------------------------------------------------------------- the two rules

def _clamp(v, R):
    return 0 if v < 0 else R if v > R else v


def act_lists(order, offsets, R):
    """multi_league.hpp: policy a gets order[clamp(offsets[a]) : clamp(offsets[a + 1])], each offset clamped to [0, R] on its
    own (empty when first >= end), entries outside [0, R) dropped.  A list of lists of row ids, in list order."""
    order, offsets = [int(r) for r in order], [int(o) for o in offsets]
    lists = []
    for a in range(len(offsets) - 1):
        first, end = _clamp(offsets[a], R), _clamp(offsets[a + 1], R)
        lists.append([order[j] for j in range(first, end) if 0 <= order[j] < R])
    return lists


Member = namedtuple('Member', ('first', 'M', 'base', 'positions', 'inert'))


def learner_lists(order, offsets, R, max_groups=256):
    """a2c_learner.hpp: league_member.  lo = clamp(offsets[0]); every later offset is clamped to [0, R] and raised to the
    one before it.  Per member: `first` and `M` (its piece of `order` is [first, first + M)), `base` = sum over the
    members before it of min(M_b, 256), `positions` = the positions first .. first + M - 1 of `order`, and `inert`, for
    each of them, whether the entry there lies outside [0, R): such a row has no input and no loss term but counts in M."""
    order, offsets = [int(r) for r in order], [int(o) for o in offsets]
    lo, base, members = _clamp(offsets[0], R), 0, []
    for a in range(len(offsets) - 1):
        hi = max(lo, min(offsets[a + 1], R))
        positions = list(range(lo, hi))
        members.append(Member(lo, hi - lo, base, positions, [not 0 <= order[j] < R for j in positions]))
        base += min(hi - lo, max_groups)
        lo = hi
    return members


def normalised_offsets(order, offsets, R):
    """the monotone, in-range offsets that give the learner the lists `learner_lists` says it takes from `offsets`"""
    members = learner_lists(order, offsets, R)
    return [members[0].first] + [m.first + m.M for m in members]


def score_table_of_lists(lists, windows):
    """tests/multi_league_ref.py: score_table over explicit lists of columns, one per policy: (A, 8) float64.  A row a
    list names twice counts twice."""
    table = np.zeros((len(lists), len(COLUMNS)), np.float64)
    for out in windows:
        T = out['rewards'].shape[0]
        for a, rows in enumerate(lists):
            cols = np.asarray(rows, np.int64)
            for c, key in enumerate(SOURCES):
                if key is None:
                    table[a, c] += float(T * len(cols))
                elif key in out:
                    col = out[key][:, cols]
                    # a flag counts as 1 whatever non-zero byte it holds; a float is added as it is
                    table[a, c] += float((col != 0).sum()) if col.dtype.kind in 'bu' else col.astype(np.float64).sum()
    return table


# ---------------------------------------------------------------------------------------------------- malformed plans

# The cases share one shape: K x N = 3 x 8 rows, five policies.  PERM is the valid `order` (a permutation, NOT ascending
# within a policy: no kernel may rely on that), CONTROL the valid offsets: policy 1 has no rows.
CASE_K, CASE_N, CASE_A = 3, 8, 5
R = CASE_K * CASE_N
PERM = [int(r) for r in np.random.default_rng(24).permutation(R)]
CONTROL = [0, 5, 5, 12, 20, 24]
BAD = (-1, -GUARD, R, R + GUARD - 1)   # the entries of `order` that name no row: just outside and at the envelope's edge
# what the margins of an embedded `order` hold: an in-range row, so that a walk that left the R entries acts on a real row
GUARD_ROW = PERM[0]


def _with(entries):
    order = list(PERM)
    for j, r in entries.items():
        order[j] = r
    return order


def _first_middle_last():
    """each of BAD at the first, a middle and the last position of a list: policy 0 has positions 0 .. 4, policy 2
    5 .. 11, policy 3 12 .. 19, policy 4 20 .. 23"""
    spots = {0: (0, 2, 4), 2: (5, 8, 11), 3: (12, 16, 19), 4: (20, 21, 23)}
    entries = {}
    for i, where in enumerate(spots.values()):
        for p, j in enumerate(where):
            entries[j] = BAD[(i + p) % 4]
    return _with(entries)


# name -> (order, offsets, A)
CASES = {
    'control': (list(PERM), CONTROL, CASE_A),
    'offsets_beyond_both_ends': (list(PERM), [-GUARD, 5, 5, 12, 20, R + GUARD], CASE_A),
    'offsets_just_beyond_both_ends': (list(PERM), [-1, 5, 5, 12, 20, R + 1], CASE_A),
    'all_offsets_equal': (list(PERM), [7] * 6, CASE_A),
    'all_offsets_below_zero': (list(PERM), [-GUARD, -3, -3, -2, -1, -1], CASE_A),
    'all_offsets_above_the_rows': (list(PERM), [R + 1, R + 2, R + 2, R + 3, R + GUARD, R + GUARD], CASE_A),
    'last_offset_short': (list(PERM), [0, 5, 5, 12, 20, 21], CASE_A),
    'first_offset_positive': (list(PERM), [3, 5, 9, 12, 20, 24], CASE_A),
    'decreasing_pair_in_the_middle': (list(PERM), [0, 10, 4, 12, 20, 24], CASE_A),
    'decreasing_pair_then_empty': (list(PERM), [0, 10, 20, 15, 15, 15], CASE_A),
    'bad_entries_first_middle_last': (_first_middle_last(), CONTROL, CASE_A),
    'whole_list_bad': (_with({j: BAD[j % 4] for j in range(5, 12)}), CONTROL, CASE_A),
    'row_twice_in_one_policy': (_with({13: PERM[12]}), CONTROL, CASE_A),
}

# The cases in which two policies' effective lists share a row.  The scores kernel only reads, so they are inputs for it;
# the acting kernel would write such a row from two workgroups (a race, the plan's business): not an acting input.
OVERLAPPING = ('decreasing_pair_in_the_middle',)
ACTING_CASES = tuple(name for name in CASES if name not in OVERLAPPING)
# the cases whose entries of `order` all name rows: what is wrong with them, if anything, is in `offsets`
OFFSET_CASES = tuple(name for name, (order, _, _) in CASES.items() if all(0 <= r < R for r in order))

# The prefetch walk of multi_act_league_kernel: K = 1, N = 70, A = 64 gives wgps = 4 workgroups of 8 waves per policy, so
# the wave that starts at list position p goes on to p + 32 and p + 64.  One policy (37) plays all 70 rows; the waves at
# p = 0 .. 5 visit three positions each, and they meet (bad: an entry outside [0, 70)):
PREFETCH_K, PREFETCH_N, PREFETCH_A, PREFETCH_POLICY = 1, 70, 64, 37
PREFETCH_PATTERNS = {0: ('bad', 'ok', 'ok'), 1: ('ok', 'bad', 'ok'), 2: ('ok', 'ok', 'bad'), 3: ('bad', 'bad', 'ok'),
                     4: ('ok', 'bad', 'bad'), 5: ('bad', 'bad', 'bad')}


def prefetch_case():
    """(order, offsets, A): the identity list of 70 rows with the bad entries of PREFETCH_PATTERNS"""
    rows = PREFETCH_K * PREFETCH_N
    bad = (-1, -GUARD, rows, rows + GUARD - 1)
    order, n = list(range(rows)), 0
    for p, pattern in PREFETCH_PATTERNS.items():
        for visit, what in enumerate(pattern):
            if what == 'bad':
                order[p + 32 * visit] = bad[n % 4]
                n += 1
    offsets = [0] * (PREFETCH_POLICY + 1) + [rows] * (PREFETCH_A - PREFETCH_POLICY)
    return order, offsets, PREFETCH_A


# The scores kernel at width: thread t of a policy's workgroup takes the list entries t, t + 256, ... and the four waves
# meet in LDS.  Lists below, at and above one wave (63, 64, 65), one pass of the workgroup (255, 256, 257) and one of more
# than two passes (600), an empty one and a single row.  (They sum to 1561 rows.)
WIDTH_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 600)
WIDTH_R = sum(WIDTH_COUNTS)
WIDTH_SEED = 5


def width_plan():
    """(order, offsets, A, lists) of a valid plan with WIDTH_COUNTS rows per policy, scattered by a seeded permutation"""
    order = [int(r) for r in np.random.default_rng(WIDTH_SEED).permutation(WIDTH_R)]
    offsets = [0] + [int(o) for o in np.cumsum(WIDTH_COUNTS)]
    lists = [order[offsets[a]:offsets[a + 1]] for a in range(len(WIDTH_COUNTS))]
    return order, offsets, len(WIDTH_COUNTS), lists


def integer_window(T, R):
    """a synthetic (T, R) window of integer values below 2^24, exact in float: rewards[t, r] = r + R t, food and size
    other linear forms of the same, the flags periodic in r + t with different periods — a dropped, doubled or
    misplaced row changes a sum"""
    x = (np.arange(R)[None, :] + R * np.arange(T)[:, None]).astype(np.int64)
    rt = np.arange(R)[None, :] + np.arange(T)[:, None]
    out = {'rewards': x.astype(np.float32), 'food': (2 * x + 1).astype(np.float32), 'size': (3 * x + 2).astype(np.float32),
           'dones': rt % 3 == 0, 'snake_collision': rt % 2 == 0, 'edge_collision': rt % 5 == 1, 'boost': rt % 7 < 3}
    assert 3 * int(x.max()) + 2 < 2 ** 24
    return out


def uniform_window(T, R, seed=WIDTH_SEED):
    """the same keys with uniform fp32 rewards in [-1, 1) and food, size in [0, 1): sums that need the double"""
    g = np.random.default_rng(seed)
    out = integer_window(T, R)
    out['rewards'] = (2 * g.random((T, R), np.float32) - 1).astype(np.float32)
    out['food'], out['size'] = g.random((T, R), np.float32), g.random((T, R), np.float32)
    return out


FLOAT_COLUMNS = {1: 'rewards', 3: 'food', 7: 'size'}   # column of the table -> the fp32 key it sums


def float_sum_bounds(lists, out):
    """{(policy, column): (float64 sum, bound, fp32 sum)} for the fp32 columns of a window.  Every term converts to
    double exactly, so a double sum of n terms in ANY order is within (n - 1) 2^-53 sum|x| of the exact one (to first
    order; the factor is rounded up to n): the kernel's order and numpy's may differ by 2 n 2^-53 sum|x|.  The fp32 sum is
    a sequential float accumulation in list order, step by step: what an accumulator of the wrong width would give."""
    cells = {}
    for a, rows in enumerate(lists):
        cols = np.asarray(rows, np.int64)
        for c, key in FLOAT_COLUMNS.items():
            x = out[key][:, cols].T.reshape(-1)          # (the kernel walks a row's column down the steps)
            n = x.size
            want = float(x.astype(np.float64).sum())
            bound = 2.0 * n * 2.0 ** -53 * float(np.abs(x.astype(np.float64)).sum())
            f32 = float(np.cumsum(x, dtype=np.float32)[-1]) if n else 0.0
            cells[a, c] = (want, bound, f32)
    return cells


def lineup_of(lists, K, N):
    """(K, N) int64: who plays each row according to `lists` (the last policy that lists it), -1 for a row nobody plays"""
    lineup = np.full(K * N, -1, np.int64)
    for a, rows in enumerate(lists):
        lineup[np.asarray(rows, np.int64)] = a
    return lineup.reshape(K, N)


# ---------------------------------------------------------------------------------------------------- guarded buffers

Guarded = namedtuple('Guarded', ('view', 'whole', 'guard', 'sentinel'))


def embed(t, guard, sentinel, device=None, rows=None):
    """`t` as a contiguous view in the middle of a larger allocation on `device`: `guard` rows of t's trailing shape
    before and after it, filled with `sentinel`.  rows: how many leading dimensions of `t` form one row index (default 1;
    2 for a (T, R, .) tensor, whose guard then is `guard` rows of the flat (T R, .) form)."""
    t = torch.as_tensor(t)
    lead = 1 if rows is None else rows
    flat = t.reshape((-1,) + tuple(t.shape[lead:]))
    whole = torch.full((flat.shape[0] + 2 * guard,) + tuple(flat.shape[1:]), sentinel, dtype=t.dtype, device=device)
    whole[guard:guard + flat.shape[0]] = flat.to(whole.device)
    view = whole[guard:guard + flat.shape[0]].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() == whole.data_ptr() + guard * whole[0].numel() * whole.element_size()
    return Guarded(view, whole, guard, sentinel)


def guards_intact(g):
    """whether both margins of an embedded tensor still hold the sentinel"""
    n = g.whole.shape[0]
    return bool((g.whole[:g.guard] == g.sentinel).all()) and bool((g.whole[n - g.guard:] == g.sentinel).all())


def embedded_plan(order, offsets, A, K, N, device):
    """(LeaguePlan, the Guarded `order`): `order` with GUARD entries of GUARD_ROW-like in-range rows around it (row 0 of the
    shape at hand where GUARD_ROW does not exist), `offsets` as it is (the kernels read its A + 1 entries whatever they
    hold), and a line-up of the right shape, which nothing reads on the device"""
    from wurm_amd.envs._multi_league import LeaguePlan
    assert len(order) == K * N and len(offsets) == A + 1
    row = GUARD_ROW if GUARD_ROW < K * N else 0
    guarded = embed(torch.tensor(order, dtype=torch.int32), GUARD, row, device)
    lineup = torch.zeros((K, N), dtype=torch.long, device=device)
    return LeaguePlan(lineup, guarded.view, torch.tensor(offsets, dtype=torch.long, device=device), A), guarded
