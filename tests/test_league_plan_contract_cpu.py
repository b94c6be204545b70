"""tests/league_lists_ref.py checked without a GPU: the two restated rules agree with `league_plan` and the brute-force plan
on valid plans, the learner's lists are disjoint pieces of `order` on every malformed case, every case stays inside the
guard envelope the GPU tests rely on, and the acting cases name no row twice across policies."""
import types

import numpy as np
import pytest
import torch

from tests import league_lists_ref as L
from tests import multi_league_ref as ref
from wurm_amd.envs._multi_league import league_plan

ALL_CASES = dict(L.CASES, prefetch=L.prefetch_case())


def _rows(name):
    return L.PREFETCH_K * L.PREFETCH_N if name == 'prefetch' else L.R


@pytest.mark.parametrize('K,N,A,seed', [(3, 8, 5, 0), (1, 70, 64, 1), (2, 4, 5, 2), (4, 20, 3, 3), (1, 1, 1, 4)])
def test_both_rules_give_the_brute_plans_lists_on_valid_plans(K, N, A, seed):
    lineup = np.random.default_rng(seed).integers(0, A, (K, N))
    plan = league_plan(types.SimpleNamespace(num_snakes=K, num_envs=N), torch.from_numpy(lineup), A)
    order, offsets = plan.order.tolist(), plan.offsets.tolist()
    want_order, want_offsets = ref.brute_plan(lineup, A)
    want = [want_order[want_offsets[a]:want_offsets[a + 1]] for a in range(A)]
    assert L.act_lists(order, offsets, K * N) == want
    members = L.learner_lists(order, offsets, K * N)
    assert [[order[j] for j in m.positions] for m in members] == want
    assert not any(any(m.inert) for m in members)
    assert L.normalised_offsets(order, offsets, K * N) == offsets == want_offsets
    base = 0
    for m, rows in zip(members, want):
        assert (m.first, m.M, m.base) == (want_offsets[members.index(m)], len(rows), base)
        base += min(len(rows), 256)


def test_base_counts_at_most_256_groups_per_member():
    order, offsets, A, lists = L.width_plan()
    members = L.learner_lists(order, offsets, L.WIDTH_R)
    assert [m.M for m in members] == list(L.WIDTH_COUNTS) and [len(l) for l in lists] == list(L.WIDTH_COUNTS)
    assert [m.base for m in members] == [0, 0, 1, 64, 128, 193, 448, 704, 960]
    assert sorted(order) == list(range(L.WIDTH_R)) and order != sorted(order) and L.WIDTH_R == 1561


@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_learner_lists_are_disjoint_pieces_of_order(name):
    order, offsets, A = ALL_CASES[name]
    R = _rows(name)
    members = L.learner_lists(order, offsets, R)
    assert len(members) == A
    seen, end = set(), 0
    for m in members:
        assert 0 <= m.first and m.M >= 0 and m.first + m.M <= R and m.first >= end
        assert m.positions == list(range(m.first, m.first + m.M)) and len(m.inert) == m.M
        assert not seen & set(m.positions)
        seen |= set(m.positions)
        end = m.first + m.M
    assert sum(m.M for m in members) <= R
    norm = L.normalised_offsets(order, offsets, R)
    assert norm == sorted(norm) and 0 <= norm[0] and norm[-1] <= R
    again = L.learner_lists(order, norm, R)           # (normalising is idempotent: the twin plan of the GPU test)
    assert again == members


@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_cases_stay_inside_the_guard_envelope(name):
    """offsets in [-G, R + G], entries of `order` in [-G, R + G), R <= 80, and where the offsets decrease somewhere no
    clamped offset lies below the first one: a learner WITHOUT the running maximum would then still keep its partials
    inside the workspace (its `base` is the current clamped offset minus the first), which is what lets a scratch build
    with that defect run under these tests."""
    order, offsets, A = ALL_CASES[name]
    R, G = _rows(name), L.GUARD
    assert len(order) == R <= 80 and len(offsets) == A + 1 and A >= 1
    assert all(isinstance(v, int) for v in order + offsets)
    assert all(-G <= o <= R + G for o in offsets), offsets
    assert all(-G <= r < R + G for r in order), order
    assert 0 <= L.GUARD_ROW < R
    clamped = [min(max(o, 0), R) for o in offsets]
    if any(b < a for a, b in zip(offsets, offsets[1:])):
        assert min(clamped) == clamped[0]


@pytest.mark.parametrize('name', sorted(ALL_CASES))
def test_only_the_overlapping_cases_share_a_row_between_policies(name):
    order, offsets, A = ALL_CASES[name]
    lists = L.act_lists(order, offsets, _rows(name))
    owners = {}
    for a, rows in enumerate(lists):
        for r in rows:
            owners.setdefault(r, set()).add(a)
    shared = sorted(r for r, who in owners.items() if len(who) > 1)
    assert bool(shared) == (name in L.OVERLAPPING), shared
    assert (name in L.ACTING_CASES or name == 'prefetch') == (not shared)


def test_the_cases_are_what_their_names_say():
    R, G, C = L.R, L.GUARD, L.CASES
    act = {name: L.act_lists(o, f, R) for name, (o, f, _) in C.items()}
    learn = {name: L.learner_lists(o, f, R) for name, (o, f, _) in C.items()}
    rows_of = lambda name: [[C[name][0][j] for j, dead in zip(m.positions, m.inert) if not dead] for m in learn[name]]
    control = [L.PERM[a:b] for a, b in zip(L.CONTROL, L.CONTROL[1:])]
    assert act['control'] == control == rows_of('control') and [len(l) for l in control] == [5, 0, 7, 8, 4]
    assert sorted(L.PERM) == list(range(R)) and L.PERM != sorted(L.PERM)
    for name in ('offsets_beyond_both_ends', 'offsets_just_beyond_both_ends'):   # the clamps give the control's lists
        assert C[name][1][0] < 0 and C[name][1][-1] > R and act[name] == control == rows_of(name)
    assert C['offsets_beyond_both_ends'][1][0] == -G and C['offsets_beyond_both_ends'][1][-1] == R + G
    # ... and a later member's base depends on the clamped first offset: unclamped, member 0 would have 5 + G columns
    assert [m.base for m in learn['offsets_beyond_both_ends']] == [0, 5, 5, 12, 20]
    for name in ('all_offsets_equal', 'all_offsets_below_zero', 'all_offsets_above_the_rows'):
        assert act[name] == [[]] * 5 and [m.M for m in learn[name]] == [0] * 5
    assert all(o < 0 for o in C['all_offsets_below_zero'][1]) and all(o > R for o in C['all_offsets_above_the_rows'][1])
    assert act['last_offset_short'][4] == L.PERM[20:21] and sum(map(len, act['last_offset_short'])) == 21
    assert act['first_offset_positive'][0] == L.PERM[3:5] == rows_of('first_offset_positive')[0]
    # THE DIFFERENCE between the two rules: offsets 0, 10, 4, 12: acting and scores give policy 1 nothing and policy 2
    # order[4:12], which shares order[4:10] with policy 0; the learner gives member 1 nothing and member 2 order[10:12]
    name = 'decreasing_pair_in_the_middle'
    assert act[name] == [L.PERM[0:10], [], L.PERM[4:12], L.PERM[12:20], L.PERM[20:24]]
    assert rows_of(name) == [L.PERM[0:10], [], L.PERM[10:12], L.PERM[12:20], L.PERM[20:24]]
    assert L.normalised_offsets(*C[name][:2], R) == [0, 10, 10, 12, 20, 24]
    name = 'decreasing_pair_then_empty'
    assert act[name] == [L.PERM[0:10], L.PERM[10:20], [], [], []] == rows_of(name)
    for name in C:   # everywhere else the two rules agree on the rows
        assert (act[name] == rows_of(name)) == (name != 'decreasing_pair_in_the_middle'), name
    # each bad value at the first, a middle and the last position of a list
    order = C['bad_entries_first_middle_last'][0]
    where = {bad: set() for bad in L.BAD}
    for a, b in zip(L.CONTROL, L.CONTROL[1:]):
        for j in range(a, b):
            if order[j] in where:
                where[order[j]].add('first' if j == a else 'last' if j == b - 1 else 'middle')
    assert L.BAD == (-1, -G, R, R + G - 1) and all(w == {'first', 'middle', 'last'} for w in where.values()), where
    assert sum(map(len, act['bad_entries_first_middle_last'])) == R - 12
    assert [sum(m.inert) for m in learn['bad_entries_first_middle_last']] == [3, 0, 3, 3, 3]
    assert act['whole_list_bad'][2] == [] and learn['whole_list_bad'][2].inert == [True] * 7
    assert set(C['whole_list_bad'][0][5:12]) == set(L.BAD)
    twice = act['row_twice_in_one_policy'][3]
    assert twice.count(L.PERM[12]) == 2 and L.PERM[13] not in sum(act['row_twice_in_one_policy'], [])
    assert set(L.OFFSET_CASES) == set(C) - {'bad_entries_first_middle_last', 'whole_list_bad'}


def test_prefetch_case_shows_every_pattern_to_one_wave():
    order, offsets, A = L.prefetch_case()
    rows = L.PREFETCH_K * L.PREFETCH_N
    lists = L.act_lists(order, offsets, rows)
    assert [a for a, l in enumerate(lists) if l] == [L.PREFETCH_POLICY]
    # the launch plan of multi_league.hpp: 8 waves per workgroup, wgps = min(ceil(rows / 8), max(1, 256 // A)) of them
    wgps = min((rows + 7) // 8, max(1, 256 // A))
    stride = 8 * wgps
    assert (wgps, stride) == (4, 32)
    seen = {}
    for p in range(stride):
        visits = tuple('ok' if 0 <= order[j] < rows else 'bad' for j in range(p, rows, stride))
        seen[p] = visits
    assert {p: seen[p] for p in L.PREFETCH_PATTERNS} == L.PREFETCH_PATTERNS
    for want in (('bad', 'ok', 'ok'), ('ok', 'bad', 'ok'), ('ok', 'ok', 'bad'), ('bad', 'bad', 'ok')):
        assert want in seen.values()
    assert all(set(v) == {'ok'} for p, v in seen.items() if p not in L.PREFETCH_PATTERNS)
    assert len(lists[L.PREFETCH_POLICY]) == rows - 10


def test_score_table_of_lists_is_score_table_and_counts_a_double_listing_twice():
    K, N, A, T = 3, 8, 5, 3
    lineup = np.random.default_rng(9).integers(0, A, (K, N))
    order, offsets = ref.brute_plan(lineup, A)
    lists = L.act_lists(order, offsets, K * N)
    windows = [L.integer_window(T, K * N), L.integer_window(1, K * N)]
    want = ref.score_table(lineup, A, windows)
    assert np.array_equal(L.score_table_of_lists(lists, windows), want) and want[:, 1:].any(axis=0).all()
    plain = [{k: w[k] for k in ('rewards', 'dones')} for w in windows]
    assert not L.score_table_of_lists(lists, plain)[:, 3:].any()
    twice = [list(l) for l in lists]
    twice[0] = twice[0] + twice[0][:1]
    extra = L.score_table_of_lists(twice, windows) - want
    one = L.score_table_of_lists([twice[0][:1]], windows)[0]
    assert np.array_equal(extra[0], one) and not extra[1:].any() and one[0] == T + 1
    # a flag held as another non-zero byte counts as 1
    loud = dict(windows[0], dones=windows[0]['dones'].astype(np.uint8) * 255, boost=windows[0]['boost'].astype(np.uint8) * 2)
    assert np.array_equal(L.score_table_of_lists(lists, [loud]), ref.score_table(lineup, A, windows[:1]))


@pytest.mark.parametrize('T', [1, 3])
def test_a_float_accumulator_would_break_the_width_bound(T):
    """the seed of the uniform window is chosen so that this holds: the bound of the GPU test tells a float accumulator
    from a double one"""
    _, _, _, lists = L.width_plan()
    cells = L.float_sum_bounds(lists, L.uniform_window(T, L.WIDTH_R))
    broken = [cell for cell, (want, bound, f32) in cells.items() if abs(f32 - want) > bound]
    assert len(broken) >= 12, broken            # (of 24 cells with rows: all but the shortest lists)
    for (a, c), (want, bound, f32) in cells.items():
        assert (bound == 0.0) == (L.WIDTH_COUNTS[a] == 0)
        # numpy's own pairwise float64 sum against the exactly rounded one: inside half the bound, as derived
        cols = np.asarray(lists[a], np.int64)
        x = L.uniform_window(T, L.WIDTH_R)[L.FLOAT_COLUMNS[c]][:, cols].reshape(-1).astype(np.float64)
        import math
        assert abs(want - math.fsum(x)) <= bound / 2


def test_embed_and_guards_intact():
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    g = L.embed(t, 5, -7.0, rows=2)
    assert torch.equal(g.view, t) and g.view.is_contiguous() and g.whole.shape == (16, 4) and L.guards_intact(g)
    g.view[0, 0, 0] = 99.0
    assert L.guards_intact(g)
    g.whole[4, 3] = 0.0                      # the last element before the view
    assert not L.guards_intact(g)
    g = L.embed(torch.tensor([1, 2, 3], dtype=torch.int32), 2, 7)
    assert g.whole.tolist() == [7, 7, 1, 2, 3, 7, 7] and L.guards_intact(g)
    g.whole[5] = 0                           # the first element behind it
    assert not L.guards_intact(g)
    g = L.embed(torch.zeros(3, dtype=torch.bool), 2, True)
    assert g.whole.tolist() == [True, True, False, False, False, True, True] and L.guards_intact(g)
