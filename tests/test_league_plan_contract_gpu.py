"""The five league kernels on plans `league_plan` never makes (tests/league_lists_ref.py: CASES), against the rule each
header documents (wurm_amd/csrc/multi_league.hpp; wurm_amd/csrc/a2c_learner.hpp: league_member), and league_scores_kernel
at lists wider than a wave and a workgroup.  Every array a malformed value indexes is a view in the middle of a larger
allocation whose margins hold a sentinel, and every malformed value stays within those margins
(tests/test_league_plan_contract_cpu.py checks the cases for that): a broken clamp or skip shows as a wrong value or a
touched margin."""
import numpy as np
import pytest
import torch

from tests import a2c_gae_ref as gae
from tests import a2c_learner_ref as a2c_ref
from tests import league_lists_ref as L
from tests import multi_act_ref as act_ref
from tests import multi_league_ref as ref
from tests.test_a2c_league_gpu import _agents, _kw, _window
from tests.test_a2c_learner_gpu import assert_within_bound
from tests.test_multi_league_gpu import SEED, _env, _league_params
from wurm_amd import _lib
from wurm_amd.envs import _multi_act, _multi_league
from wurm_amd.envs._multi_league import LeaguePlan
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation, LeagueTable

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = L.GUARD
SENTINEL = -7777          # what outputs are pre-filled with and every float / integer margin holds


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------------------------ acting

def _act_and_check(E, K, N, order, offsets, A, what):
    """one `act_league` under the hand-built plan, all of its arrays guarded; the rows of the effective lists against the
    oracle, everything else against the sentinel"""
    R, n = K * N, act_ref.OBS_N[E]
    lists = L.act_lists(order, offsets, R)
    lineup = L.lineup_of(lists, K, N)
    played = lineup >= 0
    used = sorted(set(lineup[played].tolist()))
    params = _league_params(A, E, used) if used else np.full((A, _multi_act.num_policy_params(E)), np.nan,
                                                             np.float32)
    assert all(np.isnan(params[a]).all() for a in range(A) if not lists[a])     # (a read of one would show)
    env = _env(n, K, N, seed=SEED)
    plan, g_order = L.embedded_plan(order, offsets, A, K, N, DEV)
    x = act_ref.random_rows(K, N, E, seed=E)
    g_x = L.embed(torch.from_numpy(x), G, float(SENTINEL), DEV, rows=2)
    outs = (L.embed(torch.full((K, N), SENTINEL, dtype=torch.long), G, SENTINEL, DEV, rows=2),
            L.embed(torch.full((K, N, 4), float(SENTINEL)), G, float(SENTINEL), DEV, rows=2),
            L.embed(torch.full((K, N), float(SENTINEL)), G, float(SENTINEL), DEV, rows=2))
    count = _lib.lib().wurm_launch_count
    torch.cuda.synchronize()
    before = count()
    got = _multi_league.act_league(env, _dev(params), g_x.view, plan, out=tuple(o.view for o in outs))
    assert count() - before == 1 and env.policy_calls == 1, what
    torch.cuda.synchronize()
    actions, probs, values = (o.view.cpu().numpy() for o in outs)
    assert got['actions_t'].data_ptr() == outs[0].view.data_ptr()
    if used:
        stand_in = np.where(played, lineup, used[0])     # (rows nobody plays: computed with some policy, then not compared)
        want_probs, want_values, want_actions = ref.expected_rows(params, x, stand_in, SEED, 0)
        assert np.array_equal(probs[played], want_probs[played]), (what, 'probs')
        assert np.array_equal(values[played], want_values[played]), (what, 'values')
        assert np.array_equal(actions[played], want_actions[played]), (what, 'actions')
    assert (probs[~played] == SENTINEL).all() and (values[~played] == SENTINEL).all() and \
        (actions[~played] == SENTINEL).all(), (what, 'a row no list names was written')
    for o, name in zip(outs + (g_x, g_order), ('actions', 'probs', 'values', 'observations', 'order')):
        assert L.guards_intact(o), (what, name, 'guard touched')
    return played


@pytest.mark.parametrize('name', L.ACTING_CASES)
@pytest.mark.parametrize('E', [27, 507])   # LDS below 64 KiB, and above (the hipFuncSetAttribute path)
def test_acting_follows_the_documented_lists(E, name):
    order, offsets, A = L.CASES[name]
    played = _act_and_check(E, L.CASE_K, L.CASE_N, order, offsets, A, (name, E))
    assert int(played.sum()) == len(set(sum(L.act_lists(order, offsets, L.R), [])))


def test_acting_prefetch_walk_skips_bad_entries():
    """K = 1, N = 70, A = 64: a wave visits list positions p, p + 32, p + 64, and the waves p = 0 .. 5 meet (bad, ok, ok),
    (ok, bad, ok), (ok, ok, bad), (bad, bad, ok), (ok, bad, bad) and (bad, bad, bad): the row staged and the row acted on
    must stay the same row through every skip"""
    order, offsets, A = L.prefetch_case()
    played = _act_and_check(27, L.PREFETCH_K, L.PREFETCH_N, order, offsets, A, 'prefetch')
    skipped = sorted(p + 32 * v for p, pat in L.PREFETCH_PATTERNS.items() for v, w in enumerate(pat) if w == 'bad')
    assert np.nonzero(~played.reshape(-1))[0].tolist() == skipped and len(skipped) == 10


# ------------------------------------------------------------------------------------------------ scores

FLAGS = ('dones', 'boost', 'snake_collision', 'edge_collision')


def _guarded_window(window, flags_as=None):
    """{key: Guarded} of a numpy window on the device.  flags_as 'uint8': the flags as bytes holding 2 and 255 where set"""
    out = {}
    for k, v in window.items():
        if k in FLAGS and flags_as == 'uint8':
            loud = np.where((np.arange(v.size).reshape(v.shape) % 2) == 0, 2, 255).astype(np.uint8)
            out[k] = L.embed(torch.from_numpy(np.where(v, loud, 0).astype(np.uint8)), G, 171, DEV, rows=2)
        elif k in FLAGS:
            out[k] = L.embed(torch.from_numpy(v), G, True, DEV, rows=2)
        else:
            out[k] = L.embed(torch.from_numpy(v), G, float(SENTINEL), DEV, rows=2)
    return out


def _table(A):
    """(LeagueTable whose table is a guarded view, the Guarded)"""
    table = LeagueTable(A, DEV)
    g = L.embed(torch.zeros((A, len(ref.COLUMNS)), dtype=torch.float64), G, float(SENTINEL), DEV)
    table.table = g.view
    return table, g


def _update(table, plan, guarded):
    count = _lib.lib().wurm_launch_count
    before = count()
    table.update(plan, {k: g.view for k, g in guarded.items()})
    assert count() - before == 1


@pytest.mark.parametrize('name', sorted(L.CASES))
def test_scores_follow_the_documented_lists(name):
    """every case, the overlapping lists and the row listed twice included (the kernel only reads): the table is exactly
    the float64 sum over the lists of the acting rule"""
    order, offsets, A = L.CASES[name]
    T = 3
    window = L.integer_window(T, L.R)
    plan, g_order = L.embedded_plan(order, offsets, A, L.CASE_K, L.CASE_N, DEV)
    guarded = _guarded_window(window)
    table, g_table = _table(A)
    _update(table, plan, guarded)
    want = L.score_table_of_lists(L.act_lists(order, offsets, L.R), [window])
    got = table.table.cpu().numpy()
    assert np.array_equal(got, want), (name, got, want)
    assert L.guards_intact(g_table) and L.guards_intact(g_order) and all(L.guards_intact(g) for g in guarded.values())


@pytest.mark.parametrize('flags_as', ['bool', 'uint8'])
@pytest.mark.parametrize('T', [1, 3])
def test_scores_at_width_integer_data(T, flags_as):
    """lists of 0, 1, 63, 64, 65, 255, 256, 257 and 600 rows: the stride loop and all four waves hold data.  Integer data:
    exact; exact again after a second update adds to the table; the same bits on a repeat run; a flag byte of 2 or 255
    counts as 1; without the info=True keys columns 3 .. 7 stay zero."""
    order, offsets, A, lists = L.width_plan()
    window = L.integer_window(T, L.WIDTH_R)
    plan, g_order = L.embedded_plan(order, offsets, A, 1, L.WIDTH_R, DEV)
    guarded = _guarded_window(window, flags_as)
    want = L.score_table_of_lists(lists, [window])
    assert want[2:, 1:].all() and not want[0].any() and want[:, 0].tolist() == [float(T * c) for c in L.WIDTH_COUNTS]
    tables = []
    for run in range(2):
        table, g_table = _table(A)
        _update(table, plan, guarded)
        once = table.table.cpu().numpy()
        assert np.array_equal(once, want), (run, once, want)
        _update(table, plan, guarded)
        assert np.array_equal(table.table.cpu().numpy(), 2 * want), run
        assert L.guards_intact(g_table)
        tables.append(table.table.clone())
    assert torch.equal(tables[0], tables[1])
    plain, g_plain = _table(A)
    _update(plain, plan, {k: guarded[k] for k in ('rewards', 'dones')})
    got = plain.table.cpu().numpy()
    assert np.array_equal(got[:, :3], want[:, :3]) and not got[:, 3:].any()
    assert L.guards_intact(g_plain) and L.guards_intact(g_order) and all(L.guards_intact(g) for g in guarded.values())


@pytest.mark.parametrize('T', [1, 3])
def test_scores_at_width_float_data_sum_in_double(T):
    """uniform fp32 rewards, food and size against numpy's float64 sum.  Every term converts to double exactly, so the
    kernel's sum and numpy's are each within (n - 1) 2^-53 sum|x| of the exact sum of the cell's n terms, whatever their
    order: |got - want| <= 2 n 2^-53 sum|x|.  Derived, not tuned; an fp32 accumulator breaks it on most cells
    (tests/test_league_plan_contract_cpu.py: test_a_float_accumulator_would_break_the_width_bound)."""
    order, offsets, A, lists = L.width_plan()
    window = L.uniform_window(T, L.WIDTH_R)
    plan, _ = L.embedded_plan(order, offsets, A, 1, L.WIDTH_R, DEV)
    guarded = _guarded_window(window)
    table, g_table = _table(A)
    _update(table, plan, guarded)
    got = table.table.cpu().numpy()
    cells = L.float_sum_bounds(lists, window)
    assert sum(abs(f32 - want) > bound for want, bound, f32 in cells.values()) >= 12
    worst = 0.0
    for (a, c), (want, bound, _) in cells.items():
        err = abs(got[a, c] - want)
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (a, c, got[a, c], want, err, bound)
    print(f'T={T}: worst |got - want| / bound over {len(cells)} cells: {worst:.3e}')
    counts = L.score_table_of_lists(lists, [window])
    assert np.array_equal(got[:, [0, 2, 4, 5, 6]], counts[:, [0, 2, 4, 5, 6]]) and L.guards_intact(g_table)


# ------------------------------------------------------------------------------------------------ learner

E_LEARN, T_LEARN = 27, 2
STATE_KEYS = ('params', 'exp_avg', 'exp_avg_sq')


def _guarded_learner_inputs(state, out):
    """(state, out, guards): the window's tensors as guarded views (margins of G rows of the flat (T R, .) form)"""
    g_state = L.embed(state.cpu(), G, float(SENTINEL), DEV)
    gs = {'observations': L.embed(out['observations'].cpu(), G, float(SENTINEL), DEV, rows=2),
          'actions': L.embed(out['actions'].cpu(), G, SENTINEL, DEV, rows=2),
          'rewards': L.embed(out['rewards'].cpu(), G, float(SENTINEL), DEV, rows=2),
          'dones': L.embed(out['dones'].cpu(), G, True, DEV, rows=2)}
    return g_state.view, {k: g.view for k, g in gs.items()}, [g_state] + list(gs.values())


def _snapshot(pop):
    return tuple(getattr(pop, k).clone() for k in STATE_KEYS)


@pytest.mark.parametrize('use_gae', [False, True])
@pytest.mark.parametrize('name', L.OFFSET_CASES)
def test_learner_normalises_malformed_offsets(name, use_gae):
    """offsets that leave [0, R] or decrease, entries of `order` all valid: `grad` and two `update`s equal, bit for bit,
    those of a twin population under the plan normalised as league_member documents (clamp, running maximum).  In
    'offsets_beyond_both_ends' the base of every later member depends on the clamp of the first offset."""
    order, offsets, A = L.CASES[name]
    R = L.R
    members = L.learner_lists(order, offsets, R)
    state, out = _window(E_LEARN, R, T_LEARN)
    g_state, g_out, guards = _guarded_learner_inputs(state, out)
    plan, g_order = L.embedded_plan(order, offsets, A, L.CASE_K, L.CASE_N, DEV)
    normal = LeaguePlan(plan.lineup, torch.tensor(order, dtype=torch.int32, device=DEV),
                        torch.tensor(L.normalised_offsets(order, offsets, R), dtype=torch.long, device=DEV), A)
    kw = _kw(A, use_gae, 'smooth_l1')[0]
    pop, twin = FusedA2CPopulation(_agents(A, E_LEARN), **kw), FusedA2CPopulation(_agents(A, E_LEARN), **kw)
    initial = _snapshot(pop)

    def same(a, b, what):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (name, what, k)

    grad, losses = pop.grad(g_state, g_out, plan=plan)
    grad2, losses2 = twin.grad(state, out, plan=normal)
    same(dict(losses, grad=grad), dict(losses2, grad=grad2), 'grad')
    assert ('returns' in losses) == use_gae
    for i in range(2):
        same(pop.update(g_state, g_out, plan=plan), twin.update(state, out, plan=normal), ('update', i))
        for k in STATE_KEYS:
            assert torch.equal(getattr(pop, k), getattr(twin, k)), (name, i, k)
    for a, m in enumerate(members):       # a member without columns keeps its state; the others moved
        for k, old in zip(STATE_KEYS, initial):
            assert torch.equal(getattr(pop, k)[a], old[a]) == (m.M == 0), (name, a, k)
        assert bool(grad[a].any()) == (m.M > 0)
    # the columns no member's list names are zeros, the others written
    named = sorted(set(order[j] for m in members for j in m.positions))
    rest = sorted(set(range(R)) - set(named))
    for k in ('values',) + (('returns',) if use_gae else ()):   # (a return may be an exact zero: v - v behind a done)
        assert not losses[k][:, rest].any() and (k == 'returns' or bool((losses[k][:, named] != 0).all())), (name, k)
    assert all(L.guards_intact(g) for g in guards + [g_order])


# The plan of the bad-entries test, over the R = 40 columns of a fixture of tests/a2c_learner_ref.py: member 0 has 12
# positions, inert at the first, two middle ones and the last; member 1's five are all inert; member 2 has ten valid
# columns; member 3 none.  The positions 27 .. 39 of `order` belong to nobody.
R_BAD, A_BAD = 40, 4
OFFSETS_BAD = [0, 12, 17, 27, 27]
INERT_BAD = {0: -1, 4: -G, 7: R_BAD, 11: R_BAD + G - 1, 12: -1, 13: -G, 14: R_BAD, 15: R_BAD + G - 1, 16: -1}


def _bad_orders():
    valid = [int(r) for r in np.random.default_rng(40).permutation(R_BAD)]
    bad = list(valid)
    for j, r in INERT_BAD.items():
        bad[j] = r
    return valid, bad


def _guarded_kind(pop, plan, what, made):
    """the kind of a league call whose `values` / `returns` are zeros, as the Python layer makes them, but in the middle
    of a guarded allocation"""
    def new(shape, dtype, device):
        g = L.embed(torch.zeros(shape, dtype=dtype), G, float(SENTINEL), device, rows=2)
        made.append(g)
        return g.view
    return pop._kind(plan, None, what)._replace(new=new)


@pytest.mark.parametrize('use_gae', [False, True])
def test_learner_bad_entries_are_inert_rows(use_gae):
    """An entry of `order` outside [0, R) is a row with zero input and no loss term that still counts in M: member 0's
    gradient and losses are those of its 8 valid columns times 8 / 12 (float64 specification, the stand-alone learner's
    bound); member 1, all inert, has a zero gradient and takes the Adam step of one; nothing outside the named columns
    of `values` / `returns` is written (zeros from fused_population.py's torch.zeros), no guard is touched."""
    entropy, lam = 0.01, 0.95
    fx = a2c_ref.make_fixture(E_LEARN, T_LEARN, R_BAD, seed=0, reward_scale=3.0)
    valid, bad = _bad_orders()
    members = L.learner_lists(bad, OFFSETS_BAD, R_BAD)
    assert [m.M for m in members] == [12, 5, 10, 0] and [sum(m.inert) for m in members] == [4, 5, 0, 0]
    assert [members[0].inert[i] for i in (0, 4, 7, 11)] == [True] * 4
    made = [a2c_ref.to_device(fx, DEV) for _ in range(A_BAD)]
    _, state, out = made[0]
    g_state, g_out, guards = _guarded_learner_inputs(state, out)
    pop = FusedA2CPopulation([m[0] for m in made], gamma=fx['gamma'], entropy_coef=entropy, use_gae=use_gae,
                             gae_lambda=lam if use_gae else None)
    plan_valid, _ = L.embedded_plan(valid, OFFSETS_BAD, A_BAD, 1, R_BAD, DEV)
    plan_bad, g_order = L.embedded_plan(bad, OFFSETS_BAD, A_BAD, 1, R_BAD, DEV)

    # ---- the gradient under the bad plan, from the fixture's weights
    outputs = []
    grad, losses = pop._grad(_guarded_kind(pop, plan_bad, 'grad', outputs), g_state, g_out)
    assert len(outputs) == (2 if use_gae else 1)
    columns = ('values',) + (('returns',) if use_gae else ())
    named = []
    for a in (0, 2):
        m = members[a]
        idx = torch.tensor([bad[j] for j, dead in zip(m.positions, m.inert) if not dead])
        named += idx.tolist()
        scale = len(idx) / m.M
        sub = dict(fx, N=len(idx), obs0=fx['obs0'][idx].contiguous(), obs=fx['obs'][:, idx].contiguous(),
                   **{k: fx[k][:, idx].contiguous() for k in ('actions', 'rewards', 'dones')})
        if use_gae:
            spec = gae.spec_float64_gae(sub, lam, entropy, 'smooth_l1')
            t32 = gae.example_loss_gae(sub, torch.float32, DEV, lam, entropy, 'smooth_l1')
        else:
            spec = a2c_ref.spec_float64(sub, entropy, 'smooth_l1')
            t32 = a2c_ref.example_loss(sub, torch.float32, DEV, entropy, 'smooth_l1')
        # the inert rows count in inv_B = 1 / (M T): gradient and losses are the valid columns' means times M_valid / M
        scaled = lambda d: dict(d, grad=d['grad'] * scale, losses=d['losses'] * scale)
        mine = {k: losses[k][a] for k in ('value_loss', 'policy_loss', 'entropy')}
        mine['values'] = losses['values'][:, idx.to(DEV)]
        assert_within_bound(sub, grad[a], mine, scaled(spec), scaled(t32), f'member {a}, {len(idx)} of {m.M} columns')
    for a in (1, 3):                                  # all inert / no columns: zeros
        assert not grad[a].any() and all(float(losses[k][a]) == 0.0 for k in ('value_loss', 'policy_loss', 'entropy')), a
    rest = sorted(set(range(R_BAD)) - set(named))
    assert len(named) == 18 and len(rest) == 22
    for k in columns:                                 # (a return may be an exact zero: v - v behind a done)
        assert not losses[k][:, rest].any() and (k == 'returns' or bool((losses[k][:, named] != 0).all())), k
    assert all(L.guards_intact(g) for g in guards + outputs + [g_order])

    # ---- the Adam step: one update under the valid plan (so that every member but 3 has an Adam state), then one under the
    # bad plan, each member against a stand-alone learner that applies the member's own gradient to the member's state
    pop.update(g_state, g_out, plan=plan_valid)
    assert all(bool(pop.exp_avg[a].any()) for a in range(3)) and not pop.exp_avg[3].any()
    before, step = _snapshot(pop), pop.step
    outputs = []
    res = pop._update(_guarded_kind(pop, plan_bad, 'update', outputs), g_state, g_out)
    assert pop.step == step + 1
    assert not res['grad'][1].any() and float(res['grad_norm'][1]) == 0.0 and float(res['grad_norm'][3]) == 0.0
    assert float(res['grad_norm'][0]) > 0.0 and float(res['grad_norm'][2]) > 0.0
    for a in range(3):   # member 1 too: M = 5 > 0, so a2c_ff_apply_league_kernel steps it, on its zero gradient
        single = FusedA2CLearner(_agents(1, E_LEARN)[0], gamma=fx['gamma'], entropy_coef=entropy)
        single.load_state_dict({'params': before[0][a], 'exp_avg': before[1][a], 'exp_avg_sq': before[2][a], 'step': step})
        norm = single.apply(res['grad'][a].clone())
        assert torch.equal(norm, res['grad_norm'][a]), a
        for k, old in zip(STATE_KEYS, before):
            assert torch.equal(getattr(pop, k)[a], getattr(single, k)), (a, k)
            assert not torch.equal(getattr(pop, k)[a], old[a]), (a, k, 'did not move')
    # what the step of a zero gradient is: exp_avg and exp_avg_sq decay, the weights follow the decayed momentum
    assert bool((pop.exp_avg[1].abs() <= before[1][1].abs()).all()) and bool((pop.exp_avg_sq[1] <= before[2][1]).all())
    for k, old in zip(STATE_KEYS, before):            # member 3 has no columns: untouched
        assert torch.equal(getattr(pop, k)[3], old[3]), k
    for k in columns:
        assert not res[k][:, rest].any() and (k == 'returns' or bool((res[k][:, named] != 0).all())), k
    assert all(L.guards_intact(g) for g in guards + outputs + [g_order])
