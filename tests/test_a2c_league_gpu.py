"""`FusedA2CPopulation.grad / update / apply(..., plan=, learn=)`: a population that learns from a league window, member a
from the columns the line-up gives policy a, however many (include/wurm_hip.h: wurm_a2c_ff_league_*; kernels:
a2c_ff_main_kernel<GAE, Kind::League> and a2c_ff_*_league_kernel of wurm_amd/csrc/a2c_learner.hpp).

The expected values come from code the league form does not touch: a fresh `FusedA2CLearner` per policy, loaded with that
member's row of the weights, its Adam state and the shared `step`, and updated on `index_select`ed contiguous copies of
the member's columns in list order.  Everything is compared with `torch.equal`."""
import types

import pytest
import torch

from tests import a2c_gae_ref as gae
from tests import a2c_learner_ref as ref
from tests.test_a2c_learner_gpu import assert_within_bound
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.envs._multi_league import block_lineup, league_plan
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# per-member hyper-parameters, all different
LR = [1e-3, 3e-4, 2e-3, 5e-4, 1.5e-3, 7e-4, 2.5e-3]
GAMMA = [0.99, 0.95, 0.9, 0.97, 0.999, 0.8, 0.93]
ENTROPY = [0.01, 0.0, 0.05, 0.02, 0.0, 0.03, 0.005]
LAMBDA = [0.95] * 7
# rows per member: none, one, fewer than a tile, G_a = M_a up to 256, then two envs for some workgroups (257) and for
# 44 of them (300); T = 2 keeps every workgroup on the single-tile shortcut
UNEVEN = ((0, 1, 3, 64, 256, 257, 300), 2)
# 71 rows per env: every workgroup runs two tiles (the path that forwards twice and accumulates dW1 in its partial)
TWO_TILES = ((1, 2, 5), 70)
KEYS = ('observations', 'actions', 'rewards', 'dones')


def _agents(A, E):
    agents = []
    for a in range(A):
        torch.manual_seed(20 + a)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
    return agents


def _kw(A, use_gae, value_loss):
    shared = dict(value_loss=value_loss, use_gae=use_gae, max_grad_norm=0.5)
    pop = dict(lr=LR[:A], gamma=GAMMA[:A], entropy_coef=ENTROPY[:A], gae_lambda=LAMBDA[:A] if use_gae else None, **shared)
    single = [dict(lr=LR[a], gamma=GAMMA[a], entropy_coef=ENTROPY[a], gae_lambda=LAMBDA[a] if use_gae else None, **shared)
              for a in range(A)]
    return pop, single


_WINDOWS = {}


def _window(E, R, T):
    """(state (R, E), out) of a synthetic window, made once per shape and never modified: crops of zeros and ones, actions
    in 0..3, rewards in {-1, 0, 1}, random dones"""
    key = (E, R, T)
    if key not in _WINDOWS:
        g = torch.Generator().manual_seed(7 * E + 3 * R + T)
        out = dict(observations=(torch.rand((T, R, E), generator=g) < 0.3).float().to(DEV),
                   actions=torch.randint(4, (T, R), generator=g).to(DEV),
                   rewards=torch.randint(-1, 2, (T, R), generator=g).float().to(DEV),
                   dones=(torch.rand((T, R), generator=g) < 0.15).to(DEV))
        _WINDOWS[key] = ((torch.rand((R, E), generator=g) < 0.3).float().to(DEV), out)
    return _WINDOWS[key]


def _plan(lineup, A):
    K, N = lineup.shape
    return league_plan(types.SimpleNamespace(num_snakes=K, num_envs=N), lineup.to(DEV), A)


def _interleaved(counts, seed=0):
    """a (1, sum counts) line-up in which policy a plays counts[a] rows, scattered: `order` is a real permutation"""
    who = torch.cat([torch.full((m,), a, dtype=torch.long) for a, m in enumerate(counts)])
    lineup = who[torch.randperm(len(who), generator=torch.Generator().manual_seed(seed))].view(1, -1)
    plan = _plan(lineup, len(counts))
    assert plan.offsets.diff().tolist() == list(counts)
    assert not torch.equal(plan.order.cpu(), torch.arange(len(who), dtype=torch.int32))
    return plan


def _lists(plan):
    offsets = plan.offsets.tolist()
    return [plan.order[offsets[a]:offsets[a + 1]].long() for a in range(plan.num_policies)]


def _expected(pop, kw_single, state, out, plan, learn=None, call='update'):
    """per member, from a stand-alone learner that starts where the population stands (weights, Adam state, the shared
    step): the results of `call` and the state after it; None for a member that does not learn"""
    refs = []
    for a, idx in enumerate(_lists(plan)):
        if len(idx) == 0 or (learn is not None and not learn[a]):
            refs.append(None)
            continue
        single = FusedA2CLearner(_agents(1, pop.num_inputs)[0], **kw_single[a])  # (its weights are loaded below)
        single.load_state_dict({'params': pop.params[a], 'exp_avg': pop.exp_avg[a], 'exp_avg_sq': pop.exp_avg_sq[a],
                                'step': pop.step})
        x, o = state.index_select(0, idx), {k: out[k].index_select(1, idx) for k in KEYS}
        if call == 'update':
            res = single.update(x, o)
        else:
            g, res = single.grad(x, o)
            res['grad'] = g
        refs.append(dict(res, params=single.params, exp_avg=single.exp_avg, exp_avg_sq=single.exp_avg_sq))
    return refs


def _compare(res, pop, before, refs, plan, what):
    """`res` and the population's state against `refs`; `before`: the three state buffers before the call"""
    state_keys = ('params', 'exp_avg', 'exp_avg_sq')
    scalars = ('value_loss', 'policy_loss', 'entropy') + (('grad_norm',) if 'grad_norm' in res else ())
    columns = ('values',) + (('returns',) if 'returns' in res else ())
    for a, (want, idx) in enumerate(zip(refs, _lists(plan))):
        if want is None:  # sat out: untouched state, zeros for everything it would have written
            for k, old in zip(state_keys, before):
                assert torch.equal(getattr(pop, k)[a], old[a]), (what, a, k)
            assert not res['grad'][a].any(), (what, a, 'grad')
            for k in scalars:
                assert float(res[k][a]) == 0.0, (what, a, k)
            for k in columns:
                assert not res[k][:, idx].any(), (what, a, k)
            continue
        assert torch.equal(res['grad'][a], want['grad']), (what, a, 'grad')
        for k in scalars:
            assert torch.equal(res[k][a], want[k]), (what, a, k)
        for k in columns:
            assert torch.equal(res[k][:, idx], want[k]), (what, a, k)
        if 'grad_norm' in res:
            for k in state_keys:
                assert torch.equal(getattr(pop, k)[a], want[k]), (what, a, k)


def _snapshot(pop):
    return pop.params.clone(), pop.exp_avg.clone(), pop.exp_avg_sq.clone()


def _update_and_compare(pop, kw_single, state, out, plan, learn=None, what=''):
    refs = _expected(pop, kw_single, state, out, plan, None if learn is None else learn.tolist())
    before, step = _snapshot(pop), pop.step
    res = pop.update(state, out, plan=plan, learn=learn)
    A, (T, R) = pop.num_members, out['rewards'].shape
    assert pop.step == step + 1 and res['grad'].shape == pop.params.shape and res['grad_norm'].shape == (A,)
    assert res['value_loss'].shape == (A,) and res['values'].shape == (T, R)
    _compare(res, pop, before, refs, plan, what)
    return res


# ------------------------------------------------------------------------------------------------ 1: uneven lists

@pytest.mark.parametrize('use_gae,value_loss', [(False, 'smooth_l1'), (False, 'mse'), (True, 'smooth_l1'), (True, 'mse')])
@pytest.mark.parametrize('counts,T', [UNEVEN, TWO_TILES])
@pytest.mark.parametrize('E', [27, 75])
def test_members_equal_stand_alone_learners_on_their_columns(E, counts, T, use_gae, value_loss):
    A, R = len(counts), sum(counts)
    state, out = _window(E, R, T)
    plan = _interleaved(counts)
    agents = _agents(A, E)
    kw_pop, kw_single = _kw(A, use_gae, value_loss)
    pop = FusedA2CPopulation(agents, **kw_pop)
    # grad alone first (the weights stay), then two updates: the second from a state that is not the initial one
    refs = _expected(pop, kw_single, state, out, plan, call='grad')
    grad, losses = pop.grad(state, out, plan=plan)
    assert ('returns' in losses) == use_gae
    _compare(dict(losses, grad=grad), pop, _snapshot(pop), refs, plan, 'grad')
    for i in range(2):
        _update_and_compare(pop, kw_single, state, out, plan, what=('update', i))
    assert pop.step == 2


# ------------------------------------------------------------------------------------------------ 2: the block line-up

@pytest.mark.parametrize('use_gae', [False, True])
@pytest.mark.parametrize('K,N,P', [(4, 3, 2), (4, 257, 4)])
def test_block_lineup_is_the_population_update(K, N, P, use_gae):
    E, T = 27, 5
    state, out = _window(E, K * N, T)
    plan = _plan(block_lineup(K, N, P), P)
    kw = _kw(P, use_gae, 'smooth_l1')[0]
    one, two = FusedA2CPopulation(_agents(P, E), **kw), FusedA2CPopulation(_agents(P, E), **kw)
    for i in range(2):
        a, b = one.update(state, out), two.update(state, out, plan=plan)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)
        for k in ('params', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(getattr(one, k), getattr(two, k)), (i, k)


# ------------------------------------------------------------------------------------------------ 3: independence

@pytest.mark.parametrize('use_gae', [False, True])
def test_a_member_does_not_depend_on_the_others(use_gae):
    E, T, A, R, me = 27, 5, 4, 90, 2
    state, out = _window(E, R, T)
    g = torch.Generator().manual_seed(3)
    lineup = torch.randint(A, (3, R // 3), generator=g)
    # who plays the OTHER rows changes (another draw among the other policies, so their lists and counts change too)
    others = torch.tensor([a for a in range(A) if a != me])
    lineup2 = torch.where(lineup == me, lineup, others[torch.randint(A - 1, lineup.shape, generator=g)])
    plans = _plan(lineup, A), _plan(lineup2, A)
    assert torch.equal(_lists(plans[0])[me], _lists(plans[1])[me]) and not torch.equal(plans[0].order, plans[1].order)
    kw = _kw(A, use_gae, 'smooth_l1')[0]
    pops = [FusedA2CPopulation(_agents(A, E), **kw) for _ in plans]
    with torch.no_grad():  # and the other members' weights
        for a in range(A):
            if a != me:
                pops[1].params[a].mul_(1.5).add_(0.01)
    idx = _lists(plans[0])[me]
    res = [pop.update(state, out, plan=plan) for pop, plan in zip(pops, plans)]
    for k in ('grad', 'value_loss', 'policy_loss', 'entropy', 'grad_norm'):
        assert torch.equal(res[0][k][me], res[1][k][me]), k
    for k in ('values',) + (('returns',) if use_gae else ()):
        assert torch.equal(res[0][k][:, idx], res[1][k][:, idx]), k
    for k in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(pops[0], k)[me], getattr(pops[1], k)[me]), k
    assert not torch.equal(res[0]['grad'][0], res[1]['grad'][0])


# ------------------------------------------------------------------------------------------------ 4: learn and empty members

@pytest.mark.parametrize('use_gae', [False, True])
def test_masked_and_empty_members_keep_their_state(use_gae):
    counts, T = UNEVEN
    E, A, R = 27, len(counts), sum(counts)
    state, out = _window(E, R, T)
    plan = _interleaved(counts, seed=1)
    agents = _agents(A, E)
    kw_pop, kw_single = _kw(A, use_gae, 'smooth_l1')
    pop = FusedA2CPopulation(agents, **kw_pop)
    # two consecutive updates with different masks (bool, then uint8): a member that sat the first one out makes its
    # first Adam step at the shared step 2, as the stand-alone learner that is handed step = 1 does
    masks = (torch.tensor([1, 1, 0, 1, 0, 1, 1], dtype=torch.bool, device=DEV),
             torch.tensor([1, 0, 1, 1, 1, 1, 0], dtype=torch.uint8, device=DEV))
    for i, learn in enumerate(masks):
        _update_and_compare(pop, kw_single, state, out, plan, learn=learn, what=('masked', i))
    assert pop.step == 2
    # grad / apply take the same mask: the pair is the update
    other = FusedA2CPopulation(_agents(A, E), **kw_pop)
    for learn in masks:
        grad, _ = other.grad(state, out, plan=plan, learn=learn)
        other.apply(grad, plan=plan, learn=learn)
    for k in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(pop, k), getattr(other, k)), k


# ------------------------------------------------------------------------------------------------ 5, 6: bits and launches

@pytest.mark.parametrize('use_gae', [False, True])
def test_same_bits_from_run_to_run_and_launch_counts(use_gae):
    counts, T = UNEVEN
    E, A, R = 27, len(counts), sum(counts)
    state, out = _window(E, R, T)
    plan = _interleaved(counts, seed=2)
    kw = _kw(A, use_gae, 'smooth_l1')[0]
    one, two = FusedA2CPopulation(_agents(A, E), **kw), FusedA2CPopulation(_agents(A, E), **kw)
    count = _lib.lib().wurm_launch_count
    before = count()
    g1, l1 = one.grad(state, out, plan=plan)
    assert count() - before == 2
    g2, l2 = one.grad(state, out, plan=plan)
    assert torch.equal(g1, g2) and all(torch.equal(l1[k], l2[k]) for k in l1)
    before = count()
    r1 = one.update(state, out, plan=plan)
    assert count() - before == 3
    r2 = two.update(state, out, plan=plan)
    assert all(torch.equal(r1[k], r2[k]) for k in r1) and torch.equal(r1['grad'], g1)
    assert torch.equal(one.params, two.params) and torch.equal(one.exp_avg_sq, two.exp_avg_sq)
    before = count()
    one.apply(g1, plan=plan)
    assert count() - before == 1


# ------------------------------------------------------------------------------------------------ 7: float64

@pytest.mark.parametrize('use_gae', [False, True])
def test_gradient_against_the_float64_specification(use_gae):
    """every member's gradient, losses and values against the float64 specification of its gathered columns, under the
    bound of the stand-alone learner's test (tests/test_a2c_learner_gpu.py: assert_within_bound).  The members share the
    fixture's weights: its rows were drawn to keep those weights' kinks at a distance."""
    E, T, counts, entropy, lam = 27, 5, (1, 9, 55), 0.01, 0.95  # (27, 5, 65: a fixture of that test's GRAD_CASES)
    fx = ref.make_fixture(E, T, sum(counts), seed=0, reward_scale=3.0)
    plan = _interleaved(counts, seed=4)
    made = [ref.to_device(fx, DEV) for _ in counts]
    _, state, out = made[0]
    pop = FusedA2CPopulation([m[0] for m in made], gamma=fx['gamma'], entropy_coef=entropy, use_gae=use_gae,
                             gae_lambda=lam if use_gae else None)
    grad, losses = pop.grad(state, out, plan=plan)
    for a, idx in enumerate(_lists(plan)):
        i = idx.cpu()
        sub = dict(fx, N=len(i), obs0=fx['obs0'][i].contiguous(), obs=fx['obs'][:, i].contiguous(),
                   **{k: fx[k][:, i].contiguous() for k in ('actions', 'rewards', 'dones')})
        if use_gae:
            spec = gae.spec_float64_gae(sub, lam, entropy, 'smooth_l1')
            t32 = gae.example_loss_gae(sub, torch.float32, DEV, lam, entropy, 'smooth_l1')
        else:
            spec = ref.spec_float64(sub, entropy, 'smooth_l1')
            t32 = ref.example_loss(sub, torch.float32, DEV, entropy, 'smooth_l1')
        mine = {k: losses[k][a] for k in ('value_loss', 'policy_loss', 'entropy')}
        mine['values'] = losses['values'][:, idx]
        assert_within_bound(sub, grad[a], mine, spec, t32, f'league member {a}')


# ------------------------------------------------------------------------------------------------ 8: a real window

@pytest.mark.parametrize('use_gae', [False, True])
def test_league_window_then_update(use_gae):
    """MultiSnake 8 x 3 snakes, four policies, a random line-up: the columns are k N + i and the start observations the dict
    `reset` returns"""
    from wurm_amd.envs import MultiSnake
    K, N, A, T, E = 3, 8, 4, 5, 27
    env = MultiSnake(num_envs=N, num_snakes=K, size=12, observation_mode='partial_1', device=DEV, boost=False, seed=11)
    lineup = torch.randint(A, (K, N), generator=torch.Generator().manual_seed(5)).to(DEV)
    plan = env.league_plan(lineup, A)
    agents = _agents(A, E)
    kw_pop, kw_single = _kw(A, use_gae, 'smooth_l1')
    pop = FusedA2CPopulation(agents, **kw_pop)
    state = env.reset()
    for i in range(2):
        out = env.league_window(pop.params, state, T, plan)
        assert out['rewards'].shape == (T, K * N)
        # row k N + i of the stacked start observations is snake k of env i, the row the line-up's entry [k, i] plays
        rows = torch.stack([state[f'agent_{k}'].reshape(N, E) for k in range(K)]).reshape(K * N, E)
        refs = _expected(pop, kw_single, rows, out, plan)
        before = _snapshot(pop)
        res = pop.update(state, out, plan=plan)
        _compare(res, pop, before, refs, plan, ('window', i))
        for a in range(A):  # the lists are the line-up's: policy a learns from exactly the rows it played
            assert torch.equal(_lists(plan)[a], (lineup.reshape(-1) == a).nonzero().squeeze(1))
        state = out['state']
