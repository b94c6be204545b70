"""The exploit / explore step of population-based training on the GPU (include/wurm_hip.h: wurm_a2c_ff_pop_exploit;
`FusedA2CPopulation.exploit`) against its restatement tests/a2c_pbt_ref.py.  Every comparison is exact: the step copies
rows, counts ranks in integers and does two double multiplications per replaced member."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import a2c_pbt_ref as ref
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params
from wurm_amd.rl import FusedA2CPopulation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF, NAN = math.inf, math.nan
ROWS = ('params', 'exp_avg', 'exp_avg_sq')


def num_params(E):
    return 64 * E + 4549


def _state(P, E, seed):
    """device tensors: three (P, num_params) buffers of distinct random values and a hyper table with distinct rows"""
    g = torch.Generator().manual_seed(seed)
    s = {name: torch.randn((P, num_params(E)), generator=g).to(DEV) for name in ROWS}
    p = torch.arange(P, dtype=torch.float64)
    f32 = lambda x: x.float().double()  # columns 1-3 hold floats
    s['hyper'] = torch.stack([1e-3 * (1 + p), f32(0.9 + 0.0003 * p), f32(0.01 + 0.002 * p), f32(0.8 + 0.0005 * p)],
                             dim=1).contiguous().to(DEV)
    return s


def _raw_exploit(s, scores, k, perturb=ref.DEFAULT_PERTURB, seed=0, generation=0):
    """the C ABI on the device tensors of `s` (modified in place) -> (order, parent)"""
    P, n = s['params'].shape
    order = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    table = (ctypes.c_double * 8)(*perturb)
    rc = _lib.call(0, _lib.lib().wurm_a2c_ff_pop_exploit, _lib.ptr(s['params']), _lib.ptr(s['exp_avg']),
                   _lib.ptr(s['exp_avg_sq']), _lib.ptr(s['hyper']), _lib.ptr(scores), _lib.ptr(order), _lib.ptr(parent),
                   _lib.i64(n), _lib.i64(P), _lib.i64(k), ctypes.addressof(table), _lib.u64(seed), _lib.i64(generation),
                   _lib.stream_ptr(0))
    assert rc == _lib.OK
    return order, parent


def _numpy(s):
    return {k: v.cpu().numpy() for k, v in s.items()}


def _expected(before, scores, k, perturb=ref.DEFAULT_PERTURB, seed=0, generation=0):
    return ref.exploit(before['params'], before['exp_avg'], before['exp_avg_sq'], before['hyper'], scores, k, perturb, seed,
                       generation)


def _assert_equal(s, order, parent, exp, what):
    assert np.array_equal(order.cpu().numpy(), exp['order']), (what, 'order')
    assert np.array_equal(parent.cpu().numpy(), exp['parent']), (what, 'parent')
    for name in ROWS:
        assert np.array_equal(s[name].cpu().numpy().view(np.uint32), exp[name].view(np.uint32)), (what, name)
    assert np.array_equal(s['hyper'].cpu().numpy().view(np.uint64), exp['hyper'].view(np.uint64)), (what, 'hyper')


def _tie_blocks(P, k, rng):
    """blocks of equal scores around rank k and around rank P - k (merged where they meet), distinct elsewhere, handed
    to the members in a random order"""
    blocks = [range(max(k - 2, 0), min(k + 2, P)), range(max(P - k - 2, 0), min(P - k + 2, P))]
    value = np.zeros(P)
    for r in range(1, P):
        value[r] = value[r - 1] if any(r in b and r - 1 in b for b in blocks) else -float(r)
    scores = np.empty(P)
    scores[rng.permutation(P)] = value
    return scores


def _special(P, rng):
    """NaN and the two infinities among ordinary scores; the last member is a NaN, which ranks last: inside the bottom k
    for every k >= 1"""
    scores = rng.standard_normal(P)
    scores[P - 1] = NAN
    if P >= 3:
        scores[0] = -INF
    if P >= 5:
        scores[1], scores[2], scores[3] = INF, INF, NAN
    if P >= 64:
        scores[rng.permutation(P - 1)[:P // 4]] = rng.choice([NAN, INF, -INF], size=P // 4)
    return scores


def score_vectors(P, k, rng):
    return {'distinct': rng.permutation(P) * 0.37 - 3.0, 'equal': np.full(P, 0.25), 'ties': _tie_blocks(P, k, rng),
            'special': _special(P, rng), 'all_nan': np.full(P, NAN)}


@pytest.mark.parametrize('E', [3, 4])
@pytest.mark.parametrize('P', [2, 3, 5, 64, 65, 300])
def test_exploit_equals_reference(P, E):
    """k in {0, 1, P // 2} x five kinds of scores, three generations chained each (the result of one is the input of the
    next), generation and seed varied.  num_params = 4741 / 4805: four full slices of 1024 and a ragged tail, odd rows."""
    rng = np.random.default_rng(100 * P + E)
    for k in (0, 1, P // 2):
        for kind, scores in score_vectors(P, k, rng).items():
            s = _state(P, E, seed=P + E + k)
            for generation, seed in ((0, 0), (1, 0), (5, (9 << 40) + 77)):
                what = (k, kind, generation)
                before = _numpy(s)
                dev_scores = torch.from_numpy(scores).to(DEV)
                order, parent = _raw_exploit(s, dev_scores, k, seed=seed, generation=generation)
                exp = _expected(before, scores, k, seed=seed, generation=generation)
                _assert_equal(s, order, parent, exp, what)
                assert np.array_equal(dev_scores.cpu().numpy().view(np.uint64), scores.view(np.uint64)), (what, 'scores')
                if kind in ('equal', 'all_nan'):
                    assert order.cpu().tolist() == list(range(P)), what
                if kind == 'special' and k >= 1 and generation == 0:  # (before the scores are rolled)
                    assert np.isnan(scores[P - 1]) and exp['parent'][P - 1] != P - 1, what  # a NaN in the bottom k
                scores = np.roll(scores, 1 + P // 3)  # other members are worst next time


def test_untouched_means_untouched():
    P, E, k = 65, 3, 20
    s = _state(P, E, seed=1)
    scores = torch.from_numpy(np.random.default_rng(1).standard_normal(P)).to(DEV)
    before, scores_before = {name: t.clone() for name, t in s.items()}, scores.clone()
    order, parent = _raw_exploit(s, scores, k, seed=4, generation=2)
    kept = (parent == torch.arange(P, dtype=torch.int32, device=DEV))
    assert int(kept.sum()) == P - k
    for name in ROWS + ('hyper',):
        assert torch.equal(s[name][kept], before[name][kept]), name
        assert not torch.equal(s[name][~kept], before[name][~kept]), name
    assert torch.equal(scores.view(torch.int64), scores_before.view(torch.int64))
    assert sorted(order.cpu().tolist()) == list(range(P))
    # every replaced member has the rows of its parent, which kept its own
    assert bool(kept[parent[~kept].long()].all())
    for name in ROWS:
        assert torch.equal(s[name][~kept], before[name][parent[~kept].long()]), name


def test_bounds_act():
    P, E, k = 64, 3, 32
    scores = np.random.default_rng(2).standard_normal(P)
    perturb = (0.5, 2.0, 20e-3, 30e-3, 1.0, 1.0, 0.0, INF)  # lr in [1e-3, 64e-3] x {0.5, 2}: both clamps within reach
    s = _state(P, E, seed=2)
    before = _numpy(s)
    order, parent = _raw_exploit(s, torch.from_numpy(scores).to(DEV), k, perturb, seed=8, generation=1)
    exp = _expected(before, scores, k, perturb, seed=8, generation=1)
    assert exp['hit'] == {'lo', 'hi'}, 'the reference hits both clamps'
    _assert_equal(s, order, parent, exp, 'bounds')
    hyper, replaced = s['hyper'].cpu().numpy(), exp['parent'] != np.arange(P)
    assert replaced.sum() == k
    assert (hyper[replaced, 0] >= 20e-3).all() and (hyper[replaced, 0] <= 30e-3).all()
    assert (hyper[replaced, 0] == 20e-3).any() and (hyper[replaced, 0] == 30e-3).any()
    # entropy_factors = (1, 1): column 2 is a bit-exact copy of the parent's
    assert np.array_equal(hyper[:, 2].view(np.uint64), before['hyper'][exp['parent'], 2].view(np.uint64))
    # and entropy bounds that act, rounded to float: 0.0123 is no float
    s = _state(P, E, seed=2)
    perturb = (0.8, 1.2, 0.0, INF, 0.8, 1.2, 0.0123, 0.0123)
    order, parent = _raw_exploit(s, torch.from_numpy(scores).to(DEV), k, perturb, seed=8, generation=1)
    _assert_equal(s, order, parent, _expected(before, scores, k, perturb, seed=8, generation=1), 'entropy bounds')
    assert (s['hyper'].cpu().numpy()[replaced, 2] == float(np.float32(0.0123))).all()


@pytest.mark.parametrize('k', [0, 1, 2])
def test_two_launches_and_repeatable(k):
    P, E = 5, 4
    scores = torch.tensor([0.5, NAN, 2.0, 0.5, -1.0], dtype=torch.float64, device=DEV)
    one, two = _state(P, E, seed=3), _state(P, E, seed=3)
    before = _lib.lib().wurm_launch_count()
    first = _raw_exploit(one, scores, k, seed=5, generation=3)
    assert _lib.lib().wurm_launch_count() - before == 2
    second = _raw_exploit(two, scores.clone(), k, seed=5, generation=3)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for name in one:
        assert torch.equal(one[name], two[name]), name
    assert first[0].cpu().tolist() == [2, 0, 3, 4, 1]
    if k == 0:
        assert first[1].cpu().tolist() == list(range(P))


# ---------------------------------------------------------------------------------------------- through the class


def _agents(P, E, base=10):
    agents = []
    for p in range(P):
        torch.manual_seed(base + p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
    return agents


def _kwargs(P, use_gae):
    return dict(lr=[1e-3 * (1 + p) for p in range(P)], gamma=[0.99 - 0.01 * p for p in range(P)],
                entropy_coef=[0.01 * (1 + p) for p in range(P)], use_gae=use_gae,
                gae_lambda=[0.95 - 0.02 * p for p in range(P)] if use_gae else None)


def _env(P, M, E):
    from wurm_amd.envs import SingleSnake
    return SingleSnake(num_envs=P * M, size=9, observation_mode={27: 'partial_1', 75: 'partial_2'}[E], device=DEV, seed=7)


def _train(pop, env, state, T, windows):
    for _ in range(windows):
        out = env.policy_rollout(pop.params, state, T, population=pop.num_members)
        pop.update(state, out)
        state = out['state']
    return state


def _overwrite(pop, exp, step):
    for name in ROWS + ('hyper',):
        getattr(pop, name).copy_(torch.from_numpy(exp[name]))
    pop.step = step


UPDATE_KEYS = ('grad', 'grad_norm', 'value_loss', 'policy_loss', 'entropy', 'values')


@pytest.mark.parametrize('use_gae', [False, True])
@pytest.mark.parametrize('P,M,E,T', [(4, 5, 27, 3), (6, 67, 75, 5)])
def test_training_goes_on_from_the_exploited_state(P, M, E, T, use_gae):
    env, pop = _env(P, M, E), FusedA2CPopulation(_agents(P, E), **_kwargs(P, use_gae))
    state = _train(pop, env, env.reset(), T, windows=2)
    scores = np.array([0.3, 0.9, 0.1, 0.7, 0.2, 0.8][:P])  # not sorted by member
    before = {name: getattr(pop, name).cpu().numpy() for name in ROWS + ('hyper',)}
    chosen = pop.exploit(torch.from_numpy(scores).to(DEV), num_replace=P // 2, seed=3)
    assert pop.generation == 1 and pop.step == 2
    exp = _expected(before, scores, P // 2, seed=3, generation=0)
    assert (exp['parent'] != np.arange(P)).sum() == P // 2
    assert np.array_equal(chosen['parent'].cpu().numpy(), exp['parent'])
    assert chosen['order'].dtype == torch.int32 and chosen['parent'].dtype == torch.int32 and chosen['order'].is_cuda
    # the modules follow: views of the rows, a replaced member's module equals its parent's
    for p, agent in enumerate(pop.agents):
        assert torch.equal(pack_policy_params(agent), pop.params[p]), p
        mine, parents = agent.state_dict(), pop.agents[int(exp['parent'][p])].state_dict()
        assert all(torch.equal(mine[k], parents[k]) for k in mine), p
    # a twin that is GIVEN what the reference says the exploit leaves
    twin = FusedA2CPopulation(_agents(P, E, base=50), **_kwargs(P, use_gae))
    _overwrite(twin, exp, step=2)
    out = env.policy_rollout(pop.params, state, T, population=P)
    got, want = pop.update(state, out), twin.update(state, out)
    for key in UPDATE_KEYS + (('returns',) if use_gae else ()):
        assert torch.equal(got[key], want[key]), key
    for name in ROWS:
        assert torch.equal(getattr(pop, name), getattr(twin, name)), name
    assert not torch.equal(pop.params[0], pop.params[1])


def test_exploit_takes_float32_scores_and_counts_generations():
    P, E = 4, 27
    pop = FusedA2CPopulation(_agents(P, E), **_kwargs(P, False))
    pop.exp_avg.normal_()
    pop.exp_avg_sq.uniform_()
    scores = np.array([0.3, NAN, 0.1, 0.7], dtype=np.float32)
    for generation in range(2):
        before = {name: getattr(pop, name).cpu().numpy() for name in ROWS + ('hyper',)}
        count = _lib.lib().wurm_launch_count()
        chosen = pop.exploit(torch.from_numpy(scores).to(DEV), seed=11)  # fraction 0.25: k = 1
        assert _lib.lib().wurm_launch_count() - count == 2 and pop.generation == generation + 1
        exp = _expected(before, scores.astype(np.float64), 1, seed=11, generation=generation)
        _assert_equal({name: getattr(pop, name) for name in ROWS + ('hyper',)}, chosen['order'], chosen['parent'], exp,
                      generation)
        worst = int(np.flatnonzero(np.isnan(scores))[0])
        assert exp['parent'][worst] != worst and (exp['parent'] != np.arange(P)).sum() == 1
        scores = np.roll(scores, 1)
    count = _lib.lib().wurm_launch_count()
    chosen = pop.exploit(torch.from_numpy(scores).to(DEV), num_replace=0)
    assert _lib.lib().wurm_launch_count() - count == 2 and chosen['parent'].cpu().tolist() == list(range(P))


def test_state_dict_after_an_exploit():
    P, M, E, T = 4, 5, 27, 3
    env, pop = _env(P, M, E), FusedA2CPopulation(_agents(P, E), **_kwargs(P, True))
    state = _train(pop, env, env.reset(), T, windows=2)
    pop.exploit(torch.tensor([0.3, 0.9, 0.1, 0.7], device=DEV), num_replace=2, seed=1)
    saved = pop.state_dict()
    fresh = FusedA2CPopulation(_agents(P, E, base=70), **_kwargs(P, True))
    fresh.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in saved.items()})  # as from a file
    assert not fresh._moved() and fresh.step == 2 and fresh.generation == 1
    assert fresh.hyperparameters() == pop.hyperparameters()
    assert fresh.hyperparameters()['lr'] != _kwargs(P, True)['lr']
    out = env.policy_rollout(pop.params, state, T, population=P)
    got, want = fresh.update(state, out), pop.update(state, out)
    for key in UPDATE_KEYS + ('returns',):
        assert torch.equal(got[key], want[key]), key
    for name in ROWS:
        assert torch.equal(getattr(fresh, name), getattr(pop, name)), name
    # and the next exploit draws the same
    scores = torch.tensor([0.5, 0.1, 0.9, 0.2], device=DEV)
    a, b = fresh.exploit(scores, num_replace=1, seed=1), pop.exploit(scores, num_replace=1, seed=1)
    assert torch.equal(a['parent'], b['parent']) and torch.equal(fresh.hyper, pop.hyper)


def test_pbt_example_runs():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import a2c_pbt
    lrs = (1e-4, 3e-4, 1e-3, 3e-3)
    hist = a2c_pbt.run(num_envs=64, size=9, observation='partial_2', steps=60, update_steps=5, lrs=lrs, pbt_interval=2,
                       pbt_fraction=0.25, log_interval=30, verbose=False)
    assert len(hist) == 4
    for p, rows in enumerate(hist):
        assert len(rows) == 2 and rows[-1]['step'] == 60
        for row in rows:
            assert row['member'] == p and all(math.isfinite(v) for v in row.values())
            assert row['lr'] > 0 and row['entropy_coef'] > 0 and 0 <= row['reward_rate'] <= 1
    assert any(rows[-1]['lr'] != lrs[p] for p, rows in enumerate(hist))
    assert sum(rows[-1]['replaced'] for rows in hist) == 6  # six exploits of one member each
