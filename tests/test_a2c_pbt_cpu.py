"""Population-based training without a GPU: the reference restatement (tests/a2c_pbt_ref.py) against Philox's known answers
and against the properties an exploit step must have, the refusals of wurm_a2c_ff_pop_exploit and of
`FusedA2CPopulation.exploit`, and the `state_dict` round trip of both fused learners on CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import a2c_pbt_ref as ref
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params
from wurm_amd.rl import FusedA2CLearner, FusedA2CPopulation

I64, U64 = ctypes.c_int64, ctypes.c_uint64
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
INF, NAN = math.inf, math.nan


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    assert ref.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    ones = 0xffffffff
    assert ref.philox4x32_10((ones,) * 4, (ones, ones)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    # the counter layout of rng_words: (env_id, call_lo, call_hi, purpose | sub << 8), key = (seed_lo, seed_hi)
    assert ref.rng_words((7 << 32) | 5, (3 << 32) | 2, 11, 9, 1) == ref.philox4x32_10((11, 2, 3, 9 | 256), (5, 7))
    assert ref.mulhi(0xffffffff, 5) == 4 and ref.mulhi(0, 5) == 0 and ref.mulhi(0x80000000, 3) == 1


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)  # a non-null pointer: every call below is refused before anything is read or launched

    def call(params=p, m=p, v=p, hyper=p, scores=p, order=p, parent=p, n=4741, members=4, k=1, perturb=ref.DEFAULT_PERTURB,
             generation=0):
        table = (ctypes.c_double * 8)(*perturb) if perturb is not None else None
        return lib.wurm_a2c_ff_pop_exploit(params, m, v, hyper, scores, order, parent, I64(n), I64(members), I64(k),
                                           ctypes.addressof(table) if table is not None else None, U64(0),
                                           I64(generation), None)

    for name in ('params', 'm', 'v', 'hyper', 'scores', 'order', 'parent', 'perturb'):
        assert call(**{name: None}) == INV, name
    assert call(n=0) == INV and call(n=-3) == INV and call(members=0) == INV and call(members=-4) == INV
    assert call(k=-1) == INV and call(k=3) == INV and call(members=5, k=3) == INV and call(members=1, k=1) == INV
    assert call(generation=-1) == INV
    good = list(ref.DEFAULT_PERTURB)
    for i in (0, 1, 4, 5):  # the factors: finite and > 0
        for bad in (0.0, -0.5, INF, -INF, NAN):
            assert call(perturb=good[:i] + [bad] + good[i + 1:]) == INV, (i, bad)
    for lo in (2, 6):       # the bound pairs: 0 <= lo <= hi, no NaN
        for pair in ((2.0, 1.0), (-1.0, 1.0), (NAN, 1.0), (0.0, NAN), (INF, 1.0), (0.0, -INF)):
            assert call(perturb=good[:lo] + list(pair) + good[lo + 2:]) == INV, (lo, pair)
    assert call(members=65536, k=0) == UNS and call(members=65536, k=100) == UNS
    assert call(members=65536, k=40000) == INV  # 2 k > P comes first


def _agents(P, E=4):
    agents = []
    for p in range(P):
        torch.manual_seed(20 + p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E))
    return agents


def test_exploit_refusals():
    pop = FusedA2CPopulation(_agents(5))
    for k in (3, 5, -1):
        with pytest.raises(ValueError):
            pop.exploit(torch.zeros(5, dtype=torch.float64), num_replace=k)
    with pytest.raises(ValueError):
        pop.exploit(torch.zeros(5, dtype=torch.float64), fraction=0.75)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros((5, 1), dtype=torch.float64),
                torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(RuntimeError):
            pop.exploit(bad, num_replace=1)
    with pytest.raises(_lib.WurmHipError):  # a CPU population, like `grad`
        pop.exploit(torch.zeros(5, dtype=torch.float64), num_replace=1)
    assert pop.generation == 0


def _scramble(learner, seed):
    g = torch.Generator().manual_seed(seed)
    learner.exp_avg.copy_(torch.randn(learner.params.shape, generator=g))
    learner.exp_avg_sq.copy_(torch.rand(learner.params.shape, generator=g))
    learner.step = 7


def _agents_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_state_dict_round_trip_learner():
    one = FusedA2CLearner(_agents(1)[0], lr=3e-4)
    _scramble(one, 1)
    state = one.state_dict()
    assert set(state) == {'params', 'exp_avg', 'exp_avg_sq', 'step'}
    assert state['params'].data_ptr() != one.params.data_ptr()  # clones
    torch.manual_seed(99)
    twin_agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=4)
    twin = FusedA2CLearner(twin_agent, lr=3e-4)
    assert not torch.equal(twin.params, one.params)
    twin.load_state_dict(state)
    for name in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(twin, name), getattr(one, name)), name
    assert twin.step == 7 and not twin._moved()
    assert _agents_equal(twin_agent, one.agent)
    assert torch.equal(pack_policy_params(twin_agent), one.params)


def test_state_dict_round_trip_population():
    P = 3
    one = FusedA2CPopulation(_agents(P), lr=[1e-3, 2e-3, 3e-3], entropy_coef=[0.0, 0.01, 0.02], use_gae=True,
                             gae_lambda=[0.9, 0.95, 1.0])
    _scramble(one, 2)
    one.generation = 4
    one.hyper[1, 0] = 1.2345e-3  # as after an exploit
    state = one.state_dict()
    assert set(state) == {'params', 'exp_avg', 'exp_avg_sq', 'step', 'hyper', 'generation'}
    torch.manual_seed(77)
    twin_agents = [FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=4) for _ in range(P)]
    twin = FusedA2CPopulation(twin_agents, use_gae=True, gae_lambda=0.5)
    twin.load_state_dict(state)
    for name in ('params', 'exp_avg', 'exp_avg_sq', 'hyper'):
        assert torch.equal(getattr(twin, name), getattr(one, name)), name
    assert twin.step == 7 and twin.generation == 4 and not twin._moved()
    assert all(_agents_equal(a, b) for a, b in zip(twin_agents, one.agents))
    assert twin.hyperparameters() == one.hyperparameters()
    hyper = twin.hyperparameters()
    assert hyper['lr'] == [1e-3, 1.2345e-3, 3e-3] and set(hyper) == {'lr', 'gamma', 'entropy_coef', 'gae_lambda'}
    assert np.allclose(hyper['gae_lambda'], [0.9, 0.95, 1.0], rtol=1e-6, atol=0)
    assert set(FusedA2CPopulation(_agents(2)).hyperparameters()) == {'lr', 'gamma', 'entropy_coef'}


@pytest.mark.parametrize('population', [False, True])
def test_load_state_dict_refuses_before_copying(population):
    make = (lambda E: FusedA2CPopulation(_agents(2, E))) if population else (lambda E: FusedA2CLearner(_agents(1, E)[0]))
    source, target = make(4), make(4)
    _scramble(source, 3)
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in target.state_dict().items()}

    def unchanged():
        now = target.state_dict()
        return all(torch.equal(now[k], v) if torch.is_tensor(v) else now[k] == v for k, v in before.items())

    # the LAST tensor checked is the wrong one: nothing before it may have been copied
    last = 'hyper' if population else 'exp_avg_sq'
    for bad in (torch.zeros(3), source.state_dict()[last].to(torch.float16), source.state_dict()[last][..., :-1]):
        state = source.state_dict()
        state[last] = bad
        with pytest.raises(RuntimeError):
            target.load_state_dict(state)
        assert unchanged() and not target._moved()
    with pytest.raises(RuntimeError):
        target.load_state_dict(make(27).state_dict())  # another num_inputs: params itself does not fit
    assert unchanged()
    target.load_state_dict(source.state_dict())
    assert not unchanged() and torch.equal(target.exp_avg, source.exp_avg)


def _score_vectors(P, k, rng):
    tied = np.zeros(P)
    tied[:max(1, P // 3)] = 1.0
    special = rng.standard_normal(P)
    special[rng.permutation(P)[:max(1, P // 2)]] = rng.choice([NAN, INF, -INF], size=max(1, P // 2))
    return [rng.standard_normal(P), np.full(P, 0.25), tied, special, np.full(P, NAN)]


@pytest.mark.parametrize('P', [2, 3, 5, 64, 65, 300])
def test_reference_properties(P):
    rng = np.random.default_rng(P)
    for k in (0, 1, P // 2):
        for i, scores in enumerate(_score_vectors(P, k, rng)):
            for generation, seed in ((0, 0), (3, 12345678901234567)):
                order, parent, words = ref.select(scores, k, seed, generation)
                rank = ref.ranks(scores)
                assert sorted(order.tolist()) == list(range(P)), 'order is a permutation'
                assert all(rank[order[r]] == r for r in range(P))
                key = np.where(np.isnan(scores), -INF, scores)[order]
                assert all(key[r] > key[r + 1] or (key[r] == key[r + 1] and order[r] < order[r + 1]) for r in range(P - 1))
                for p in range(P):
                    if rank[p] < P - k:
                        assert parent[p] == p and words[p] is None
                    else:
                        assert rank[parent[p]] < k and parent[p] != p
                if k == 0:
                    assert parent.tolist() == list(range(P))
                if i in (1, 4):  # all equal, all NaN: the identity
                    assert order.tolist() == list(range(P))


def test_reference_exploit_copies_and_perturbs():
    P, n, k = 6, 11, 3
    rng = np.random.default_rng(0)
    rows = [rng.standard_normal((P, n)).astype(np.float32) for _ in range(3)]
    hyper = np.stack([np.linspace(1e-3, 6e-3, P), np.full(P, 0.99), np.float32(np.linspace(0.01, 0.06, P)).astype(np.float64),
                      np.full(P, 0.94)], axis=1)
    scores = np.array([5.0, 1.0, NAN, 4.0, 3.0, 2.0])
    out = ref.exploit(*rows, hyper, scores, k, (0.5, 2.0, 2e-3, 5e-3, 1.0, 1.0, 0.0, INF), seed=1, generation=0)
    assert out['order'].tolist() == [0, 3, 4, 5, 1, 2]
    for p in (0, 3, 4):
        assert out['parent'][p] == p and np.array_equal(out['hyper'][p], hyper[p])
    for p in (5, 1, 2):
        src = out['parent'][p]
        assert src in (0, 3, 4)
        assert all(np.array_equal(out[name][p], rows[i][src]) for i, name in enumerate(('params', 'exp_avg', 'exp_avg_sq')))
        assert out['hyper'][p][0] in (min(max(hyper[src][0] * 0.5, 2e-3), 5e-3), min(max(hyper[src][0] * 2.0, 2e-3), 5e-3))
        assert out['hyper'][p][2] == hyper[src][2] and out['hyper'][p][1] == 0.99 and out['hyper'][p][3] == 0.94
