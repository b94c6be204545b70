"""The checker tests' own footing, proved without a GPU: tests/test_checker_batches_gpu.py compares the checker kernels
with the specification of tests/checker_ref.py on the batches that module builds, so here
  * the specification gives the REAL reference's verdict on every recorded state of both fixtures
    (tests/golden/checker_failing_states.npz and checker_failing_states_sizes.npz, tests/golden/make_golden_checker.py);
  * the specification and the oracle give the same mask, bit for bit, on every batch the GPU file uses;
  * the batches reach what they are meant to reach, for each checker and each of its bits: env 0, env N - 1, an env that
    is not the first wave of its workgroup, and the last group of 64 cells;
  * every needle batch fails in one env only.
"MultiSnake: non-integer food" below records a defect these tests found."""
import os

import numpy as np
import pytest

from oracle import oracle as _o
from tests import checker_ref as R
from tests.test_checker_failing_states import FX, _agrees, _multi_states, _multi_verdict, _single_states, _verdict

FX2 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'checker_failing_states_sizes.npz'))


def test_the_bits_are_the_oracles():
    assert R.SINGLE_BITS == (_o.CHK_FOOD_VALUE, _o.CHK_ONE_HEAD, _o.CHK_HAS_SNAKE, _o.CHK_HEAD_AT_END, _o.CHK_BODY_RANGE,
                             _o.CHK_MIN_LENGTH, _o.CHK_HEAD_ON_FOOD, _o.CHK_ONE_FOOD)
    assert (R.OVERLAP, R.DEAD_NONZERO) == (0x100, 0x200)


# ------------------------------------------------------------------------------------------------ the fixtures

def test_specification_gives_the_references_verdicts_on_the_first_fixture():
    names, envs = _single_states()
    for name, e, snake_msg, env_msg in zip(names, envs, FX['single_snake_msg'], FX['single_env_msg']):
        mask = R.spec_single_mask(e[0])
        _agrees(_verdict(mask, one_food=False), str(snake_msg), f'snake_consistency {name}')
        _agrees(_verdict(mask, one_food=True), str(env_msg), f'env_consistency {name}')
        assert mask == int(_o.single_check(np.ascontiguousarray(e))[0]), name
    for S in (9, 12):
        mask = 0
        for n, e in zip(names, envs):
            if n.startswith(f'S{S}:'):
                mask |= R.spec_single_mask(e[0])
        _agrees(_verdict(mask, one_food=True), str(FX[f'single_batch_msg_S{S}']), f'batch S={S}')
    mnames, states = _multi_states()
    for name, st, msg in zip(mnames, states, FX['multi_msg']):
        mask = R.spec_multi_mask(st['foods'], st['heads'], st['bodies'], st['dones'])
        _agrees(_multi_verdict(mask), str(msg), f'check_consistency {name}')
        assert mask == int(_o.multi_check(st)[0]), name


@pytest.mark.parametrize('S', [int(s) for s in FX2['single_sizes']])
def test_specification_gives_the_references_verdicts_at_every_single_size(S):
    envs, seen = FX2[f'single_S{S}_envs'], 0
    assert envs.shape[1:] == (3, S, S)
    for name, e, snake_msg, env_msg in zip(FX2[f'single_S{S}_names'], envs, FX2[f'single_S{S}_snake_msg'], FX2[f'single_S{S}_env_msg']):
        mask = R.spec_single_mask(e)
        _agrees(_verdict(mask, one_food=False), str(snake_msg), f'snake_consistency S{S}:{name}')
        _agrees(_verdict(mask, one_food=True), str(env_msg), f'env_consistency S{S}:{name}')
        assert mask == int(_o.single_check(np.ascontiguousarray(e[None]))[0]), (S, name)
        seen |= mask
    assert seen == 0xff                                          # every check fails somewhere at this size
    _agrees(_verdict(seen, one_food=True), str(FX2[f'single_S{S}_batch_msg']), f'batch S={S}')


def fixture_multi_states(K, S):
    key = f'multi_K{K}_S{S}'
    for i, name in enumerate(FX2[key + '_names']):
        st = _o.multi_empty_state(1, K, S)
        for k in ('foods', 'heads', 'bodies', 'dones'):
            st[k][...] = FX2[f'{key}_{k}'][i].reshape(st[k].shape)
        yield str(name), st, str(FX2[key + '_msg'][i])


@pytest.mark.parametrize('K,S', [tuple(int(v) for v in ks) for ks in FX2['multi_shapes']])
def test_specification_gives_the_references_verdicts_at_every_multi_shape(K, S):
    """MultiSnake: non-integer food.  The reference checks `living_envs.round()` (multi_snake.py:742): a food value of 0.5
    is a 0 to it and 0.6 a 1, under a head or anywhere.  The oracle and multi_check_kernel compared the raw value with
    0 and 1 and so called both 'invalid food pixel'; they round now, and the masks agree on these states too."""
    seen = 0
    for name, st, msg in fixture_multi_states(K, S):
        mask = R.spec_multi_mask(st['foods'], st['heads'], st['bodies'], st['dones'])
        _agrees(_multi_verdict(mask), msg, f'check_consistency K{K} S{S}:{name}')
        assert mask == int(_o.multi_check(st)[0]), (K, S, name)
        seen |= mask
    assert seen == (0x37f if K > 1 else 0x27f)


# ------------------------------------------------------------------------------------------------ the batches

@pytest.mark.parametrize('S,N', R.SINGLE_CASES + R.NEEDLE_SINGLE[1:])
def test_specification_and_oracle_agree_on_every_single_batch(S, N):
    batch = R.single_case(S, N)
    spec = R.spec_single_masks(batch.state)
    assert np.array_equal(spec, _o.single_check(batch.state))
    assert not R.spec_single_masks(batch.base).any()                        # what the corruptions started from is valid
    for i, kind in enumerate(batch.kinds):
        assert (spec[i] == 0) == (kind in R.SINGLE_ACCEPTED), (i, kind, hex(spec[i]))
    assert N == 1 or set(batch.kinds) == set(R.SINGLE_KINDS)
    values = np.unique(batch.state)
    assert np.array_equal(values, np.round(values)) and set(np.unique(batch.state[:, 0])) <= {0.0, 1.0, 2.0}


@pytest.mark.parametrize('K,S,N', R.MULTI_CASES)
def test_specification_and_oracle_agree_on_every_multi_batch(K, S, N):
    batch = R.multi_case(K, S, N)
    spec = R.spec_multi_masks(batch.state)
    assert np.array_equal(spec, _o.multi_check(batch.state))
    assert not R.spec_multi_masks(batch.base).any()
    for i, kind in enumerate(batch.kinds):
        assert (spec[i] == 0) == (kind in R.MULTI_ACCEPTED), (i, kind, hex(spec[i]))
    assert N < 19 or set(batch.kinds) == set(R.multi_kind_names(K))
    assert N < 19 or {0, K - 1} == set(batch.targets)
    for k in ('foods', 'heads', 'bodies'):
        values = np.unique(batch.state[k])
        assert np.array_equal(values, np.round(values))
    assert set(np.unique(batch.state['foods'])) <= {0.0, 1.0, 2.0}
    if N >= 75:  # the four kinds of dones: alive, dead and cleared, dead and not cleared, all dead
        d = batch.state['dones'].reshape(N, K)
        cells = (batch.state['heads'] + batch.state['bodies']).reshape(N, K, -1).any(axis=2)
        assert (d == 0).any() and ((d != 0) & ~cells).any() and ((d != 0) & cells).any() and (d != 0).all(axis=1).any()


def _coverage(cases, get, spec_masks, K_of):
    """bit -> the set of places it is seen at: 'first' (env 0), 'last' (env N - 1), 'wave' (an env that is not the first
    wave of a workgroup of four) and 'tail' (the bit CHANGES when the last group of 64 cells of every plane is cleared:
    its value hangs on cells that only a tier's validity mask admits)"""
    seen = {}
    for case in cases:
        batch = get(*case)
        spec = spec_masks(batch.state)
        cut = spec_masks(R.without_tail(batch.state, K_of(case)))
        for i in range(batch.N):
            for bit in R.SINGLE_BITS + (R.OVERLAP, R.DEAD_NONZERO):
                where = seen.setdefault(bit, set())
                if spec[i] & bit:
                    where.update(w for w, ok in (('first', i == 0), ('last', i == batch.N - 1), ('wave', i % 4 != 0)) if ok)
                if (spec[i] ^ cut[i]) & bit:
                    where.add('tail')
    return seen


def test_single_batches_put_every_bit_everywhere():
    seen = _coverage([c for c in R.SINGLE_CASES if c[1] > 1], R.single_case, R.spec_single_masks, lambda c: None)
    for bit in R.SINGLE_BITS:
        assert seen[bit] == {'first', 'last', 'wave', 'tail'}, (hex(bit), seen[bit])


def test_multi_batches_put_every_bit_everywhere():
    seen = _coverage(R.MULTI_CASES, R.multi_case, R.spec_multi_masks, lambda c: c[0])
    for bit in R.MULTI_BITS:
        assert seen[bit] == {'first', 'last', 'wave', 'tail'}, (hex(bit), seen[bit])


def test_the_added_cells_are_the_listed_ones():
    assert R.cell_list(81) == [0, 63, 64, 80] and R.cell_list(144) == [0, 63, 64, 127, 128, 143]
    assert R.cell_list(46 * 46, multi=True) == [0, 63, 64, 2111, 2112, 2115, 704, 1408]
    for cases, get, multi in ((R.SINGLE_CASES, R.single_case, False), (R.MULTI_CASES, R.multi_case, True)):
        for case in cases:
            batch = get(*case)
            used = {c for c in batch.cells if c >= 0}
            assert used <= set(R.cell_list(batch.S ** 2, multi))
            assert batch.N < 75 or used == set(R.cell_list(batch.S ** 2, multi)), case


@pytest.mark.parametrize('case', R.NEEDLE_SINGLE + R.NEEDLE_MULTI)
def test_every_needle_batch_fails_in_one_env_only(case):
    multi = len(case) == 3
    batch = R.multi_case(*case) if multi else R.single_case(*case)
    spec_masks, check = (R.spec_multi_masks, _o.multi_check) if multi else (R.spec_single_masks, _o.single_check)
    assert not spec_masks(batch.base).any()
    planes = ('foods', 'heads', 'bodies', 'dones') if multi else (None,)
    count = 0
    for p, kind, cell, nb in R.needles(batch):
        for k in planes:  # the needle batch is the valid batch outside env p ...
            a, b = (nb.state, batch.base) if k is None else (nb.state[k], batch.base[k])
            differs = (a != b).reshape(batch.N, -1).any(axis=1)
            differs[p] = False
            assert not differs.any(), (p, kind, cell, k)
        one = {k: v.reshape(batch.N, -1)[p:p + 1] for k, v in nb.state.items()} if multi else nb.state[p:p + 1]
        if multi:
            one = {k: v.reshape((-1, 1, batch.S, batch.S)) if k in ('foods', 'heads', 'bodies') else v.reshape(-1) for k, v in one.items()}
        spec_p = int(spec_masks(one)[0])                                    # ... and env p fails
        got = check(nb.state)
        assert spec_p != 0 and got[p] == spec_p and np.count_nonzero(got) == 1, (p, kind, cell)
        count += 1
    assert count == 8 * (4 if multi else 2)
