"""wurm_single_check, wurm_multi_check, wurm_orientations and the classes' check_consistency() on FAILING batches, at every
size at which the kernels take another path.

The stand-alone checkers end every parity, fuzz and host-layer test of this suite, so a checker that misses a broken env
weakens all of them at once.  Here they run on the batches of tests/checker_ref.py — every corruption kind, at the cells
where a lane mask or an item boundary cuts, in every wave of a workgroup, in permuted and straggler workgroups — and every
comparison is exact equality of uint32 masks with BOTH the oracle and the float64 specification
(tests/test_checker_batches_cpu.py proves the specification against the reference's recorded verdicts, and that the batches
reach what they claim to).  Every call gets an `err` one element longer than the batch: the extra element keeps its
sentinel, and every other element loses the value the buffer was filled with."""
import numpy as np
import pytest
import torch

from oracle import oracle as _o
from tests import checker_ref as R
from tests.test_checker_batches_cpu import FX2, fixture_multi_states
from tests.test_checker_failing_states import FX, PHRASES, _agrees, _multi_verdict, _single_states, _verdict

pytestmark = pytest.mark.gpu

SENTINEL, FILL = 0x7E57ED, 0x5A5A5A5A      # neither is a mask: masks are below 0x400
DEV = 'cuda:0'


def _run(fn, what, N, *args):
    from wurm_amd import _lib
    err = torch.full((N + 1,), FILL, dtype=torch.int32, device=DEV)
    err[N] = SENTINEL
    _lib.check(fn(*args[:-1], _lib.ptr(err), _lib.i64(N), *args[-1], _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    out = err.cpu().numpy()
    assert out[N] == SENTINEL, f'{what}: wrote behind the last env'
    assert not (out[:N] == FILL).any(), f'{what}: envs {np.nonzero(out[:N] == FILL)[0][:8]} were not written'
    return out[:N].astype(np.uint32)


def hip_single_check(envs):
    from wurm_amd import _lib
    N, _, S, _ = envs.shape
    e = torch.from_numpy(np.ascontiguousarray(envs)).to(DEV)
    return _run(_lib.lib().wurm_single_check, 'wurm_single_check', N, _lib.ptr(e), (S,))


def hip_multi_check(st):
    from wurm_amd import _lib
    N, _, S, _ = st['foods'].shape
    K = st['heads'].shape[0] // N
    d = [torch.from_numpy(np.ascontiguousarray(st[k])).to(DEV) for k in ('foods', 'heads', 'bodies', 'dones')]
    return _run(_lib.lib().wurm_multi_check, 'wurm_multi_check', N, *[_lib.ptr(t) for t in d], (K, S))


def _same(got, want, what, batch=None):
    bad = np.nonzero(got != want)[0]
    detail = '' if batch is None or not len(bad) else f' ({batch.kinds[bad[0]]} at cell {batch.cells[bad[0]]})'
    assert not len(bad), f'{what}: {len(bad)} envs differ, first env {bad[0]}: {hex(got[bad[0]])} != {hex(want[bad[0]])}{detail}'


# ------------------------------------------------------------------------------------------------ the failing batches

@pytest.mark.parametrize('S,N', R.SINGLE_CASES)
def test_single_check_on_a_failing_batch(S, N):
    batch = R.single_case(S, N)
    got = hip_single_check(batch.state)
    _same(got, _o.single_check(batch.state), f'S={S} N={N} against the oracle', batch)
    _same(got, R.spec_single_masks(batch.state), f'S={S} N={N} against the specification', batch)
    assert got.any() and not hip_single_check(batch.base).any()


@pytest.mark.parametrize('K,S,N', R.MULTI_CASES)
def test_multi_check_on_a_failing_batch(K, S, N):
    batch = R.multi_case(K, S, N)
    got = hip_multi_check(batch.state)
    _same(got, _o.multi_check(batch.state), f'K={K} S={S} N={N} against the oracle', batch)
    _same(got, R.spec_multi_masks(batch.state), f'K={K} S={S} N={N} against the specification', batch)
    assert got.any() and not hip_multi_check(batch.base).any()


# ------------------------------------------------------------------------------------------------ needles

def _needles(batch, check, spec_one):
    """one failing env in a valid batch: its mask is the specification's and every other mask is zero — an env that is
    skipped or read twice, or LDS that two waves share, shows here"""
    for p, kind, cell, nb in R.needles(batch):
        got = check(nb.state)
        want = np.zeros(batch.N, np.uint32)
        want[p] = spec_one(nb, p)
        assert want[p] != 0
        _same(got, want, f'needle {kind} at cell {cell} in env {p} of {batch.N}')
        _same(got, (_o.single_check if batch.K is None else _o.multi_check)(nb.state), f'needle {kind} in env {p}: oracle')


@pytest.mark.parametrize('S,N', R.NEEDLE_SINGLE)
def test_single_check_finds_the_needle(S, N):
    _needles(R.single_case(S, N), hip_single_check, lambda nb, p: R.spec_single_mask(nb.state[p]))


@pytest.mark.parametrize('K,S,N', R.NEEDLE_MULTI)
def test_multi_check_finds_the_needle(K, S, N):
    def spec_one(nb, p):
        st = nb.state
        return R.spec_multi_mask(st['foods'][p], st['heads'].reshape(N, K, -1)[p], st['bodies'].reshape(N, K, -1)[p],
                                 st['dones'].reshape(N, K)[p])
    _needles(R.multi_case(K, S, N), hip_multi_check, spec_one)


# ------------------------------------------------------------------------------------------------ the recorded states

@pytest.mark.parametrize('S', [int(s) for s in FX2['single_sizes']])
def test_single_check_gives_the_references_verdicts_at_every_size(S):
    envs = np.ascontiguousarray(FX2[f'single_S{S}_envs'])
    got = hip_single_check(envs)
    _same(got, _o.single_check(envs), f'S={S} against the oracle')
    _same(got, R.spec_single_masks(envs), f'S={S} against the specification')
    for name, m, msg in zip(FX2[f'single_S{S}_names'], got, FX2[f'single_S{S}_env_msg']):
        _agrees(_verdict(int(m), one_food=True), str(msg), f'S{S}:{name}')


@pytest.mark.parametrize('K,S', [tuple(int(v) for v in ks) for ks in FX2['multi_shapes']])
def test_multi_check_gives_the_references_verdicts_at_every_shape(K, S):
    """Non-integer food among them — 0.5, 0.6 and 1.5 under a head.  Only the VERDICT is what the reference defines
    there ('' for 0.5: it rounds the living envs' planes, half to even, before it checks them; 'food and head pixel is
    overlapping' for 0.6; 'invalid food pixel' for 1.5), so the verdict is compared with the recorded message.  Before
    this file multi_check_kernel rounded food for its head-on-food sum only and compared the raw value with 0 and 1,
    and the oracle did not round at all: both called 0.5 an invalid food pixel where the reference accepts the state.
    Both round now, so the masks are compared as well."""
    states = list(fixture_multi_states(K, S))
    st = _o.multi_empty_state(len(states), K, S)
    for k in ('foods', 'heads', 'bodies', 'dones'):
        st[k][...] = np.concatenate([s[k] for _, s, _ in states])
    got = hip_multi_check(st)
    for (name, _, msg), m in zip(states, got):
        _agrees(_multi_verdict(int(m)), msg, f'K{K} S{S}:{name}')
    assert sum(1 for name, _, _ in states if name.startswith('food_0.5_under_the_head')) >= 1
    _same(got, _o.multi_check(st), f'K={K} S={S} against the oracle')
    _same(got, R.spec_multi_masks(st), f'K={K} S={S} against the specification')


# ------------------------------------------------------------------------------------------------ host layer

def _raised(fn, *args):
    try:
        fn(*args)
        return ''
    except RuntimeError as e:
        return str(e)


def _phrase_raised(ours, phrase, what):
    if phrase == '':
        assert ours == '', f'{what}: raised {ours!r}'
    else:
        assert phrase in ours, f'{what}: expected {phrase!r}, raised {ours!r}'


@pytest.mark.parametrize('S', [9, 12])
def test_utils_raise_the_first_failing_check_of_the_batch(S):
    """_or_reduce over a batch names the first check ANY env fails, in the reference's order (recorded from it for
    env_consistency; for snake_consistency the same masks without the one-food check)"""
    from wurm_amd.utils import env_consistency, snake_consistency
    names, envs = _single_states()
    batch = np.ascontiguousarray(np.concatenate([e for n, e in zip(names, envs) if n.startswith(f'S{S}:')]))
    t = torch.from_numpy(batch).to(DEV)
    ref = str(FX[f'single_batch_msg_S{S}'])
    key = [p for _, p in PHRASES if p in ref]
    assert len(key) == 1
    _phrase_raised(_raised(env_consistency, t), key[0], f'env_consistency S={S}')
    mask = int(np.bitwise_or.reduce(R.spec_single_masks(batch)))
    _phrase_raised(_raised(snake_consistency, t), _verdict(mask, one_food=False), f'snake_consistency S={S}')
    only_food = np.ascontiguousarray(np.concatenate([e for n, e in zip(names, envs) if n in (f'S{S}:valid', f'S{S}:two_foods', f'S{S}:no_food')]))
    assert _raised(snake_consistency, torch.from_numpy(only_food).to(DEV)) == ''
    _phrase_raised(_raised(env_consistency, torch.from_numpy(only_food).to(DEV)), 'exactly one food instance', 'one food')


def test_single_snake_class_on_a_needle_batch():
    from wurm_amd.envs import SingleSnake
    S, N = R.NEEDLE_SINGLE[0]
    batch = R.single_case(S, N)
    env = SingleSnake(num_envs=N, size=S, device=torch.device(DEV), manual_setup=True, seed=0)
    env.envs = torch.from_numpy(batch.base).to(DEV)
    assert _raised(env.check_consistency) == ''
    for p, kind, cell, nb in R.needles(batch):
        env = SingleSnake(num_envs=N, size=S, device=torch.device(DEV), manual_setup=True, seed=0)
        env.envs = torch.from_numpy(nb.state).to(DEV)
        phrase = _verdict(R.spec_single_mask(nb.state[p]), one_food=True)
        assert phrase
        _phrase_raised(_raised(env.check_consistency), phrase, f'{kind} in env {p}')
        others = torch.ones(N, dtype=torch.bool, device=DEV)
        others[p] = False
        assert _raised(env.check_consistency, others) == '', f'{kind} in env {p}: masked out, still raised'
        _phrase_raised(_raised(env.check_consistency, ~others), phrase, f'{kind} in env {p}: the only env asked about')


def test_multi_snake_class_sees_the_last_env():
    from wurm_amd.envs import MultiSnake
    K, S, N = R.NEEDLE_MULTI[0]
    batch = R.multi_case(K, S, N)

    def verdict(st):
        env = MultiSnake(num_envs=N, num_snakes=K, size=S, device=torch.device(DEV), manual_setup=True, seed=0)
        env.foods, env.heads, env.bodies = (torch.from_numpy(st[k]).to(DEV) for k in ('foods', 'heads', 'bodies'))
        env.dones = torch.from_numpy(st['dones']).to(DEV).bool()
        return _raised(env.check_consistency)

    assert verdict(batch.base) == ''
    for kind, phrase in (('snake_on_top_of_snake', 'overlapping snakes'), ('dead_snake_with_a_body', 'Dead snake contains non-zero elements'),
                         ('overlap_segment', None), ('food_under_the_head', 'food and head pixel is overlapping')):
        for p in (N - 1, 0):
            nb = R.needle(batch, p, kind, S * S - 1)
            st = nb.state
            mask = R.spec_multi_mask(st['foods'][p], st['heads'].reshape(N, K, -1)[p], st['bodies'].reshape(N, K, -1)[p],
                                     st['dones'].reshape(N, K)[p])
            assert phrase is None or _multi_verdict(mask) == phrase
            _phrase_raised(verdict(st), _multi_verdict(mask), f'{kind} in env {p}')


# ------------------------------------------------------------------------------------------------ orientations

@pytest.mark.parametrize('S', [9, 14, 20, 25, 36, 45, 50, 64])     # one size per cells-per-lane tier
def test_orientations_at_every_tier(S):
    from tests.hip_backend import HipBackend
    N = 75
    rng = np.random.RandomState(S)
    envs = np.zeros((N, 3, S, S), np.float32)
    _o.single_reset(envs, np.ones(N), 'none', seed=S, call=0)
    for t in range(10):
        _o.single_step(envs, rng.randint(0, 4, size=N).astype(np.int64), 'none', seed=S, call=1 + t)
    want = _o.orientations(envs)
    assert set(want.tolist()) == {0, 1, 2, 3}
    got = HipBackend().orientations(envs)
    assert np.array_equal(got, want), f'S={S}: envs {np.nonzero(got != want)[0][:8]}'
