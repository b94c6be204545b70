"""wurm_amd.rl.MultiRolloutStats on the GPU against the float64 / integer numpy restatement
(tests/multi_rollout_stats_ref.py): synthetic windows at the shapes that reach every code path (one lane; one full wave; a
wave plus one lane; several workgroups with a ragged tail; one env past a workgroup boundary), chained so that lives
straddle windows, and `MultiSnake.act_window(..., info=True)` / `MultiSnake.rollout` windows of a real env."""
import types

import numpy as np
import pytest
import torch

from tests.multi_rollout_stats_ref import COLS, RATIOS, SUMS, RefMultiStats
from tests.rollout_stats_ref import entropy64
from wurm_amd import _lib
from wurm_amd.envs import MultiSnake
from wurm_amd.envs._multi_act import species_of
from wurm_amd.rl import MultiRolloutStats

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WINDOWS = 3
# (T, K, N)
CASES = [(1, 1, 1), (5, 2, 64), (7, 3, 65), (3, 2, 700), (4, 4, 257)]
KEYS = ('rewards', 'food', 'size', 'dones', 'boost', 'snake_collision', 'edge_collision')
EXACT_SUMS = [0, 1, 5, 6, 7, 8, 9]   # flags and sizes: integers
FLOAT_SUMS = [2, 4]                  # reward, food
RTOL = 1e-12
# Per-step MEAN entropy against float64 on the same fp32 probabilities: four terms of magnitude <= 1/e, each with about
# four fp32 roundings (logf, the product, two adds): 4 * 0.37 * 4 * 6e-8 = 3.5e-7 (the bound of tests/test_rollout_stats_gpu.py)
ENTROPY_ATOL = 1e-6


def _window(T, K, N, seed):
    """rewards in {-1, -0.25, 0, 0.75, 1}; dones at rate 0.1, none at step 0, agent 0 in every env at step 1; collision
    flags as subsets of dones; sizes 0 .. 12; probs a softmax of normals with every fifth row one-hot (the clamp)"""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *shape: torch.rand(shape, generator=g)
    dones = rand(T, K, N) < 0.1
    dones[0] = False
    if T > 1:
        dones[1, 0] = True
    values = torch.tensor([-1.0, -0.25, 0.0, 0.75, 1.0])
    rewards = values[torch.randint(5, (T, K, N), generator=g)]
    food = (rand(T, K, N) < 0.3).float()
    size = torch.randint(13, (T, K, N), generator=g).float()
    boost = rand(T, K, N) < 0.4
    edge = dones & (rand(T, K, N) < 0.5)
    snake = dones & ~edge & (rand(T, K, N) < 0.7)
    probs = torch.softmax(2 * torch.randn((T * K * N, 4), generator=g), dim=-1)
    probs[::5] = torch.roll(torch.tensor([1.0, 0.0, 0.0, 0.0]), seed % 4)
    w = dict(rewards=rewards, food=food, size=size, dones=dones, boost=boost, snake_collision=snake, edge_collision=edge)
    w = {k: v.reshape(T, K * N) for k, v in w.items()}
    w.update(probs=probs.reshape(T, K * N, 4), all_done=dones.all(dim=1))
    return w


def _device(w, agent=None, N=None, steps=slice(None)):
    """the window on the device; agent: a contiguous copy of that agent's N columns (all_done stays the envs')"""
    cols = slice(None) if agent is None else slice(agent * N, (agent + 1) * N)
    return {k: (v[steps] if k == 'all_done' else v[steps, cols]).contiguous().to(DEV) for k, v in w.items()}


def _stats(K, N, alpha=0.025):
    return MultiRolloutStats(types.SimpleNamespace(num_envs=N, num_snakes=K, device=torch.device(DEV)), alpha=alpha)


def _ref_update(refs, w, N, probs=True, all_done=True):
    """one RefMultiStats per agent on its block of columns; returns the (K, T, 10) table"""
    n = {k: v.numpy() for k, v in w.items() if v is not None}
    tables = []
    for k, r in enumerate(refs):
        c = slice(k * N, (k + 1) * N)
        tables.append(r.update(*[n[key][:, c] for key in KEYS], n['probs'][:, c] if probs else None,
                               n['all_done'] if all_done else None))
    return np.stack(tables)


def _bits(stats):
    return [t.cpu().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32).copy()
            for t in (stats.carry, stats.accum, stats.smooth)]


@pytest.fixture(scope='module', params=CASES, ids=lambda c: f'T{c[0]}_K{c[1]}_N{c[2]}')
def run(request):
    """three chained windows of one case, computed once: the inputs, what the GPU gave after each window, and the same
    from the numpy restatement"""
    T, K, N = request.param
    windows = [_window(T, K, N, 100 * N + 10 * K + w) for w in range(WINDOWS)]
    stats = _stats(K, N)
    refs = [RefMultiStats(N) for _ in range(K)]
    got, want, launches = [], [], []
    count = _lib.lib().wurm_launch_count
    for w in windows:
        dev = _device(w)
        before = count()
        table = stats.update(dev, per_step=True)
        launches.append(count() - before)
        assert table.shape == (K, T, SUMS) and table.dtype == torch.float64
        got.append(dict(table=table.cpu().numpy(), carry=stats.carry.cpu().numpy(), accum=stats.accum.cpu().numpy(),
                        smooth=stats.smooth.cpu().numpy()))
        tables = _ref_update(refs, w, N)
        want.append(dict(table=tables, ret=np.concatenate([r.ret for r in refs]),
                         length=np.concatenate([r.length for r in refs]), accum=np.stack([r.accum.copy() for r in refs]),
                         smooth=np.stack([r.smooth.copy() for r in refs])))
    return types.SimpleNamespace(T=T, K=K, N=N, windows=windows, got=got, want=want, launches=launches)


def test_two_launches_per_update(run):
    assert run.launches == [2] * WINDOWS


def test_exact_columns(run):
    """the seven flag or size sums, steps, episodes, the lives' lengths and both maxima, with =="""
    exact_acc = [0] + [1 + j for j in EXACT_SUMS] + [12, 13, 14, 15]
    for got, want in zip(run.got, run.want):
        assert np.array_equal(got['table'][..., EXACT_SUMS], want['table'][..., EXACT_SUMS])
        assert np.array_equal(got['carry'][1], want['length'])
        assert np.array_equal(got['accum'][:, exact_acc], want['accum'][:, exact_acc])
    last = run.want[-1]['accum']
    if run.T > 1:
        assert last[0, 2] >= WINDOWS * run.N and (last[:, 2] > 0).all()   # deaths happened, in every agent
    else:
        assert not last[:, 2].any() and (run.got[-1]['accum'][:, 13:15] == -np.inf).all()


def test_reward_food_and_life_return(run):
    for got, want in zip(run.got, run.want):
        np.testing.assert_allclose(got['table'][..., FLOAT_SUMS], want['table'][..., FLOAT_SUMS], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['accum'][:, [3, 5, 11]], want['accum'][:, [3, 5, 11]], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got['carry'][0].view(np.float32), want['ret'], rtol=RTOL, atol=0)


def test_entropy(run):
    worst = 0.0
    for got, want, w in zip(run.got, run.want, run.windows):
        alive = np.maximum(want['table'][..., 0], 1)
        err = np.abs(got['table'][..., 3] - want['table'][..., 3]) / alive   # of the per-step mean over the alive
        worst = max(worst, float(err.max()))
        assert np.abs(got['smooth'][:, 1] - want['smooth'][:, 1]).max() <= ENTROPY_ATOL
    print(f'max |mean entropy - float64| = {worst:.3e}')
    assert worst <= ENTROPY_ATOL
    # the clamp was met: a one-hot row has the entropy of the clamp, not nan and not 0
    w = _device(_window(1, run.K, run.N, 0))
    w['probs'] = torch.zeros_like(w['probs'])
    w['probs'][..., 1] = 1.0
    table = _stats(run.K, run.N).update(w, per_step=True)
    h = float(entropy64(np.array([0, 1, 0, 0], np.float32)))
    assert h > 0 and table[:, 0, 3].cpu().numpy() == pytest.approx(run.N * h, rel=1e-6)


def test_smoother(run):
    other = [c for c in range(COLS) if c != 1]
    for got, want in zip(run.got, run.want):
        np.testing.assert_allclose(got['smooth'][:, other], want['smooth'][:, other], rtol=RTOL, atol=0)
    if run.T == 1:   # nobody dies at step 0: nothing has been seen over the done mask
        assert np.isnan(run.got[-1]['smooth'][:, 8]).all() and not np.isnan(run.got[-1]['smooth'][:, :8]).any()


@pytest.mark.parametrize('run', [c for c in CASES if c[0] > 1], ids=lambda c: f'T{c[0]}_K{c[1]}_N{c[2]}', indirect=True)
def test_smoother_skips_an_empty_mask(run):
    """step 0 has no death (the `return` mask is empty), step 1 kills agent 0 everywhere (its `~done` masks are empty)"""
    w = run.windows[0]
    stats = _stats(run.K, run.N)
    stats.update(_device(w, steps=slice(0, 1)))
    first = stats.smooth.cpu().numpy().copy()
    assert np.isnan(first[:, 8]).all() and not np.isnan(first[:, :8]).any()
    stats.update(_device(w, steps=slice(1, 2)))
    second = stats.smooth.cpu().numpy()
    masked = [c for c, (_, den) in enumerate(RATIOS) if den == 0]
    assert masked == [0, 1, 2, 5, 6]
    assert np.array_equal(second[0, masked].view(np.int64), first[0, masked].view(np.int64))
    assert second[0, 7] == 0.025 * 1.0 + (1 - 0.025) * first[0, 7] and not np.isnan(second[0, 8])
    # ... and the two one-step windows are the two-step window
    both = _stats(run.K, run.N)
    both.update(_device(w, steps=slice(0, 2)))
    assert all(np.array_equal(a, b) for a, b in zip(_bits(both), _bits(stats)))


def test_two_runs_have_the_same_bits(run):
    again = _stats(run.K, run.N)
    for w, got in zip(run.windows, run.got):
        table = again.update(_device(w), per_step=True).cpu().numpy()
        assert np.array_equal(table.view(np.int64), got['table'].view(np.int64))
        assert np.array_equal(again.accum.cpu().numpy().view(np.int64), got['accum'].view(np.int64))
        assert np.array_equal(again.smooth.cpu().numpy().view(np.int64), got['smooth'].view(np.int64))
    # and without the table (it then lives in the workspace)
    plain = _stats(run.K, run.N)
    for w in run.windows:
        assert plain.update(_device(w)) is None
    assert all(np.array_equal(a, b) for a, b in zip(_bits(plain), _bits(again)))


def test_agent_equals_stand_alone(run):
    N = run.N
    for k in range(run.K):
        alone = _stats(1, N)
        for w, got in zip(run.windows, run.got):
            table = alone.update(_device(w, agent=k, N=N), per_step=True).cpu().numpy()
            assert np.array_equal(table.view(np.int64)[0], got['table'].view(np.int64)[k])
            assert np.array_equal(alone.carry.cpu().numpy(), got['carry'][:, k * N:(k + 1) * N])
            assert np.array_equal(alone.accum.cpu().numpy().view(np.int64)[0], got['accum'].view(np.int64)[k])
            assert np.array_equal(alone.smooth.cpu().numpy().view(np.int64)[0], got['smooth'].view(np.int64)[k])


def test_null_probs_and_all_done_leave_their_columns_zero():
    T, K, N = 5, 2, 65
    w = _window(T, K, N, 3)
    dev = {k: v for k, v in _device(w).items() if k not in ('probs', 'all_done')}
    stats = _stats(K, N)
    table = stats.update(dev, per_step=True).cpu().numpy()
    refs = [RefMultiStats(N) for _ in range(K)]
    want = _ref_update(refs, w, N, probs=False, all_done=False)
    assert not table[..., 3].any() and np.array_equal(table, want)
    accum, smooth = stats.accum.cpu().numpy(), stats.smooth.cpu().numpy()
    assert not accum[:, 4].any() and not accum[:, 15].any() and accum[:, 2].all() and not smooth[:, 1].any()
    assert np.array_equal(accum, np.stack([r.accum for r in refs]))


def test_read_and_state_dict():
    T, K, N = 5, 3, 64
    first, second = _window(T, K, N, 21), _window(T, K, N, 22)
    stats, refs = _stats(K, N, alpha=0.1), [RefMultiStats(N, alpha=0.1) for _ in range(K)]
    stats.update(_device(first))
    _ref_update(refs, first, N)
    carry, smooth = stats.carry.clone(), stats.smooth.clone()
    kept = stats.read(reset=False)
    by_species = {P: stats.read(reset=False, num_species=P) for P in (1, 2, 3)}   # 2 does not divide 3
    rows = stats.read()
    assert kept == rows and len(rows) == K
    names = ('reward', 'policy_entropy', 'food', 'edge_collisions', 'snake_collisions', 'boost', 'size', 'done', 'return')
    for k, (row, ref) in enumerate(zip(rows, refs)):
        a = ref.accum
        assert row['steps'] == T * N and row['episodes'] == int(a[15]) and a[2] > 0
        for c, (name, (num, den)) in enumerate(zip(names, RATIOS)):
            want = a[1 + num] / (a[0] if den is None else a[1 + den])
            if c == 1:
                assert row[name] == pytest.approx(want, abs=ENTROPY_ATOL)
                assert row['ewm_' + name] == pytest.approx(ref.smooth[c], abs=ENTROPY_ATOL)
            else:
                assert row[name] == pytest.approx(want, rel=RTOL)
                assert row['ewm_' + name] == pytest.approx(ref.smooth[c], rel=RTOL)
        assert row['life_return_mean'] == a[11] / a[2] and row['life_length_mean'] == a[12] / a[2]
        assert row['size_at_death_max'] == a[13] and row['life_return_max'] == a[14]
    # species: the host sum of the per-agent accumulator rows, divided afterwards
    acc = np.stack([r.accum for r in refs])
    for P, species in by_species.items():
        assert len(species) == P
        for s, row in enumerate(species):
            mine = [k for k in range(K) if species_of(k, K, P) == s]
            assert mine, (P, s)
            tot = acc[mine].sum(0)
            assert row['steps'] == T * N * len(mine) and row['episodes'] == int(acc[0, 15])
            assert row['done'] == tot[2] / tot[0] and row['size'] == tot[7] / tot[1] and row['return'] == tot[10] / tot[2]
            assert row['reward'] == pytest.approx(tot[3] / tot[1], rel=RTOL)
            assert row['life_length_mean'] == tot[12] / tot[2]
            assert row['size_at_death_max'] == acc[mine, 13].max() and row['life_return_max'] == acc[mine, 14].max()
            assert not any(name.startswith('ewm_') for name in row)
    assert by_species[3] == [{k: v for k, v in r.items() if not k.startswith('ewm_')} for r in rows]
    # the sums are gone, the carry and the smoother are not
    assert stats.accum[0].tolist() == [0.0] * 13 + [-np.inf] * 2 + [0.0]
    assert torch.equal(stats.carry, carry) and torch.equal(stats.smooth, smooth)
    empty = stats.read()
    assert empty[0]['steps'] == 0 and np.isnan(empty[0]['life_return_mean']) and np.isnan(empty[0]['size_at_death_max'])
    assert empty[0]['ewm_size'] == rows[0]['ewm_size']
    # a resumed run continues the curves
    resumed = _stats(K, N, alpha=0.1)
    resumed.load_state_dict({k: v.cpu().to(DEV) for k, v in stats.state_dict().items()})
    stats.update(_device(second))
    resumed.update(_device(second))
    assert all(np.array_equal(a, b) for a, b in zip(_bits(stats), _bits(resumed)))
    assert stats.read() == resumed.read()


# ---------------------------------------------------------------------------------------------- a real env, end to end

INFO = (('food', 'food_'), ('size', 'size_'), ('boost', 'boost_'), ('snake_collision', 'snake_collision_'),
        ('edge_collision', 'edge_collision_'))


def _env(seed=33):
    return MultiSnake(num_envs=8, num_snakes=2, size=12, observation_mode='partial_2', boost=False, device=DEV, seed=seed)


def _params(E=75):
    from wurm_amd.agents import FeedforwardAgent, pack_policy_params
    rows = []
    for p in range(2):
        torch.manual_seed(10 + p)
        rows.append(pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)))
    return torch.stack(rows).to(DEV)


def _check_against_ref(stats, refs, out, N, probs):
    host = {k: out[k].reshape(out[k].shape[0], -1).cpu() for k in KEYS}
    host['probs'] = out['probs'].cpu() if probs else None
    host['all_done'] = out['all_done'].cpu()
    table = stats.update(out, per_step=True).cpu().numpy()
    want = _ref_update(refs, host, N, probs=probs)
    exact = [j for j in range(SUMS) if j != 3]   # (rewards are -1, 0 or 1 and food 0 or 1 here: every sum an integer)
    assert np.array_equal(table[..., exact], want[..., exact])
    assert np.abs(table[..., 3] - want[..., 3]).max() <= ENTROPY_ATOL * N
    accum, smooth = stats.accum.cpu().numpy(), stats.smooth.cpu().numpy()
    ref_accum, ref_smooth = np.stack([r.accum for r in refs]), np.stack([r.smooth for r in refs])
    cols = [j for j in range(16) if j != 4]
    assert np.array_equal(accum[:, cols], ref_accum[:, cols])
    np.testing.assert_allclose(smooth, ref_smooth, rtol=0, atol=ENTROPY_ATOL, equal_nan=True)
    other = [c for c in range(COLS) if c != 1]
    np.testing.assert_allclose(smooth[:, other], ref_smooth[:, other], rtol=RTOL, atol=0, equal_nan=True)
    assert np.array_equal(stats.life_length.cpu().numpy(), np.concatenate([r.length for r in refs]))
    assert np.array_equal(stats.life_return.cpu().numpy(), np.concatenate([r.ret for r in refs]).astype(np.float32))


def test_act_window_info_end_to_end():
    T, K, N = 6, 2, 8
    params = _params()
    env, plain, hand = _env(), _env(), _env()
    state, state_plain, state_hand = env.reset(), plain.reset(), hand.reset()
    stats, refs = MultiRolloutStats(env), [RefMultiStats(N) for _ in range(K)]
    count = _lib.lib().wurm_launch_count
    for window in range(2):
        before = count()
        out = env.act_window(params, state, T, info=True)
        assert count() - before == 2 * T   # the info keys cost no launch of the library's
        for name, _ in INFO:
            want = torch.float32 if name in ('food', 'size') else torch.bool
            assert out[name].shape == (T, K * N) and out[name].dtype == want, name
        # the other keys and the env's state: those of a twin's window without info
        base = plain.act_window(params, state_plain, T)
        assert set(out) == set(base) | {name for name, _ in INFO}
        for key, v in base.items():
            if key == 'state':
                assert all(torch.equal(out['state'][a], v[a]) for a in v)
            else:
                assert torch.equal(out[key], v), key
        assert env._call == plain._call and env.policy_calls == plain.policy_calls
        # the info rows: those of a twin stepped by hand with the window's actions
        for t in range(T):
            actions = {f'agent_{k}': out['actions'][t, k * N:(k + 1) * N].clone() for k in range(K)}
            _, rewards, dones, info = hand.step(actions)
            hand.reset(dones['__all__'], return_observations=False)
            for name, prefix in INFO:
                rows = torch.cat([info[f'{prefix}{k}'] for k in range(K)])
                assert torch.equal(out[name][t], rows), (window, t, name)
            assert torch.equal(out['rewards'][t], torch.cat([rewards[f'agent_{k}'] for k in range(K)]))
        _check_against_ref(stats, refs, out, N, probs=True)
        state, state_plain = out['state'], base['state']
    for name in ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours'):
        assert torch.equal(getattr(env, name), getattr(plain, name)), name
        assert torch.equal(getattr(env, name), getattr(hand, name)), name
    rows = stats.read()
    assert rows[0]['steps'] == 2 * T * N and 0 < rows[0]['policy_entropy'] <= np.log(4) + 1e-6 and rows[0]['size'] >= 3
    # T = 0: empty tensors of the right type, no launch
    before = count()
    empty = env.act_window(params, state, 0, info=True)
    assert count() == before
    for name, _ in INFO:
        assert empty[name].shape == (0, K * N) and empty[name].dtype == out[name].dtype and empty[name].device == out[name].device
    assert not set(env.act_window(params, state, 0)) & {name for name, _ in INFO}


def test_rollout_output_end_to_end():
    T, K, N = 6, 2, 8
    env = _env(seed=5)
    env.reset()
    stats, refs = MultiRolloutStats(env), [RefMultiStats(N) for _ in range(K)]
    g = torch.Generator().manual_seed(9)
    for window in range(2):
        actions = torch.randint(4, (T, K, N), generator=g).to(DEV)
        out = env.rollout(actions)
        assert out['rewards'].shape == (T, K, N) and 'probs' not in out
        _check_against_ref(stats, refs, dict(out, probs=None), N, probs=False)
    rows = stats.read()
    assert rows[1]['steps'] == 2 * T * N and rows[1]['policy_entropy'] == 0.0 and rows[1]['size'] >= 3
