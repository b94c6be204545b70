"""wurm_amd.rl.RolloutStats on the GPU against the float64 / integer numpy restatement (tests/rollout_stats_ref.py):
synthetic windows at the shapes that reach every code path (one env; one wave; a wave and one lane; three workgroups with
a ragged last one; populations whose members are no multiple of a wave), chained so that episodes straddle windows, and
ten chained `policy_rollout` windows of a real env, after each of which the carried snake length is the env's own."""
import types

import numpy as np
import pytest
import torch

from tests.rollout_stats_ref import COLS, RefStats, entropy64
from wurm_amd.rl import RolloutStats

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WINDOWS = 3
# (T, N, population)
CASES = [(1, 1, None), (5, 64, None), (7, 65, None), (3, 700, None), (3, 700, 7), (3, 15, 3)]
# Per-step MEAN entropy against float64 on the same fp32 probabilities: four terms of magnitude <= 1/e, each with about
# four fp32 roundings (logf, the product, two adds): 4 * 0.37 * 4 * 6e-8 = 3.5e-7
ENTROPY_ATOL = 1e-6


def _window(T, N, seed):
    """dones at rate 0.2, rewards in {0, 1}, flags as subsets of dones, probs a softmax of normals with every fifth row
    a probability of exactly 1 beside three of exactly 0 (the clamp)"""
    rng = np.random.default_rng(seed)
    dones = rng.random((T, N)) < 0.2
    rewards = (rng.random((T, N)) < 0.3).astype(np.float32)
    edge = dones & (rng.random((T, N)) < 0.5)
    selfc = dones & ~edge & (rng.random((T, N)) < 0.7)
    z = rng.normal(size=(T, N, 4)) * 2
    probs = np.exp(z - z.max(-1, keepdims=True))
    probs = (probs / probs.sum(-1, keepdims=True)).astype(np.float32).reshape(-1, 4)
    probs[::5] = np.roll(np.array([1, 0, 0, 0], np.float32), seed % 4)
    return dict(rewards=rewards, dones=dones, edge_collision=edge, self_collision=selfc, probs=probs.reshape(T, N, 4))


def _sizes(N, seed):
    return np.random.default_rng(1000 + seed).integers(3, 9, N).astype(np.int32)


def _device(window, cols=slice(None)):
    return {k: torch.from_numpy(np.ascontiguousarray(v[:, cols])).to(DEV) for k, v in window.items()}


def _stats(N, sizes, population=None, alpha=0.025, snake=True):
    env = types.SimpleNamespace(num_envs=N, device=torch.device(DEV))
    if snake:
        env.initial_snake_length = 3
        env.envs = torch.zeros((N, 3, 3, 3), device=DEV)
    stats = RolloutStats(env, population=population, alpha=alpha)
    stats.carry[2] = torch.from_numpy(sizes).to(DEV)
    return stats


def _bits(stats):
    return [t.cpu().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32).copy()
            for t in (stats.carry, stats.accum, stats.smooth)]


@pytest.fixture(scope='module', params=CASES, ids=lambda c: f'T{c[0]}_N{c[1]}_P{c[2]}')
def run(request):
    """three chained windows of one case, computed once: the inputs, what the GPU gave after each window, and the same
    from the numpy restatement (one RefStats per member)"""
    T, N, population = request.param
    P = population or 1
    M = N // P
    sizes = _sizes(N, T + N)
    windows = [_window(T, N, 10 * N + w) for w in range(WINDOWS)]
    stats = _stats(N, sizes, population)
    refs = [RefStats(sizes[m * M:(m + 1) * M]) for m in range(P)]
    got, want = [], []
    for w in windows:
        table = stats.update(_device(w), per_step=True)
        assert table.shape == ((P, T, COLS) if population else (T, COLS)) and table.dtype == torch.float64
        got.append(dict(table=table.cpu().numpy().reshape(P, T, COLS), carry=stats.carry.cpu().numpy(),
                        accum=stats.accum.cpu().numpy(), smooth=stats.smooth.cpu().numpy()))
        tables = [r.update(*[w[k][:, m * M:(m + 1) * M] for k in ('rewards', 'dones', 'edge_collision', 'self_collision',
                                                                   'probs')]) for m, r in enumerate(refs)]
        want.append(dict(table=np.stack(tables), ret=np.concatenate([r.ret for r in refs]),
                         length=np.concatenate([r.length for r in refs]), size=np.concatenate([r.size for r in refs]),
                         accum=np.stack([r.accum.copy() for r in refs]), smooth=np.stack([r.smooth.copy() for r in refs])))
    return types.SimpleNamespace(T=T, N=N, P=P, M=M, population=population, sizes=sizes, windows=windows, got=got,
                                 want=want)


def test_exact_columns(run):
    """integer sums: the table, the carry after every window and the accumulator after three of them, with =="""
    exact = [k for k in range(12) if k != 6]
    for got, want in zip(run.got, run.want):
        assert np.array_equal(got['table'][..., :5], want['table'][..., :5])
        assert np.array_equal(got['carry'][0].view(np.float32), want['ret'].astype(np.float32))
        assert np.array_equal(got['carry'][1], want['length']) and np.array_equal(got['carry'][2], want['size'])
        assert np.array_equal(got['accum'][:, exact], want['accum'][:, exact])
    if run.N > 1:  # (one env at rate 0.2 may not have finished an episode in three steps)
        assert run.want[-1]['accum'][:, 1].sum() > 0


def test_smoother_of_the_exact_columns(run):
    for got, want in zip(run.got, run.want):
        np.testing.assert_allclose(got['smooth'][:, :5], want['smooth'][:, :5], rtol=1e-12, atol=0)


def test_entropy(run):
    worst = 0.0
    for got, want in zip(run.got, run.want):
        err = np.abs(got['table'][..., 5] - want['table'][..., 5]) / run.M  # of the per-step mean
        worst = max(worst, float(err.max()))
        assert abs(got['accum'][:, 6] - want['accum'][:, 6]).max() / (run.T * run.M * WINDOWS) <= ENTROPY_ATOL
        assert abs(got['smooth'][:, 5] - want['smooth'][:, 5]).max() <= ENTROPY_ATOL
    print(f'max |mean entropy - float64| = {worst:.3e}')
    assert worst <= ENTROPY_ATOL
    # the clamp was met: a one-hot row has the entropy of the clamp, not nan and not 0
    one_hot = torch.zeros((1, run.N, 4), device=DEV)
    one_hot[..., 1] = 1.0
    w = _device(_window(1, run.N, 0))
    w['probs'] = one_hot
    table = _stats(run.N, run.sizes).update(w, per_step=True)
    # (logf within 3 ulp and the product's rounding: 4 * 6e-8 of the value)
    assert float(table[0, 5]) == pytest.approx(run.N * float(entropy64(np.array([0, 1, 0, 0], np.float32))), rel=1e-6)
    assert float(table[0, 5]) > 0


def test_two_runs_have_the_same_bits(run):
    again = _stats(run.N, run.sizes, run.population)
    for w, got in zip(run.windows, run.got):
        table = again.update(_device(w), per_step=True).cpu().numpy().reshape(run.P, run.T, COLS)
        assert np.array_equal(table.view(np.int64), got['table'].view(np.int64))
        assert np.array_equal(again.accum.cpu().numpy().view(np.int64), got['accum'].view(np.int64))
        assert np.array_equal(again.smooth.cpu().numpy().view(np.int64), got['smooth'].view(np.int64))
    # and without the table (it then lives in the workspace)
    plain = _stats(run.N, run.sizes, run.population)
    for w in run.windows:
        assert plain.update(_device(w)) is None
    assert all(np.array_equal(a, b) for a, b in zip(_bits(plain), _bits(again)))


@pytest.mark.parametrize('run', [c for c in CASES if c[2]], ids=lambda c: f'T{c[0]}_N{c[1]}_P{c[2]}', indirect=True)
def test_member_equals_stand_alone(run):
    M = run.M
    for m in range(run.P):
        cols = slice(m * M, (m + 1) * M)
        alone = _stats(M, run.sizes[cols])
        for w, got in zip(run.windows, run.got):
            table = alone.update(_device(w, cols), per_step=True).cpu().numpy()
            assert np.array_equal(table.view(np.int64), got['table'][m].view(np.int64))
            assert np.array_equal(alone.carry.cpu().numpy(), got['carry'][:, cols])
            assert np.array_equal(alone.accum.cpu().numpy().view(np.int64)[0], got['accum'].view(np.int64)[m])
            assert np.array_equal(alone.smooth.cpu().numpy().view(np.int64)[0], got['smooth'].view(np.int64)[m])


def test_gridworld_columns_stay_zero():
    T, N = 5, 65
    w = _window(T, N, 3)
    del w['self_collision']
    stats = _stats(N, np.zeros(N, np.int32), snake=False)
    assert stats.initial_size == 0 and not stats.size.any()
    no_probs = {k: v for k, v in _device(w).items() if k != 'probs'}
    table = stats.update(no_probs, per_step=True).cpu().numpy()
    ref = RefStats(np.zeros(N, np.int64), initial_size=0)
    want = ref.update(w['rewards'], w['dones'], w['edge_collision'])
    assert np.array_equal(table[:, :3], want[:, :3]) and not table[:, 3:].any()
    accum = stats.accum.cpu().numpy()[0]
    assert np.array_equal(accum[[0, 1, 2, 3, 7, 8, 10]], ref.accum[[0, 1, 2, 3, 7, 8, 10]]) and ref.accum[1] > 0
    assert accum[4] == 0 and accum[5] == 0 and accum[9] == 0 and accum[11] == 0 and not stats.size.any()


def test_read_and_state_dict():
    T, N = 5, 64
    sizes, first, second = _sizes(N, 7), _window(T, N, 21), _window(T, N, 22)
    stats, ref = _stats(N, sizes, alpha=0.1), RefStats(sizes, alpha=0.1)
    stats.update(_device(first))
    ref.update(*[first[k] for k in ('rewards', 'dones', 'edge_collision', 'self_collision', 'probs')])
    carry, smooth = stats.carry.clone(), stats.smooth.clone()
    kept = stats.read(reset=False)
    row = stats.read()
    assert kept == row
    steps, episodes = T * N, int(ref.accum[1])
    assert row['steps'] == steps and row['episodes'] == episodes and episodes > 0
    for k, name in enumerate(('done_rate', 'reward_rate', 'edge_collisions', 'self_collisions', 'avg_size')):
        assert row[name] == ref.accum[1 + k] / steps and row['ewm_' + name] == pytest.approx(ref.smooth[k], rel=1e-12)
    assert row['policy_entropy'] == pytest.approx(ref.accum[6] / steps, abs=ENTROPY_ATOL)
    assert row['episode_return_mean'] == ref.accum[7] / episodes and row['episode_length_mean'] == ref.accum[8] / episodes
    assert row['episode_size_mean'] == ref.accum[9] / episodes
    assert row['episode_return_max'] == ref.accum[10] and row['episode_size_max'] == ref.accum[11]
    # the sums are gone, the carry and the smoother are not
    assert stats.accum[0, :10].tolist() == [0.0] * 10 and stats.accum[0, 10:].tolist() == [-np.inf] * 2
    assert torch.equal(stats.carry, carry) and torch.equal(stats.smooth, smooth)
    empty = stats.read()
    assert empty['steps'] == 0 and np.isnan(empty['episode_return_mean']) and np.isnan(empty['episode_size_max'])
    assert empty['ewm_avg_size'] == row['ewm_avg_size']
    # a resumed run continues the curves
    resumed = _stats(N, np.zeros(N, np.int32), alpha=0.1)
    resumed.load_state_dict({k: v.cpu().to(DEV) for k, v in stats.state_dict().items()})
    stats.update(_device(second))
    resumed.update(_device(second))
    assert all(np.array_equal(a, b) for a, b in zip(_bits(stats), _bits(resumed)))
    assert stats.read() == resumed.read()


def _chained(env, E, snake):
    from wurm_amd.agents import FeedforwardAgent, pack_policy_params
    from wurm_amd.constants import BODY_CHANNEL
    torch.manual_seed(5)
    params = pack_policy_params(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)).to(DEV)
    state = env.reset()
    stats = RolloutStats(env)
    dones = rewards = edge = 0
    for _ in range(10):
        out = env.policy_rollout(params, state, 20)
        state = out['state']
        stats.update(out)
        if snake:  # the carry is the env's own snake length at every window boundary (main.py:273)
            assert torch.equal(stats.size, env.envs[:, BODY_CHANNEL].flatten(1).amax(1).to(torch.int32))
        dones += int(out['dones'].sum())
        rewards += float(out['rewards'].sum(dtype=torch.float64))
        edge += int(out['edge_collision'].sum())
    accum = stats.accum[0].tolist()
    row = stats.read()
    assert row['steps'] == 200 * env.num_envs and row['episodes'] == dones and dones > 0
    assert accum[2] == rewards and accum[3] == edge
    return accum, row


def test_chained_windows_of_a_snake_env():
    from wurm_amd.envs import SingleSnake
    env = SingleSnake(num_envs=64, size=9, observation_mode='partial_2', device=DEV, seed=11)
    accum, row = _chained(env, 75, snake=True)
    # every finished snake was 3 long at its reset and grew by one per reward of ITS episode
    assert 0 <= accum[9] - 3 * accum[1] <= accum[2]
    assert accum[9] - 3 * accum[1] == accum[7]  # ... which is the episodes' return, as long as episodes start at a reset
    assert row['avg_size'] >= 3 and row['episode_size_max'] >= 3 and 0 < row['policy_entropy'] <= np.log(4) + 1e-6


def test_chained_windows_of_a_gridworld():
    from wurm_amd.envs import SimpleGridworld
    env = SimpleGridworld(num_envs=64, size=5, observation_mode='positions', start_location=(2, 2), device=DEV, seed=11)
    accum, row = _chained(env, 4, snake=False)
    assert row['self_collisions'] == 0 and row['avg_size'] == 0 and row['episode_length_mean'] >= 1
