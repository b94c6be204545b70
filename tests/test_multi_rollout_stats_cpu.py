"""MultiSnake training statistics without a GPU: the numpy restatement the GPU tests compare with
(tests/multi_rollout_stats_ref.py) against hand-computed tiny cases and a literal loop of the reference's log lines
(experiments/multiagent.py:491-505), what the C ABI refuses before any HIP call, the workspace query and the Python
argument errors."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from tests.multi_rollout_stats_ref import RefMultiStats
from wurm_amd import _lib
from wurm_amd.rl import MultiRolloutStats

I64 = ctypes.c_int64
F64 = ctypes.c_double
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
LN4 = 1.3862943611198906


def test_symbols_are_declared():
    assert 'wurm_multi_rollout_stats_workspace_bytes' in _lib.SYMBOLS and 'wurm_multi_rollout_stats' in _lib.SYMBOLS
    lib = _lib.lib()
    assert lib.wurm_multi_rollout_stats.restype is ctypes.c_int and len(lib.wurm_multi_rollout_stats.argtypes) == 20
    assert lib.wurm_multi_rollout_stats.argtypes[-6:] == [I64, I64, I64, I64, F64, ctypes.c_void_p]
    assert lib.wurm_multi_rollout_stats_workspace_bytes.restype is I64
    assert lib.wurm_multi_rollout_stats_workspace_bytes.argtypes == [I64, I64, I64]


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    N, K, T = 12, 2, 3
    nbytes = lib.wurm_multi_rollout_stats_workspace_bytes(N, K, T)
    assert nbytes > 0
    buf = (ctypes.c_float * 32)()
    p = (ctypes.addressof(buf) + 15) & ~15  # non-null and 16-byte aligned: every call below is refused before it is read

    def call(rewards=p, food=p, size=p, dones=p, boost=p, snake=p, edge=p, probs=p, all_done=p, carry=p, accum=p, smooth=p,
             table=p, ws=p, ws_bytes=nbytes, n=N, k=K, t=T, alpha=0.025):
        return lib.wurm_multi_rollout_stats(rewards, food, size, dones, boost, snake, edge, probs, all_done, carry, accum,
                                            smooth, table, ws, I64(ws_bytes), I64(n), I64(k), I64(t), F64(alpha), None)

    for name in ('rewards', 'food', 'size', 'dones', 'boost', 'snake', 'edge', 'carry', 'accum', 'smooth', 'ws'):
        assert call(**{name: None}) == INV, name
    assert call(n=0) == INV and call(n=-12) == INV and call(t=0) == INV and call(t=-1) == INV
    assert call(k=0) == INV and call(k=-2) == INV
    for alpha in (-0.1, 1.5, float('nan'), float('inf')):
        assert call(alpha=alpha) == INV
    assert call(k=65536) == UNS
    assert call(ws_bytes=nbytes - 1) == INV and call(ws_bytes=0) == INV and call(ws_bytes=-1) == INV
    assert call(ws_bytes=lib.wurm_multi_rollout_stats_workspace_bytes(N, 1, T)) == INV  # one agent's is not two agents'
    assert call(ws=p + 8) == INV and call(probs=p + 4) == INV                           # misaligned


def test_workspace_query():
    q = _lib.lib().wurm_multi_rollout_stats_workspace_bytes
    assert q(0, 2, 5) == 0 and q(-3, 2, 5) == 0 and q(8, 0, 5) == 0 and q(8, -1, 5) == 0 and q(8, 2, 0) == 0
    assert q(8, 2, -1) == 0 and q(8, 65536, 5) == 0
    assert q(1, 1, 1) > 0 and q(1, 1, 1) % 16 == 0
    envs, steps = (1, 64, 65, 256, 257, 700, 100000), (1, 5, 7, 20, 1000)
    for T in steps:
        sizes = [q(N, 1, T) for N in envs]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    for N in envs:
        sizes = [q(N, 1, T) for T in steps]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert q(700, 7, 3) == 7 * q(700, 1, 3)
    # 10 T + 5 doubles per wave, four waves per 256 envs, and the (T, 10) table
    assert q(257, 1, 3) == 8 * (2 * 4 * 35 + 30)


def _env(num_envs=4, num_snakes=2):
    """an env object without a device: what MultiRolloutStats reads of it"""
    return types.SimpleNamespace(num_envs=num_envs, num_snakes=num_snakes, device=torch.device('cpu'))


def _out(T=2, N=4, K=2, lead=None):
    shape = (T, K * N) if lead is None else (T, K, N)
    flag = lambda: torch.zeros(shape, dtype=torch.bool)
    out = {'rewards': torch.zeros(shape), 'food': torch.zeros(shape), 'size': torch.full(shape, 3.0), 'dones': flag(),
           'boost': flag(), 'snake_collision': flag(), 'edge_collision': flag(),
           'all_done': torch.zeros((T, N), dtype=torch.bool)}
    if lead is None:
        out['probs'] = torch.full(shape + (4,), 0.25)
    return out


def test_constructor_and_empty_read():
    stats = MultiRolloutStats(_env())
    assert stats.carry.shape == (2, 8) and stats.carry.dtype == torch.int32 and not stats.carry.any()
    assert stats.life_return.dtype == torch.float32 and stats.life_length.dtype == torch.int32
    assert stats.accum.shape == (2, 16) and stats.accum.dtype == torch.float64
    assert stats.accum[0].tolist() == [0.0] * 13 + [-math.inf] * 2 + [0.0]
    assert stats.smooth.shape == (2, 9) and stats.smooth.isnan().all()
    for bad in (-0.5, 1.01, float('nan')):
        with pytest.raises(RuntimeError):
            MultiRolloutStats(_env(), alpha=bad)
    with pytest.raises(RuntimeError):
        MultiRolloutStats(_env(num_snakes=0))
    rows = stats.read()
    assert len(rows) == 2 and rows[0]['steps'] == 0 and rows[0]['episodes'] == 0
    assert all(math.isnan(rows[1][k]) for k in ('reward', 'size', 'done', 'return', 'life_return_mean',
                                                'size_at_death_max', 'life_return_max', 'ewm_reward'))
    species = stats.read(num_species=1)
    assert len(species) == 1 and species[0]['steps'] == 0 and 'ewm_reward' not in species[0]
    for bad in (0, 3):
        with pytest.raises(RuntimeError):
            stats.read(num_species=bad)


def test_read_divides_the_sums():
    stats = MultiRolloutStats(_env(num_envs=4, num_snakes=3))
    #            steps alive done rew  H    food boost size edge snake size_d ret  len  maxs maxr episodes
    stats.accum[0] = torch.tensor([40., 30., 10., 15., 33., 6., 3., 120., 4., 5., 70., 20., 50., 9., 4., 2.])
    stats.accum[1] = torch.tensor([40., 40., 0., 10., 44., 8., 0., 160., 0., 0., 0., 0., 0., -math.inf, -math.inf, 2.])
    stats.accum[2] = torch.tensor([40., 20., 20., 5., 22., 2., 1., 60., 10., 10., 100., 10., 60., 7., 2.5, 2.])
    stats.smooth[0] = torch.arange(9, dtype=torch.float64)
    kept = stats.read(reset=False)
    a, b, c = stats.read(reset=False)
    assert kept[0] == a  # (reset=False left the sums; the other rows have nans, looked at below)
    assert a == dict(steps=40, episodes=2, reward=0.5, policy_entropy=1.1, food=0.2, edge_collisions=0.1,
                     snake_collisions=0.125, boost=0.1, size=4.0, done=0.25, **{'return': 7.0}, life_return_mean=2.0,
                     life_length_mean=5.0, size_at_death_max=9.0, life_return_max=4.0,
                     **{'ewm_' + n: float(i) for i, n in enumerate(('reward', 'policy_entropy', 'food', 'edge_collisions',
                                                                    'snake_collisions', 'boost', 'size', 'done',
                                                                    'return'))})
    # an agent that never died: the columns over the done mask are nan, the others are not
    assert b['reward'] == 0.25 and b['done'] == 0.0 and math.isnan(b['return']) and math.isnan(b['life_return_mean'])
    assert math.isnan(b['size_at_death_max']) and math.isnan(b['life_return_max']) and math.isnan(b['ewm_reward'])
    # species: snakes {0, 1} and {2} for two of them (k * P // K), all three for one; sums are added BEFORE dividing
    s0, s1 = stats.read(reset=False, num_species=2)
    assert s0['steps'] == 80 and s0['episodes'] == 2 and s0['reward'] == 25 / 70 and s0['size'] == 4.0
    assert s0['done'] == 10 / 80 and s0['return'] == 7.0 and s0['size_at_death_max'] == 9.0 and 'ewm_size' not in s0
    assert s1 == {k: v for k, v in c.items() if not k.startswith('ewm_')}
    (every,) = stats.read(num_species=1)
    assert every['steps'] == 120 and every['return'] == 170 / 30 and every['life_return_max'] == 4.0
    assert every['life_length_mean'] == 110 / 30
    # the read cleared the sums, not the smoother
    assert stats.accum[2].tolist() == [0.0] * 13 + [-math.inf] * 2 + [0.0] and stats.smooth[0, 3] == 3.0


def test_update_argument_errors_come_before_the_library(monkeypatch):
    def untouched(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', untouched)
    monkeypatch.setattr(_lib, 'call', untouched)
    stats = MultiRolloutStats(_env())
    bad = [('rewards', torch.zeros(2, 9)), ('rewards', torch.zeros(8)), ('rewards', torch.zeros(0, 8)),
           ('rewards', torch.zeros(2, 8, dtype=torch.float64)), ('rewards', torch.zeros(2, 8, dtype=torch.half)),
           ('food', torch.zeros(2, 8, dtype=torch.half)), ('size', torch.zeros(2, 8, dtype=torch.half)),
           ('size', torch.zeros(2, 2, 4)), ('food', torch.zeros(3, 8)), ('dones', torch.zeros(3, 8, dtype=torch.bool)),
           ('dones', torch.zeros(2, 8)), ('boost', torch.zeros(2, 8, dtype=torch.int32)),
           ('snake_collision', torch.zeros(2, 7, dtype=torch.bool)), ('edge_collision', torch.zeros(2, 8)),
           ('probs', torch.zeros(2, 8, 3)), ('probs', torch.zeros(2, 8, 4, dtype=torch.float64)),
           ('probs', torch.zeros(2, 8, 4, dtype=torch.half)), ('all_done', torch.zeros(2, 8, dtype=torch.bool)),
           ('all_done', torch.zeros(2, 4)), ('size', [1, 2])]
    for key, value in bad:
        out = _out()
        out[key] = value
        with pytest.raises(RuntimeError) as e:
            stats.update(out)
        assert not isinstance(e.value, _lib.WurmHipError), key
        assert key in str(e.value), (key, str(e.value))
    # a window without the info keys: the message says how to get them
    for key in ('food', 'size', 'boost', 'snake_collision', 'edge_collision'):
        out = _out()
        del out[key]
        with pytest.raises(RuntimeError) as e:
            stats.update(out)
        assert key in str(e.value) and 'info=True' in str(e.value)
    out = _out()
    del out['dones']
    with pytest.raises(RuntimeError) as e:
        stats.update(out)
    assert 'dones' in str(e.value) and 'info=True' not in str(e.value)
    # the (T, K, N) form of MultiSnake.rollout is one form for every tensor of the window
    out = _out(lead=True)
    out['food'] = out['food'].reshape(2, 8)
    with pytest.raises(RuntimeError) as e:
        stats.update(out)
    assert 'food' in str(e.value)
    with pytest.raises(RuntimeError):
        stats.load_state_dict({'carry': torch.zeros(3, 8, dtype=torch.int32), 'accum': stats.accum, 'smooth': stats.smooth})
    with pytest.raises(RuntimeError):
        stats.load_state_dict({'carry': stats.carry, 'accum': stats.accum.float(), 'smooth': stats.smooth})


def test_cpu_tensors_are_refused():
    stats = MultiRolloutStats(_env())
    for out in (_out(), _out(lead=True)):
        with pytest.raises(_lib.WurmHipError):
            stats.update(out)
        with pytest.raises(_lib.WurmHipError):
            stats.update(out, per_step=True)


class _Tracker(object):
    """the reference's smoother as its log loop uses it, with this build's one deviation: a NaN value (the mean over an
    empty mask) is skipped instead of being folded in"""

    def __init__(self, alpha):
        self.alpha, self.values = alpha, {}

    def __call__(self, **kw):
        for k, v in kw.items():
            if not math.isnan(v):
                self.values[k] = v if k not in self.values else self.alpha * v + (1 - self.alpha) * self.values[k]


def _mean(x):
    return float(np.mean(np.asarray(x, np.float64))) if len(x) else math.nan  # (.mean() of an empty selection: nan)


def test_reference_restatement_on_a_hand_written_case():
    """One agent, 3 envs, 4 steps: nobody is done at step 0 (the `return` mask is empty), everybody at step 1 (the `~done`
    masks are empty), env 1 stays dead at step 2, env 2 dies at step 3."""
    rewards = np.array([[1, 0, -1], [-1, -1, 0.5], [0, 0, 1], [1, 0, -1]], np.float32)
    dones = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 0], [0, 0, 1]], bool)
    food = np.array([[1, 0, 0], [0, 0, 1], [0, 0, 1], [1, 0, 0]], np.float32)
    size = np.array([[4, 3, 3], [4, 3, 6], [3, 0, 4], [4, 3, 5]], np.float32)
    boost = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 1], [0, 0, 1]], bool)
    snake = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1]], bool)
    edge = np.array([[0, 0, 0], [0, 1, 1], [0, 0, 0], [0, 0, 0]], bool)
    probs = np.full((4, 3, 4), 0.25, np.float32)
    all_done = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0]], bool)

    # multiagent.py:470, 493-502, one step at a time
    tracker, episodes = _Tracker(0.5), 0
    for t in range(4):
        d = dones[t]
        episodes += int(all_done[t].sum())
        tracker(reward=_mean(rewards[t][~d]), policy_entropy=_mean(np.full(3, LN4)[~d]), food=_mean(food[t][~d]),
                edge_collisions=_mean(edge[t].astype(float)), snake_collisions=_mean(snake[t].astype(float)),
                boost=_mean(boost[t][~d].astype(float)), size=_mean(size[t][~d]), done=_mean(d.astype(float)),
                **{'return': _mean(size[t][d])})
    assert tracker.values['reward'] == 0.5 * 0.5 + 0.5 * (0.5 * 0.5 + 0.5 * 0.0)        # steps 0, 2, 3: step 1 skipped
    assert tracker.values['return'] == 0.5 * 5.0 + 0.5 * (0.5 * 0.0 + 0.5 * (13 / 3))   # steps 1, 2, 3: step 0 skipped

    ref = RefMultiStats(3, alpha=0.5)
    table = ref.update(rewards, food, size, dones, boost, snake, edge, probs, all_done)
    #                           alive done rew  H  food boost size edge snake size_done
    assert table[:, [0, 1, 2, 4, 5, 6, 7, 8, 9]].tolist() == [[3, 0, 0.0, 1, 1, 10, 0, 0, 0],
                                                             [0, 3, 0.0, 0, 0, 0, 2, 1, 13],      # the all-done step
                                                             [2, 1, 1.0, 1, 1, 7, 0, 0, 0],
                                                             [2, 1, 1.0, 1, 0, 7, 0, 1, 5]]
    assert table[:, 3] == pytest.approx([3 * LN4, 0, 2 * LN4, 2 * LN4], rel=1e-12)
    names = ('reward', 'policy_entropy', 'food', 'edge_collisions', 'snake_collisions', 'boost', 'size', 'done', 'return')
    assert ref.smooth.tolist() == pytest.approx([tracker.values[n] for n in names], rel=1e-12)
    # lives: all three die at step 1 (returns 0, -1, -0.5; length 2), env 1 again at step 2 (0; 1), env 2 at step 3 (0; 2)
    assert ref.accum[0] == 12 and ref.accum[1:3].tolist() == [7, 5] and ref.accum[3] == 2.0
    assert ref.accum[5:11].tolist() == [3, 2, 24, 2, 2, 18]
    assert ref.accum[11:].tolist() == [-1.5, 9, 6, 0, episodes] and episodes == 3
    assert ref.ret.tolist() == [1, 0, 0] and ref.length.tolist() == [2, 1, 0]
    # a second window without a death or a mask: the life goes on, `return` keeps its value, episodes its count
    before = ref.smooth.copy()
    ref.update(rewards[:1], food[:1], size[:1], dones[:1], boost[:1], snake[:1], edge[:1])
    assert ref.ret.tolist() == [2, 0, -1] and ref.length.tolist() == [3, 2, 1]
    assert ref.smooth[8] == before[8] and ref.smooth[0] == 0.5 * 0.0 + 0.5 * before[0] and ref.smooth[1] == 0.5 * before[1]
    assert ref.accum[15] == 3 and ref.accum[11:15].tolist() == [-1.5, 9, 6, 0]
    ref.reset()
    assert ref.accum.tolist() == [0.0] * 13 + [-np.inf] * 2 + [0.0] and ref.smooth[8] == before[8]


def test_smoother_stays_nan_until_its_mask_holds():
    ref = RefMultiStats(2, alpha=0.1)
    z, f = np.zeros((3, 2), np.float32), np.zeros((3, 2), bool)
    ref.update(z + 1, z, z + 3, f, f, f, f)
    assert np.isnan(ref.smooth[8]) and ref.smooth[0] == 1.0 and ref.smooth[6] == 3.0 and ref.smooth[7] == 0.0
    assert ref.accum[13] == -np.inf and ref.accum[14] == -np.inf and ref.accum[2] == 0
