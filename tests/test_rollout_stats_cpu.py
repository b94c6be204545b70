"""Rollout statistics without a GPU: what the C ABI refuses before any HIP call, the workspace query, the Python argument
errors, and the numpy restatement the GPU tests compare with (tests/rollout_stats_ref.py) against a literal per-step
loop of the reference's logging (experiments/main.py:252-274) on a hand-written case."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from tests.rollout_stats_ref import RefStats
from wurm_amd import _lib
from wurm_amd.rl import RolloutStats

I64 = ctypes.c_int64
F64 = ctypes.c_double
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    N, T, P = 12, 3, 2
    nbytes = lib.wurm_rollout_stats_workspace_bytes(N, T, P)
    assert nbytes > 0
    buf = (ctypes.c_float * 32)()
    p = (ctypes.addressof(buf) + 15) & ~15  # non-null and 16-byte aligned: every call below is refused before it is read

    def call(rewards=p, dones=p, edge=p, selfc=p, probs=p, carry=p, accum=p, smooth=p, table=p, ws=p, ws_bytes=nbytes,
             n=N, t=T, members=P, alpha=0.025):
        return lib.wurm_rollout_stats(rewards, dones, edge, selfc, probs, carry, accum, smooth, table, ws, I64(ws_bytes),
                                      I64(n), I64(t), I64(members), 3, F64(alpha), None)

    for name in ('rewards', 'dones', 'edge', 'carry', 'accum', 'smooth', 'ws'):
        assert call(**{name: None}) == INV, name
    assert call(n=0) == INV and call(n=-12) == INV and call(t=0) == INV and call(t=-1) == INV
    assert call(members=0) == INV and call(members=-2) == INV and call(members=5) == INV  # 12 % 5
    for alpha in (-0.1, 1.5, float('nan'), float('inf')):
        assert call(alpha=alpha) == INV
    assert call(n=65536 * 2, members=65536) == UNS
    assert call(ws_bytes=nbytes - 1) == INV and call(ws_bytes=0) == INV and call(ws_bytes=-1) == INV
    assert call(ws_bytes=lib.wurm_rollout_stats_workspace_bytes(N // P, T, 1)) == INV  # one member's is not two members'
    assert call(ws=p + 8) == INV                                                       # misaligned


def test_workspace_query():
    q = _lib.lib().wurm_rollout_stats_workspace_bytes
    assert q(0, 5, 1) == 0 and q(-3, 5, 1) == 0 and q(8, 0, 1) == 0 and q(8, 5, 0) == 0 and q(9, 5, 2) == 0
    assert q(65536 * 2, 5, 65536) == 0
    assert q(1, 1, 1) > 0 and q(1, 1, 1) % 8 == 0
    envs, steps = (1, 64, 65, 256, 257, 700, 100000), (1, 5, 7, 20, 1000)
    for T in steps:
        sizes = [q(N, T, 1) for N in envs]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    for N in envs:
        sizes = [q(N, T, 1) for T in steps]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert q(700, 3, 7) == 7 * q(100, 3, 1)


def _env(num_envs=4, snake=True):
    """an env object without a device: what RolloutStats reads of it"""
    env = types.SimpleNamespace(num_envs=num_envs, device=torch.device('cpu'))
    if snake:
        env.initial_snake_length = 3
        env.envs = torch.zeros(num_envs, 3, 9, 9)
        env.envs[:, 2, 4, 3:6] = torch.tensor([1.0, 2.0, 3.0])
        env.envs[1, 2, 5, 5] = 4.0
    return env


def _out(T=2, N=4):
    return {'rewards': torch.zeros(T, N), 'dones': torch.zeros(T, N, dtype=torch.bool),
            'edge_collision': torch.zeros(T, N, dtype=torch.bool), 'self_collision': torch.zeros(T, N, dtype=torch.bool),
            'probs': torch.full((T, N, 4), 0.25)}


def test_constructor():
    stats = RolloutStats(_env())
    assert stats.size.tolist() == [3, 4, 3, 3] and stats.size.dtype == torch.int32
    assert not stats.episode_return.any() and stats.episode_return.dtype == torch.float32 and not stats.episode_length.any()
    assert stats.accum.shape == (1, 12) and stats.accum.dtype == torch.float64
    assert stats.accum[0, :10].tolist() == [0.0] * 10 and stats.accum[0, 10:].tolist() == [-math.inf] * 2
    assert stats.smooth.shape == (1, 6) and stats.smooth.isnan().all()
    grid = RolloutStats(_env(6, snake=False), population=3)
    assert not grid.size.any() and grid.accum.shape == (3, 12) and grid.smooth.shape == (3, 6)
    for bad in (0, -1, 3):  # must divide 4
        with pytest.raises(RuntimeError):
            RolloutStats(_env(), population=bad)
    for bad in (-0.5, 1.01, float('nan')):
        with pytest.raises(RuntimeError):
            RolloutStats(_env(), alpha=bad)
    # nothing has been seen: the means are nan, not a division error
    row = stats.read()
    assert row['steps'] == 0 and row['episodes'] == 0
    assert all(math.isnan(row[k]) for k in ('reward_rate', 'avg_size', 'episode_return_mean', 'episode_size_max',
                                            'ewm_avg_size'))
    assert [r['steps'] for r in grid.read()] == [0, 0, 0]


def test_update_argument_errors_come_before_the_library(monkeypatch):
    def untouched(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', untouched)
    monkeypatch.setattr(_lib, 'call', untouched)
    stats = RolloutStats(_env())
    bad = [('rewards', torch.zeros(2, 5)), ('rewards', torch.zeros(8)), ('rewards', torch.zeros(0, 4)),
           ('rewards', torch.zeros(2, 4, dtype=torch.float64)), ('dones', torch.zeros(3, 4, dtype=torch.bool)),
           ('dones', torch.zeros(2, 4)), ('edge_collision', torch.zeros(2, 4, dtype=torch.int32)),
           ('self_collision', torch.zeros(2, 3, dtype=torch.bool)), ('probs', torch.zeros(2, 4, 3)),
           ('probs', torch.zeros(2, 4, 4, dtype=torch.float64))]
    for key, value in bad:
        out = _out()
        out[key] = value
        with pytest.raises(RuntimeError) as e:
            stats.update(out)
        assert not isinstance(e.value, _lib.WurmHipError), key
    with pytest.raises(RuntimeError):
        stats.load_state_dict({'carry': torch.zeros(3, 5, dtype=torch.int32), 'accum': stats.accum, 'smooth': stats.smooth})


def test_cpu_tensors_are_refused():
    for stats in (RolloutStats(_env()), RolloutStats(_env(snake=False), population=2)):
        with pytest.raises(_lib.WurmHipError):
            stats.update(_out())
        with pytest.raises(_lib.WurmHipError):
            stats.update(_out(), per_step=True)


class _Tracker(object):
    """the reference's smoother as its log loop uses it: keyword values in, the first one of a key initialises it"""

    def __init__(self, alpha):
        self.alpha, self.values = alpha, {}

    def __call__(self, **kw):
        for k, v in kw.items():
            self.values[k] = v if k not in self.values else self.alpha * v + (1 - self.alpha) * self.values[k]


def test_reference_restatement_on_a_hand_written_case():
    """3 steps, 2 envs, snakes of length 3 and 5 at the start; env 1 dies at step 1 (edge), env 0 eats at steps 0 and 2,
    env 1 at step 2.  The literal loop keeps the snakes' lengths as the env would (grow on eating, 3 after the reset)."""
    rewards = np.array([[1, 0], [0, 0], [1, 1]], np.float32)
    dones = np.array([[0, 0], [0, 1], [0, 0]], bool)
    edge = np.array([[0, 0], [0, 1], [0, 0]], bool)
    selfc = np.zeros((3, 2), bool)
    probs = np.array([[[.25, .25, .25, .25], [1, 0, 0, 0]]] * 3, np.float32)
    ln4, h_one = 1.3862943611198906, 1.1920929665620e-07  # -log(1 - 2^-23): a probability of 1 meets the clamp

    # main.py:252-274, one step at a time
    lengths, tracker, num_episodes, num_steps = [3, 5], _Tracker(0.5), 0, 0
    for t in range(3):
        for n in range(2):                       # env.step, then env.reset(done)
            lengths[n] += int(rewards[t, n] == 1)
            if dones[t, n]:
                lengths[n] = 3
        num_episodes += int(dones[t].sum())
        num_steps += 2
        tracker(reward_rate=float(rewards[t].mean()), edge_collisions=float(edge[t].mean()),
                self_collisions=float(selfc[t].mean()), avg_size=float(np.mean(lengths)))
    assert lengths == [5, 4] and num_episodes == 1 and num_steps == 6
    assert tracker.values == {'reward_rate': 0.625, 'edge_collisions': 0.125, 'self_collisions': 0.0, 'avg_size': 4.25}

    ref = RefStats([3, 5], initial_size=3, alpha=0.5)
    table = ref.update(rewards, dones, edge, selfc, probs)
    assert table[:, :5].tolist() == [[0, 1, 0, 0, 9], [1, 0, 1, 0, 7], [0, 2, 0, 0, 9]]
    assert table[:, 5] == pytest.approx([ln4 + h_one] * 3, rel=1e-12)
    assert ref.size.tolist() == lengths and ref.ret.tolist() == [2, 1] and ref.length.tolist() == [3, 1]
    # steps, dones, rewards, edge, self, sizes | the one finished episode: return 0, length 2, final size 5
    assert ref.accum[:6].tolist() == [num_steps, num_episodes, 3, 1, 0, 25]
    assert ref.accum[6] == pytest.approx(3 * (ln4 + h_one), rel=1e-12)
    assert ref.accum[7:].tolist() == [0, 2, 5, 0, 5]
    assert ref.smooth[:5].tolist() == [0.125, tracker.values['reward_rate'], tracker.values['edge_collisions'],
                                       tracker.values['self_collisions'], tracker.values['avg_size']]
    assert ref.smooth[5] == pytest.approx((ln4 + h_one) / 2, rel=1e-12)
    # a second window continues the episodes: env 0 dies having eaten once more (return 3, length 4, final size 6)
    ref.update(np.array([[1, 0]], np.float32), np.array([[1, 0]], bool), np.zeros((1, 2), bool), np.array([[1, 0]], bool))
    assert ref.accum[:6].tolist() == [8, 2, 4, 1, 1, 25 + 3 + 4]
    assert ref.accum[7:].tolist() == [3, 6, 11, 3, 6]
    assert ref.size.tolist() == [3, 4] and ref.ret.tolist() == [0, 1] and ref.length.tolist() == [0, 2]
    ref.reset()
    assert ref.accum[:10].tolist() == [0] * 10 and ref.accum[10:].tolist() == [-np.inf] * 2 and ref.smooth[4] == 3.875
