"""What of MultiSnake's frame recording can be checked without a GPU: the C ABI's refusals, the Python refusals that come
before any tensor is touched, the tiling of int16 frames, the recorder over a stand-in env, and that the windows
tests/test_multi_frames_gpu.py counts events on are not quiet ones (on the CPU oracle alone)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import multi_frames_cases as C
from wurm_amd import _lib, _render
from wurm_amd.envs import _multi_frames

I64, U64 = ctypes.c_int64, ctypes.c_uint64
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
POINTERS = ('foods', 'heads', 'bodies', 'dones', 'orientations', 'colours', 'boost', 'select', 'actions', 'frames',
            'final_foods', 'final_heads', 'final_bodies', 'final_dones', 'final_orientations', 'final_colours',
            'final_boost', 'status')


def _call(lib, cfg, p, k=4, n=65, K=4, S=12, T=5, **ptrs):
    a = [ptrs.get(name, p) for name in POINTERS]
    return lib.wurm_multi_rollout_frames(*a, I64(k), I64(n), K, S, I64(T), cfg, U64(1), U64(1), I64(0), None)


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)  # non-null and 8-byte aligned: every call below is refused before anything is read or launched
    cfg = ctypes.byref(_lib.multi_config(4, True, 0.5, 0.5, 'only_one', 5e-4, -1, 'all', 'random'))
    call = lambda **kw: _call(lib, kw.pop('cfg', cfg), p, **kw)
    for name in POINTERS:
        assert call(**{name: None}) == INV, name
    assert call(cfg=None) == INV
    assert call(k=0) == INV and call(k=-3) == INV and call(T=-1) == INV and call(n=0) == INV and call(n=-65) == INV
    assert call(K=0) == INV and call(K=-1) == INV and call(S=2) == INV
    # a pointer that is not aligned to its element
    for name in ('foods', 'heads', 'bodies', 'final_foods', 'final_heads', 'final_bodies'):
        assert call(**{name: p + 2}) == INV, name
    for name in ('orientations', 'final_orientations', 'select', 'actions'):
        assert call(**{name: p + 4}) == INV, name
    for name in ('colours', 'final_colours', 'frames'):
        assert call(**{name: p + 1}) == INV, name
    # outside what wurm_multi_rollout serves
    assert call(K=65) == UNS and call(S=65) == UNS and call(S=200) == UNS and call(S=4) == UNS and call(S=3) == UNS
    assert call(K=64, S=64) == UNS           # 2 K S^2 bytes of body grids alone: 512 KB of LDS
    assert call(k=1 << 31) == UNS


def test_symbol_is_declared():
    assert 'wurm_multi_rollout_frames' in _lib.SYMBOLS
    assert len(_lib.lib().wurm_multi_rollout_frames.argtypes) == 28


def _stand_in(device='cpu'):
    """what record_start / record_frames read of an env before they touch a tensor of it"""
    return types.SimpleNamespace(device=torch.device(device), num_envs=8, num_snakes=2, size=12, seed=1, env_offset=0)


def test_record_start_refuses_an_empty_select():
    for empty in ([], torch.zeros(0, dtype=torch.long), np.zeros((0,), np.int64)):
        with pytest.raises(RuntimeError, match='empty'):
            _multi_frames.record_start(_stand_in(), empty)


def test_record_frames_refuses_foreign_records_and_wrong_actions():
    env, other = _stand_in(), _stand_in()
    rec = object.__new__(_multi_frames.MultiFrameRecord)
    rec.owner = lambda: other
    good = torch.zeros((3, 2, 8), dtype=torch.long)
    with pytest.raises(RuntimeError, match='another env object'):
        _multi_frames.record_frames(env, rec, good)
    with pytest.raises(RuntimeError, match='another env object'):
        _multi_frames.record_frames(env, object(), good)
    rec.owner = lambda: env
    bad = [good.int(),                                    # dtype
           good.float(),
           torch.zeros((3, 2, 7), dtype=torch.long),      # shape: another batch
           torch.zeros((3, 15), dtype=torch.long),        # (T, K N) with the wrong K N
           torch.zeros((3, 8, 2), dtype=torch.long),      # (T, N, K)
           torch.zeros((16,), dtype=torch.long),
           torch.zeros((3, 2, 16), dtype=torch.long)[:, :, ::2],  # not contiguous
           good.numpy()]
    for a in bad:
        with pytest.raises(RuntimeError, match='actions must be'):
            _multi_frames.record_frames(env, rec, a)
    # another device than the env's
    on_gpu = _stand_in('cuda:0')
    rec.owner = lambda: on_gpu
    with pytest.raises(RuntimeError, match='actions must be'):
        _multi_frames.record_frames(on_gpu, rec, good)


def _hand_made(k, S, T=None):
    """an int16 clip with what _get_env_images() can hold: 0 .. 255 and, where food lies under a snake, a little more"""
    rs = np.random.RandomState(k * 100 + S)
    shape = (k, 3, S, S) if T is None else (T, k, 3, S, S)
    return rs.randint(0, 447, size=shape).astype(np.int16)


@pytest.mark.parametrize('k,render_args', [(1, {'num_rows': 1, 'num_cols': 1, 'size': 64}),
                                           (4, {'num_rows': 2, 'num_cols': 2, 'size': 32}),
                                           (5, {'num_rows': 1, 'num_cols': 3, 'size': 16}),
                                           (3, None)])
def test_tile_frames_converts_int16_as_render_does(k, render_args):
    S, T = 7, 3
    args = _render.DEFAULT_RENDER_ARGS if render_args is None else render_args
    clip = _hand_made(k, S, T)
    got = _render.tile_frames(torch.from_numpy(clip), render_args)
    assert got.dtype == np.uint8 and got.shape == (T, args['size'] * args['num_rows'], args['size'] * args['num_cols'], 3)
    for t in range(T):  # (what MultiSnake.render('rgb_array') does with _get_env_images())
        assert np.array_equal(got[t], _render.frame(clip[t], k, args))
    assert np.array_equal(_render.tile_frames(clip[0], render_args), _render.frame(clip[0], k, args))


def test_window_recorder_takes_int16_frames(tmp_path):
    from wurm_amd.recording import VideoRecorder, WindowRecorder

    class Env(object):
        def record_start(self, select):
            return list(select)

        def record_frames(self, rec, actions):
            T = actions.shape[0]
            return dict(frames=torch.full((T + 1, 3, 3, 5, 5), 200, dtype=torch.short))

    path = str(tmp_path / 'clip.npy')
    wr = WindowRecorder(Env(), path, [0, 1, 2], tile_pixels=10)
    for window in range(2):
        wr.finish(wr.start(window), torch.zeros((4, 2 * 8), dtype=torch.long))
    wr.close()
    clip = np.load(path)
    assert clip.dtype == np.uint8 and clip.shape == (5 + 4, 20, 20, 3)
    assert (clip[:, 15:, 15:] == 0).all() and (clip[:, :5, :5] == 200).all()
    rec = VideoRecorder(None, str(tmp_path / 'direct.npy'))
    rec.capture_frames(_render.tile_frames(_hand_made(4, 9, 2), {'num_rows': 2, 'num_cols': 2, 'size': 18}))
    assert len(rec.frames) == 2 and rec.frames[0].dtype == np.uint8
    rec.close()


# ---------------------------------------------------------------------------------------------- the windows' seeds

def test_table_covers_what_the_kernel_can_take():
    cs = C.CASES.values()
    assert {(c.K, c.S, c.N) for c in cs} == {(2, 12, 64), (6, 10, 65), (4, 25, 33), (10, 36, 5)}
    assert {c.env_offset for c in cs} == {0, 1000}
    assert any(c.options.get('boost') is False for c in cs) and any('boost' not in c.options for c in cs)
    assert any(c.options.get('agent_colours') == 'fixed' for c in cs) and any('agent_colours' not in c.options for c in cs)
    assert C.TS['k2_s12'] == C.TS['crowded'] == (0, 1, 3, 70, 130) and C.TS['respawn'] == C.TS['k10_s36'] == (0, 1, 3)
    for c in cs:
        sel = C.select_of(c)
        assert 0 in sel and c.N - 1 in sel and sel != sorted(sel) and len(set(sel)) == len(sel) - 1
        a = C.tape(c, 130)
        assert a.min() == 0 and a.max() == 7


@pytest.mark.parametrize('name,T', C.EVENT_WINDOWS)
def test_event_windows_are_not_quiet(name, T):
    """The condition the GPU test puts on its twin, on the CPU oracle alone.  Observed over the selected envs
    (seed 4102) crowded, T = 130: 4 rebuilds, 9 meals, 10 boosted steps, 16 snake collisions (no single respawn: its
    respawn_mode is 'all'); (seed 4203) respawn, T = 130: 1 rebuild, 91 respawns, 80 meals, 151 boosted steps, 29 snake
    collisions."""
    case = C.CASES[name]
    ev = C.events(C.oracle_window(case, T), C.select_of(case))
    print(name, T, ev)
    for n in C.EVENT_NAMES:
        if n == 'respawn' and case.options.get('respawn_mode', 'all') != 'any':
            assert ev[n] == 0
        else:
            assert ev[n] >= 1, (n, ev)
