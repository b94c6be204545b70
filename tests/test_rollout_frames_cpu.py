"""What of the frame recording can be checked without a GPU: the C ABI's refusals, the tiling helper, the recorder's
capture_frames, and that the windows tests/test_rollout_frames_gpu.py replays show what they are meant to show (an
episode's end and a meal among the selected envs of every window of five steps or more) on the CPU oracle alone."""
import ctypes

import numpy as np
import pytest

from tests import rollout_frames_cases as C
from wurm_amd import _lib, _render
from wurm_amd.recording import VideoRecorder

I64, U64 = ctypes.c_int64, ctypes.c_uint64
INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)  # a non-null pointer: every call below is refused before anything is read or launched

    def single(start=p, select=p, actions=p, frames=p, final=p, status=p, k=4, n=65, size=9, t=5):
        return lib.wurm_single_rollout_frames(start, select, actions, frames, final, status, I64(k), I64(n), size, I64(t),
                                              U64(1), U64(1), I64(0), None)

    def grid(start=p, select=p, actions=p, frames=p, final=p, status=p, k=4, n=65, size=9, t=5, sy=3, sx=5):
        return lib.wurm_grid_rollout_frames(start, select, actions, frames, final, status, I64(k), I64(n), size, I64(t),
                                            sy, sx, U64(1), U64(1), I64(0), None)

    for fn in (single, grid):
        for name in ('start', 'select', 'actions', 'frames', 'final', 'status'):
            assert fn(**{name: None}) == INV, name
        assert fn(k=0) == INV and fn(k=-3) == INV and fn(t=-1) == INV and fn(n=0) == INV and fn(n=-65) == INV
        assert fn(size=2) == INV and fn(size=65) == UNS and fn(size=200) == UNS
        assert fn(k=1 << 31) == UNS
    assert single(size=8) == UNS and single(size=4) == UNS  # no snake can be rebuilt there (single_snake.py:346-347)
    assert grid(size=4) == UNS and grid(size=3) == UNS      # simple_gridworld.py:249-250
    assert grid(sy=-1) == UNS and grid(sx=9) == UNS and grid(sy=9) == UNS and grid(size=5, sy=3, sx=5) == UNS


def test_symbols_are_declared():
    assert {'wurm_single_rollout_frames', 'wurm_grid_rollout_frames'} <= set(_lib.SYMBOLS)
    lib = _lib.lib()
    assert len(lib.wurm_single_rollout_frames.argtypes) == 14 and len(lib.wurm_grid_rollout_frames.argtypes) == 16


def _hand_made(k, S, T=None):
    rs = np.random.RandomState(k * 100 + S)
    shape = (k, 3, S, S) if T is None else (T, k, 3, S, S)
    return rs.randint(0, 256, size=shape).astype(np.uint8)


@pytest.mark.parametrize('k,render_args', [(1, {'num_rows': 1, 'num_cols': 1, 'size': 64}),
                                           (4, {'num_rows': 2, 'num_cols': 2, 'size': 32}),
                                           (6, {'num_rows': 2, 'num_cols': 3, 'size': 20}),
                                           (5, {'num_rows': 1, 'num_cols': 3, 'size': 16}),
                                           (3, None)])
def test_tile_frames_is_render_for_k_envs(k, render_args):
    S, T = 7, 3
    args = _render.DEFAULT_RENDER_ARGS if render_args is None else render_args
    one = _hand_made(k, S)
    want = _render.frame(one.astype(np.int16), k, args)   # (what render('rgb_array') hands it: the int16 batch of _get_rgb)
    got = _render.tile_frames(one, render_args)
    assert got.dtype == np.uint8 and got.shape == (args['size'] * args['num_rows'], args['size'] * args['num_cols'], 3)
    assert np.array_equal(got, want)
    clip = _hand_made(k, S, T)
    got = _render.tile_frames(clip, render_args)
    assert got.shape == (T,) + want.shape
    for t in range(T):
        assert np.array_equal(got[t], _render.frame(clip[t].astype(np.int16), k, args))
    with pytest.raises(ValueError):
        _render.tile_frames(clip[0, 0])


def test_tile_frames_takes_tensors():
    import torch
    clip = _hand_made(4, 9, 2)
    args = {'num_rows': 2, 'num_cols': 2, 'size': 18}
    assert np.array_equal(_render.tile_frames(torch.from_numpy(clip), args), _render.tile_frames(clip, args))


def test_capture_frames_npy_round_trip(tmp_path):
    clip = _render.tile_frames(_hand_made(4, 9, 5), {'num_rows': 2, 'num_cols': 2, 'size': 18})
    path = str(tmp_path / 'sub' / 'clip.npy')
    rec = VideoRecorder(None, path)
    rec.capture_frames(clip[:2])
    rec.capture_frames(list(clip[2:]))
    assert len(rec.frames) == 5
    with pytest.raises(RuntimeError):
        rec.capture_frames(clip[0])       # one (H, W, 3) frame is not a sequence of frames
    rec.close()
    back = np.load(path)
    assert back.dtype == np.uint8 and np.array_equal(back, clip)
    rec.capture_frames(clip)              # closed: ignored, as capture_frame is
    assert rec.frames == []
    off = VideoRecorder(None, str(tmp_path / 'off.npy'), enabled=False)
    off.capture_frames(clip)
    off.close()
    assert not (tmp_path / 'off.npy').exists()


def test_capture_frames_gif(tmp_path):
    from PIL import Image
    clip = _render.tile_frames(_hand_made(1, 9, 4), {'num_rows': 1, 'num_cols': 1, 'size': 27})
    path = str(tmp_path / 'clip.gif')
    rec = VideoRecorder(None, path)
    rec.capture_frames(clip)
    rec.close()
    assert Image.open(path).n_frames == 4


# ---------------------------------------------------------------------------------------------- the windows' seeds

def test_table_covers_the_shapes():
    fams = {(w.family, w.S) for w in C.WINDOWS}
    assert {('snake', S) for S in (9, 11, 12, 36)} | {('grid', 5), ('grid', 9)} <= fams
    assert any(w.family == 'tape' for w in C.WINDOWS) and any(w.env_offset != 0 for w in C.WINDOWS)
    for fam, S in fams - {('tape', 9), ('tape', 12)}:
        assert {w.N for w in C.WINDOWS if (w.family, w.S) == (fam, S)} >= {65, 130}
    assert all(C.START[S] != (0, 0) for S in C.START)


@pytest.mark.parametrize('i', range(len(C.WINDOWS)), ids=[f'{w.family}-S{w.S}-N{w.N}-off{w.env_offset}' for w in C.WINDOWS])
def test_every_window_shows_an_episode_end_and_a_meal(i):
    """the event condition of the GPU test, on the CPU oracle alone: for every T >= 5 and every k, k = 1 (the last env by
    itself) included"""
    w = C.WINDOWS[i]
    win = C.oracle_window(w, 70)
    assert win['actions'].shape == (70, w.N)
    for T in (5, 70):
        for k in C.KS:
            sel = C.select_of(w, k)
            assert len(sel) == k and len(set(sel)) == k and sel[0] == w.N - 1 and (k == 1 or sel != sorted(sel))
            died, ate = C.events(win, sel, T)
            assert died and ate, (T, k, died, ate)
    assert C.find_window(w.family, w.S, w.N, w.env_offset, seeds=[w.seed]) == w   # (the anchors are the rule's)
    if w.family != 'tape':  # what policy_rollout returns is sanitised: stepping on it again changes nothing
        assert win['actions'].min() >= 0 and win['actions'].max() <= 3 and len(np.unique(win['actions'])) == 4


def test_window_recorder_on_a_stand_in_env(tmp_path):
    """every `interval`-th window, tiles padded to a full grid, the shared frame of consecutive windows kept once"""
    import torch
    from wurm_amd.recording import WindowRecorder

    class Env(object):
        calls = []

        def record_start(self, select):
            self.calls.append(('start', list(select)))
            return len(self.calls)

        def record_frames(self, rec, actions):
            self.calls.append(('frames', rec))
            T = actions.shape[0]
            return dict(frames=torch.full((T + 1, 3, 3, 5, 5), rec, dtype=torch.uint8))

    actions = torch.zeros((4, 8), dtype=torch.long)
    for interval, frames in ((1, 5 + 4 + 4), (2, 5 + 5)):
        env, path = Env(), str(tmp_path / f'every{interval}.npy')
        env.calls = []
        wr = WindowRecorder(env, path, [0, 1, 2], interval=interval, tile_pixels=10)
        for window in range(3):
            rec = wr.start(window)
            assert (rec is None) == (window % interval != 0)
            wr.finish(rec, actions)
        wr.close()
        clip = np.load(path)
        assert clip.shape == (frames, 20, 20, 3) and (clip[:, 15:, 15:] == 0).all() and clip[:, :5, :5].min() > 0
        assert [c[0] for c in env.calls] == ['start', 'frames'] * (3 if interval == 1 else 2)
