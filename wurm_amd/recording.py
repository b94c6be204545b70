"""Frame recording for the render / record path of the reference's experiment scripts (experiments/main.py:184-186,
201-202, 255-262 use gym's `VideoRecorder(env, path=...)`, `.capture_frame()`, `.close()`).

gym is not part of this build's environment; this recorder keeps the same three-call interface, takes its frames from
`env.render(mode='rgb_array')` (the GPU renders the RGB batch, `wurm_amd/_render.py` tiles it on the host — bit-equal
to the reference's frames, tests/test_render_golden.py) and writes, by file extension: `.mp4` through an `ffmpeg`
binary on PATH exactly as gym's recorder does (raw RGB frames piped in, libx264 / yuv420p; RuntimeError if there is no
ffmpeg, like gym's DependencyNotInstalled), `.npy` the raw (frames, H, W, 3) uint8 array, anything else an animated
GIF with Pillow.  Host side only; nothing here is on the step path.
"""
import os

import numpy as np


class VideoRecorder(object):
    def __init__(self, env, path: str, frames_per_sec: int = 12, enabled: bool = True):
        self.env = env
        self.path = path
        self.frames_per_sec = frames_per_sec
        self.enabled = enabled
        self.frames = []
        self.closed = False

    def capture_frame(self):
        """Appends the env's current frame (reference: called once per loop iteration before `model(state)`)."""
        if not self.enabled or self.closed:
            return
        frame = np.asarray(self.env.render(mode='rgb_array'))
        if frame.ndim != 3 or frame.shape[-1] != 3:
            raise RuntimeError(f'render(mode="rgb_array") returned shape {frame.shape}, expected (H, W, 3)')
        self.frames.append(frame.astype(np.uint8))

    def capture_frames(self, array):
        """Appends many finished (H, W, 3) frames at once, in order: a (T, H, W, 3) array or a sequence of frames, e.g.
        `wurm_amd._render.tile_frames(env.record_frames(rec, actions)['frames'], env.render_args)` for a fused window
        (the env is not asked to render)."""
        if not self.enabled or self.closed:
            return
        for frame in array:
            frame = np.asarray(frame)
            if frame.ndim != 3 or frame.shape[-1] != 3:
                raise RuntimeError(f'capture_frames: a frame of shape {frame.shape}, expected (H, W, 3)')
            self.frames.append(frame.astype(np.uint8))

    def close(self):
        """Writes the file (nothing if no frame was captured) and releases the frames."""
        if self.closed:
            return
        self.closed = True
        if not self.enabled or not self.frames:
            self.frames = []
            return
        directory = os.path.dirname(self.path)
        if directory:
            os.makedirs(directory, exist_ok=True)
        if self.path.endswith('.mp4'):
            self._write_mp4()
        elif self.path.endswith('.npy'):
            np.save(self.path, np.stack(self.frames))
        else:
            from PIL import Image
            images = [Image.fromarray(f) for f in self.frames]
            images[0].save(self.path, save_all=True, append_images=images[1:], loop=0,
                           duration=max(1, int(round(1000 / self.frames_per_sec))))
        self.frames = []

    def _write_mp4(self):
        import shutil
        import subprocess
        ffmpeg = shutil.which('ffmpeg') or shutil.which('avconv')
        if ffmpeg is None:
            raise RuntimeError('VideoRecorder: writing .mp4 needs an ffmpeg (or avconv) binary on PATH; use a .gif or '
                               '.npy path instead')
        h, w = self.frames[0].shape[:2]
        cmd = [ffmpeg, '-nostats', '-loglevel', 'error', '-y', '-f', 'rawvideo', '-s:v', f'{w}x{h}', '-pix_fmt', 'rgb24',
               '-framerate', str(self.frames_per_sec), '-i', '-', '-vf', 'scale=trunc(iw/2)*2:trunc(ih/2)*2',
               '-vcodec', 'libx264', '-pix_fmt', 'yuv420p', '-r', str(self.frames_per_sec), self.path]
        proc = subprocess.Popen(cmd, stdin=subprocess.PIPE)
        for f in self.frames:
            proc.stdin.write(np.ascontiguousarray(f).tobytes())
        proc.stdin.close()
        if proc.wait() != 0:
            raise RuntimeError(f'VideoRecorder: {ffmpeg} failed with exit code {proc.returncode}')

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowRecorder(object):
    """Video of chosen envs of a loop of FUSED windows (examples/a2c_fused_learner.py, a2c_pbt.py: `--save-video`), which
    never materialise the states between their steps: every `interval`-th window is replayed for the envs `select` after
    the fact (`env.record_start` / `env.record_frames`, one launch and one device-to-host copy per recorded window) and its
    frames are tiled row-major into a near-square picture.  A window that is not recorded costs one integer comparison.
    Of two recorded windows in a row the second one's first frame is dropped (it is the first one's last): this assumes
    that nothing but the windows touches the env between them, as in the examples' loops.  The env is a SingleSnake or a
    SimpleGridworld (uint8 frames) or a MultiSnake with its `act_window` / `rollout` (examples/a2c_multi_species.py; int16
    frames, converted as `render('rgb_array')` converts `_get_env_images()`).

        rec = recorder.start(window)                 # in front of env.policy_rollout / env.act_window / env.rollout
        out = env.policy_rollout(...)
        recorder.finish(rec, out['actions'])         # before the next call on the env; nothing to do if rec is None
        recorder.close()                             # writes the file (VideoRecorder: .mp4 / .npy / GIF)
    """

    def __init__(self, env, path: str, select, interval: int = 1, tile_pixels: int = 128, frames_per_sec: int = 12):
        self.env, self.select, self.interval = env, [int(i) for i in select], max(1, int(interval))
        k = len(self.select)
        cols = int(np.ceil(np.sqrt(k)))
        self.render_args = {'num_rows': -(-k // cols), 'num_cols': cols, 'size': int(tile_pixels)}
        self.video = VideoRecorder(None, path, frames_per_sec=frames_per_sec)
        self._window, self._last = None, None

    def start(self, window: int):
        """the record of window number `window` (0, 1, ...), or None if it is not one of every `interval`-th"""
        if window % self.interval != 0:
            return None
        self._window = window
        return self.env.record_start(self.select)

    def finish(self, rec, actions):
        if rec is None:
            return
        from wurm_amd._render import tile_frames
        frames = self.env.record_frames(rec, actions)['frames']
        if self._last is not None and self._window == self._last + 1:
            frames = frames[1:]          # (the state a window leaves behind is the first frame of the one that follows)
        self._last = self._window
        frames = frames.cpu().numpy()
        tiles = self.render_args['num_rows'] * self.render_args['num_cols']
        if tiles > frames.shape[1]:      # (the last row of tiles is not full: black tiles)
            pad = np.zeros((frames.shape[0], tiles - frames.shape[1]) + frames.shape[2:], frames.dtype)
            frames = np.concatenate([frames, pad], axis=1)
        self.video.capture_frames(tile_frames(frames, self.render_args))

    def close(self):
        self.video.close()
