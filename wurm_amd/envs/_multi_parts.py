"""What MultiSnake (wurm_amd/envs/multi_snake.py) keeps per env object besides the state, one small object per role; all of
them are derived state, made by `MultiSnake._make_machine`:

  * `_LazyInfo`, `_LazyResetObs`: the dicts `step` / `reset(done)` hand out that fill themselves when somebody looks;
  * `Masks`: check_consistency()'s masks from inside the step launch (wurm_multi_call.check_mask) and their arming;
  * `ResetObs`: does the caller keep what `reset(done)` returns?  ("discarded reset observations");
  * `Outputs`: the output slab the next steps write, and the `rewards` / `boost_this_step` views of the last step's part.
"""
import sys
import weakref
from collections import OrderedDict

import torch

from wurm_amd import _lib


class _LazyDict(dict):
    """A dict that fills itself (`_fill() -> True if it just did`) the first time anything reads or writes it, so that it
    behaves as the plain dict it then is, and pickles as one."""
    __slots__ = ()

    def __missing__(self, key):
        if not self._fill():
            raise KeyError(key)
        return dict.__getitem__(self, key)

    def __reduce__(self):
        self._fill()
        return (dict, (dict(self),))


def _filling(name):
    method = getattr(dict, name)

    def wrapper(self, *a, **kw):
        self._fill()
        return method(self, *a, **kw)
    wrapper.__name__ = name
    return wrapper


for _name in ('__contains__', '__iter__', '__len__', '__eq__', '__ne__', '__repr__', '__setitem__', '__delitem__', '__or__',
              '__ror__', '__ior__', '__reversed__', 'get', 'keys', 'values', 'items', 'copy', 'pop', 'popitem', 'setdefault',
              'update', 'clear'):
    setattr(_LazyDict, _name, _filling(_name))


class _LazyInfo(_LazyDict):
    """`info` of one step (reference :707-729: snake_collision_i, edge_collision_i, food_i, size_i, boost_i).  Its 5 K
    tensors are carved from the step's output block the first time anything looks at it: a view object per row is most of
    what a step costs on the host, and callers that read `info` every step are rare (the reference's loops log from it every
    few hundred steps)."""
    __slots__ = ('_src',)

    def __init__(self, src):
        dict.__init__(self)
        self._src = src

    def _fill(self):
        src = self._src
        if src is None:
            return False
        self._src = None
        f, b, keys, K = src  # the step's packed floats (6K, N) / flags (7K + 1, N): agent-major rows from 3K on
        rf, rb = f[3 * K:].unbind(0), b[3 * K:7 * K].unbind(0)
        k_snake, k_edge, k_food, k_boost, k_size = keys
        dict.update(self, zip(k_snake, rb[2 * K:3 * K]))
        dict.update(self, zip(k_edge, rb[3 * K:]))
        dict.update(self, zip(k_food, rf[K:2 * K]))
        dict.update(self, zip(k_size, rf[2 * K:]))
        dict.update(self, zip(k_boost, rb[K:2 * K]))
        return True


class _LazyResetObs(_LazyDict):
    """What `reset(done)` returns once the caller has been seen to DISCARD it (experiments/speeds.py:30-38 does: `env.reset(
    done['__all__'])` as a statement): the K observations of the reference's return value (:834-836) are not worth a second
    observation stream out of every step launch for a caller that drops them.  The dict fills itself — the postponed reset
    applied, `_observe` of the mode the reset was called in — the first time anything reads it; and if the caller still
    holds it when the state is about to change (the next step, anything that flushes the postponed reset) the env fills it
    first, so it always holds what the reference would have returned.  Either way the env goes back to precomputing."""
    __slots__ = ('_env', '_mode', '__weakref__')

    def __init__(self, env, mode):
        dict.__init__(self)
        self._env, self._mode = env, mode

    def _fill(self):
        env = self._env
        if env is None:
            return False
        self._env = None
        env._reset_obs.settle(self)
        return True


class Masks(object):
    """check_consistency()'s masks of the post-step / post-reset state, written by the step launch on the mirror while the
    caller keeps calling that method (`buf`: (2, N) int32, made with the mirror)."""
    __slots__ = ('fs', 'c', 'buf', 'has_after', 'armed_at', 'void_at', 'calls', 'step')

    def __init__(self, fs, block):
        self.fs, self.c = fs, block
        self.buf, self.has_after = None, False
        self.armed_at, self.void_at = 1 << 62, -1
        self.calls = self.step = 0

    def void(self):
        """the masks the last step's launch wrote no longer describe the state (something looked at it or wrote it)"""
        self.void_at = self.fs.steps

    def fresh(self) -> bool:
        c, st = self.c, self.fs.steps
        return bool(c.resident) and bool(c.check_mask) and st > self.armed_at and st > self.void_at

    def asked(self):
        """check_consistency() was called"""
        self.calls += 1
        self.step = self.fs.steps

    def arm(self):
        """asked for while the caller keeps calling check_consistency(), dropped again if it stops doing so"""
        c = self.c
        if self.buf is None:
            return
        want = self.calls > 0 and self.fs.steps - self.step <= 64
        if want != bool(c.check_mask):
            c.check_mask = self.buf[0].data_ptr() if want else None
            c.check_mask_after = self.buf[1].data_ptr() if want else None
            self.armed_at = self.fs.steps if want else 1 << 62  # (steps from here on write them)

    def current(self, pend):
        """(N) int32 masks of the state as it is now, or None if the last launch's do not apply; -1 marks an env the launch
        could not vouch for.  pend: the kernels' copy of the flags of the postponed reset."""
        c = self.c
        if not self.fresh() or not c.resident_valid:
            return None
        if not self.fs.pending:
            return self.buf[0]
        if self.has_after:       # the postponed reset of the step's own mask: what obs_after observed
            return self.buf[1]
        # postponed, but the launch did not build that state: envs the reset rebuilds are not vouched for
        return self.buf[0].masked_fill(pend != 0, -1)


class ResetObs(object):
    """Whether the caller keeps what `reset(done)` returns.  `probe`: the precomputed dict the last reset(done) handed out,
    looked at by the next step; `drops`: consecutive resets whose dict nobody held then — after DROPS of them reset(done)
    returns a _LazyResetObs and the steps stop precomputing (`lazy_mode`); `ref`: weak reference to the _LazyResetObs of the
    postponed reset, while it may still need filling."""
    __slots__ = ('env', 'probe', 'drops', 'lazy_mode', 'ref')
    DROPS = 3

    def __init__(self, env):
        self.env, self.probe, self.drops, self.lazy_mode, self.ref = env, None, 0, False, None

    def hand_out(self, mode):
        """the self-filling dict of a reset that has just been postponed without its observation"""
        lz = _LazyResetObs(self.env, mode)
        self.ref = weakref.ref(lz)
        return lz

    def before_change(self):
        """the state is about to change: the dict that reset returned, if the caller still holds it, is filled NOW"""
        ref, self.ref = self.ref, None
        if ref is not None:
            lz = ref()
            if lz is not None:
                lz._fill()

    def before_step(self):
        """in front of a step: did the caller keep what the last reset(done) returned?"""
        probe, self.probe = self.probe, None
        if probe is not None:
            # the references of a dict nobody else holds: the slab's list of precomputed dicts, `probe`, getrefcount's argument
            if sys.getrefcount(probe) <= 3:
                self.drops += 1
                if self.drops >= self.DROPS and not self.env._half:
                    self.lazy_mode = True
            else:
                self.drops = min(self.drops, 0)
        self.before_change()

    def settle(self, lz):
        """fills the _LazyResetObs `lz`: the postponed reset applied (if it still is postponed), then the observation of the
        mode that reset was called in — what the reference's reset returned (:834-836).  The caller reads, or still holds,
        what reset returns after all: back to precomputing it in the step launch."""
        env = self.env
        self.ref = None
        if env._pending:
            env._flush()
        dict.update(lz, env._observe(lz._mode))
        self.lazy_mode = False
        self.drops = -(1 << 20)   # (no flapping: a caller that reads it once is a caller that reads it)
        env._fs.want_obs_after = True


class Outputs(object):
    """The output slab: fresh tensors for the next R steps, and `rewards` / `boost_this_step` of the last step as views of
    its part of the slab, each made on first use and stamped with the step count it belongs to."""
    __slots__ = ('env', 'rows', 'mode', 'rewards_t', 'rewards_at', 'rewards_src', 'boost_t', 'boost_at')

    def __init__(self, env):
        self.env, self.rows, self.mode = env, None, None    # rows: (out_f32, out_u8) of the current slab, per step
        self.rewards_t = self.rewards_src = self.boost_t = None
        self.rewards_at = self.boost_at = 0

    def rewards(self):
        fs, env = self.env._fs, self.env
        st = fs.steps
        if self.rewards_at != st:  # (the env-major block at the start of the last step's packed floats)
            self.rewards_t, self.rewards_at = self.rows[0][fs.slot - 1].view(-1)[:env.num_envs * env.num_snakes], st
        elif self.rewards_t is None:  # (after a rollout: its last step's (K, N) block, env-major on demand)
            self.rewards_t, self.rewards_src = self.rewards_src.t().reshape(-1), None
        return self.rewards_t

    def boost(self):
        fs, env = self.env._fs, self.env
        st = fs.steps
        if self.boost_at != st:
            self.boost_t, self.boost_at = self.rows[1][fs.slot - 1].view(-1)[:env.num_envs * env.num_snakes], st
        return self.boost_t

    def new(self):
        """Fresh output tensors for the next R steps in two allocations, and the R x (8 K + 1) per-agent views and 4 dicts
        `step` returns (reference :701-729) made ONCE per slab — a view object per row was most of what a step cost on the
        host.  A slab is never written twice; it is released when the last tensor carved from it is."""
        env = self.env
        N, K, dev, fs = env.num_envs, env.num_snakes, env.device, env._fs
        if self.rows is not None and fs.steps > 0:
            self.rewards(), self.boost()  # (views of the slab that is being replaced: made while it is at hand)
        c = env._mc
        self.mode = mode = env.observation_mode
        c.obs_mode, c.obs_n, o = env._obs_args(mode)
        inner = tuple(o.shape[2:])
        elems = int(torch.Size(inner).numel())
        want_after = bool(fs.want_obs_after)
        per_step = K * N * (4 * elems * (2 if want_after else 1) + 24 + 7) + N
        # 64 MB per slab at most: a caller that drops what a step returned before the next one gets the SAME block back from
        # torch's allocator, and one call's outputs (123 MB at cfg4 'full': one step per slab) then stay in the 256 MB
        # Infinity Cache; a slab of several such steps would stream to HBM (measured: 39 against 35 us per iteration at cfg4)
        R = max(1, min(64, (64 << 20) // max(per_step, 1)))
        # TWO allocations for the slab's four blocks (round 6: four torch.empty were 10 of the 28 us a step of cfg4 'full' — one
        # step per slab — cost on the host, which is what bounded that loop): one block of floats (rewards / food / sizes,
        # observations, reset observations; each part on a 256-byte boundary) and the flags on their own — their version
        # counter is what proves `dones['__all__']` unmodified, and an in-place edit of an observation must not touch it
        n_of, n_obs = R * 6 * K * N, R * K * N * elems
        n_of_pad, n_obs_pad = (n_of + 63) & ~63, (n_obs + 63) & ~63
        floats = torch.empty(n_of_pad + n_obs_pad + (n_obs if want_after else 0), dtype=torch.float32, device=dev)
        of = floats[:n_of].view(R, 6 * K, N)
        obs = floats[n_of_pad:n_of_pad + n_obs].view((R, K, N) + inner)
        after = floats[n_of_pad + n_obs_pad:].view((R, K, N) + inner) if want_after else None
        ob = torch.empty((R, 7 * K + 1, N), dtype=torch.bool, device=dev)
        sl = env._sl
        sl.out_f32, sl.out_u8, sl.obs, sl.steps, sl.obs_elems = of.data_ptr(), ob.data_ptr(), obs.data_ptr(), R, elems
        sl.obs_after = after.data_ptr() if after is not None else None
        self.rows = (of.unbind(0), ob.unbind(0))
        try:
            fs.slab_version = ob._version
        except RuntimeError:   # allocated under torch.inference_mode(): no version counters, so no deferral (eager resets)
            fs.slab_version = -1
        # what callers read every step — observations, rewards, dones — is carved now (row_views: ~0.3 us per tensor); the
        # 5 K tensors of `info` when somebody looks (_LazyInfo)
        K3, K4 = 3 * K, 4 * K
        ofs, obs_ = self.rows
        rf = _lib.row_views(of, 2, K3, K4)                      # rewards (agent-major rows 3K .. 4K)
        ob2 = ob.view(R, 7 * K + 1, N)
        rd = _lib.row_views(ob2, 2, K3, K4)                     # dones
        ra = _lib.row_views(ob2, 2, 7 * K, 7 * K + 1)           # all_done
        ov = _lib.row_views(obs, 2)
        av = _lib.row_views(after, 2) if after is not None else None
        k_agent, k_snake, k_edge, k_food, k_boost, k_size = env._keys
        info_keys = (k_snake, k_edge, k_food, k_boost, k_size)
        outs, done2s, afters = [], [], []
        for i in range(R):
            f, b = rf[i * K:(i + 1) * K], rd[i * K:(i + 1) * K] + [ra[i]]
            dones_out = dict(zip(k_agent, b[:K]))
            dones_out['__all__'] = b[K]
            info = _LazyInfo((ofs[i], obs_[i], info_keys, K))
            outs.append((OrderedDict(zip(k_agent, ov[i * K:(i + 1) * K])), dict(zip(k_agent, f)), dones_out, info))
            done2s.append(b[K])
            if av is not None:
                afters.append(OrderedDict(zip(k_agent, av[i * K:(i + 1) * K])))
        fs.outs, fs.done2s, fs.obs_afters = outs, done2s, (afters if av is not None else None)
        fs.R, fs.slot = R, 0
        fs.lazy_ok = env._lazy_ok()
        env._masks.arm()
