"""Per-call machinery shared by SingleSnake and SimpleGridworld: one launch per `step(a); reset(done)` iteration.

At a few hundred envs the loop of experiments/main.py:212-227 / tests/test_single_snake_env.py:24-31 is bound by host
time per call, not by the GPU, so:
  * `step` is ONE launch (wurm_single_step_slot / wurm_grid_step_slot, include/wurm_hip.h) described by a persistent
    argument block; the tensors it returns are carved from slabs that hold the next few dozen steps' worth of FRESH
    outputs (a slab is never written twice: it is dropped once used up and lives as long as any tensor handed out from
    it) and are handed back as one PREBUILT tuple per slot;
  * `reset(done)` with the very `done` that `step` just returned is DEFERRED (`lazy_reset=True`, the default): the next
    `step` rebuilds those envs in front of its own transition, in the same launch, with the RNG counter the eager call
    would have used — bit-identical results.  Anything that looks at the state in between (`env.envs`, `_observe`,
    `check_consistency`, `rollout`, `render`, another `reset`) first flushes the postponed reset with the ordinary reset
    kernel, so `env.envs` always is what the reference would show.  If the caller reads the observation `reset(done)`
    returns (the reference's `reset` always returns it, single_snake.py:322-342), the step launch writes that one too
    (the observation of every env once the finished ones are rebuilt).
    A reset is only postponed while nobody else holds a tensor on the state's storage (`_alias_free`: the storage's use
    count; the `envs` attribute hands out a tensor object of the caller's own on the same storage and version counter), so an
    alias the caller keeps — `e = env.envs; env.step(a); env.reset(d); e[...]` — shows the reset state, as the reference's
    would (round 5; rounds 2-4 documented this as a deviation);
  * the bodies of `step` and of the deferred `reset` are a small state machine, `Stepper`: in C where the extension
    wurm_amd/_fastcall is built (wurm_amd/csrc/fastcall.c), else `PyStepper` below — the same logic, and the
    specification of the C type (tests/test_host_lazy_reset.py drives both through the same call patterns).

  * large batches (SingleSnake 9 x 9 `partial_2` / no observation from 4096 envs, 12 x 12 and larger from 2^20 cells:
    wurm_single_resident_bytes) hand the launch a compact MIRROR of the state (wurm_single_call.resident) which it steps
    instead of re-reading the fp32 tensor every call; the tensor stays the state: reading `env.envs` writes it out (and from
    then on every step writes it), any other entry point goes through `_touch()`, a tensor the caller holds is watched for
    in-place edits through its version counter (DESIGN.md §5, §7 deviation 9).

`reset`, `rollout`, `_get_rgb`, `record_start` / `record_frames` and the common part of `policy_rollout` are the mixin's as
well: the two classes differ there in names and in SimpleGridworld's start location only.

The host class provides: num_envs, size, device, seed, env_offset, observation_mode, lazy_reset, _mode_cache, _CHANNELS,
_NAME, _STEP_SLOT / _ROLLOUT_FNS (plain, with a mirror) / _POLICY_FN / _FRAMES_FN (entry point names), _FLAG_KEYS (result keys of the flag
rows an entry point writes), _BAD_STATUS, _parse_mode(mode) -> (mode code, n), _obs_shape(mode), _observe(mode),
_lazy_supported(), _cannot_reset() -> the exception a reset that has to create an env raises (None: it can; what no reset at all
can do, SingleSnake's other snake lengths, it raises itself), _start_args()
-> the start location the resetting entry points take, or (), _launch_reset(envs, done, obs, mode code, n, call),
_configure_call(block), _make_out(i) -> what step returns for slot i.
"""
import ctypes

import torch

from wurm_amd import _lib
from wurm_amd.envs._mirror import Mirror, parse_mirror_policy  # noqa: F401 (parse_mirror_policy: imported from here too)


_storage_use_count = torch._C._storage_Use_Count


class PyStepper(object):
    """Pure-Python twin of wurm_amd._fastcall.Stepper (same attributes, same methods, same results).

    `fn` is a callable fn(call_block_addr, slabs_addr, slot, actions_ptr, actions_dtype, call, apply_pending, pre_call,
    want_obs_after, stream) -> return code: the ctypes function, or a recording stand-in in the host tests."""

    def __init__(self, fn, blk, slabs, get_device, get_stream, dt_i64, dt_i32, dt_i16):
        self.fn, self.blk, self.slabs = fn, blk, slabs
        self.get_device, self.get_stream = get_device, get_stream
        self.dt_i64, self.dt_i32, self.dt_i16 = dt_i64, dt_i32, dt_i16
        self.slot = self.R = self.num_envs = self.dev_index = 0
        self.slab_version = -1
        self.call = self.pend_call = self.steps = 0
        self.ok = self.pending = self.last_fresh = self.want_obs_after = self.lazy_ok = False
        self.outs = self.done2s = self.obs_afters = None
        self.last_done2 = self.done_view = self.obs_after = None
        self.watch, self.watch_version = None, -1  # a tensor the caller may edit in place, and its version when last looked at

    def step(self, actions):
        """The prebuilt output tuple of this step; None: the caller has to prepare something first (new slab, state tensor
        to re-validate or edited in place, actions on another device / not a contiguous vector, another device current) and call again; a
        non-zero int: the entry point's error code.  Argument errors as the reference raises them
        (single_snake.py:198-203; int16 passes its check and then fails in scatter_ at :229)."""
        dt = actions.dtype
        if dt is self.dt_i64:
            code = 0  # _lib.ACT_I64
        elif dt is self.dt_i32:
            code = 1  # _lib.ACT_I32
        elif dt is self.dt_i16:
            raise RuntimeError('scatter_(): Expected dtype int32/int64 for index')
        else:
            raise TypeError('actions Tensor must be an integer type i.e. '
                            '{torch.ShortTensor, torch.IntTensor, torch.LongTensor}')
        if actions.size(0) != self.num_envs:
            raise RuntimeError('Must have the same number of actions as environments.')
        i = self.slot
        if not self.ok or i >= self.R or (self.want_obs_after and self.obs_afters is None):
            return None
        w = self.watch
        if w is not None:
            try:
                ver = w._version
            except RuntimeError:
                ver = -1
            if ver != self.watch_version:
                return None  # the state tensor has been edited in place since the caller took it
        idx = self.dev_index
        if actions.get_device() != idx or actions.dim() != 1 or not actions.is_contiguous():
            return None
        if self.get_device() != idx:  # kernels launch on the current device
            return None
        rc = self.fn(self.blk, self.slabs, i, actions.data_ptr(), code, self.call, self.pending, self.pend_call,
                     self.want_obs_after, self.get_stream(idx))
        if rc:
            return int(rc)  # nothing consumed: the counter, the postponed reset and the slot stay
        self.call += 1
        self.steps += 1
        self.pending = False
        self.slot = i + 1
        self.last_done2 = self.done2s[i]
        self.done_view = None
        self.last_fresh = True
        self.obs_after = self.obs_afters[i] if self.want_obs_after else None
        return self.outs[i]

    # ---- MultiSnake: the same machine over wurm_multi_step_slot (`mfn`), actions a dict of K tensors
    mfn = None
    num_agents = 0
    last_out = None
    state = None        # (the C machine: the tuple of state tensors for its own storage-use-count check)
    alias_free = None   # callable: nobody else holds a tensor on the state's storage

    def step_multi(self, actions):
        """MultiSnake.step(actions: dict): the prebuilt (observations, rewards, dones, info) of this step; None: the caller
        has to prepare something first (as `step`; also: action tensors of another type or device) and calls launch_multi;
        False: everything is in place but the action block — K int64 device vectors that are not the rows of one (K, N)
        tensor: the caller stacks them and calls launch_multi; a non-zero int: the entry point's error code.
        Argument errors as the reference raises them (multi_snake.py:463-472)."""
        if actions.__class__ is not dict:
            return None  # (an OrderedDict may iterate in another order than its dict storage: the caller's generic path)
        if len(actions) != self.num_agents:
            raise RuntimeError('Must have a Tensor of actions for each snake')
        a_ptr, row, n = 0, 8 * self.num_envs, 0
        rows_ok = stackable = True
        for act in actions.values():
            dt = act.dtype
            if dt is not self.dt_i64 and dt is not self.dt_i32 and dt is not self.dt_i16:
                raise TypeError('actions Tensor must be an integer type i.e. '
                                '{torch.ShortTensor, torch.IntTensor, torch.LongTensor}')
            if act.size(0) != self.num_envs:
                raise RuntimeError('Must have the same number of actions as environments.')
            if dt is not self.dt_i64 or act.dim() != 1 or act.get_device() != self.dev_index:
                stackable = False
            if rows_ok:
                if dt is not self.dt_i64 or act.dim() != 1 or not act.is_contiguous() or act.get_device() != self.dev_index:
                    rows_ok = False
                else:
                    ptr = act.data_ptr()
                    if n == 0:
                        a_ptr = ptr
                    elif ptr != a_ptr + n * row:
                        rows_ok = False
            n += 1
        i = self.slot
        if not self.ok or i >= self.R or (self.want_obs_after and self.obs_afters is None):
            return None
        if self.get_device() != self.dev_index:
            return None
        if not rows_ok:   # False: all that is missing is the (K, N) action block (the caller stacks the K vectors)
            return False if stackable else None
        return self.launch_multi(a_ptr)

    def launch_multi(self, a_ptr):
        """the launch of slot `slot` on a prepared (K, N) int64 action block, and the bookkeeping after it"""
        i = self.slot
        rc = self.mfn(self.blk, self.slabs, i, a_ptr, self.call, self.pending, self.pend_call, self.want_obs_after,
                      self.get_stream(self.dev_index))
        if rc:
            return int(rc)
        self.call += 1
        self.steps += 1
        self.pending = False
        self.slot = i + 1
        self.last_done2 = self.done2s[i]
        self.done_view = None
        self.last_fresh = True
        self.obs_after = self.obs_afters[i] if self.want_obs_after else None
        self.last_out = self.outs[i]
        return self.last_out

    def reset_lazy(self, done, return_observations):
        """What reset(done) returns if the reset could be postponed into the next step's launch (None, or the observation
        the last step's launch already wrote), else NotImplemented."""
        if self.last_fresh and self.lazy_ok and (done is self.last_done2 or
                                                 (self.done_view is not None and done is self.done_view)):
            # only while nobody else holds a tensor on the state's storage: through an alias the caller could read or edit the
            # un-reset state, which the reference would show reset (single_snake.py:322-342, multi_snake.py:771-836)
            if self.alias_free is not None and not self.alias_free():
                return NotImplemented
            try:
                ver = done._version
            except RuntimeError:  # inference tensors do not track versions: cannot prove `done` is unmodified
                ver = -1
            if ver >= 0 and ver == self.slab_version:
                if not return_observations:
                    self.want_obs_after = False
                    self.pending, self.pend_call, self.last_fresh = True, self.call, False
                    self.call += 1
                    return None
                if self.obs_after is not None:
                    obs, self.obs_after = self.obs_after, None
                    self.pending, self.pend_call, self.last_fresh = True, self.call, False
                    self.call += 1
                    return obs
                self.want_obs_after = True  # from the next step on, the step launch also writes this observation
            elif ver >= 0:
                self.slab_version = ver  # an in-place edit of one step's flags costs one eager reset, not the slab's rest
        return NotImplemented


def _make_stepper(name, blk_addr, slabs_addr):
    """C Stepper over the entry point's address when wurm_amd/_fastcall is built and the entry point is a real C function;
    else PyStepper over whatever callable _lib.step_slot_fn hands out (ctypes function / test stand-in).  MultiSnake's
    entry point (wurm_multi_step_slot) has another signature: the machine's `mfn` / step_multi / launch_multi side."""
    get_device, get_stream = _lib.accessors()
    fn = _lib.step_slot_fn(name)
    multi = name == 'wurm_multi_step_slot'
    addr = getattr(fn, 'c_address', None)
    if addr is not None:
        try:
            from wurm_amd import _fastcall
            helpers = _lib.torch_helpers() or (None, None, None)
            fs = _fastcall.Stepper(addr, blk_addr, slabs_addr, get_device, get_stream, torch.int64, torch.int32,
                                   torch.int16, *helpers)
            if multi:
                fs.multi = True  # (AttributeError with an older build of the extension: the Python machine)
            return fs
        except (ImportError, AttributeError):
            pass
    fs = PyStepper(None if multi else fn, blk_addr, slabs_addr, get_device, get_stream, torch.int64, torch.int32, torch.int16)
    if multi:
        fs.mfn = fn
    return fs


class FastStepMixin(object):
    # the library's mirror entry points of the class: size with / without the batch-size threshold, flush
    _RESIDENT_FNS = ('wurm_single_resident_bytes', 'wurm_single_resident_size', 'wurm_single_resident_flush')
    # rollout() of no steps: True = the mirror is not looked at (SingleSnake), False = it is brought in line with the mode first
    _EMPTY_ROLLOUT_SKIPS_MIRROR = False
    # the texts of mirror_state()['why'] that name the classes' tensor
    _MIRROR_WORDS = {
        'written': '`envs`',
        'touched': 'adaptive: the state was written by something other than the step launch after %d of the last %d steps',
        'held': 'the caller holds the state tensor: every step writes `envs`, in-place edits are watched',
        'unwatchable': 'the state tensor has no version counter (inference mode): cannot be watched',
        'unserved': 'shape / observation mode not served by the mirror kernels, or batch below the threshold',
        'refused': "refused: the launch that built it found envs outside the lane kernel's domain (hand-made states) — the "
                   'state tensor is stepped as it is, two launches per call, until something writes the state again'}
    _mirror = property(lambda self: self._mir.buf)   # (the name tests and tools read)

    def _fast_init(self, envs=None):
        """Derived state, ALL of it (`envs`: the state tensor of a copy; None: a fresh one).  Whatever this method adds to
        the object is left out of a copy / pickle and made again by this method on the other side."""
        d = self.__dict__
        before = set(d)
        N = self.num_envs
        c = self._c = _lib.SingleCall()
        c.num_envs, c.env_offset, c.seed, c.size = N, self.env_offset, _lib.u64(self.seed), self.size
        self._sl = _lib.SingleSlabs()
        self._fs = _make_stepper(self._STEP_SLOT, ctypes.addressof(c), ctypes.addressof(self._sl))
        self._fs.alias_free = self._alias_free
        self._fs.num_envs = N
        self._fs.dev_index = -1 if self.device.index is None else self.device.index
        self._get_device = _lib.accessors()[0]
        self._pend = None              # (N) bytes: the kernels' own copy of the last step's `done`
        self._slab_mode = None
        self._envs = torch.zeros((N, self._CHANNELS, self.size, self.size), device=self.device) if envs is None else envs
        self._fs.state = (self._envs,)
        self._envs_ok = None           # the state tensor that has been validated (None: validate before the next launch)
        # env.done: what the caller (or the constructor / rollout) assigned, valid until the next step overwrites it
        self._done, self._done_stamp = torch.zeros(N, dtype=torch.bool, device=self.device), 0
        # compact mirror of the state the step launch reads instead of `envs` (wurm_single_call.resident; large 9 x 9
        # batches).  The library marks it current after each step launch; everything else that writes the state clears
        # the mark (_touch); a state tensor the caller got hold of is watched for in-place edits through its version counter
        # (`fs.watch`: the step machine compares it in front of every launch)
        self._mir = Mirror(c, ctypes.addressof(c), self._RESIDENT_FNS, getattr(self, '_resident_policy', None),
                           self._MIRROR_WORDS, False, self.device)
        # check_consistency()'s masks from inside the step launch (wurm_single_call.check_mask): asked for once the caller
        # has called check_consistency(), valid for the state the last step left until anything else touches the state
        self._chk, self._chk_armed_at, self._chk_void_at, self._check_calls, self._check_step = None, 1 << 62, -1, 0, 0
        self._stor = None
        self._v_obs = self._v_reward = self._v_done2 = self._v_selfc = self._v_edgec = None   # rows of the output slab
        self._fast_made = frozenset(set(d) - before) | {'_fast_made'}

    # ------------------------------------------------------------------ copy / pickle
    # The reference's envs are plain attribute bags: copy.deepcopy(env) and pickle work on them (single_snake.py:55-102).
    # Here the object also owns ctypes blocks, a step machine and device buffers that are derived state: they are left out
    # and rebuilt on the other side (`_fast_init`), after the postponed reset and a lazy mirror have been applied to the
    # tensor that IS the state.
    def __getstate__(self):
        envs = self._state()   # (applies a postponed reset, writes a lazy mirror out)
        st = {k: v for k, v in self.__dict__.items() if k not in self._fast_made}
        st['_copy_envs'] = envs
        st['_copy_call'], st['_copy_done'] = int(self._fs.call), self.done
        return st

    def __setstate__(self, st):
        st = dict(st)
        call, done, envs = st.pop('_copy_call'), st.pop('_copy_done'), st.pop('_copy_envs')
        self.__dict__.update(st)
        # (our own tensor object, as the `envs` setter makes one: after copy.copy the two env objects share the state's storage
        # and `_alias_free` must see the other holder; nobody else holds the restored tensor: not watched)
        self._fast_init(envs.detach() if isinstance(envs, torch.Tensor) else envs)
        self._fs.call = call
        self.done = done

    # state of the step machine that other methods of the classes read and write
    _call = property(lambda self: self._fs.call, lambda self, v: setattr(self._fs, 'call', v))
    _pending = property(lambda self: self._fs.pending, lambda self, v: setattr(self._fs, 'pending', v))
    _pend_call = property(lambda self: self._fs.pend_call, lambda self, v: setattr(self._fs, 'pend_call', v))
    _last_fresh = property(lambda self: self._fs.last_fresh, lambda self, v: setattr(self._fs, 'last_fresh', v))

    @property
    def observation_mode(self) -> str:
        return self._observation_mode

    @observation_mode.setter
    def observation_mode(self, value: str):
        self._observation_mode = value
        fs = getattr(self, '_fs', None)
        if fs is not None:
            fs.ok = False  # the next step builds output slabs of the new shape
            # the observation the last step's launch pre-computed for `reset(done)` is one of the OLD mode: the reference
            # observes at reset time in the mode of that moment (single_snake.py:342) — that reset runs eagerly
            fs.obs_after = None

    @property
    def lazy_reset(self) -> bool:
        return self._lazy_reset

    @lazy_reset.setter
    def lazy_reset(self, value: bool):
        self._lazy_reset = bool(value)
        fs = getattr(self, '_fs', None)
        if fs is not None:
            fs.lazy_ok = self._lazy_reset and self._lazy_supported()

    def _next_call(self, n: int = 1) -> int:
        fs = self._fs
        c = fs.call
        fs.call = c + n
        fs.last_fresh = False  # the counter the last step's `obs_after` assumed for its reset is gone
        return c

    # ------------------------------------------------------------------ state

    @property
    def envs(self) -> torch.Tensor:
        """The state tensor, caller-visible and caller-mutable as in the reference (tests/test_single_snake_env.py:54,
        experiments/main.py:215,273).  Reading it applies a postponed reset; the caller may edit what it gets, so an
        observation the last step's launch pre-computed for `reset(done)` is dropped (that reset then runs eagerly)."""
        fs = self._fs
        if fs.pending:
            self._flush()
        fs.obs_after = None
        self._chk_void_at = fs.steps  # (the caller may edit what it gets)
        self._write_out()  # (lazy mirror: the step launches have not been writing `envs`; eager from now on, _watch)
        self._mirror_sync()  # (an edit through an alias since the last look must not be forgotten when _watch takes the
                             # tensor's version again: edit, look, step would step on a stale mirror)
        self._watch(self._envs)
        # a tensor object of the caller's own on the same storage (and version counter): `_alias_free` can then tell from
        # the storage's use count whether the caller still holds the state — or any view of it
        return self._envs.detach()

    @envs.setter
    def envs(self, value: torch.Tensor):
        # the reference would have applied reset(done) to the OLD tensor before this assignment replaced it
        fs = self._fs
        fs.pending = False
        fs.last_fresh = False
        fs.ok = False
        self._touch()  # (a lazy mirror is written out to the tensor that is being replaced, which is still ours here)
        self._envs_ok = None
        self._envs = value.detach() if isinstance(value, torch.Tensor) else value  # (our own tensor object: see the getter)
        self._fs.state = (self._envs,)
        self._watch(self._envs)

    def _alias_free(self) -> bool:
        """Nobody but this object holds a tensor on the state's storage (the caller's `e = env.envs`, a slice of it, the
        tensor it assigned): only then may a reset be postponed — with an alias alive the caller could read or edit the
        un-reset state through it, which the reference would show reset (single_snake.py:322-342)."""
        e = self._envs
        st = self._stor
        if st is None or st[0] is not e:
            s = e.untyped_storage()
            st = self._stor = (e, s, s._cdata)
        return _storage_use_count(st[2]) <= 2  # this object's tensor + the storage handle kept in `_stor`

    def _flush(self):
        """Applies the postponed reset(done) now, with the ordinary reset kernel and the counter it was given."""
        fs = self._fs
        self._touch()
        self._launch_reset(self._checked(self._envs), self._pend, None, _lib.OBS_NONE, 0, fs.pend_call)
        fs.pending = False  # (only once the launch is known to have been accepted)

    def _state(self, write: bool = True) -> torch.Tensor:
        """The state tensor, validated, with any postponed reset applied; the caller is about to change it or to
        consume an RNG counter (write=False: it only reads it with another kernel — the mirror stays current)."""
        fs = self._fs
        if fs.pending:
            self._flush()
        fs.last_fresh = False
        if write:
            self._touch()
        else:
            self._write_out()
        return self._checked(self._envs)

    def _touch(self):
        """Something other than the step launch is about to look at the state or to write it: a lazy mirror is written
        out to `envs` first (the step launches have not been writing them), and the next step rebuilds the mirror."""
        self._chk_void_at = self._fs.steps  # the masks of the last step's launch no longer describe the state
        self._mir.touch(self._fs.steps)

    def _write_out(self):
        """`envs` from a lazy mirror (which stays current)"""
        self._mir.write_out()

    def _watch(self, t):
        """The caller holds the state tensor `t` from now on and may edit it in place at any time: every step compares its
        version counter (in-place torch ops bump it) and rebuilds the mirror after a change.  Tensors without version
        counters (made under torch.inference_mode()) cannot be watched: no mirror from then on."""
        fs = self._fs
        self._mir.holds()
        try:
            fs.watch, fs.watch_version = t, t._version
        except (RuntimeError, AttributeError):
            fs.watch, fs.watch_version = None, -1
            self._mir.unwatchable()

    def _mirror_sync(self):
        """the step machine saw another version of the watched state tensor: the mirror is stale"""
        fs = self._fs
        w = fs.watch
        if w is not None:
            try:
                ver = w._version
            except RuntimeError:
                ver = -1
            if ver != fs.watch_version:
                self._touch()
                self._watch(w)

    def _setup_mirror(self, m: int, n: int):
        if (m, n) == self._mir.key:
            return
        # another observation mode: a LAZY mirror holds steps `envs` has not seen — written out while the old mirror is
        # still the one the call block names, before it is replaced or dropped
        self._touch()
        args = (m, n) if self._CHANNELS == 3 else (m,)   # (SimpleGridworld's observations have no crop radius)
        self._mir.setup((m, n), (_lib.i64(self.num_envs), self.size) + args, self._fs.steps, self._fs.watch is not None,
                        self.device)

    def mirror_state(self) -> dict:
        """What the resident mirror of the state is doing for this env object right now:
        `state` 'off' (every step reads `envs`), 'eager' (steps read the mirror and write `envs`) or 'lazy' (steps do
        not write `envs`; they are written out when something looks at them); `why`; `policy` (the `resident_mirror`
        keyword: None = automatic); `current`: the mirror describes the state (False: the next step rebuilds it)."""
        return self._mir.state()

    def _step_check_mask(self):
        """(N) int32 masks of wurm_single_check for the state as it is now, computed inside the last step's launch
        (wurm_single_call.check_mask) — -1 where the launch could not vouch for an env or the env finished in that step —
        or None if they do not describe the current state; arms the request for the following steps."""
        fs, c = self._fs, self._c
        self._check_calls += 1
        self._check_step = fs.steps
        if self._mirror is None or not c.resident or self.size != 9:
            return None      # (only the 9 x 9 lane-resident step computes masks: a grid mirror would pay a fill per step for -1s)
        self._mirror_sync()  # (an in-place edit of a state tensor the caller holds voids the masks)
        if self._chk is None:
            self._chk = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
        if not c.check_mask:
            c.check_mask = self._chk.data_ptr()
            self._chk_armed_at = fs.steps          # steps from here on write the masks
            return None
        if not c.resident_valid or fs.steps <= self._chk_armed_at or fs.steps <= self._chk_void_at:
            return None
        if fs.pending:  # the postponed reset(done) rebuilds exactly the envs the masks left out: fresh envs are consistent
            return self._chk.masked_fill(self._pend != 0, 0)
        return self._chk

    def _checked(self, e: torch.Tensor) -> torch.Tensor:
        if e is self._envs_ok:
            return e
        want = (self.num_envs, self._CHANNELS, self.size, self.size)
        if e.shape != want:
            raise RuntimeError(f'env.envs has shape {tuple(e.shape)}, expected {want}')
        if e.dtype != torch.float32 or e.device != self.device or not e.is_contiguous():
            # callers rebind env.envs (reference tests/test_single_snake_env.py:54): normalise once
            e = e.to(device=self.device, dtype=torch.float32).contiguous()
            self._envs = e
            self._fs.state = (e,)
        self._envs_ok = e
        self._c.envs = e.data_ptr()
        self._c.resident_valid = 0  # another tensor (its setter already dealt with a lazy mirror of the old one)
        return e

    @property
    def done(self) -> torch.Tensor:
        """(num_envs,) bool — the `done` of the last step (the reference assigns `self.done = done` in step), or whatever
        was assigned to the attribute since."""
        fs = self._fs
        if self._done_stamp == fs.steps:
            if self._done is None:  # after a rollout: every finished env was reset (made on first use: no fill kernel per launch)
                self._done = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            return self._done
        self._done = None  # a step has run since the assignment
        d = fs.done_view
        if d is None:  # the 1-D view of what the last step returned, made on first use
            d = fs.done_view = fs.last_done2.view(self.num_envs)
        return d

    @done.setter
    def done(self, value: torch.Tensor):
        self._done, self._done_stamp = value, self._fs.steps

    def _done_all_false(self):
        """env.done after a fused rollout (every finished env has been reset)"""
        self._done, self._done_stamp = None, self._fs.steps

    # ------------------------------------------------------------------ step

    def _new_slab(self):
        """Fresh output tensors for the next R steps in a few allocations (instead of four per step): R observations,
        R (N,1) rewards, 3 x R flag vectors (wurm_single_slabs), and the R tuples `step` returns.  A slab is never written
        twice; it is released when the last tensor carved from it is."""
        N = self.num_envs
        fs = self._fs
        m, n, shape = self._mode_info(self.observation_mode)
        elems = int(torch.Size(shape).numel()) // max(N, 1)
        per_step = N * (4 * elems + 4 + 3)
        R = max(1, min(64, (256 << 20) // max(per_step, 1)))  # (65 536 x 9 x 9 'partial_2': 20 MB per step)
        dev = self.device
        want_after = bool(fs.want_obs_after)
        obs = torch.empty((R,) + tuple(shape), dtype=torch.float32, device=dev)
        reward = torch.empty((R, N, 1), dtype=torch.float32, device=dev)
        flags = torch.empty((3, R, N), dtype=torch.bool, device=dev)
        obs_after = torch.empty((R,) + tuple(shape), dtype=torch.float32, device=dev) if want_after else None
        self._v_obs, self._v_reward = obs.unbind(0), reward.unbind(0)
        self._v_done2 = flags[0].unsqueeze(-1).unbind(0)
        self._v_selfc, self._v_edgec = flags[1].unbind(0), flags[2].unbind(0)
        if self._pend is None:
            self._pend = torch.zeros(N, dtype=torch.uint8, device=dev)
            self._c.done_copy = self._pend.data_ptr()
        self._configure_call(self._c)
        if self._c.check_mask and fs.steps - self._check_step > 64:
            # check_consistency() has not been called for a while: the step launches stop writing its masks
            self._c.check_mask, self._chk_armed_at = None, 1 << 62
        self._c.obs_mode, self._c.obs_n = m, n
        self._setup_mirror(m, n)
        sl = self._sl
        sl.obs, sl.reward, sl.flags, sl.steps = obs.data_ptr(), reward.data_ptr(), flags.data_ptr(), R
        sl.obs_after = obs_after.data_ptr() if obs_after is not None else None
        self._slab_mode = self.observation_mode
        try:
            fs.slab_version = flags._version
        except RuntimeError:   # allocated under torch.inference_mode(): no version counters, so no deferral (eager resets)
            fs.slab_version = -1
        fs.outs = [self._make_out(i) for i in range(R)]
        fs.done2s = list(self._v_done2)
        fs.obs_afters = list(obs_after.unbind(0)) if obs_after is not None else None
        fs.R, fs.slot = R, 0
        fs.lazy_ok = self._lazy_reset and self._lazy_supported()

    def _fast_step(self, actions: torch.Tensor, what: str):
        """`step`: one launch — [postponed reset] + step + observation (+ the observation reset(done) will return)."""
        fs = self._fs
        out = fs.step(actions)
        if out.__class__ is tuple:
            return out
        return self._slow_step(actions, out, what)

    def _slow_step(self, actions: torch.Tensor, out, what: str):
        """What the step machine could not do by itself (it returned None), or an error code of the entry point."""
        fs = self._fs
        if out is None:
            self._mirror_sync()
            if fs.slot >= fs.R or self._slab_mode != self.observation_mode or \
                    (fs.want_obs_after and fs.obs_afters is None):
                self._new_slab()
            else:
                self._configure_call(self._c)  # (attributes the call block carries may have been assigned: start_location)
            e = self._envs
            if e is not self._envs_ok:
                self._checked(e)
            fs.ok = True
            idx = fs.dev_index
            act = actions
            if act.get_device() != idx or act.dim() != 1 or not act.is_contiguous():
                act = actions.to(self.device).reshape(self.num_envs).contiguous()
            if self._get_device() != idx:
                with torch.cuda.device(idx):  # a process driving several GPUs has another device current
                    out = fs.step(act)
            else:
                out = fs.step(act)
            if out.__class__ is tuple:
                if act is not actions:
                    actions.copy_(act.view_as(actions))  # SingleSnake sanitises actions in place (single_snake.py:222)
                return out
        if out is None:
            raise RuntimeError(f'{what}: the step machine refused a prepared call')  # not reachable
        _lib.check(int(out), what)
        raise RuntimeError(f'{what}: unexpected return {out!r}')

    # ------------------------------------------------------------------ reset

    def _try_lazy_reset(self, done: torch.Tensor, return_observations: bool):
        """(True, obs) if reset(done) could be postponed into the next step's launch, else (False, None)."""
        obs = self._fs.reset_lazy(done, return_observations)
        if obs is NotImplemented:
            return False, None
        return True, obs

    def reset(self, done: torch.Tensor = None, return_observations: bool = True):
        """Resets environments that have finished (reference single_snake.py:322-342, simple_gridworld.py:225-245).

        Args:
            done: A 1D Tensor of length self.num_envs (any dtype; (N,1) is accepted). A non-zero value means the
                corresponding environment needs to be reset.  None: use the `done` of the last step.
            return_observations: extension — pass False to skip the observation the reference's callers discard
                (experiments/main.py:227).

        Called with the very `done` the last `step` returned (and nothing in between), the reset is postponed into the
        next step's launch (module docstring); the observation it returns then comes from the step's launch as well.
        """
        if done is None:
            done = self.done
        handled, obs = self._try_lazy_reset(done, return_observations)
        if handled:
            return obs
        done = done.view((done.shape[0]))
        if done.dtype != torch.bool:
            done = done != 0
        if done.device != self.device:
            done = done.to(self.device)
        return self._reset(done.contiguous(), observe=return_observations)

    def _reset(self, done: torch.Tensor, observe: bool = True):
        err = self._cannot_reset()
        if err is not None:
            # the reference raises only when an env actually has to be created
            if bool(done.any()):
                raise err
            return self._observe(self.observation_mode) if observe else None
        envs = self._state()
        m, n, obs = self._out_obs(observe)
        self._launch_reset(envs, done, obs, m, n, self._next_call())
        return obs

    # ------------------------------------------------------------------ observations, fused loops

    def _mode_info(self, observation_mode: str):
        """(mode code, window size, observation shape) of an observation mode string, cached per string."""
        key = (observation_mode, self.observation_mode if isinstance(observation_mode, str) and
               observation_mode.startswith('partial_') else None)
        info = self._mode_cache.get(key)
        if info is None:
            m, n = self._parse_mode(observation_mode)
            shape = self._obs_shape(observation_mode if m != _lib.OBS_PARTIAL else f'partial_{n}')
            info = self._mode_cache[key] = (m, n, shape)
        return info

    def _out_mode(self):
        """`_mode_info` of the env's own mode, as reset and rollout ask for it"""
        return self._mode_info(self.observation_mode)

    def _out_obs(self, want: bool, lead: tuple = ()):
        """(mode code, window size, a fresh observation tensor with `lead` in front of its shape), or "no observation" """
        if not want:
            return _lib.OBS_NONE, 0, None
        m, n, shape = self._out_mode()
        return m, n, torch.empty(lead + tuple(shape), dtype=torch.float32, device=self.device)

    def _get_rgb(self) -> torch.Tensor:
        """reference single_snake.py:104-128, simple_gridworld.py:88-109 — int16 RGB image (N,3,S,S)"""
        return (self._observe('default') * 255).round().short()

    def rollout(self, actions: torch.Tensor, return_observations: bool = True) -> dict:
        """T iterations of `obs, r, d, info = env.step(actions[t]); env.reset(d)` in one kernel launch.

        actions: (T, num_envs) int64/int32 on the device (SingleSnake sanitises them in place).  Returns a dict of
        (T, N, ...) tensors (`observations`, `rewards`, `dones` and the class's collision flags), bit-identical to the
        Python loop.
        """
        if actions.dtype not in (torch.int, torch.long):
            raise TypeError('actions Tensor must be an integer type i.e. {torch.IntTensor, torch.LongTensor}')
        if actions.dim() != 2 or actions.shape[1] != self.num_envs:
            raise RuntimeError('Must have the same number of actions as environments.')
        if not actions.is_contiguous() or actions.device != self.device:
            raise RuntimeError('rollout actions must be a contiguous device tensor')
        start = self._start_args()
        T, N = actions.shape
        m, n, obs = self._out_obs(return_observations, (T,))
        reward = torch.empty((T, N), dtype=torch.float32, device=self.device)
        flags = torch.empty((len(self._FLAG_KEYS), T, N), dtype=torch.bool, device=self.device).unbind(0)
        dt = _lib.ACT_I64 if actions.dtype == torch.long else _lib.ACT_I32
        # With a mirror (large batches) the launch reads it instead of the planes where its kernels serve the rollout and
        # keeps it current, lazy: without writing the planes (wurm_single_rollout_resident, wurm_grid_rollout_resident);
        # where they do not, the library writes a lazy mirror out, rolls out on the planes and reports the mirror stale.
        # Same protocol as step(): a postponed reset is applied first, a watched tensor is checked for in-place edits,
        # nothing is "touched".
        mirrored = False
        if T > 0 or not self._EMPTY_ROLLOUT_SKIPS_MIRROR:
            if self._fs.pending:
                self._flush()
            self._mirror_sync()
            self._setup_mirror(*((m, n) if return_observations else self._out_mode()[:2]))
            mirrored = T > 0 and bool(self._c.resident)
        c = self._c
        if mirrored:
            envs = self._checked(self._envs)
            self._fs.last_fresh = False
            self._chk_void_at = self._fs.steps
            valid = ctypes.c_int(c.resident_valid)
            mirror = (c.resident, ctypes.addressof(valid), int(c.resident_lazy))
        else:
            envs = self._state()
            mirror = (None, None)   # (the plain entry point: no recorded outcomes to inject)
        rc = _lib.call(self.device.index, getattr(_lib.lib(), self._ROLLOUT_FNS[mirrored]),
                       _lib.ptr(envs), _lib.ptr(actions), dt, _lib.ptr(reward), *[_lib.ptr(f) for f in flags], _lib.ptr(obs),
                       m, n, _lib.i64(N), self.size, _lib.i64(T), *start, _lib.u64(self.seed),
                       _lib.u64(self._next_call(2 * T)), _lib.i64(self.env_offset), *mirror,
                       _lib.stream_ptr(self.device.index))
        if mirrored:
            c.resident_valid = valid.value if rc == _lib.OK else 0
        _lib.check(rc, self._NAME + '.rollout')
        self._done_all_false()  # every done env was reset
        return dict(observations=obs, rewards=reward, **dict(zip(self._FLAG_KEYS, flags)))

    def _policy_rollout(self, params: torch.Tensor, state: torch.Tensor, num_steps: int, check: bool, mode_args: tuple,
                        population: int = None) -> dict:
        """What the classes' policy_rollout share once their preconditions hold (mode_args: what the class's entry point
        takes between `status` and the batch size).  population: None, or the number of members P — params is then
        (P, num_params) and member p acts in the envs [p N / P, (p + 1) N / P) (the entry point _POLICY_POP_FN)."""
        shape = self._mode_info(self.observation_mode)[2]
        N, T, E = self.num_envs, int(num_steps), int(torch.Size(shape[1:]).numel())
        num_params = 64 * E + 64 + 64 * 64 + 64 + 4 * 64 + 4 + 64 + 1
        if population is not None:  # (argument errors first: nothing below touches the library before them)
            P = int(population)
            if P <= 0 or N % P != 0:
                raise RuntimeError(f'population must be a positive divisor of num_envs ({N}), got {population}')
            if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.device != self.device or \
                    not params.is_contiguous() or tuple(params.shape) != (P, num_params):
                raise RuntimeError(f'params must be a contiguous fp32 ({P}, {num_params}) device tensor: one row of '
                                   f'pack_policy_params per member')
        elif params.dtype != torch.float32 or params.device != self.device or not params.is_contiguous() or \
                params.numel() != num_params:
            raise RuntimeError('params must be the contiguous fp32 device tensor of pack_policy_params for this observation size')
        if state.device != self.device or state.numel() != N * E:
            raise RuntimeError('state must be the current observation of every env on the env device')
        state = state.to(torch.float32).contiguous()
        envs = self._state()
        dev = self.device
        actions = torch.empty((T, N), dtype=torch.long, device=dev)
        probs = torch.empty((T, N, 4), dtype=torch.float32, device=dev)
        values = torch.empty((T, N), dtype=torch.float32, device=dev)
        reward = torch.empty((T, N), dtype=torch.float32, device=dev)
        flags = torch.empty((len(self._FLAG_KEYS), T, N), dtype=torch.bool, device=dev).unbind(0)
        obs = torch.empty((T,) + tuple(shape), dtype=torch.float32, device=dev)
        status = torch.empty(N, dtype=torch.uint8, device=dev)
        members = () if population is None else (_lib.i64(population),)
        rc = _lib.call(dev.index, getattr(_lib.lib(), self._POLICY_FN if population is None else self._POLICY_POP_FN),
                       _lib.ptr(envs), _lib.ptr(state), _lib.ptr(params), _lib.ptr(actions), _lib.ptr(probs),
                       _lib.ptr(values), _lib.ptr(reward), *[_lib.ptr(f) for f in flags], _lib.ptr(obs), _lib.ptr(status),
                       *mode_args, _lib.i64(N), self.size, _lib.i64(T), *self._start_args(), _lib.u64(self.seed),
                       _lib.u64(self._next_call(2 * T)), _lib.i64(self.env_offset), _lib.stream_ptr(dev.index), *members)
        _lib.check(rc, self._NAME + '.policy_rollout')
        if check and T > 0 and bool(status.any()):
            raise RuntimeError(f'policy_rollout: {self._BAD_STATUS} (status != 0); they were left untouched')
        self._done_all_false()  # every done env was reset
        return dict(actions=actions, probs=probs, values=values, rewards=reward, **dict(zip(self._FLAG_KEYS, flags)),
                    observations=obs, state=obs[-1] if T > 0 else state.reshape(shape), status=status)

    # ------------------------------------------------------------------ frames of a fused window (extension)

    def record_start(self, select) -> 'FrameRecord':
        """Call right before a fused window (`rollout`, `policy_rollout`) whose frames are wanted for the envs `select`
        (a list or int64 tensor of env indices of this object, any order; an index outside [0, num_envs) is reported by
        `record_frames` in `status`, not here).  Applies a postponed reset, copies those envs' planes and notes the call
        counter, seed, env_offset, size and start location the window will run with.  Nothing a later call returns
        changes: the counter is not consumed and the planes are only read.  What it does besides reading: the postponed
        reset runs now instead of inside the next launch, and a lazy mirror is written out to `envs` (it stays current)."""
        sel = torch.as_tensor(select, dtype=torch.long).to(self.device).reshape(-1).contiguous()
        if sel.numel() == 0:
            raise RuntimeError('record_start: select is empty')
        start_args = self._start_args()
        if self._fs.pending:
            self._flush()
        self._write_out()
        # (not `_state`: a `reset(done)` that follows a step directly keeps the observation that step's launch made for it)
        envs = self._checked(self._envs)
        # (the gather itself must stay inside the tensor: what is out of range is the replay kernel's to report)
        start = envs.index_select(0, sel.clamp(0, self.num_envs - 1))
        return FrameRecord(self, sel, start, int(self._fs.call), start_args)

    def record_frames(self, rec: 'FrameRecord', actions: torch.Tensor) -> dict:
        """The frames of the window run right after `rec = env.record_start(select)`: `actions` is `out['actions']` of
        that `policy_rollout` (any `population=`: indices are the object's) or `rollout` call, (T, num_envs) int64.
        One launch replays the selected envs from their saved planes (wurm_amd/csrc/rollout_frames.hpp).  Returns
        `frames` (T + 1, k, 3, S, S) uint8 on the device — frame t is what `_get_rgb()[select]` shows before step t,
        frame T what the window left behind —, `final` (k, C, S, S): the planes after the window (== env.envs[select]) and
        `status` (k) uint8: 1 where `select` was outside [0, num_envs) (that env's frames and planes are zeros).

        The rule that ties `rec` to the window: every entry point that draws random numbers takes its counters from
        `_next_call` — `step` 1, a `reset` (postponed or not) 1, `_create_envs` 1, a window of T steps 2 T (step t uses
        c + 2 t, its reset c + 2 t + 1).  `record_start` notes the counter c it saw; here the object's counter must be
        exactly c + 2 T, T = actions.shape[0]: the window, and nothing else that consumed a counter, ran in between
        — and `record_frames` comes before the next such call.  RuntimeError otherwise, for a `rec` of another object and
        for actions of another shape, dtype or device, and if `start_location` is no longer the one `record_start` saw.
        What cannot be seen here, because it consumes no counter: assigning or editing `env.envs` between `record_start`
        and the window (`final` then differs from `env.envs[select]`).  And `policy_rollout` leaves an env outside its
        domain untouched (its `status` != 0: not a well-formed snake / not one agent and one food, only ever by hand)
        while the replay steps whatever planes it was given: for such an env the frames are not what the window did,
        and again `final` differs from `env.envs[select]` — look at the window's own `status` for the selected envs."""
        if not isinstance(rec, FrameRecord) or rec.owner() is not self:
            raise RuntimeError('record_frames: this record was started on another env object')
        N = self.num_envs
        if not isinstance(actions, torch.Tensor) or actions.dtype != torch.long or actions.dim() != 2 or \
                actions.shape[1] != N or actions.device != self.device or not actions.is_contiguous():
            raise RuntimeError(f'record_frames: actions must be the contiguous int64 (T, {N}) device tensor the window returned')
        T = int(actions.shape[0])
        if rec.start_args != tuple(self._start_args()):
            raise RuntimeError(f'record_frames: stale record — start_location was {rec.start_args} at record_start and is '
                               f'{tuple(self._start_args())} now')
        if int(self._fs.call) != rec.call + 2 * T or (rec.seed, rec.env_offset, rec.size) != (
                int(self.seed), int(self.env_offset), int(self.size)):
            raise RuntimeError(f'record_frames: stale record — it was started at call counter {rec.call} and a window of '
                               f'{T} steps ends at {rec.call + 2 * T}, but the counter is {int(self._fs.call)}: another '
                               f'call that draws random numbers ran since record_start besides the window')
        k, S, dev = rec.select.numel(), self.size, self.device
        frames = torch.empty((T + 1, k, 3, S, S), dtype=torch.uint8, device=dev)
        final = torch.empty((k, self._CHANNELS, S, S), dtype=torch.float32, device=dev)
        status = torch.empty(k, dtype=torch.uint8, device=dev)
        rc = _lib.call(dev.index, getattr(_lib.lib(), self._FRAMES_FN), _lib.ptr(rec.start), _lib.ptr(rec.select),
                       _lib.ptr(actions) if T > 0 else None, _lib.ptr(frames), _lib.ptr(final), _lib.ptr(status),
                       _lib.i64(k), _lib.i64(N), S, _lib.i64(T), *rec.start_args, _lib.u64(rec.seed), _lib.u64(rec.call),
                       _lib.i64(rec.env_offset), _lib.stream_ptr(dev.index))
        _lib.check(rc, self._NAME + '.record_frames')
        return dict(frames=frames, final=final, status=status)


class FrameRecord(object):
    """What `record_start` keeps of the moment before a window: the selected envs' planes and what keys their random draws."""

    def __init__(self, env, select, start, call, start_args):
        import weakref
        self.owner = weakref.ref(env)
        self.select, self.start, self.call, self.start_args = select, start, call, tuple(start_args)
        self.seed, self.env_offset, self.size = int(env.seed), int(env.env_offset), int(env.size)
