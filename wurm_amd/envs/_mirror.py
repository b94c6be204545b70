"""The resident mirror of an env object's state, as the host sees it (DESIGN.md §4.10, §5, §7 deviation 9): one controller
for SingleSnake, SimpleGridworld (wurm_single_call, through FastStepMixin) and MultiSnake (wurm_multi_call).

The step launch reads a compact image of the state (`resident`) instead of the fp32 tensors and marks it current
(`resident_valid`); in the lazy form (`resident_lazy`) it does not write the tensors either.  The tensors stay the state:
`write_out()` brings them up to date before something reads them, `touch()` also marks the mirror stale because something
other than the step launch writes them.  WHO holds a state tensor, and whether one was edited in place, is the env class's
business (the step machine's `watch` / MultiSnake's `_watched`): the controller is told `holds()`, `touch()`, `unwatchable()`.

Two adaptive rules, both only under the automatic policy (`resident_mirror=None`): the state looked at twice -> every step
writes the tensors from now on; the state written by something else after >= 8 and >= half of the steps since the mirror was
set up -> no mirror for this env object.
"""
import os

import torch

from wurm_amd import _lib


def parse_mirror_policy(value):
    """`resident_mirror` keyword of the env classes -> None (automatic: by batch size, with the adaptive rules), False
    (never), 'lazy' (whenever the shape is served, no adaptive rule; True means this) or 'eager' (the same, but every step
    also writes the state tensors)."""
    if value is None or value is False:
        return value
    if value is True or value == 'lazy':
        return 'lazy'
    if value == 'eager':
        return 'eager'
    raise ValueError("resident_mirror must be None, True, False, 'lazy' or 'eager'")


class Mirror(object):
    """block: the class's SingleCall / MultiCall (its `resident`, `resident_valid`, `resident_lazy` fields); fns: the
    library's size entry point with and without the batch threshold, and its flush; words: the texts of `why` that name the
    class's tensors ('written', 'touched', 'held', 'unwatchable', 'unserved', and 'refused' where the library has that verdict);
    held_without_mirror: `holds()` says so in `why` even while there is no mirror (MultiSnake: True, the single-env classes
    False — kept as it is because `mirror_state()` shows it)."""
    __slots__ = ('c', 'addr', 'fns', 'words', 'held_without_mirror', 'dev', 'policy', 'lazy', 'off', 'why', 'buf', 'key',
                 'write_outs', 'touches', 'step0')

    def __init__(self, block, addr, fns, policy, words, held_without_mirror, device):
        self.c, self.addr, self.fns, self.words, self.held_without_mirror = block, addr, fns, words, held_without_mirror
        self.dev = device.index
        self.policy = pol = parse_mirror_policy(policy)
        self.off = pol is False
        self.lazy = pol != 'eager' and os.environ.get('WURM_RESIDENT_LAZY', '1') != '0'
        self.why = 'resident_mirror=False' if pol is False else 'no step yet'
        self.buf = self.key = None       # the device buffer, and what it was set up for (None: not set up)
        self.write_outs = self.touches = self.step0 = 0

    def setup(self, key, size_args, steps, held, device):
        """the mirror for `key` (the single-env classes: one per observation mode), where the library offers one for
        `size_args`; the caller has written a lazy mirror for another key out (touch)"""
        c = self.c
        self.key = key
        nbytes = 0
        if not self.off:
            nbytes = int(getattr(_lib.lib(), self.fns[0 if self.policy is None else 1])(*size_args))
            self.why = 'on' if nbytes > 0 else self.words['unserved']
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes > 0 else None
        # the window of the "off" rule starts here (MultiSnake sets its mirror up once, before its first step: 0)
        self.touches, self.step0 = 0, steps
        c.resident = self.buf.data_ptr() if nbytes > 0 else None
        c.resident_valid = 0
        # lazy as long as the caller has never got hold of a state tensor, and has not been seen to keep looking at the state
        c.resident_lazy = int(nbytes > 0 and not held and self.lazy and (self.write_outs < 2 or self.policy is not None))
        if nbytes > 0 and held:
            self.why = self.words['held']

    def write_out(self):
        """the state tensors from a lazy mirror (which stays current)"""
        c = self.c
        # (== 1: 2 is SimpleGridworld's "refused" — the planes are the state; the other two libraries write 0 and 1 only)
        if c.resident_valid == 1 and c.resident and c.resident_lazy:
            rc = _lib.call(self.dev, getattr(_lib.lib(), self.fns[2]), self.addr, _lib.stream_ptr(self.dev))
            _lib.check(rc, self.fns[2])
            # a caller that keeps looking at the state (check_consistency() every step, experiments/main.py:214-215,
            # experiments/speeds.py:30-38) pays a whole-state write per look in the lazy form: from the second one on the
            # steps write the tensors themselves
            self.write_outs += 1
            if self.write_outs >= 2 and self.policy is None:
                c.resident_lazy = 0
                self.why = 'adaptive: the state was looked at twice, every step writes %s from now on' % self.words['written']

    def touch(self, steps):
        """something other than the step launch is about to write the state tensors (`steps`: the step machine's count)"""
        self.write_out()
        c = self.c
        if c.resident_valid and c.resident:
            # a loop in which (nearly) every step is followed by something that writes the state some other way — an eager
            # reset, a rollout — rebuilds the mirror every step for nothing (SimpleGridworld: with a synchronous read of the
            # build's verdict each time, and 2 = refused again while a hand-made env stays): off for this env object
            self.touches += 1
            window = steps - self.step0
            if self.policy is None and self.touches >= 8 and 2 * self.touches >= window:
                self.drop(self.words['touched'] % (self.touches, window))
        c.resident_valid = 0

    def holds(self):
        """the caller holds a state tensor from now on and may read it at any time: every step writes the tensors"""
        self.c.resident_lazy = 0
        self.lazy = False
        if self.buf is not None or (self.held_without_mirror and not self.off):
            self.why = self.words['held']

    def drop(self, why=None):
        """no mirror for this env object from now on"""
        self.off, self.buf, self.key = True, None, None
        self.c.resident = None
        if why is not None:
            self.why = why

    def unwatchable(self):
        """a state tensor the caller holds has no version counter (made under torch.inference_mode())"""
        self.drop(self.words['unwatchable'])
        self.c.resident_valid = 0

    def state(self) -> dict:
        """`mirror_state()` of the env classes: `state` 'off' / 'eager' (steps read the mirror and write the tensors) /
        'lazy' (steps do not write them; they are written out when something looks at them), `why`, `policy` (the
        `resident_mirror` keyword; None = automatic), `current` (the mirror describes the state; False: the next step
        rebuilds it), `bytes`."""
        c = self.c
        on = bool(c.resident) and self.buf is not None
        why = self.words['refused'] if on and c.resident_valid == 2 else self.why
        return {'state': 'off' if not on else ('lazy' if c.resident_lazy else 'eager'), 'why': why, 'policy': self.policy,
                'current': bool(on and c.resident_valid == 1), 'bytes': int(self.buf.numel()) if on else 0}
