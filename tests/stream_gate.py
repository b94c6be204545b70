"""The stream gate: makes a launch on the wrong stream, or a hidden host synchronisation, fail a test deterministically.

include/wurm_hip.h: "Nothing is allocated, freed or synchronised here: each call enqueues kernels on `stream`".  On the
legacy default stream, where the rest of the suite runs, everything serialises with everything else and neither breach
can be seen.  Here a case's call is made on a side stream behind a GATE: a `torch.cuda._sleep` of at least 50 ms, then an
event `opened`, then the in-place copy of the inputs B over the inputs A the warm call ran on, then the call.

    after the call returns:  default_stream().synchronize();  assert not opened.query()

says that the call did not block the host, and that whatever it put on the default stream has already run — while the
inputs still held A.  Afterwards every output and every piece of state is compared bit for bit with a run of the same
calls on the default stream: a launch that went to the default stream computed on A (or on outputs not yet written) and
shows as a mismatch.  The gate's length is no tolerance: a gate that is too short fails the assertion, it cannot pass a case.
Torch operations only: no kernel of its own, no flag polled by the host."""
import torch

from wurm_amd import _lib

GATE_MS = 50.0


class GateFailure(AssertionError):
    """a case was reported: `kind` is 'open' (the gate had opened when the call returned: the call waited on the host, or
    the side stream does not run beside the default stream), 'mismatch' (a result differs from the default-stream run) or
    'blind' (the two calls of the expected run gave the same results: the case could not see anything)"""

    def __init__(self, kind, text):
        super().__init__(f'[{kind}] {text}')
        self.kind = kind


class Case(object):
    """make() -> x: one object or one set of buffers;  call(x, inputs) -> dict of the tensors the call returned or wrote,
    free of synchronisation by contract;  a() / b() -> two tuples of valid device inputs of the same shapes;
    state(x) -> dict of the tensors the object holds (read after everything has run);  covers: the entry points of
    include/wurm_hip.h the call reaches;  knobs: library options in force for the whole case;
    route: None or (function that names the launch the case is about, the expected name), asserted on the expected run;
    min_launches: how many kernels the second call of the expected run must at least launch (wurm_launch_count)."""

    def __init__(self, name, make, call, a, b, covers, state=None, knobs=None, route=None, patch=None, min_launches=1):
        self.name, self.make, self.call, self.a, self.b = name, make, call, a, b
        self.min_launches = min_launches
        self.covers, self.state, self.knobs, self.route, self.patch = tuple(covers), state, dict(knobs or {}), route, patch

    def __repr__(self):
        return self.name


_cycles = None


def calibrate():
    """(cycles, milliseconds) of the gate: `_sleep` timed between two events on a side stream, doubled from 10^6 until it
    lasts GATE_MS; once per session."""
    global _cycles
    if _cycles is None:
        s = torch.cuda.Stream()
        cycles = 10 ** 6
        while True:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                start.record()
                torch.cuda._sleep(cycles)
                end.record()
            end.synchronize()
            ms = start.elapsed_time(end)
            if ms >= GATE_MS:
                break
            cycles *= 2
            if cycles > 2 ** 40:
                raise RuntimeError(f'stream gate: torch.cuda._sleep(2^40) lasts {ms} ms, less than {GATE_MS} ms')
        _cycles = (cycles, ms)
        print(f'stream gate: {cycles} cycles = {ms:.1f} ms')
    return _cycles


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8) if t.dtype != torch.bool else t.to(torch.uint8)


def _flat(prefix, value, into):
    """tensors of a (nested) result under dotted names; what is no tensor (None, numbers, strings) is left out"""
    if isinstance(value, torch.Tensor):
        into[prefix] = value
    elif isinstance(value, dict):
        for k, v in value.items():
            _flat(f'{prefix}.{k}', v, into)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _flat(f'{prefix}.{i}', v, into)
    return into


def _snapshot(out, buf, state):
    torch.cuda.synchronize()
    snap = _flat('out', out, {})
    _flat('in', list(buf), snap)
    if state is not None:
        _flat('state', state, snap)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in snap.items()}


def _differs(p, q):
    return sorted(p) != sorted(q) or any(p[k].shape != q[k].shape or not torch.equal(_bits(p[k]), _bits(q[k])) for k in p)


def expected(case):
    """The case on the default stream: make(), call(x, A), call(x, B) on the same input buffers.  Returns everything the
    second call wrote, the inputs as it left them and the state the object holds; GateFailure('blind') if the first
    call's results do not differ from it."""
    x = case.make()
    buf = [t.clone() for t in case.a()]
    first = _snapshot(case.call(x, buf), buf, None)
    for t, b in zip(buf, case.b()):
        t.copy_(b)
    count = _lib.lib().wurm_launch_count if case.min_launches else (lambda: 0)
    before = count()
    out = case.call(x, buf)
    launched = count() - before
    assert launched >= case.min_launches, f'{case.name}: the call launched {launched} kernels, expected at least {case.min_launches}'
    if case.route is not None:
        name, want = case.route
        got = name()
        assert got == want, f'{case.name}: served by {got!r}, the case is about {want!r}'
    second = _snapshot(out, buf, case.state(x) if case.state else None)
    outs = lambda snap: {k: v for k, v in snap.items() if k.startswith('out')}   # noqa: E731
    if not _differs(outs(first), outs(second)):
        raise GateFailure('blind', f'{case.name}: call(x, A) and call(x, B) gave the same results')
    return second


class Gated(object):
    """One gated run in its steps, so that two of them can be interleaved (tests of two streams at once)."""

    def __init__(self, case, cycles=None):
        self.case, self.cycles = case, cycles if cycles is not None else calibrate()[0]
        self.stream = torch.cuda.Stream()
        self.opened = torch.cuda.Event()

    def warm(self):
        """twin object and the warm call on the default stream: mirrors, workspaces and first-call costs are paid, and every
        buffer a misrouted launch could read holds the valid state of A"""
        self.x = self.case.make()
        self.buf = [t.clone() for t in self.case.a()]
        self.b = [t.clone() for t in self.case.b()]
        self.case.call(self.x, self.buf)
        torch.cuda.synchronize()
        return self

    def enqueue(self):
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(self.cycles)
            self.opened.record()
            for t, b in zip(self.buf, self.b):
                t.copy_(b)
            self.out = self.case.call(self.x, self.buf)
        return self

    def still_closed(self):
        """after the call(s) returned: what is on the default stream runs to completion, and the gate must not have opened"""
        torch.cuda.default_stream().synchronize()
        if self.opened.query():
            raise GateFailure('open', f'{self.case.name}: the gate had opened when the call returned — the call '
                                      f'synchronised with the host, or the side stream did not run beside the default stream')
        return self

    def collect(self):
        self.stream.synchronize()
        return _snapshot(self.out, self.buf, self.case.state(self.x) if self.case.state else None)


def compare(case, want, got):
    if sorted(want) != sorted(got):
        raise GateFailure('mismatch', f'{case.name}: results {sorted(got)} instead of {sorted(want)}')
    bad = [k for k in want if want[k].shape != got[k].shape or not torch.equal(_bits(want[k]), _bits(got[k]))]
    if bad:
        raise GateFailure('mismatch', f'{case.name}: {bad} differ from the default-stream run — a launch did not wait '
                                      f'for prior work on the current stream')


def _patched(case):
    import contextlib
    stack = contextlib.ExitStack()
    stack.enter_context(_lib.knobs(**case.knobs))
    if case.patch is not None:
        stack.enter_context(case.patch())
    return stack


def run_case(case):
    """expected run, gated run, comparison; GateFailure if the case is reported"""
    with _patched(case):
        try:
            want = expected(case)
            g = Gated(case).warm().enqueue().still_closed()
            compare(case, want, g.collect())
        finally:
            torch.cuda.synchronize()


def run_pair(case1, case2):
    """Two objects gated on two streams, every call enqueued before either gate opens, the second gate twice the first:
    completion order is the reverse of enqueue order.  Each must equal its run alone (no state shared between calls)."""
    with _patched(case1), _patched(case2):
        try:
            want1, want2 = expected(case1), expected(case2)
            cycles = calibrate()[0]
            g2, g1 = Gated(case2, 2 * cycles).warm(), Gated(case1, cycles).warm()
            g2.enqueue()
            g1.enqueue()
            g2.still_closed()
            g1.still_closed()
            compare(case1, want1, g1.collect())
            compare(case2, want2, g2.collect())
        finally:
            torch.cuda.synchronize()
