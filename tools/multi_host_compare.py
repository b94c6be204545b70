"""MultiSnake's host layer from outside, without a GPU: which library entry points a scripted set of caller sequences
reaches, in which order and with which scalar arguments, and what `mirror_state()` says after every call — to compare two
checkouts of the package (a refactor of wurm_amd/envs/multi_snake.py must leave all of it equal) — and the host time per
iteration of the per-call loop over the same stand-in.

    python tools/multi_host_compare.py record OUT.json [--root CHECKOUT]    the log of this (or another) checkout
    python tools/multi_host_compare.py compare A.json B.json                equal? (exit status 1 if not)
    python tools/multi_host_compare.py time [--root CHECKOUT]               one JSON line: us per iteration, K = 4, N = 64

The stand-in is the recording one of tests/test_host_multi_mirror.py, extended to record the scalars it is given (counters,
modes, flags, T, the configuration block) and what the argument block says; pointers are recorded as null / not null.
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time


def _install(root):
    sys.path.insert(0, root)
    import torch
    from wurm_amd import _lib
    from tests.test_host_multi_mirror import _Lib

    def val(x):
        if x is None:
            return None
        if isinstance(x, ctypes.c_void_p):
            return 'ptr' if x.value else 'null'
        if hasattr(x, '_obj'):                       # byref(configuration block)
            return bytes(x._obj).hex()
        if hasattr(x, 'value'):
            return x.value
        return x

    def block(c_addr):
        c = _lib.MultiCall.from_address(c_addr)
        d = {n: bool(getattr(c, n)) for n in ('foods', 'heads', 'bodies', 'dones', 'orientations', 'colours', 'all_done_copy',
                                              'resident', 'check_mask', 'check_mask_after')}
        d.update({n: int(getattr(c, n)) for n in ('num_envs', 'env_offset', 'seed', 'num_snakes', 'size', 'obs_mode', 'obs_n',
                                                  'resident_valid', 'resident_lazy')})
        d['cfg'] = bytes(c.cfg).hex()
        return d

    class Recorder(_Lib):
        def _rec(self, name, args):
            self.calls.append((name, args))

        def wurm_multi_colours(self, *a):
            self._rec('colours', [val(x) for x in a[1:7]])
            return 0

        def wurm_multi_reset(self, *a):
            self._rec('reset', [val(x) for x in a[:20]])
            return 0

        def wurm_multi_observe(self, *a):
            self._rec('observe', [val(x) for x in a[:12]])
            return 0

        def wurm_multi_check(self, *a):
            self._rec('check', [val(x) for x in a[5:8]])
            ctypes.memset(a[4].value, 0, 4 * int(val(a[5])))
            return 0

        def wurm_multi_rollout(self, *a):
            self._rec('rollout', [val(x) for x in a[:24]])
            return 0

        def wurm_multi_rollout_resident(self, *a):
            valid = ctypes.c_int.from_address(a[23])
            self._rec('rollout_resident', [val(x) for x in a[:22]] + [bool(a[22]), valid.value, a[24]])
            if self.rollout_keeps_mirror:
                valid.value = 1
            else:
                if a[24] and valid.value:
                    self._rec('flush_by_library', [])
                valid.value = 0
            return 0

        def wurm_multi_resident_bytes(self, N, K, S):
            self._rec('resident_bytes', [val(N), val(K), val(S)])
            return self.mirror_bytes * int(val(N)) if int(val(N)) >= self.threshold else 0

        def wurm_multi_resident_size(self, N, K, S):
            self._rec('resident_size', [val(N), val(K), val(S)])
            return self.mirror_bytes * int(val(N))

        def wurm_multi_resident_flush(self, c_addr, stream):
            self._rec('flush', block(c_addr))
            return 0

        def step_slot(self, c_addr, sl_addr, slot, actions, call, pending, pre_call, want_after, stream):
            sl = _lib.MultiSlabs.from_address(sl_addr)
            d = block(c_addr)
            d.update(slot=int(slot), call=int(call), pending=bool(pending), pre_call=int(pre_call) if pending else None,
                     want_after=bool(want_after), slab_steps=int(sl.steps), obs_elems=int(sl.obs_elems),
                     obs_after=bool(sl.obs_after))
            self._rec('step', d)
            c = _lib.MultiCall.from_address(c_addr)
            if c.resident:
                c.resident_valid = 1
            return 0

    lib = Recorder()
    lib.threshold = 0
    _lib.lib = lambda: lib
    _lib.require_device = lambda d: torch.device('cpu')
    _lib.stream_ptr = lambda i=None: 0
    _lib.call = lambda idx, fn, *a: fn(*a)
    _lib.accessors = lambda: ((lambda: None), (lambda i: 0))
    _lib.step_slot_fn = lambda name='wurm_multi_step_slot': lib.step_slot
    _lib.torch_helpers = lambda: None
    _lib.ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return lib, torch


N, K, S = 6, 2, 12


def _sequences(torch, MultiSnake, lib):
    """name -> a generator function of (label, value the caller saw) over one env object"""
    keys = ['agent_%d' % i for i in range(K)]
    tape = torch.zeros((64, K, N), dtype=torch.long)

    def acts(t):
        return dict(zip(keys, tape[t]))

    def seen(x):
        if isinstance(x, dict):
            return [type(x).__name__] + [[k, seen(v)] for k, v in x.items()]
        if isinstance(x, (tuple, list)):
            return [seen(v) for v in x]
        if isinstance(x, torch.Tensor):
            return [list(x.shape), str(x.dtype)]
        return x

    def plain(env, obs):
        for t in range(12):
            o = env.step(acts(t))
            yield 'step', seen(o)
            yield 'reset', seen(env.reset(o[2]['__all__'], return_observations=obs) if obs is not None else
                                env.reset(o[2]['__all__']))

    def attributes(env):
        yield from plain(env, False)
        for name in ('foods', 'heads', 'bodies', 'dones', 'orientations', 'agent_colours'):
            x = getattr(env, name)
            yield 'read ' + name, seen(x)
            yield 'step', seen(env.step(acts(0)))
            del x
            yield 'step', seen(env.step(acts(1)))
            setattr(env, name, getattr(env, name).clone())
            yield 'assign ' + name, None
            o = env.step(acts(2))
            yield 'step', seen(o)
            yield 'reset', seen(env.reset(o[2]['__all__'], return_observations=False))

    def alias(env):
        yield from plain(env, False)
        b = env.bodies
        yield 'read', None
        yield 'step', seen(env.step(acts(0)))
        b[0, 0, 1, 1] = 3.0
        yield 'edit', None
        yield 'step', seen(env.step(acts(1)))
        yield 'step', seen(env.step(acts(2)))
        b[0, 0, 1, 2] = 3.0
        yield 'check', env.check_consistency()
        f = env.foods
        yield 'read another', None
        del b, f
        yield 'step', seen(env.step(acts(3)))
        yield 'step', seen(env.step(acts(4)))

    def checks(env):
        for t in range(14):
            o = env.step(acts(t))
            yield 'step', seen(o)
            yield 'reset', seen(env.reset(o[2]['__all__'])) if t % 2 else seen(env.reset(o[2]['__all__'], False))
            if env._chk is not None:
                env._chk.zero_()
            yield 'check', env.check_consistency()
        for t in range(70):                      # ... and stopping it: the masks are dropped again
            o = env.step(acts(t % 64))
            yield 'step', None
            env.reset(o[2]['__all__'], return_observations=False)
            yield 'reset', None

    def dynamics(env):
        for t, (name, value) in enumerate((('food_rate', 0.25), ('respawn_mode', 'any'), ('observation_mode', 'partial_2'),
                                           ('food_rate', 0.5), ('respawn_mode', 'all'), ('observation_mode', 'full'))):
            o = env.step(acts(t))
            yield 'step', seen(o)
            yield 'reset', seen(env.reset(o[2]['__all__'], return_observations=bool(t % 2)))
            setattr(env, name, value)
            yield 'assign ' + name, None
        yield 'step', seen(env.step(acts(7)))

    def rollouts(env):
        for keeps in (True, False):
            lib.rollout_keeps_mirror = keeps
            yield 'rollout 0', seen(env.rollout(tape[:0]))
            yield 'rollout 3', seen(env.rollout(tape[:3]))
            yield 'rewards', seen(env.rewards)
            o = env.step(acts(0))
            yield 'step', seen(o)
            yield 'reset', seen(env.reset(o[2]['__all__'], return_observations=False))
            yield 'rollout 2', seen(env.rollout(tape[:2], return_observations=False))
            yield 'step', seen(env.step(acts(1)))
            yield 'observe', seen(env._observe('full'))
            yield 'rollout 0', seen(env.rollout(tape[:0]))
        lib.rollout_keeps_mirror = False

    def lifetimes(env):
        yield from plain(env, False)
        yield 'env_lifetimes', seen(env.env_lifetimes)
        yield from plain(env, None)

    def eager_resets(env):
        for t in range(12):                      # every step followed by a foreign write: the "off" rule
            yield 'step', seen(env.step(acts(t)))
            yield 'reset', seen(env.reset(torch.ones(N, dtype=torch.bool), return_observations=False))

    def stacked(env):
        for t in range(4):
            a = {k: torch.zeros(N, dtype=torch.long) for k in keys}
            yield 'step', seen(env.step(a))
        yield 'step int32', seen(env.step({k: torch.zeros(N, dtype=torch.int32) for k in keys}))
        yield 'info', seen(dict(env.info))
        yield 'rewards', seen(env.rewards)
        yield 'boost', seen(env.boost_this_step)

    def copies(env):
        yield from plain(env, False)
        o = env.step(acts(0))
        env.reset(o[2]['__all__'], return_observations=False)
        e2 = copy.deepcopy(env)
        yield 'deepcopy', e2.mirror_state()
        for e in (env, e2):
            yield from plain(e, None)
            yield 'state', e.mirror_state()

    def dropped_reset_obs(env):
        kept = None
        for t in range(8):
            o = env.step(acts(t))
            yield 'step', seen(o)
            env.reset(o[2]['__all__'])
            yield 'reset dropped', env._lazy_obs_mode
        o = env.step(acts(9))
        kept = env.reset(o[2]['__all__'])
        yield 'reset kept', type(kept).__name__
        yield 'step', seen(env.step(acts(10)))
        yield 'kept', seen(dict(kept))

    seqs = {}
    for pol in (None, True, False, 'eager'):
        for name, fn in (('plain noobs', lambda e: plain(e, False)), ('plain obs', lambda e: plain(e, None)),
                         ('attributes', attributes), ('alias', alias), ('checks', checks), ('dynamics', dynamics),
                         ('rollouts', rollouts), ('lifetimes', lifetimes), ('eager resets', eager_resets), ('stacked', stacked),
                         ('copies', copies), ('dropped reset obs', dropped_reset_obs)):
            seqs['%s, resident_mirror=%r' % (name, pol)] = (fn, dict(resident_mirror=pol))
    seqs['plain, below the threshold'] = (lambda e: plain(e, False), dict(_threshold=1 << 20))
    seqs['attributes, below the threshold'] = (attributes, dict(_threshold=1 << 20))
    seqs['plain noobs, half'] = (lambda e: plain(e, False), dict(dtype=torch.half))
    seqs['plain obs, half'] = (lambda e: plain(e, None), dict(dtype=torch.half))
    seqs['rollouts, half'] = (rollouts, dict(dtype=torch.half))
    seqs['plain noobs, lazy_reset=False'] = (lambda e: plain(e, False), dict(lazy_reset=False))
    seqs['plain obs, lazy_reset=False'] = (lambda e: plain(e, None), dict(lazy_reset=False))
    seqs['checks, lazy_reset=False'] = (checks, dict(lazy_reset=False))
    return seqs


def record(root):
    lib, torch = _install(root)
    from wurm_amd.envs import MultiSnake
    out = {}
    for name, (fn, kw) in _sequences(torch, MultiSnake, lib).items():
        kw = dict(kw)
        lib.threshold = kw.pop('_threshold', 0)
        lib.calls.clear()
        env = MultiSnake(N, K, S, device='cpu', seed=1, **kw)
        rows = [['construct', None, list(lib.calls), env.mirror_state()]]
        lib.calls.clear()
        for label, saw in fn(env):
            rows.append([label, saw, list(lib.calls), env.mirror_state()])
            lib.calls.clear()
        out[name] = rows
    return json.loads(json.dumps(out))


def host_time(root):
    """us per iteration of `step; reset(d, return_observations=False)` and `step; reset(d)` over the stand-in: K = 4, N = 64"""
    lib, torch = _install(root)
    from wurm_amd.envs import MultiSnake
    lib.step_slot = lambda *a: 0
    k, n = 4, 64
    res = {}
    for key, kw in (('step_reset_noobs', dict(return_observations=False)), ('step_reset_obs', {})):
        env = MultiSnake(n, k, 12, device='cpu', seed=1, resident_mirror=False)
        tape = torch.zeros((k, n), dtype=torch.long)
        a = {'agent_%d' % i: tape[i] for i in range(k)}
        times = []
        for rnd in range(16):                    # (the first round warms up; the fastest of the rest: the box is shared)
            iters = 5000
            t0 = time.perf_counter()
            for _ in range(iters):
                d = env.step(a)[2]
                env.reset(d['__all__'], **kw)
            times.append((time.perf_counter() - t0) / iters * 1e6)
        res[key] = round(min(times[1:]), 4)
    return res


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['record', 'compare', 'time'])
    ap.add_argument('files', nargs='*')
    ap.add_argument('--root', default=here)
    args = ap.parse_args()
    if args.what == 'record':
        with open(args.files[0], 'w') as f:
            json.dump(record(os.path.abspath(args.root)), f)
        return 0
    if args.what == 'time':
        print(json.dumps(host_time(os.path.abspath(args.root))))
        return 0
    a, b = (json.load(open(p)) for p in args.files)
    bad = 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if ra == rb:
            continue
        bad += 1
        for i, (x, y) in enumerate(zip(ra or [], rb or [])):
            if x != y:
                print('DIFFERENT %s, call %d (%s):\n  %s\n  %s' % (name, i, x[0], x, y))
                break
        else:
            print('DIFFERENT %s: lengths %s / %s' % (name, len(ra or []), len(rb or [])))
    calls = sum(len(r) for r in a.values())
    launches = sum(len(row[2]) for r in a.values() for row in r)
    print('%d sequences, %d caller events, %d library calls: %s' % (len(a), calls, launches,
                                                                    'EQUAL' if not bad else '%d sequences differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
