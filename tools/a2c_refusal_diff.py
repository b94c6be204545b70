#!/usr/bin/env python3
"""Do two builds of libwurm_hip.so refuse the same calls of the fused A2C learner with the same codes?  A CPU-box tool.

Every wurm_a2c_ff_* entry point of both libraries (the 15 that launch, the three workspace queries, pop_hyper and
hyper_parameter; not pop_exploit of a2c_pbt.hip) is called over a lattice of arguments: a well-formed base point with
non-null, 16-byte-aligned dummy addresses, then every single defect and every pair of defects of the lists below.  Pairs
pin which of WURM_ERR_INVALID_ARG and WURM_ERR_UNSUPPORTED wins.  Arguments are placed by the parameter names of
include/wurm_hip.h (`_lib.call_named`), so a defect applies to every entry point that has a parameter of its name.
Nothing is dereferenced or launched: every point of a launching entry point holds at least one refusing defect (the
base point is left out, and a nullable pointer set to null counts only beside one), and the tool stops if a point comes
back as anything but a refusal.  It exits at once where a GPU is visible.  pop_hyper and hyper_parameter work on host
memory: they get real buffers, the base point included, and what they write is compared too.

usage: tools/a2c_refusal_diff.py OTHER_LIBRARY [THIS_LIBRARY] > profiles/rNN_a2c_refusal_diff.txt   (exit status 1 on a difference)"""
import ctypes
import itertools
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the libraries, as wurm_amd._lib loads them)

from wurm_amd import _lib  # noqa: E402

N, T, E, MEMBERS = 8, 5, 75, 2
NUM_PARAMS = 64 * E + 64 + 4096 + 64 + 256 + 4 + 64 + 1
NULLABLE = ('values_out', 'returns_out', 'grad_norm', 'learn')
NAN, INF = math.nan, math.inf

# (parameter name, value): a defect of every entry point that has the parameter.  'short' / 'odd': see `point`
SIZES = [(n, v) for n in ('num_envs', 'num_rows') for v in (0, -1, N + 1, 2 ** 31)] + \
        [('num_steps', 0), ('num_inputs', 0), ('num_inputs', 5), ('num_inputs', 508), ('value_loss_kind', 2),
         ('num_members', 0), ('num_members', 65536)]
WORKSPACE = [('workspace', 'odd'), ('workspace_bytes', -1), ('workspace_bytes', 'short')]
OPTIMISER = [('step', 0), ('lr', NAN), ('lr', -1.0), ('beta1', 1.0), ('beta2', 1.0), ('eps', -1.0), ('num_params', 0),
             ('gamma_lambda', NAN), ('gamma_lambda', -1.0), ('gamma_lambda', INF)]


def base(fn, query):
    """the well-formed arguments of `fn` by name: distinct dummy addresses for its pointers"""
    values = {'num_envs': N, 'num_rows': N, 'num_steps': T, 'num_inputs': E, 'num_members': MEMBERS, 'value_loss_kind': 0,
              'gamma': 0.99, 'entropy_coef': 0.01, 'gamma_lambda': 0.9405, 'step': 1, 'lr': 1e-3, 'beta1': 0.9,
              'beta2': 0.999, 'eps': 1e-8, 'max_grad_norm': 0.5, 'num_params': NUM_PARAMS, 'stream': None}
    pointers = [n for n, t in zip(fn.argnames, fn.argtypes) if t is ctypes.c_void_p and n != 'stream']
    values.update((n, 0x10000 * (i + 1)) for i, n in enumerate(pointers))
    if query is not None:
        values['workspace_bytes'] = _lib.call_named(None, query, values)
    return values, pointers


def point(values, defects):
    v = dict(values)
    for name, value in defects:
        v[name] = {'odd': values.get('workspace', 0) + 4, 'short': values.get('workspace_bytes', 0) - 1}.get(value, value) \
            if isinstance(value, str) else value
    return v


def lattice(fn, pointers, never_launches=False):
    """every single defect and every pair on different parameters; for a launching entry point only those that refuse"""
    defects = [(n, None) for n in pointers] + [d for d in SIZES + WORKSPACE + OPTIMISER if d[0] in fn.argnames]

    def refuses(d):  # a nullable pointer may be null; N + 1 columns are refused for the base point's workspace only
        return not (d[1] is None and d[0] in NULLABLE) and (d[1] != N + 1 or 'workspace' in fn.argnames)
    points = [(d,) for d in defects] + [p for p in itertools.combinations(defects, 2) if p[0][0] != p[1][0]]
    return ([()] if never_launches else []) + [p for p in points if never_launches or any(map(refuses, p))]


def host_calls(lib):
    """pop_hyper and hyper_parameter on real host buffers: [(what, (return value, what it wrote))]"""
    rows, P = [], 65536
    for lr, gl, members, null in itertools.product((1e-3, NAN, -1.0, 0.0), (None, 0.9405, NAN, -1.0, INF), (MEMBERS, 0, P),
                                                   (None, 'lr', 'gamma', 'entropy_coef', 'gamma_lambda', 'table')):
        cols = {'lr': np.full(P, lr, np.float32), 'gamma': np.full(P, 0.99, np.float32),
                'entropy_coef': np.full(P, 0.01, np.float32),
                'gamma_lambda': None if gl is None else np.full(P, gl, np.float32), 'table': np.full((P, 4), -7.0)}
        values = {n: None if c is None or n == null else c.ctypes.data for n, c in cols.items()}
        values['num_members'] = members
        rc = _lib.call_named(None, lib.wurm_a2c_ff_pop_hyper, values)
        rows.append((f'wurm_a2c_ff_pop_hyper lr={lr} gamma_lambda={gl} members={members} null={null}',
                     (rc, cols['table'].tobytes())))
    for x in (0.999, 1e-3, 1e-8, 0.1, 0.0, -0.0, 1.0, 3.4e38, 1e-45, NAN, INF, -INF, 0.99900001287460327, 1 / 3):
        out = ctypes.c_double(-7.0)
        rc = _lib.call_named(None, lib.wurm_a2c_ff_hyper_parameter, {'x': x, 'value': ctypes.addressof(out)})
        rows.append((f'wurm_a2c_ff_hyper_parameter x={x}', (rc, bytes(out))))
    rows.append(('wurm_a2c_ff_hyper_parameter value=NULL',
                 _lib.call_named(None, lib.wurm_a2c_ff_hyper_parameter, {'x': 0.5, 'value': None})))
    return rows


def results(lib):
    """[(what, result)] of every point, in one fixed order"""
    rows = host_calls(lib)
    for kind in ('', 'pop_', 'league_'):
        query = getattr(lib, f'wurm_a2c_ff_{kind}workspace_bytes')
        values, _ = base(query, None)
        rows += [(f'{query.__name__} {p}', _lib.call_named(None, query, point(values, p)))
                 for p in lattice(query, [], never_launches=True)]
        for what in ('grad', 'grad_gae', 'apply', 'update', 'update_gae'):
            fn = getattr(lib, f'wurm_a2c_ff_{kind}{what}')
            values, pointers = base(fn, query)
            for p in lattice(fn, pointers):
                rc = _lib.call_named(None, fn, point(values, p))
                if rc not in (_lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED):
                    sys.exit(f'{fn.__name__} {p}: returned {rc}, not a refusal: the lattice is wrong')
                rows.append((f'{fn.__name__} {p}', rc))
    return rows


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    if os.path.exists('/dev/kfd') or torch.cuda.is_available():
        sys.exit('a GPU is visible: this tool runs on a CPU box only')
    libs = []
    for path in (sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else _lib.LIB_PATH):
        lib = ctypes.CDLL(os.path.abspath(path))
        _lib._declare_prototypes(lib)
        libs.append(lib)
    other, this = results(libs[0]), results(libs[1])
    assert [w for w, _ in other] == [w for w, _ in this]
    differ = [(w, a, b) for (w, a), (_, b) in zip(other, this) if a != b]
    per_fn = {}  # name: [points, of them WURM_ERR_INVALID_ARG, WURM_ERR_UNSUPPORTED]
    for what, res in this:
        row = per_fn.setdefault(what.split()[0], [0, 0, 0])
        rc = res[0] if isinstance(res, tuple) else res
        row[0] += 1
        row[1] += rc == _lib.ERR_INVALID_ARG
        row[2] += rc == _lib.ERR_UNSUPPORTED
    print(f'# refusal codes, queried byte counts and host results of the wurm_a2c_ff_* entry points, two libraries, base point '
          f'N={N} T={T} E={E} members={MEMBERS}')
    print(f'# {"entry point":34s} {"points":>6s} {"invalid":>8s} {"unsupported":>12s}   (of this library)')
    for name, (count, invalid, unsupported) in per_fn.items():
        print(f'{name:36s} {count:6d} {invalid:8d} {unsupported:12d}')
    print(f'{"total":36s} {len(this):6d} points, {len(differ)} differ')
    for w, a, b in differ:
        print(f'DIFFERS {w}: {a!r} -> {b!r}')
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
