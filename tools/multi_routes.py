#!/usr/bin/env python3
"""Which kernel serves which MultiSnake call — seen from OUTSIDE the library, to compare two builds of it.

  run      one launch of the library per case of tests/test_multi_dispatch_table.py (its CASES, its run_case), in order,
           and the too-large case that launches nothing; prints one line per case.  A target for
               rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python3 tools/multi_routes.py run [--root TREE]
           (no counters, no other tracing).  --root: the checkout whose wurm_amd / tests / oracle are imported (another
           revision, built); the cases are always this checkout's.
  compare  two such kernel traces, row by row over the library's MultiSnake kernels (the backend's torch copies and fills
           are dropped by name): kernel name, grid size, workgroup size, LDS size.  Exit status 1 on a difference.
               python3 tools/multi_routes.py compare BASE_kernel_trace.csv HEAD_kernel_trace.csv > profiles/rNN_multi_routes.txt"""
import argparse
import csv
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(root):
    sys.path.insert(0, os.path.abspath(root))
    spec = importlib.util.spec_from_file_location('multi_dispatch_cases', os.path.join(HERE, 'tests', 'test_multi_dispatch_table.py'))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    from tests.hip_backend import HipBackend
    from wurm_amd import _lib
    lib = _lib.lib()
    named = hasattr(lib, 'wurm_multi_last_route')
    for case, cid in zip(cases.CASES, cases.IDS):
        n0 = lib.wurm_launch_count()
        got, want = cases.run_case(HipBackend, case)
        same = all(a.tobytes() == b.tobytes() for (_, a), (_, b) in zip(got, want))
        print(f'{cid:60s} launches {lib.wurm_launch_count() - n0}  oracle {"same" if same else "DIFFERENT"}  '
              f'route {lib.wurm_multi_last_route().decode() if named else "-":32s} expected {case[-1]}', flush=True)
    if named:
        cases.test_an_env_too_large_for_the_lds_is_unsupported_and_launches_nothing(HipBackend)
        print('too large: unsupported, no launch')


def rows(path):
    out = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if 'wurm::multi_' in r['Kernel_Name']:
                out.append((r['Kernel_Name'].replace('void ', '').replace('(wurm::MultiArgs)', '').replace('wurm::', ''),
                            int(r['Grid_Size_X']), int(r['Workgroup_Size_X']), int(r['LDS_Block_Size'])))
    return out


def compare(base, head):
    b, h = rows(base), rows(head)
    print(f'# MultiSnake kernels of two rocprofv3 --kernel-trace runs of tools/multi_routes.py run, in order of dispatch: {len(b)} / {len(h)} rows')
    print(f'# {"#":>3s} {"same":4s} {"grid":>6s} {"wg":>4s} {"lds":>7s}  kernel (base; head beside it where it differs)')
    bad = len(b) != len(h)
    for i in range(max(len(b), len(h))):
        x, y = b[i] if i < len(b) else None, h[i] if i < len(h) else None
        bad |= x != y
        k, g, w, l = x or y
        print(f'{i:5d} {"yes" if x == y else "NO":4s} {g:6d} {w:4d} {l:7d}  {k}' + ('' if x == y else f'   |   head: {y}'))
    print(f'# {"every row equal" if not bad else "DIFFERENT"}')
    return int(bad)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['run', 'compare'])
    ap.add_argument('traces', nargs='*')
    ap.add_argument('--root', default=HERE)
    a = ap.parse_args()
    sys.exit(run(a.root) if a.what == 'run' else compare(*a.traces))
