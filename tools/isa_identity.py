#!/usr/bin/env python3
"""Is the generated device code of this tree the same as that of another revision?  No GPU needed.

Every wurm_amd/csrc/*.hip of the base revision (git archive) and of the working tree is compiled with the Makefile's flags
plus `--cuda-device-only -S`; each assembly file is cut into per-symbol bodies (label to .size, the kernel descriptor
apart) and the bodies are compared BY NAME, because the order of emission follows the order of the source.  Local labels
and the compiler's loop comments carry the function's ordinal (.LBB12_3, BB12_3, .Lfunc_end12), which is dropped first.
One line per unit: kernels, identical code, identical descriptors, the demangled names of any that differ / come / go.
A kernel that only changed its NAME (it became the instantiation of a template, say) is compared with its successor when
told so: --alias BASE_SYMBOL=HEAD_SYMBOL (mangled names; may be repeated) reads the base's assembly with the one name
written as the other.
Another flavour of the library (the Makefile's `timeline` and `probe` targets) is compared with --define NAME (may be
repeated): both trees are compiled with -DNAME, and the header line says so.

usage: tools/isa_identity.py BASE_REV [--jobs N] [--keep DIR [--reuse]] [--alias OLD=NEW] [--define NAME] > profiles/rNN_isa_identity.txt    (exit status 1 on a difference)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = '-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function --cuda-device-only -S'.split()


def compile_unit(tree, unit, out, defines=()):
    r = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', *FLAGS, *defines, unit + '.hip', '-o', out],
                       cwd=os.path.join(tree, 'wurm_amd', 'csrc'), capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f'{tree}: {unit}.hip does not compile\n{r.stderr[-4000:]}')


def symbols(path, alias=()):
    """{name: (code, descriptor or None)} for every function of an assembly file; alias: (old, new) symbol names"""
    out, name, code, desc, in_desc = {}, None, [], [], False
    ordinal = re.compile(r'(?<![0-9A-Za-z])(\.LBB|BB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp)\d+')
    for ln in open(path):
        ln = ln.rstrip()
        for old, new in alias:
            ln = re.sub(r'(?<![0-9A-Za-z_])' + re.escape(old) + r'(?![0-9A-Za-z_])', new, ln)
        if ln.startswith('\t.type\t') and ln.endswith(',@function'):
            name, code, desc, in_desc = ln.split('\t')[2][:-len(',@function')], [], [], False
            end = '\t.size\t' + name + ','
            continue
        if name is None:
            continue
        if ln == '\t.text' or ln.startswith('\t.section\t'):  # where the body is placed (an instantiation of a template
            continue                                           # has a section of its own) is not part of it
        if 'BB' in ln or '.L' in ln: # (and the comment column, which moves with the ordinal's width)
            ln = re.sub(r'\s+;', ' ;', ordinal.sub(r'\1', ln))
        if ln.startswith('\t.amdhsa_kernel'):
            in_desc = True
        (desc if in_desc else code).append(ln)
        if ln.startswith('\t.end_amdhsa_kernel'):
            in_desc = False
        if ln.startswith(end):
            out[name] = ('\n'.join(code), '\n'.join(desc) if desc else None)
            name = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('base')
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--keep', help='directory that keeps the assembly files (base/, head/)')
    ap.add_argument('--reuse', action='store_true', help='compare the assembly files --keep already holds, compile nothing')
    ap.add_argument('--alias', action='append', default=[], metavar='OLD=NEW',
                    help='a symbol of the base that the working tree has under another (mangled) name')
    ap.add_argument('--define', action='append', default=[], metavar='NAME',
                    help='compile both trees with -DNAME (WURM_TIMELINE, WURM_GROUP_PROBE: the other flavours of the library)')
    a = ap.parse_args()
    defines = ['-D' + d for d in a.define]
    alias = [tuple(x.split('=', 1)) for x in a.alias]
    work = a.keep or tempfile.mkdtemp(prefix='isa_identity_')
    base_tree = os.path.join(work, 'base_tree')
    for d in ('base', 'head', 'base_tree'):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    tar = subprocess.run(['git', '-C', ROOT, 'archive', a.base, 'wurm_amd/csrc', 'include'], capture_output=True, check=True)
    subprocess.run(['tar', '-x', '-C', base_tree], input=tar.stdout, check=True)
    units = lambda tree: sorted(f[:-4] for f in os.listdir(os.path.join(tree, 'wurm_amd', 'csrc')) if f.endswith('.hip'))
    jobs = [(base_tree, u, os.path.join(work, 'base', u + '.s')) for u in units(base_tree)]
    jobs += [(ROOT, u, os.path.join(work, 'head', u + '.s')) for u in units(ROOT)]
    if not a.reuse:
        with ThreadPoolExecutor(a.jobs) as ex:
            list(ex.map(lambda j: compile_unit(*j, defines), jobs))
    rev = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', a.base], capture_output=True, text=True).stdout.strip()
    print(f'# device assembly of the working tree against {rev}: hipcc --offload-arch=gfx950 {" ".join(FLAGS + defines)}')
    for old, new in alias:
        print(f'# base symbol {old} is compared as {new}')
    print(f'# {"unit":18s} {"kernels":>8s} {"same code":>10s} {"same descr":>11s}  differing / added / removed symbols')
    same = units(base_tree) == units(ROOT)
    if not same:
        print(f'# translation units differ: {units(base_tree)} -> {units(ROOT)}')
    for u in sorted(set(units(base_tree)) & set(units(ROOT))):
        b, h = symbols(os.path.join(work, 'base', u + '.s'), alias), symbols(os.path.join(work, 'head', u + '.s'))
        kernels = [n for n in h if h[n][1] is not None]
        both = [n for n in kernels if n in b]
        odd = [n for n in both if b[n] != h[n]] + [n for n in set(b) ^ set(h)] + \
              [n for n in set(b) & set(h) if h[n][1] is None and b[n] != h[n]]
        names = subprocess.run(['c++filt'], input='\n'.join(odd), capture_output=True, text=True).stdout.split('\n') if odd else []
        print(f'{u:20s} {len(kernels):8d} {sum(b[n][0] == h[n][0] for n in both):10d} {sum(b[n][1] == h[n][1] for n in both):11d}  '
              + ('; '.join(n.replace('wurm::', '') for n in names if n) or '-'))
        same = same and not odd
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
