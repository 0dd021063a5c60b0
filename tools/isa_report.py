"""Per-kernel code-generation comparison of two builds: did a source change move any instruction?

    hipcc <build.py's FLAGS> --cuda-device-only -S csrc/X.hip -o before/X.s        (one .s per translation unit, both trees)
    python tools/isa_report.py before/ after/ [--only SUBSTRING] [--rename BEFORE=AFTER ...]

Takes two device assemblies, or two directories of them (a kernel is found in whichever file of a side holds it, so a side may be
one translation unit and the other several).  Kernels are paired by symbol; one that the change renamed (a new template parameter,
say) is paired by hand with --rename, BEFORE and AFTER each a substring that picks one demangled name of its side.  For every
kernel symbol: instruction count, whether the instruction text is identical, if not the difference of the opcode multisets (after
minus before), and the kernel metadata that decides occupancy.  The tool only compares the two sides; it knows no instruction by
name.  Exit status 1 when the symbol sets or any metadata differ."""
from __future__ import annotations

import argparse
import collections
import os
import re
import shutil
import subprocess
import sys

META = [('.vgpr_count', 'vgpr'), ('.sgpr_count', 'sgpr'), ('.agpr_count', 'agpr'), ('.vgpr_spill_count', 'vgpr_spill'),
        ('.sgpr_spill_count', 'sgpr_spill'), ('.group_segment_fixed_size', 'lds'), ('.private_segment_fixed_size', 'scratch')]
LABEL = re.compile(r'^[A-Za-z_.$][\w.$]*:')
BLOCK_REF = re.compile(r'\.LBB\d+_(\d+)')
LOCAL_REF = re.compile(r'\.L([A-Za-z_]+)\d+\b')        # .Lpost_getpc12 (long branches), .Lfunc_end3, ...: ordinals of the translation unit


def parse(path: str) -> dict:
    """kernel symbol -> {'text': [instruction lines], 'meta': {key: int}}"""
    with open(path) as f:
        lines = f.read().split('\n')
    kernels = {m.group(1) for ln in lines if (m := re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln))}
    out = {k: {'text': [], 'meta': {}} for k in kernels}
    cur = None
    for ln in lines:
        s = ln.split(';', 1)[0].strip()
        if not s:
            continue
        if LABEL.match(s):
            name = s[:-1]
            if name in kernels:
                cur = name
            elif name.startswith('.Lfunc_end'):
                cur = None
            continue
        if cur is None or s.startswith('.'):
            continue
        # local labels carry ordinals of the translation unit (the function's in .LBB<f>_<b>, a running count in .Lpost_getpc<n>):
        # not part of the code, and different as soon as a kernel moves to another unit
        out[cur]['text'].append(BLOCK_REF.sub(r'.LBB_\1', LOCAL_REF.sub(r'.L\1', ' '.join(s.split()))))     # (LOCAL_REF leaves .LBB<f>_<b> alone: no word boundary)
    # .amdgpu_metadata: one YAML list entry per kernel; the keys wanted are plain scalars
    entry: dict = {}
    for ln in lines + ['  - end']:
        s = ln.strip()
        if s.startswith('- ') and ln.startswith('  - '):
            if entry.get('.symbol', '').removesuffix('.kd') in out:
                out[entry['.symbol'].removesuffix('.kd')]['meta'] = {short: int(entry.get(key, -1)) for key, short in META}
            entry = {}
            s = s[2:]
        if (m := re.match(r'(\.\w+):\s*(\S+)$', s)):
            entry[m.group(1)] = m.group(2).strip("'\"")
    return out


def side(path: str) -> dict:
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith('.s')) if os.path.isdir(path) else [path]
    out: dict = {}
    for f in files:
        for k, v in parse(f).items():
            v['unit'] = os.path.basename(f)
            out[k] = v
    return out


def demangle(names: list) -> dict:
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or next((p for p in ('/opt/rocm/llvm/bin/llvm-cxxfilt',) if os.path.exists(p)), None)
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True)
    got = r.stdout.split('\n')
    return {n: (got[i] if i < len(got) and got[i] else n) for i, n in enumerate(names)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('before')
    ap.add_argument('after')
    ap.add_argument('--only', default='', help='report kernels whose demangled name contains this')
    ap.add_argument('--rename', action='append', default=[], metavar='BEFORE=AFTER',
                    help='pair the one kernel of the "before" side whose demangled name contains BEFORE with the one of the "after" side '
                         'whose demangled name contains AFTER (a kernel the change renamed); repeatable')
    a = ap.parse_args()
    A, B = side(a.before), side(a.after)
    names = demangle(sorted(set(A) | set(B)))
    for r in a.rename:
        old, _, new = r.partition('=')
        ka, kb = [k for k in A if old in names[k]], [k for k in B if new in names[k]]
        if not old or not new or len(ka) != 1 or len(kb) != 1 or ka[0] in B or kb[0] in A:
            ap.error(f'--rename {r}: {len(ka)} kernels before, {len(kb)} after (one of each wanted, neither of them present on the other side)')
        A[kb[0]] = A.pop(ka[0])
        names[kb[0]] = f'{names.pop(ka[0])}  ->  {names[kb[0]]}'
    bad = same = 0
    shown = [k for k in sorted(names, key=names.get) if a.only in names[k]]
    for k in shown:
        print(names[k])
        if k not in A or k not in B:
            print(f'    ONLY {"before" if k in A else "after"} ({(A.get(k) or B.get(k))["unit"]})')
            bad += 1
            continue
        x, y = A[k], B[k]
        ident = x['text'] == y['text']
        same += ident
        print(f'    units {x["unit"]} -> {y["unit"]}   instructions {len(x["text"])} -> {len(y["text"])}   text {"identical" if ident else "DIFFERS"}')
        if not ident:
            ca = collections.Counter(t.split()[0] for t in x['text'])
            cb = collections.Counter(t.split()[0] for t in y['text'])
            d = {op: cb[op] - ca[op] for op in sorted(set(ca) | set(cb)) if cb[op] != ca[op]}
            print('    opcode multiset: ' + (', '.join(f'{op} {n:+d}' for op, n in d.items()) if d else 'identical (operands or order differ)'))
        mx = ' '.join(f'{s}={x["meta"].get(s)}' for _, s in META)
        if x['meta'] == y['meta']:
            print(f'    metadata identical: {mx}')
        else:
            bad += 1
            print(f'    metadata DIFFERS: before {mx}')
            print('                       after  ' + ' '.join(f'{s}={y["meta"].get(s)}' for _, s in META))
    print(f'{len(shown)} kernels: {same} with identical text, {len(shown) - same} not; {bad} with differing metadata or missing on one side')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
