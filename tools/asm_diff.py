#!/usr/bin/env python3
"""Device assembly of two source trees, kernel by kernel: the check of a refactor that must not move the compiler's output.

    python tools/asm_diff.py PARENT_TREE TREE aivc_amd/csrc/conv_wino.hip [more .hip files, relative to the trees]

Each file is compiled in both trees with the flags of build_hip() plus `--cuda-device-only -S`.  A function's body is
normalised (comments and directives dropped, local labels renumbered in order of appearance, the per-build `__hip_cuid_*`
symbol ignored) and compared with the body of the same name in the other tree.  Per kernel: VGPR / AGPR / SGPR, LDS and scratch
bytes of both trees, and `equal` or the first differing line with the opcode counts that differ.  Exit status 1 on any
difference (a kernel only one tree has is one).  Reads what the compiler wrote; needs no GPU."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402

RESOURCES = (('VGPR', 'NumVgprs'), ('AGPR', 'NumAgprs'), ('SGPR', 'TotalNumSgprs'), ('LDS', 'LDSByteSize'), ('scratch', 'ScratchSize'))
LABEL = re.compile(r'\.L[A-Za-z_]*\d+(?:_\d+)?')


def compile_asm(tree, rel, tmp, tag):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = os.path.join(tmp, '%s_%s.s' % (tag, os.path.basename(rel)[:-4]))
    flags = [f for f in HIPCC_FLAGS if f != '-shared']
    r = subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', os.path.join(tree, rel), '-o', out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:  # (warnings stay out of the report, as in build_hip(); a failing compile shows everything)
        sys.exit(r.stdout.decode(errors='replace'))
    with open(out) as f:
        return f.read().splitlines()


def demangle(names):
    try:
        out = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(lines):
    """-> {symbol: (normalised body, {resource: value})} of one assembly file"""
    symbols = [m.group(1) for m in (re.match(r'\s*\.type\s+([\w.$]+),@function', ln) for ln in lines) if m]
    found, i = {}, 0
    for sym in symbols:
        while lines[i].split(';')[0].strip() != sym + ':':
            i += 1
        body, labels = [], {}
        i += 1
        while not re.match(r'\.Lfunc_end\d+:', lines[i].strip()):
            ln = lines[i].split(';')[0].strip()
            i += 1
            if not ln or '__hip_cuid_' in ln or (ln.startswith('.') and not ln.endswith(':')):
                continue  # comment, the per-build symbol, directive (a local label is no directive)
            body.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), ln))
        res = {}
        while i < len(lines) and '@function' not in lines[i]:
            for short, key in RESOURCES:  # the compiler's own summary behind the function
                m = re.match(r';\s*%s:\s*(\d+)' % key, lines[i].strip())
                if m:
                    res[short] = int(m.group(1))
            i += 1
        found[sym] = (body, res)
    return found


def opcode_counts(body):
    return collections.Counter(ln.split()[0] for ln in body if not ln.endswith(':'))


def compare(rel, parent, tree):
    names = demangle(sorted(set(parent) | set(tree)))
    differences = 0
    for sym in sorted(names, key=names.get):
        print('%s  %s' % (os.path.basename(rel), names[sym]))
        if sym not in parent or sym not in tree:
            print('    only in the %s' % ('parent' if sym in parent else 'tree'))
            differences += 1
            continue
        (pb, pr), (tb, tr) = parent[sym], tree[sym]
        print('    ' + '  '.join('%s %s' % (k, pr.get(k) if pr.get(k) == tr.get(k) else '%s -> %s' % (pr.get(k), tr.get(k)))
                                 for k, _ in RESOURCES))
        if pb == tb and pr == tr:
            print('    stream: equal (%d lines)' % len(pb))
            continue
        differences += 1
        if pb != tb:
            k = next((n for n, (x, y) in enumerate(zip(pb, tb)) if x != y), min(len(pb), len(tb)))
            print('    stream: %d -> %d lines, first difference at line %d' % (len(pb), len(tb), k))
            print('        parent: %s' % (pb[k] if k < len(pb) else '<end>'))
            print('        tree:   %s' % (tb[k] if k < len(tb) else '<end>'))
            pc, tc = opcode_counts(pb), opcode_counts(tb)
            for op in sorted(set(pc) | set(tc)):
                if pc[op] != tc[op]:
                    print('        %-28s %5d -> %5d' % (op, pc[op], tc[op]))
    return differences


def main(argv):
    if len(argv) < 4:
        sys.exit(__doc__)
    parent_tree, tree, files = argv[1], argv[2], argv[3:]
    differences = 0
    with tempfile.TemporaryDirectory() as tmp:
        for rel in files:
            differences += compare(rel, functions(compile_asm(parent_tree, rel, tmp, 'parent')), functions(compile_asm(tree, rel, tmp, 'tree')))
    print('%d difference(s)' % differences)
    return 1 if differences else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
