#!/usr/bin/env python3
"""Compares the device assembly of two builds kernel by kernel, branch labels aside.  The project's standing rule: a feature pull
request leaves every existing kernel's instructions as they were; a refactor pull request names the kernels it changes (--except),
and every other kernel stays identical.

    hipcc $(FLAGS) -S --cuda-device-only -o before.s realrobot.hip      (on the parent commit)
    hipcc $(FLAGS) -S --cuda-device-only -o after.s realrobot.hip
    python tools/compare_kernel_asm.py before.s after.s [--except k_closest_points,k_posture_clearance]

Comments are dropped, `.LBB<function>_<block>` labels lose the function number (a new kernel renumbers them), and the
kernel descriptors (.amdhsa_ lines: registers, LDS, scratch) are compared too.  Exit status 1 if a kernel of `before` is missing
from `after` or differs; kernels only `after` has are listed.  A kernel named by --except (its plain name, as in the source) is
reported when it differs but not counted."""
import re
import sys


def kernels(path):
    text = open(path).read()
    text = text[:text.index('.amdgpu_metadata')] if '.amdgpu_metadata' in text else text
    out = {}
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        body = []
        for line in m.group(2).splitlines():
            line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0]).strip()
            if line:
                body.append(line)
        out[m.group(1)] = body
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.S | re.M):
        out.setdefault(m.group(1), []).extend(l.strip() for l in m.group(2).splitlines())
    return out


def main():
    args = sys.argv[1:]
    named = set()
    if '--except' in args:
        i = args.index('--except')
        named = set(args[i + 1].split(',')) if i + 1 < len(args) else set()
        del args[i:i + 2]
    if len(args) != 2 or (not named and '--except' in sys.argv):
        sys.exit('usage: compare_kernel_asm.py before.s after.s [--except kernel_a,kernel_b]')
    a, b = kernels(args[0]), kernels(args[1])
    excepted = lambda k: any(k == n or k.startswith('_Z%d%s' % (len(n), n)) for n in named)      # the plain name, or mangled with its length
    bad = 0
    for k in sorted(a):
        if k not in b:
            print('MISSING  %s' % k)
            bad += 1
        elif a[k] != b[k]:
            first = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print('%s  %s: %d -> %d lines, first at line %d' % ('excepted' if excepted(k) else 'DIFFERS ', k, len(a[k]), len(b[k]), first))
            bad += not excepted(k)
    for k in sorted(set(b) - set(a)):
        print('new      %s (%d lines)' % (k, len(b[k])))
    print('%d kernels and functions compared, %d differ' % (len(a), bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
