#!/usr/bin/env python3
"""Compares the device assembly of two builds kernel by kernel, branch labels aside.  The project's standing rule: a feature pull
request leaves every existing kernel's instructions as they were; a refactor pull request names the kernels it changes (--except)
or renames (--map), and every other kernel stays identical.

    hipcc $(FLAGS) -S --cuda-device-only -o before.s realrobot.hip      (on the parent commit)
    hipcc $(FLAGS) -S --cuda-device-only -o after.s realrobot.hip
    python tools/compare_kernel_asm.py before.s after.s [--except k_closest_points,k_posture_clearance]
                                                        [--map 'k_posture_clearance_carry=k_posture_clearance<true>,k_posture_clearance=k_posture_clearance<false>']
                                                        [--kernarg k_posture_clearance=+8]

Comments are dropped, `.LBB<function>_<block>` labels lose the function number (a new kernel renumbers them), and the
kernel descriptors (.amdhsa_ lines: registers, LDS, scratch) are compared too.  Exit status 1 if a kernel of `before` is missing
from `after` or differs; kernels only `after` has are listed.  A kernel named by --except (its plain name, as in the source) is
reported when it differs but not counted.

--map old=new pairs a kernel of `before` with one of `after` that has another name: both are plain source names, and a `new` that
is an instantiation of a kernel template over one bool says which, `name<true>` or `name<false>`.  The `before` kernel whose symbol
is `old` (plain or mangled) is compared with the `after` kernel whose symbol is `new`'s; inside the two bodies and descriptors both
symbols read as one placeholder, and the `.text` / `.section ..., comdat` directive in front of the function's end label -- a
template instantiation lives in a comdat section of its own -- is left out of the comparison.  A mapped kernel is held to the same
identity as any other: instructions and descriptor.
--kernarg kernel=+N allows, for the `before` kernel of that plain name, `.amdhsa_kernarg_size` to be exactly N bytes larger in
`after` (arguments added at the end that the kernel never reads), and nothing else of its descriptor to differ."""
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


def symbol_prefix(name):
    """the start of the mangled symbol of a kernel given by its source name: `k` -> _Z1k, `k<true>` -> _Z1kILb1EE"""
    m = re.fullmatch(r'(\w+)(?:<(true|false)>)?', name)
    if not m:
        sys.exit('compare_kernel_asm.py: %r is not a kernel name, or a name with <true> or <false>' % name)
    return '_Z%d%s' % (len(m.group(1)), m.group(1)) + ('ILb%dEE' % (m.group(2) == 'true') if m.group(2) else '')


def find(table, name, path):
    """the one symbol of a build that the source name means"""
    pre = symbol_prefix(name)
    hits = [k for k in table if k == name or (k.startswith(pre) and ('<' in name or not k.startswith(pre + 'I')))]
    if len(hits) != 1:
        sys.exit('compare_kernel_asm.py: %s names %d kernels of %s' % (name, len(hits), path))
    return hits[0]


def neutral(body, symbol):
    """a mapped kernel's lines with its own symbol as a placeholder and without the section directive behind its descriptor"""
    return [l.replace(symbol, '<kernel>') for l in body if l != '.text' and not (l.startswith('.section') and l.endswith('comdat'))]


def option(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    value = args[i + 1] if i + 1 < len(args) else ''
    del args[i:i + 2]
    return value


def main():
    args = sys.argv[1:]
    usage = 'usage: compare_kernel_asm.py before.s after.s [--except kernel_a,kernel_b] [--map old=new,old=new] [--kernarg kernel=+8,kernel=+16]'
    exc, mapped, grown = option(args, '--except'), option(args, '--map'), option(args, '--kernarg')
    if len(args) != 2 or '' in (exc, mapped, grown):
        sys.exit(usage)
    named = set(exc.split(',')) if exc else set()
    a, b = kernels(args[0]), kernels(args[1])
    pairs, shown = {}, {}                                       # symbol of `before` -> symbol of `after`, -> the two source names
    for item in mapped.split(',') if mapped else ():
        old, sep, new = item.partition('=')
        if not sep:
            sys.exit(usage)
        pairs[find(a, old, args[0])] = find(b, new, args[1])
        shown[find(a, old, args[0])] = '%s = %s' % (old, new)
    if len(set(pairs.values())) != len(pairs):
        sys.exit('compare_kernel_asm.py: --map gives one kernel of %s twice' % args[1])
    growth = {}                                                 # symbol of `before` -> allowed growth of its kernarg segment
    for item in grown.split(',') if grown else ():
        k, sep, n = item.partition('=')
        if not sep or not re.fullmatch(r'\+\d+', n):
            sys.exit(usage)
        growth[find(a, k, args[0])] = int(n)
    excepted = lambda k: any(k == n or k.startswith('_Z%d%s' % (len(n), n)) for n in named)      # the plain name, or mangled with its length
    bad = 0
    for k in sorted(a):
        kb = pairs.get(k, k)
        if kb not in b:
            print('MISSING  %s' % k)
            bad += 1
            continue
        x, y = (neutral(a[k], k), neutral(b[kb], kb)) if k in pairs else (a[k], b[kb])
        if k in growth:
            size = [int(l.split()[1]) for l in x if l.startswith('.amdhsa_kernarg_size')]
            x = [('.amdhsa_kernarg_size %d' % (size[0] + growth[k])) if l.startswith('.amdhsa_kernarg_size') else l for l in x]
        if x != y:
            first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            print('%s  %s: %d -> %d lines, first at line %d' % ('excepted' if excepted(k) else 'DIFFERS ', k, len(x), len(y), first))
            if first < min(len(x), len(y)):
                print('           - %s\n           + %s' % (x[first], y[first]))
            bad += not excepted(k)
        elif k in pairs:
            print('mapped   %s: identical%s' % (shown[k], ', kernarg +%d' % growth[k] if k in growth else ''))
    for k in sorted(set(b) - set(a) - set(pairs.values())):
        print('new      %s (%d lines)' % (k, len(b[k])))
    print('%d kernels and functions compared, %d differ' % (len(a), bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
