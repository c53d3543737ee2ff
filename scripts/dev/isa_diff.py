#!/usr/bin/env python
"""Are the kernel instances of two builds of a translation unit the same instructions?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I safeopt_amd/csrc \\
          --cuda-device-only -S safeopt_amd/csrc/sweep_pair.hip -o new.s      (same for old.s)
    python scripts/dev/isa_diff.py old.s new.s

Compares function by function, comments and directives dropped and block labels renumbered.  An
instance that gained trailing template arguments with default values (`..., false>`) is matched
with its old name.  Prints the instances that differ (with the first differing lines), those
that exist on one side only, and a count."""
import re
import sys


def funcs(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:', s, re.S):
        lines = [re.sub(r'\s*;.*', '', l).strip() for l in m.group(2).split('\n')]
        out[m.group(1)] = [re.sub(r'\.LBB\d+_', '.LBB_', l) for l in lines
                           if l and (not l.startswith('.') or l.endswith(':'))]
    return out


def old_name(n):      # k_sweep_pair<D, SINGLE, R, SEP, false> -> k_sweep_pair<D, SINGLE, R, SEP>
    return re.sub(r'(k_sweep_pairILi\dELb[01]ELi\dELi\d)ELb0(EEEv)', r'\1\2', n)


def main():
    a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
    bk = {old_name(n): v for n, v in b.items()}
    same = diff = 0
    for n, v in a.items():
        w = bk.get(n)
        if w is None:
            print("only in", sys.argv[1], n)
        elif v == w:
            same += 1
        else:
            diff += 1
            d = [(x, y) for x, y in zip(v, w) if x != y]
            print("DIFF %s: %d / %d instructions, %d lines differ, first: %s" %
                  (n, len(v), len(w), len(d) + abs(len(v) - len(w)), d[:2]))
    for n in bk:
        if n not in a:
            print("only in", sys.argv[2], n)
    print("same %d, different %d" % (same, diff))
    return 0


if __name__ == "__main__":
    sys.exit(main())
