#!/usr/bin/env python3
"""Are the kernels of two device assembly files the same, instruction for instruction?

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/train_slow.hip -o after.s     (and before.s at the parent commit)
    scripts/compare_kernels.py before.s after.s

Compares function by function: the order in which the compiler emits the functions may differ (it follows the order of
instantiation in the source), and a basic-block label carries its function's ordinal (.LBB4_22), which is taken out.  Comments are
dropped.  Prints one line per kernel; exit status 1 if the sets of functions or any function's instructions differ.
"""
import re
import sys


def functions(path):
    """{mangled name: [instruction and directive lines]} of every function of the file"""
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
            elif name is not None:
                if line.startswith(".Lfunc_end"):
                    out[name], name = body, None
                else:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip()))
    return out


def main(argv):
    a, b = functions(argv[1]), functions(argv[2])
    same = sorted(a) == sorted(b)
    for name in sorted(set(a) | set(b)):
        ok = a.get(name) == b.get(name)
        same &= ok
        print("%-9s %5d lines  %s" % ("identical" if ok else "DIFFERENT", len(a.get(name, [])), name))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
