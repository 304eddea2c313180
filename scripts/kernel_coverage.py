#!/usr/bin/env python3
"""Which of the libraries' kernels a profiled run launched.

    scripts/kernel_coverage.py KERNEL_STATS_CSV [KERNEL_STATS_CSV ...] [--inventory FILE ...]   (default: the inventory files under tests/)

Reads the kernel_stats.csv files that `rocprofv3 --kernel-trace --stats` writes (e.g. for `pytest tests -m gpu`), normalises the
kernel names the way the inventory files list them, and prints the inventory kernels the run never launched and the library kernels
it launched that no inventory lists.  The inventory files are tests/kernel_inventory*.txt, one per library (the two oldest libraries
share tests/kernel_inventory.txt); tests/libraries.py says which library each serves.  Only the libraries' own kernels (namespace mc::)
count: torch's and the reference's kernels of the same run are ignored.  Exit status 1 if either list is not empty.

A name is normalised by dropping `void`, the namespaces, `__device_stub__` (nm's spelling of a kernel's host stub) and the argument
list: `void mc::sgm_pass_kernel<0, 4, 0, false, true, 8, true, false>(mc::SgmPassArgs)` -> `sgm_pass_kernel<0, 4, 0, false, true,
8, true, false>`.
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVENTORY = os.path.join(ROOT, "tests", "kernel_inventory.txt")
NAMESPACE = "mc::"


def inventories():
    """every inventory file under tests/"""
    return sorted(glob.glob(os.path.join(ROOT, "tests", "kernel_inventory*.txt")))


def normalise(name):
    """a demangled kernel or stub name -> `kernel<template args>`"""
    n = name.strip().strip('"').strip()
    if n.startswith("void "):
        n = n[len("void "):]
    n = n.replace("__device_stub__", "")
    depth = 0
    for i, ch in enumerate(n):   # the argument list: the first '(' outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            n = n[:i]
            break
    base, sep, targs = n.partition("<")
    return base.rsplit("::", 1)[-1].strip() + sep + targs.replace(NAMESPACE, "")


def is_library_kernel(name):
    n = name.strip().strip('"').strip()
    if n.startswith("void "):
        n = n[len("void "):]
    return n.startswith(NAMESPACE)


def read_inventory(path=INVENTORY):
    """{normalised name: [tests]} of the inventory file: `name | test [test ...]` per line, '#' starts a comment line"""
    inv = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            name, _, tests = line.partition(" | ")
            name = name.strip()
            if name in inv:
                raise ValueError("%s: %s listed twice" % (path, name))
            inv[name] = tests.split()
    return inv


def launched(csv_paths):
    """{normalised name: calls} of the library's kernels in rocprofv3 kernel_stats.csv files"""
    calls = {}
    for p in csv_paths:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                if not is_library_kernel(row["Name"]):
                    continue
                k = normalise(row["Name"])
                calls[k] = calls.get(k, 0) + int(row.get("Calls") or 0)
    return calls


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("stats", nargs="+", help="kernel_stats.csv of rocprofv3 --kernel-trace --stats")
    ap.add_argument("--inventory", nargs="+", default=inventories())
    a = ap.parse_args(argv)
    inv = {}
    for path in a.inventory:
        inv.update(read_inventory(path))
    calls = launched(a.stats)
    never = sorted(k for k in inv if k not in calls)
    unlisted = sorted(k for k in calls if k not in inv)
    print("inventory: %d kernels; launched by the run: %d library kernels (%d launches)" % (len(inv), len(calls), sum(calls.values())))
    print("inventory kernels the run never launched: %d" % len(never))
    for k in never:
        print("  " + k)
    print("launched kernels missing from the inventory: %d" % len(unlisted))
    for k in unlisted:
        print("  %s  (%d launches)" % (k, calls[k]))
    return 1 if never or unlisted else 0


if __name__ == "__main__":
    sys.exit(main())
