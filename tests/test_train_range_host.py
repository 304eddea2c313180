"""The four mc_train*_run entry points ask mc-cnn_amd/csrc/train_range.h, through the run driver they share, whether steps [t0, t0 + n_steps * n_pairs) fit the
permutation.  The sum they used to form themselves overflows int64_t for t0 near 2^63, wraps to a negative number and passes
`<= n_perm`; the step would then read perm + t0.  tests/train_range_check.cpp walks the limits on the host -- the last legal
offset and one more, t0 = -1, 2^63 - 1 and 2^63 - 1 - k, n_steps = 2^31 - 1 with n_pairs = 1024, n_perm = 0 and < 0, and six
thousand random triples around every boundary against a 128-bit restatement -- built with the undefined-behaviour and address
sanitizers, non-recoverable: an overflow inside the check ends the program.  No GPU and no library is involved."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mc-cnn_amd", "csrc")
SOURCES = ("train.hip", "train_slow.hip", "train_mb.hip", "train_mb_slow.hip")
DRIVER = "train_net.h"       # run_steps: the one place the range is checked and the step loop runs


def test_range_check_has_no_overflow_and_agrees_with_128_bit_arithmetic(tmp_path):
    exe = str(tmp_path / "train_range_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "train_range_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, universal_newlines=True)
    assert out.returncode == 0, out.stderr[-4000:]
    n_checked, n_failed = (int(v) for v in out.stdout.split())
    assert n_checked >= 10000 and n_failed == 0, (n_checked, n_failed)


def _code(src):
    """src without its // comments"""
    return re.sub(r"//[^\n]*", "", src)


def test_every_run_entry_point_uses_the_shared_check():
    """No `t0 + <product>` is left in a condition or a message: the one run driver (run_steps in train_net.h) includes the
    header, asks train_steps_fit once and prints the end it returns; each mc_train*_run goes through the driver, and the only
    sums with t0 left are the steps' own offsets, formed inside the callable the driver invokes after the check."""
    assert re.findall(r"#include\s+(\S+)", open(os.path.join(CSRC, "train_range.h")).read()) == ["<stdint.h>"]   # no HIP header
    # every file that can reach a run loop: the four sources and each header they include, directly or not
    reach, todo = {}, list(SOURCES)
    while todo:
        name = todo.pop()
        if name not in reach and os.path.exists(os.path.join(CSRC, name)):
            reach[name] = open(os.path.join(CSRC, name)).read()
            todo += re.findall(r'#include\s+"([^"/]+)"', reach[name])
    assert set(SOURCES) | {DRIVER, "train_range.h"} <= set(reach)
    ask = r"MC_REQUIRE\(train_steps_fit\(t0, n_steps, n_pairs, n_perm, &end\),"
    for name, src in reach.items():
        assert len(re.findall(ask, src)) == (name == DRIVER), name                  # asked exactly once, in the driver
        assert not re.search(r"t0 \+ \(int64_t\)n_steps", src), name
        if name not in SOURCES + (DRIVER,):
            assert name == "train_range.h" or not re.search(r"\bt0\b", _code(src)), name   # no other header touches t0
    src = reach[DRIVER]
    assert '#include "train_range.h"' in src
    assert "(long long)t0, (long long)end, (long long)n_perm);" in src
    assert "steps [%lld, %lld) of the permutation exceed its %lld rows" in src
    check = src.index("train_steps_fit(")
    for m in re.finditer(r"t0 \+", src):
        if "//" in src[src.rfind("\n", 0, m.start()):m.start()]:
            continue                                   # a comment
        assert m.start() > check, (DRIVER, src[m.start() - 40:m.start() + 40])
    body = src[src.index("static int run_steps("):]
    body = body[:body.index("\n}\n")]
    assert body.index("train_steps_fit(") < body.index("prepare()") < body.index("step(s,")      # the callable runs after the check
    for name in SOURCES:
        src = reach[name]
        runs = re.findall(r"^int (mc_train\w*_run)\(", src, re.M)
        assert len(runs) == 1, name
        fn = src[src.index("int %s(" % runs[0]):]
        fn = fn[:fn.index("\n}\n")]
        assert len(re.findall(r"\breturn run_steps\(", fn)) == 1 and "for (" not in fn, name     # through the driver, no loop of its own
        callable_at = src.index(fn) + fn.index("[&](int s, int64_t first)")
        callable_end = src.index(fn) + len(fn)
        for m in re.finditer(r"t0 \+", src):
            if "//" in src[src.rfind("\n", 0, m.start()):m.start()]:
                continue                               # a comment
            assert callable_at < m.start() < callable_end, (name, src[m.start() - 40:m.start() + 40])
        assert "run_steps(" not in src.replace(fn, ""), name                                      # and nowhere else
