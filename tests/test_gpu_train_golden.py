"""GPU: the four training libraries give, bit for bit, what they gave before their layer chains, LDS layouts and host code
were stated once in shared headers, and libmctraindepth.so at l1 1, 2 and 3 what it gave before the fast net's kernels were
stated once in csrc/train_fast.h.  tests/golden/train_bitwise.json (tests/golden/make_train_bitwise.py) holds SHA-256 of the
parameters, the momenta and the losses of the cases of tests/train_golden_cases.py, recorded from the libraries of the
commit before each change; every arithmetic order is fixed by the source under -ffp-contract=off, so the comparison is of
hashes alone and has no tolerance."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_golden_cases as tg  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "train_bitwise.json")))


@pytest.fixture(scope="module")
def results():
    return tg.run_all()


def test_the_cases_are_the_recorded_ones(results):
    assert set(results) == set(GOLDEN["cases"]) and len(results) == 32
    for name, r in results.items():
        assert tg.vacuous(r) is None, (name, tg.vacuous(r))


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_bits_are_those_of_the_parent_commit(results, name):
    got = tg.hashes(results[name])
    if "losses" in results[name]:
        print(name, "losses", results[name]["losses"].tolist())
    assert got == GOLDEN["cases"][name], "%s differs in %s (golden recorded with ROCm %s)" % (
        name, sorted(k for k in got if got[k] != GOLDEN["cases"][name].get(k)), GOLDEN["rocm"])
