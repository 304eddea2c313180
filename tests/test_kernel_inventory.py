"""CPU: tests/kernel_inventory.txt lists exactly the kernels libmcadcensus.so contains (nm's __device_stub__ symbols, one per
kernel instantiation the host code can launch), each with the test or tests that launch it.  A new instantiation, or one that
is taken out, has to be entered here together with the test that reaches it (scripts/kernel_coverage.py checks a profiled
-m gpu run against the same list)."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coverage():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "scripts", "kernel_coverage.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def library_kernels(lib_path, normalise):
    out = subprocess.check_output(["nm", "-C", lib_path]).decode()
    names = set()
    for line in out.splitlines():
        if "__device_stub__" not in line:
            continue
        names.add(normalise(re.sub(r"^[0-9a-fA-F]*\s+[a-zA-Z]\s+", "", line)))
    return names


def test_normalise():
    kc = _coverage()
    assert kc.normalise('"void mc::sgm_pass_kernel<0, 4, 0, false, true, 8, true, false>(mc::SgmPassArgs)"') == \
        "sgm_pass_kernel<0, 4, 0, false, true, 8, true, false>"
    assert kc.normalise("void mc::__device_stub__median_kernel<3>(float const*, float*, int, int)") == "median_kernel<3>"
    assert kc.normalise("mc::__device_stub__mean2d_kernel(float const*, float const*, float*, int, int, int, float)") == "mean2d_kernel"
    assert kc.is_library_kernel("void mc::scale_kernel(float const*, float*, long, float)")
    assert not kc.is_library_kernel("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >(int)")


def test_inventory_matches_the_library(mc):
    kc = _coverage()
    inv = kc.read_inventory()
    built = library_kernels(mc._lib.LIB_PATH, kc.normalise)
    assert built, "no __device_stub__ symbols in %s" % mc._lib.LIB_PATH
    missing = sorted(built - set(inv))
    stale = sorted(set(inv) - built)
    assert not missing and not stale, "kernels of the library not in tests/kernel_inventory.txt: %s; listed there but not built: %s" % (
        missing, stale)


def test_every_listed_kernel_names_an_existing_test():
    kc = _coverage()
    inv = kc.read_inventory()
    assert inv
    for name, tests in inv.items():
        assert tests, "%s: no test named" % name
        for t in tests:
            path, _, func = t.partition("::")
            full = os.path.join(ROOT, path)
            assert os.path.isfile(full), "%s: %s does not exist" % (name, path)
            if func:
                assert re.search(r"^def %s\(" % re.escape(func), open(full).read(), re.M), "%s: no test %s" % (name, t)
