"""CPU: tests/kernel_inventory.txt lists exactly the kernels libmcadcensus.so and libmctrain.so contain (nm's __device_stub__
symbols, one per kernel instantiation the host code can launch), each with the test or tests that launch it.  A new instantiation, or one that
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


def built_kernels(mc, kc):
    """{library file name: its kernels}; both libraries have to exist and hold kernels"""
    from mc_cnn_amd import _train_lib
    out = {}
    for path in (mc._lib.LIB_PATH, _train_lib.LIB_PATH):
        assert os.path.isfile(path), "%s is not built" % path
        out[os.path.basename(path)] = library_kernels(path, kc.normalise)
        assert out[os.path.basename(path)], "no __device_stub__ symbols in %s" % path
    return out


def inventory_errors(inv, built):
    """(kernels of either library the inventory does not list, entries no library holds)"""
    union = set().union(*built.values())
    return sorted(union - set(inv)), sorted(set(inv) - union)


def test_inventory_matches_the_library(mc):
    kc = _coverage()
    inv = kc.read_inventory()
    built = built_kernels(mc, kc)
    assert len(built) == 2 and not set.intersection(*built.values()), "a kernel name in both libraries"
    missing, stale = inventory_errors(inv, built)
    assert not missing and not stale, "kernels of the libraries not in tests/kernel_inventory.txt: %s; listed there but not built: %s" % (
        missing, stale)


def test_inventory_check_fails_on_a_missing_or_stale_entry_of_either_library(mc):
    kc = _coverage()
    inv = kc.read_inventory()
    built = built_kernels(mc, kc)
    for lib, names in built.items():
        victim = sorted(names)[0]
        less = {k: v for k, v in inv.items() if k != victim}
        assert inventory_errors(less, built) == ([victim], []), lib
        grown = {k: set(v) for k, v in built.items()}
        grown[lib].add("no_such_kernel<1>")
        assert inventory_errors(inv, grown) == (["no_such_kernel<1>"], []), lib
        shrunk = {k: set(v) - {victim} for k, v in built.items()}
        assert inventory_errors(inv, shrunk) == ([], [victim]), lib
    assert built["libmctrain.so"] == {"train_sample_kernel", "train_step_kernel<true>", "train_step_kernel<false>", "train_sgd_kernel",
                                      "gt_filter_kernel", "nnz_count_kernel", "nnz_scan_kernel", "nnz_fill_kernel"}


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
