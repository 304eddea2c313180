"""The project's shared libraries, one row each, and the helpers with which the tests read a library, its header, its kernel inventory
and the build.  tests/test_libraries_host.py holds every row to the same contract; a library's own test file keeps what only that
library has (its literal kernel and symbol sets, its constants), through the same helpers.  A new library is one row here, one
OBJS_ line in mc-cnn_amd/csrc/Makefile and one inventory file."""
import collections
import functools
import glob
import importlib
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mc-cnn_amd")
CSRC = os.path.join(PKG, "csrc")

# file: under mc-cnn_amd/; module: its loader, mc_cnn_amd.<module>; header: under include/; inventory: under tests/;
# symbols: what a library without loader and header exports, literally
Library = collections.namedtuple("Library", "file module header inventory symbols")
LIBRARIES = [
    # kernel_inventory.txt serves the two oldest libraries: their kernels together are the file's, and they share none
    Library("libmcadcensus.so", "_lib", "mc_adcensus.h", "kernel_inventory.txt", None),
    Library("libmctrain.so", "_train_lib", "mc_train.h", "kernel_inventory.txt", None),
    Library("libmctrainslow.so", "_train_slow_lib", "mc_train_slow.h", "kernel_inventory_train_slow.txt", None),
    Library("libmctrainmb.so", "_train_mb_lib", "mc_train_mb.h", "kernel_inventory_train_mb.txt", None),
    Library("libmctrainmbslow.so", "_train_mb_slow_lib", "mc_train_mb_slow.h", "kernel_inventory_train_mb_slow.txt", None),
    Library("libmceval.so", "_eval_lib", "mc_eval.h", "kernel_inventory_eval.txt", None),
    Library("libmctraindepth.so", "_train_depth_lib", "mc_train_depth.h", "kernel_inventory_train_depth.txt", None),
    Library("libmcfcsplit.so", "_fc_split_lib", "mc_fc_split.h", "kernel_inventory_fc_split.txt", None),
    Library("libmcconvsplit.so", "_conv_split_lib", "mc_conv_split.h", "kernel_inventory_conv_split.txt", None),
    Library("libmctrainslowdepth.so", "_train_slow_depth_lib", "mc_train_slow_depth.h", "kernel_inventory_train_slow_depth.txt", None),
    Library("libmcops.so", "_ops_lib", "mc_ops.h", "kernel_inventory_ops.txt", None),
    # no loader and no public header: libmcadcensus.so links against it and calls its one entry point
    Library("libmcsgmrecompute.so", None, None, "kernel_inventory_sgm_recompute.txt", ("mc_sgm_recompute_launch",)),
]
BY_FILE = {row.file: row for row in LIBRARIES}
# the entry points that libmcadcensus.so exports for the GPU tests and no header declares: the ABI and its version stay
# without them.  They are the only mc_* symbols of any library outside a header.
TEST_HOOKS = {"libmcadcensus.so": {"mc_test_predict_lanes", "mc_test_sgm_vertical", "mc_test_stereo_join_hwd"}}

# the only kernel names that more than one inventory lists: train_slow_fc.h's FC kernels, compiled into each accurate trainer
SHARED_KERNELS = {"fc_forward_kernel", "fc_head_kernel", "fc_backward_kernel<true>", "fc_backward_kernel<false>"}
SHARED_BY = {"libmctrainslow.so", "libmctrainmbslow.so", "libmctrainslowdepth.so"}


def path(file):
    return os.path.join(PKG, file)


def module(row):
    return importlib.import_module("mc_cnn_amd." + row.module)


def header_text(row):
    return open(os.path.join(ROOT, "include", row.header)).read()


@functools.lru_cache(None)
def kernel_coverage():
    """scripts/kernel_coverage.py, imported by path"""
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "scripts", "kernel_coverage.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def read_inventory(name):
    """{kernel: [tests]} of tests/<name>"""
    return kernel_coverage().read_inventory(os.path.join(ROOT, "tests", name))


@functools.lru_cache(None)
def built_kernels(lib_path):
    """the kernels a library holds, spelled as the inventories spell them: nm's __device_stub__ symbols, one per instantiation the host
    code can launch"""
    assert os.path.isfile(lib_path), "%s is not built" % lib_path
    out = subprocess.check_output(["nm", "-C", lib_path]).decode()
    return frozenset(kernel_coverage().normalise(re.sub(r"^[0-9a-fA-F]*\s+[a-zA-Z]\s+", "", line)) for line in out.splitlines()
                     if "__device_stub__" in line)


def built_by_inventory(inventory):
    """{library file: its kernels} of the libraries that an inventory file serves"""
    return {row.file: set(built_kernels(path(row.file))) for row in LIBRARIES if row.inventory == inventory}


def inventory_errors(inv, built):
    """(kernels of the libraries that the inventory does not list, entries that no library holds)"""
    union = set().union(*built.values())
    return sorted(union - set(inv)), sorted(set(inv) - union)


def exported_symbols(lib_path):
    """{name: nm's type letter} of a library's defined dynamic symbols"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    return {f[2]: f[1] for f in (line.split() for line in out.splitlines()) if len(f) == 3}


def exported_abi(lib_path):
    """the mc_* functions and data a library exports"""
    return {name for name, kind in exported_symbols(lib_path).items() if kind in "TtDBW" and name.startswith("mc_")}


def header_symbols(text, prefix="mc_"):
    """the functions a header declares, comments left out"""
    return set(re.findall(r"\b(%s\w*)\s*\(" % prefix, re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def listed_tests_exist(inv):
    """every entry of an inventory names at least one test, and each names a function that its file defines"""
    for name, tests in inv.items():
        assert tests, "%s: no test named" % name
        for t in tests:
            file, _, func = t.partition("::")
            full = os.path.join(ROOT, file)
            assert os.path.isfile(full), "%s: %s does not exist" % (name, file)
            assert func and re.search(r"^def %s\(" % re.escape(func), open(full).read(), re.M), "%s: no test %s" % (name, t)


@functools.lru_cache(None)
def make(*args):
    """the output of `make <args>` in mc-cnn_amd/csrc"""
    return subprocess.check_output(["make", "-C", CSRC] + list(args)).decode()


def print_libraries():
    """{library file: [objects]}, the build's own list"""
    return {lib: objs.split() for lib, objs in (line.split(": ", 1) for line in make("-s", "print-libraries").splitlines())}


def inventory_files():
    """the inventory files on disk"""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "kernel_inventory*.txt")))
