"""CPU: the contract that every shared library of the project keeps, checked for each row of tests/libraries.py.  The build lists,
links and leaves on disk exactly the manifest's libraries.  A library's kernels are exactly its inventory's, each entry naming a test
that exists, and the check itself reports a dropped entry, an extra and a missing kernel as that.  Two inventories share a name only
where the manifest says so, and every inventory file belongs to a library.  A library exports exactly its header's functions (and the
manifest's test hooks), which are its loader's, under the header's ABI version, and no other function.  Every header is a prerequisite
of every object.  No GPU is needed: every library loads without one."""
import glob
import itertools
import os
import re

import pytest

import libraries as L

EACH = pytest.mark.parametrize("row", L.LIBRARIES, ids=[row.file for row in L.LIBRARIES])


# ---- the build's view ----------------------------------------------------------------------------------------------------------
def test_the_build_the_manifest_and_the_disk_name_the_same_libraries():
    printed, manifest = set(L.print_libraries()), set(L.BY_FILE)
    on_disk = {os.path.basename(p) for p in glob.glob(os.path.join(L.PKG, "lib*.so"))}
    assert len(L.BY_FILE) == len(L.LIBRARIES), "a library listed twice"
    assert printed == manifest, "only the Makefile lists %s; only tests/libraries.py lists %s" % (sorted(printed - manifest), sorted(manifest - printed))
    assert on_disk == manifest, "built but not listed: %s; listed but not built: %s" % (sorted(on_disk - manifest), sorted(manifest - on_disk))


@EACH
def test_make_all_links_the_library_from_its_objects(row):
    objs = L.print_libraries()[row.file]
    links = [line.split() for line in L.make("-n", "-B", "all").splitlines() if " -o ../%s " % row.file in line + " "]
    assert len(links) == 1 and "-shared" in links[0], links
    assert [w for w in links[0] if w.endswith(".o")] == objs
    for obj in objs:                 # and each object is compiled from a unit that exists
        assert any(os.path.isfile(os.path.join(L.CSRC, obj[:-2] + ext)) for ext in (".hip", ".cpp")), obj
    removed = L.make("-n", "clean").split()
    assert "../" + row.file in removed and set(objs) <= set(removed)


def test_every_header_is_a_prerequisite_of_every_object():
    headers = {os.path.relpath(p, L.CSRC) for p in glob.glob(os.path.join(L.CSRC, "*.h")) + glob.glob(os.path.join(L.ROOT, "include", "*.h"))}
    assert len(headers) >= 24
    database = L.make("-pn", "-B", "all")
    for obj in sorted({o for objs in L.print_libraries().values() for o in objs}):
        prerequisites = re.search(r"^%s: (.*)$" % re.escape(obj), database, re.M).group(1).split()
        assert headers <= set(prerequisites), "%s does not depend on %s" % (obj, sorted(headers - set(prerequisites)))


# ---- the kernel inventories ------------------------------------------------------------------------------------------------------
@EACH
def test_kernel_inventory_lists_exactly_the_librarys_kernels(row):
    built = L.built_by_inventory(row.inventory)
    assert built[row.file], "no __device_stub__ symbols in %s" % row.file
    inv = L.read_inventory(row.inventory)
    missing, stale = L.inventory_errors(inv, built)
    assert not missing and not stale, "kernels of %s not in tests/%s: %s; listed there but not built: %s" % (
        sorted(built), row.inventory, missing, stale)
    for other, names in built.items():       # libraries that share a file share no kernel
        assert other == row.file or not names & built[row.file], "%s in %s and %s" % (sorted(names & built[row.file]), row.file, other)
    L.listed_tests_exist(inv)


@EACH
def test_inventory_check_fails_on_a_missing_or_stale_entry(row):
    built = L.built_by_inventory(row.inventory)
    inv = L.read_inventory(row.inventory)
    victim = sorted(built[row.file])[0]
    less = {k: v for k, v in inv.items() if k != victim}
    assert L.inventory_errors(less, built) == ([victim], [])
    grown = {k: set(v) for k, v in built.items()}
    grown[row.file].add("no_such_kernel<1>")
    assert L.inventory_errors(inv, grown) == (["no_such_kernel<1>"], [])
    shrunk = {k: set(v) - {victim} for k, v in built.items()}
    assert L.inventory_errors(inv, shrunk) == ([], [victim])


def test_inventories_share_only_the_declared_kernels():
    shared_files = {L.BY_FILE[lib].inventory for lib in L.SHARED_BY}
    assert len(shared_files) == len(L.SHARED_BY)
    inv = {name: set(L.read_inventory(name)) for name in L.inventory_files()}
    for a, b in itertools.combinations(sorted(inv), 2):
        allowed = L.SHARED_KERNELS if {a, b} <= shared_files else set()
        assert inv[a] & inv[b] == allowed, "tests/%s and tests/%s share %s, the manifest allows them %s" % (
            a, b, sorted(inv[a] & inv[b]), sorted(allowed))


def test_every_inventory_file_belongs_to_a_library():
    claimed = sorted({row.inventory for row in L.LIBRARIES})
    assert L.inventory_files() == claimed, "on disk: %s; in tests/libraries.py: %s" % (L.inventory_files(), claimed)
    # and the coverage script reads exactly these by default
    assert [os.path.relpath(p, os.path.join(L.ROOT, "tests")) for p in L.kernel_coverage().inventories()] == claimed
    assert L.kernel_coverage().INVENTORY in L.kernel_coverage().inventories()


# ---- what a library exports ------------------------------------------------------------------------------------------------------
@EACH
def test_library_loads_without_a_gpu_and_exports_exactly_its_headers_symbols(row):
    exported = L.exported_abi(L.path(row.file))
    if row.module is None:
        assert exported == set(row.symbols)
    else:
        m, text = L.module(row), L.header_text(row)
        assert m.LIB_PATH == L.path(row.file)
        hooks = L.TEST_HOOKS.get(row.file, set())
        assert hooks <= exported and not hooks & set(m.SYMBOLS)
        assert exported - hooks == L.header_symbols(text) == set(m.SYMBOLS), (sorted(exported ^ set(m.SYMBOLS)), sorted(L.header_symbols(text) ^ set(m.SYMBOLS)))
        lib = m.load() if hasattr(m, "load") else m.lib
        define = int(re.search(r"#define %s_ABI_VERSION (\d+)" % m.PREFIX.upper(), text).group(1))
        assert getattr(lib, m.PREFIX + "_version")() == m.ABI_VERSION == define
    # -fvisibility=hidden: no function but the ABI's leaves the library
    functions = [name for name, kind in L.exported_symbols(L.path(row.file)).items() if kind == "T"]
    assert functions and all(name.startswith("mc_") for name in functions), functions
