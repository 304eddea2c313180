"""CPU: the host side of libmcops.so (include/mc_ops.h): symbols and prototypes against the header, every refusal's code and
message, the Lua shim's cdef block token by token, make_dataset2 / subset_dataset (host functions) against numpy, the kernel
inventory, and that importing the package does not need the library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import test_lua_shim as shim  # noqa: E402  (its header / cdef parsers)
from mc_cnn_amd import _ops_lib as ol  # noqa: E402

HEADER = os.path.join(ROOT, "include", "mc_ops.h")
LUA = os.path.join(ROOT, "mc-cnn_amd", "lua", "adcensus_train.lua")
SEVEN = ("Normalize_backward_input", "Margin2", "remove_nonvisible", "remove_occluded", "remove_white", "make_dataset2", "subset_dataset")
P = 1 << 20                      # a pointer that is never dereferenced: every check precedes the first launch


def header_decls():
    return shim._decls(shim._strip_c(open(HEADER).read()))


def ctype_of(decl, is_return=False):
    d = decl.replace("const", "").strip()
    if "*" in d:
        return C.c_char_p if is_return and "char" in d else C.c_void_p
    return {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "size_t": C.c_size_t}[d.split()[0]]


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmcops.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    text = open(HEADER).read()
    assert ol.load().mc_ops_version() == ol.ABI_VERSION == 1
    exported = L.exported_abi(ol.LIB_PATH)
    assert exported == set(header_decls()) == set(ol.SYMBOLS) and len(exported) == 9
    for name, value in (("MAX_C", ol.MAX_C), ("MAX_W", ol.MAX_W), ("SUBSET_IMAGES", ol.SUBSET_IMAGES)):
        assert re.search(r"#define MC_OPS_%s %d\b" % (name, value), text), name
    assert (ol.MAX_C, ol.MAX_W, ol.SUBSET_IMAGES, ol.EINVAL) == (128, 8192, 200, -22)


def test_ctypes_signatures_equal_the_headers_prototypes():
    for name, d in header_decls().items():
        m = re.match(r"(.*?)\b%s\((.*)\)$" % name, d)
        ret, args = m.group(1), m.group(2)
        argtypes = [] if args.strip() == "void" else [ctype_of(a) for a in args.split(",")]
        assert ol.SIGNATURES[name] == (ctype_of(ret, True), argtypes), (name, d)


def test_the_library_is_built_from_its_own_units_and_holds_its_own_kernels():
    built = L.print_libraries()
    assert built["libmcops.so"] == ["ops.o", "ops_normalize.o", "error.o"]
    for older in ("libmcadcensus.so", "libmctrain.so"):       # the older kernel sets stay as they are
        assert not any("ops" in obj for obj in built[older])
    assert L.built_kernels(ol.LIB_PATH) == {"normalize_backward_kernel", "margin2_kernel<1>", "margin2_kernel<2>", "remove_nonvisible_kernel",
                                            "remove_occluded_kernel", "remove_white_kernel"}


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = ol.load()

    def nb(go=P, x=P, norm=P, gi=P, N=2, Cn=64, H=3, W=5):
        return lib.mc_normalize_backward_input(go, x, norm, gi, N, Cn, H, W, None)

    def margin(x=P, tmp=P, gi=P, n=4, pow_=1):
        return lib.mc_margin2(x, tmp, gi, n, 0.2, pow_, None)

    t_out = C.c_int64(-7)
    disp = np.full((2, 3), 1.0, np.float32)                  # six pixels above 0.5
    nnz = np.full((8, 4), -1.0, np.float32)

    def md2(d=disp.ctypes.data, H=2, W=3, out=nnz.ctypes.data, rows=8, t=0, t_out=C.addressof(t_out)):
        return lib.mc_make_dataset2(d, H, W, out, rows, 9, t, t_out)

    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    subset_out = np.full((3, 4), -1.0, np.float32)

    def subset(index=(1,), idx_ptr=True, inp=rows.ctypes.data, n_rows=3, out=subset_out.ctypes.data, n_out=C.addressof(t_out), n_index=None):
        idx = np.asarray(index, np.int64)
        return lib.mc_subset_dataset(idx.ctypes.data if idx_ptr else None, idx.size if n_index is None else n_index, inp, n_rows, out, n_out)

    bad = [("nb: null grad_output", lambda: nb(go=None), "null"), ("nb: null input", lambda: nb(x=None), "null"),
           ("nb: null norm", lambda: nb(norm=None), "null"), ("nb: null grad_input", lambda: nb(gi=None), "null"),
           ("nb: C 0", lambda: nb(Cn=0), "C 0 outside [1, 128]"), ("nb: C 129", lambda: nb(Cn=129), "C 129 outside [1, 128]"),
           ("nb: C -1", lambda: nb(Cn=-1), "outside [1, 128]"), ("nb: N 0", lambda: nb(N=0), "bad dims"), ("nb: W 0", lambda: nb(W=0), "bad dims"),
           ("nb: 2^40 elements", lambda: nb(N=1 << 20, Cn=128, H=1 << 10, W=8), "2^40"),
           ("margin2: null input", lambda: margin(x=None), "null"), ("margin2: null tmp", lambda: margin(tmp=None), "null"),
           ("margin2: null grad_input", lambda: margin(gi=None), "null"), ("margin2: pow 3", lambda: margin(pow_=3), "pow 3"),
           ("margin2: pow 0", lambda: margin(pow_=0), "pow 0"), ("margin2: negative n_pairs", lambda: margin(n=-1), "n_pairs"),
           ("remove_nonvisible: null", lambda: lib.mc_remove_nonvisible(None, 8, 4, None), "null"),
           ("remove_nonvisible: W 0", lambda: lib.mc_remove_nonvisible(P, 8, 0, None), "bad size"),
           ("remove_nonvisible: ragged", lambda: lib.mc_remove_nonvisible(P, 9, 4, None), "no whole number of rows"),
           ("remove_occluded: null", lambda: lib.mc_remove_occluded(None, 8, 4, None), "null"),
           ("remove_occluded: negative n", lambda: lib.mc_remove_occluded(P, -4, 4, None), "bad size"),
           ("remove_occluded: ragged", lambda: lib.mc_remove_occluded(P, 9, 4, None), "no whole number of rows"),
           ("remove_occluded: too wide", lambda: lib.mc_remove_occluded(P, 8193, 8193, None), "width 8193 exceeds 8192"),
           ("remove_white: null x", lambda: lib.mc_remove_white(None, P, 8, None), "null"),
           ("remove_white: null disp", lambda: lib.mc_remove_white(P, None, 8, None), "null"),
           ("remove_white: negative n", lambda: lib.mc_remove_white(P, P, -1, None), "bad size"),
           ("make_dataset2: null disp", lambda: md2(d=None), "null"), ("make_dataset2: null nnz", lambda: md2(out=None), "null"),
           ("make_dataset2: null t_out", lambda: md2(t_out=None), "null"), ("make_dataset2: H 0", lambda: md2(H=0), "bad dims"),
           ("make_dataset2: negative t", lambda: md2(t=-1), "bad list"),
           ("make_dataset2: one row short", lambda: md2(rows=5), "does not fit: 6 pixels from row 0 on, 5 rows"),
           ("make_dataset2: short from t on", lambda: md2(t=3), "does not fit: 6 pixels from row 3 on, 8 rows"),
           ("make_dataset2: t past the list", lambda: md2(t=9), "does not fit"),
           ("subset: index 200", lambda: subset(index=(3, 200)), "index 200 (at 1) outside [0, 199]"),
           ("subset: index -1", lambda: subset(index=(-1,)), "index -1 (at 0) outside [0, 199]"),
           ("subset: null index", lambda: subset(idx_ptr=False, n_index=2), "null"), ("subset: null input", lambda: subset(inp=None), "null"),
           ("subset: null output", lambda: subset(out=None), "null"), ("subset: null n_out", lambda: subset(n_out=None), "null"),
           ("subset: negative rows", lambda: subset(n_rows=-1), "bad sizes")]
    for what, call, word in bad:
        rc = call()
        assert rc == ol.EINVAL, (what, rc)
        assert word in ol.last_error() and ol.last_error().startswith("mc_"), (what, ol.last_error())
    # a refusal writes nothing
    assert t_out.value == -7 and (nnz == -1).all() and (subset_out == -1).all()
    with pytest.raises(ol.OpsError, match="pow 3"):
        ol.check(margin(pow_=3), "mc_margin2")
    # what fits exactly is taken, and empty calls launch nothing (no GPU here)
    assert md2(rows=6) == 0 and t_out.value == 6 and md2(t=2) == 0 and t_out.value == 8
    assert margin(n=0) == 0 and lib.mc_remove_nonvisible(P, 0, 4, None) == 0 and lib.mc_remove_occluded(P, 0, 4, None) == 0 and \
        lib.mc_remove_white(P, P, 0, None) == 0


# ---- the host pair against numpy --------------------------------------------------------------------------------------------------
def np_make_dataset2(disp, nnz, img, t):
    ys, xs = np.nonzero(disp > np.float32(0.5))
    nnz[t:t + ys.size] = np.stack([np.full(ys.size, img), ys, xs, disp[ys, xs]], 1).astype(np.float32)
    return t + ys.size


def test_make_dataset2_equals_numpy(mc):
    import torch
    rng = np.random.default_rng(1)
    maps = (rng.integers(0, 400, (2, 5, 9)) / 256).astype(np.float32)
    maps[0, 0, :3] = (0.5, np.float32(0.5) + np.float32(2.0 ** -24), 129 / 256)       # the threshold: 0.5 itself is not listed
    got, want = torch.full((90, 4), -1.0), np.full((90, 4), -1.0, np.float32)
    t = tw = 0
    for k, img in enumerate((7, 3)):                          # t is carried across two images
        t = mc.adcensus.make_dataset2(torch.from_numpy(maps[k]).reshape(1, 1, 5, 9), got, img, t)
        tw = np_make_dataset2(maps[k], want, img, tw)
        assert t == tw
    assert 0 < t < 90 and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    first = got.numpy()[0]
    assert tuple(first) == (7, 0, 1, maps[0, 0, 1]) and maps[0, 0, 0] == 0.5        # 0-based row and column; 0.5 skipped
    assert (got.numpy()[:t, 0] == np.repeat([7, 3], [(maps[0] > 0.5).sum(), (maps[1] > 0.5).sum()])).all()
    with pytest.raises(ol.OpsError, match="does not fit"):
        mc.adcensus.make_dataset2(torch.from_numpy(maps[0]).reshape(1, 1, 5, 9), torch.zeros((3, 4)), 1, 0)
    with pytest.raises(TypeError):
        mc.adcensus.make_dataset2(torch.from_numpy(maps[0]).double(), got, 1, 0)


def test_subset_dataset_equals_numpy(mc):
    import torch
    rng = np.random.default_rng(2)
    rows = np.stack([rng.integers(0, 200, 300), rng.integers(0, 50, 300), rng.integers(0, 60, 300), rng.uniform(1, 90, 300)], 1).astype(np.float32)
    rows[5, 0], rows[6, 0], rows[7, 0] = 200, -1, np.nan                             # image numbers outside the table: in no subset
    for index in ([0, 199, 17, 17, 60], [5], []):
        out = torch.full((300, 4), -1.0)
        n = mc.adcensus.subset_dataset(torch.tensor(index, dtype=torch.int64), torch.from_numpy(rows), out)
        want = rows[np.isin(rows[:, 0], index)]
        assert n == want.shape[0] and np.array_equal(out.numpy()[:n].view(np.uint32), want.view(np.uint32)) and (out.numpy()[n:] == -1).all()
        assert n > 0 or index != [0, 199, 17, 17, 60]
    assert n == 0 == mc.adcensus.subset_dataset(torch.tensor([], dtype=torch.int64), torch.from_numpy(rows), out)      # an empty subset
    for index in ([200], [-1]):
        with pytest.raises(ol.OpsError, match="outside"):
            mc.adcensus.subset_dataset(torch.tensor(index, dtype=torch.int64), torch.from_numpy(rows), torch.zeros((300, 4)))
    with pytest.raises(ValueError):
        mc.adcensus.subset_dataset(torch.tensor([1]), torch.from_numpy(rows), torch.zeros((299, 4)))


# ---- the Lua shim ------------------------------------------------------------------------------------------------------------------
def test_lua_cdef_matches_the_header_token_by_token():
    lua = open(LUA).read()
    hdr = header_decls()
    cdef = shim._decls(shim._strip_c(shim._cdef(lua)))
    assert cdef == hdr and len(cdef) == 9                     # every prototype, none missing, none drifted
    used = set(re.findall(r"\blib\.(mc_[a-z0-9_]+)", lua))
    assert used <= set(cdef) and used == set(hdr)
    for fn in SEVEN:
        assert re.search(r"function adcensus\.%s\(" % fn, lua), fn
    want = int(re.search(r"#define MC_OPS_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert int(re.search(r"local MC_OPS_ABI_VERSION = (\d+)", lua).group(1)) == want
    assert "lib.mc_ops_version() == MC_OPS_ABI_VERSION" in lua and "ffi.load('mcops')" in lua and "require 'adcensus'" in lua


def test_python_table_has_the_seven_names_with_the_references_arguments(mc):
    import inspect
    want = {"Normalize_backward_input": ["grad_output", "input", "norm", "grad_input"], "Margin2": ["input", "tmp", "gradInput", "margin", "pow"],
            "remove_nonvisible": ["y"], "remove_occluded": ["y"], "remove_white": ["x", "y"], "make_dataset2": ["disp", "nnz", "img", "t"],
            "subset_dataset": ["index", "input", "output"]}
    assert set(want) == set(SEVEN)
    for fn, args in want.items():
        assert list(inspect.signature(getattr(mc.adcensus, fn)).parameters) == args, fn


# ---- the package without the library -----------------------------------------------------------------------------------------------
def test_importing_the_package_does_not_need_the_library(tmp_path):
    """A copy of the package (links to its files) without libmcops.so: the import works, the first use says what is missing."""
    pkg = os.path.join(ROOT, "mc-cnn_amd")
    os.makedirs(tmp_path / "mc-cnn_amd")
    os.symlink(os.path.join(ROOT, "mc_cnn_amd.py"), tmp_path / "mc_cnn_amd.py")
    for name in os.listdir(pkg):
        if name not in ("libmcops.so", "__pycache__"):
            os.symlink(os.path.join(pkg, name), tmp_path / "mc-cnn_amd" / name)
    code = ("import os, sys; sys.path.insert(0, %r); import mc_cnn_amd; from mc_cnn_amd import _ops_lib, adcensus, modules\n"
            "assert os.path.dirname(os.path.abspath(mc_cnn_amd.__file__)) == %r and not os.path.exists(_ops_lib.LIB_PATH)\n"
            "assert callable(adcensus.Margin2) and callable(modules.Normalize2)\n"
            "try:\n    _ops_lib.load()\nexcept ImportError as e:\n    assert 'libmcops.so not found' in str(e) and 'no CPU fallback' in str(e)\n"
            "else:\n    raise SystemExit('loaded a library that is not there')\nprint('ok')\n") % (str(tmp_path), str(tmp_path / "mc-cnn_amd"))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
