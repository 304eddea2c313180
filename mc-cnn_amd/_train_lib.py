"""ctypes loader for libmctrain.so (include/mc_train.h), the training kernels of the fast architecture and the KITTI
dataset preparation of preprocess_kitti.py.  There is NO fallback: if the HIP library is missing or fails to load, `load()`
raises.  Imported lazily (by train.py and preprocess_kitti.py), so inference users need only libmcadcensus.so."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmctrain.so")

# include/mc_train.h
ABI_VERSION = 2
WS = 9
FM = 64
L1 = 4
NPRM = 18
NPARAMS = 111424
GT_MAX_W = 8192
SYMBOLS = ["mc_train_version", "mc_train_last_error", "mc_train_workspace_bytes", "mc_train_sample", "mc_train_step_batch",
           "mc_train_run", "mc_train_filter_gt", "mc_train_nnz_workspace_bytes", "mc_train_nnz_count", "mc_train_nnz_fill"]

_lib = None


class TrainError(RuntimeError):
    """A libmctrain.so call returned non-zero."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "mc-cnn_amd: %s not found. Build it with `make -C mc-cnn_amd/csrc` (hipcc, gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for s in SYMBOLS:
        getattr(lib, s)
    vp, i, f, i64, sz = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_size_t
    lib.mc_train_version.restype = i
    lib.mc_train_last_error.restype = C.c_char_p
    lib.mc_train_workspace_bytes.argtypes = [i]
    lib.mc_train_workspace_bytes.restype = sz
    lib.mc_train_sample.argtypes = [vp, vp, i, i, i, vp, i64, vp, vp, i, vp, vp]
    lib.mc_train_step_batch.argtypes = [vp, i, vp, vp, f, f, f, i, vp, vp, sz, vp]
    lib.mc_train_run.argtypes = [vp, vp, i, i, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]
    lib.mc_train_filter_gt.argtypes = [vp, vp, i, i, i, vp]
    lib.mc_train_nnz_workspace_bytes.argtypes = [i, i]
    lib.mc_train_nnz_workspace_bytes.restype = sz
    lib.mc_train_nnz_count.argtypes = [vp, i, i, i, vp, vp, sz, vp]
    lib.mc_train_nnz_fill.argtypes = [vp, vp, i, i, i, vp, i64, vp, sz, vp]
    for name in ("mc_train_sample", "mc_train_step_batch", "mc_train_run", "mc_train_filter_gt", "mc_train_nnz_count",
                 "mc_train_nnz_fill"):
        getattr(lib, name).restype = i
    if lib.mc_train_version() != ABI_VERSION:
        raise ImportError("mc-cnn_amd: libmctrain.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().mc_train_last_error()
        raise TrainError("%s failed (rc=%d): %s" % (what, rc, msg.decode("utf-8", "replace") if msg else ""))
