"""ctypes loader for libmctrainmbslow.so (include/mc_train_mb_slow.h), the training kernels of Middlebury's accurate net.
There is NO fallback: if the HIP library is missing or fails to load, `load()` raises.  Imported lazily (by
train_mb_slow.py), so inference users need only libmcadcensus.so."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmctrainmbslow.so")

# include/mc_train_mb_slow.h
ABI_VERSION = 1
WS = 11
FM = 112
L1 = 5
L2 = 3
NH2 = 384
NPRM = 18
NCONV = 453152
NFC = 382465
NPARAMS = 835617
MAX_PAIRS = 256
EINVAL = -22
SYMBOLS = ["mc_train_mb_slow_version", "mc_train_mb_slow_last_error", "mc_train_mb_slow_workspace_bytes", "mc_train_mb_slow_step_batch",
           "mc_train_mb_slow_run"]

_lib = None


class TrainMbSlowError(RuntimeError):
    """A libmctrainmbslow.so call returned non-zero."""


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
    lib.mc_train_mb_slow_version.restype = i
    lib.mc_train_mb_slow_last_error.restype = C.c_char_p
    lib.mc_train_mb_slow_workspace_bytes.argtypes = [i]
    lib.mc_train_mb_slow_workspace_bytes.restype = sz
    lib.mc_train_mb_slow_step_batch.argtypes = [vp, i, vp, vp, f, f, vp, vp, sz, vp]
    lib.mc_train_mb_slow_run.argtypes = [vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, vp, vp, sz, vp]
    for name in ("mc_train_mb_slow_step_batch", "mc_train_mb_slow_run"):
        getattr(lib, name).restype = i
    if lib.mc_train_mb_slow_version() != ABI_VERSION:
        raise ImportError("mc-cnn_amd: libmctrainmbslow.so ABI version mismatch")
    _lib = lib
    return lib


def last_error():
    msg = load().mc_train_mb_slow_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what):
    if rc != 0:
        raise TrainMbSlowError("%s failed (rc=%d): %s" % (what, rc, last_error()))
