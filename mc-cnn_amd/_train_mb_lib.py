"""ctypes loader for libmctrainmb.so (include/mc_train_mb.h), the training kernels of Middlebury's five-layer fast net.
There is NO fallback: if the HIP library is missing or fails to load, `load()` raises.  Imported lazily (by train_mb.py),
so inference users need only libmcadcensus.so."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmctrainmb.so")

# include/mc_train_mb.h
ABI_VERSION = 1
WS = 11
L1 = 5
FM = 64
NPRM = 18
NPARAMS = 148352
MAX_PAIRS = 1024
EINVAL = -22
PLANE_BYTES = 16            # mc_train_mb_plane: int64 offset, int32 H, int32 W
MIN_SIDE, MAX_SIDE = 4, 32767   # the sampler's limits on a plane's H and W: this loader's callers refuse the rest
SYMBOLS = ["mc_train_mb_version", "mc_train_mb_last_error", "mc_train_mb_workspace_bytes", "mc_train_mb_sample",
           "mc_train_mb_step_batch", "mc_train_mb_run"]

_lib = None


class TrainMbError(RuntimeError):
    """A libmctrainmb.so call returned non-zero."""


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
    lib.mc_train_mb_version.restype = i
    lib.mc_train_mb_last_error.restype = C.c_char_p
    lib.mc_train_mb_workspace_bytes.argtypes = [i]
    lib.mc_train_mb_workspace_bytes.restype = sz
    lib.mc_train_mb_sample.argtypes = [vp, vp, i, vp, i64, vp, vp, vp, i, vp, vp]
    lib.mc_train_mb_step_batch.argtypes = [vp, i, vp, vp, f, f, f, i, vp, vp, sz, vp]
    lib.mc_train_mb_run.argtypes = [vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]
    for name in ("mc_train_mb_sample", "mc_train_mb_step_batch", "mc_train_mb_run"):
        getattr(lib, name).restype = i
    if lib.mc_train_mb_version() != ABI_VERSION:
        raise ImportError("mc-cnn_amd: libmctrainmb.so ABI version mismatch")
    _lib = lib
    return lib


def last_error():
    msg = load().mc_train_mb_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what):
    if rc != 0:
        raise TrainMbError("%s failed (rc=%d): %s" % (what, rc, last_error()))
