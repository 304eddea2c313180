"""libmctraindepth.so (include/mc_train_depth.h), the training kernels of the fast net at -l1 1..5 on either image store, as
_train_loader.Loader binds it.  Imported lazily (by train_depth.py), so inference users need only libmcadcensus.so.

Every call of the library takes l1 first.  `at_depth(l1)` is the library at one depth in the shape of the other libraries'
modules (PREFIX, MAX_PAIRS, LIB_PATH, load, check), so that train_common's TrainerBase, new_workspace and step_batch serve it
as they serve those."""
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train_depth.h
PREFIX = "mc_train_depth"
ABI_VERSION = 1
MIN_L1, MAX_L1 = 1, 5
FM = 64
NPRM = 18
MAX_PAIRS = 1024
EINVAL = -22
SIGNATURES = {
    "mc_train_depth_version": (i, []),
    "mc_train_depth_last_error": (text, []),
    "mc_train_depth_ws": (i, [i]),
    "mc_train_depth_nparams": (i, [i]),
    "mc_train_depth_workspace_bytes": (sz, [i, i]),
    "mc_train_depth_step_batch": (i, [i, vp, i, vp, vp, f, f, f, i, vp, vp, sz, vp]),
    "mc_train_depth_sample": (i, [i, vp, vp, i, i, i, vp, i64, vp, vp, i, vp, vp]),
    "mc_train_depth_run": (i, [i, vp, vp, i, i, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]),
    "mc_train_depth_mb_sample": (i, [i, vp, vp, i, vp, i64, vp, vp, vp, i, vp, vp]),
    "mc_train_depth_mb_run": (i, [i, vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


def ws_of(l1):
    """The patch side of depth l1 (get_window_size of l1 valid 3x3 convolutions)."""
    return 2 * l1 + 1


def nparams_of(l1):
    """Floats of the flat parameter buffer: w1 b1 (640), then l1 - 1 times w b of 64 -> 64 (36 928)."""
    return FM * 9 + FM + (l1 - 1) * (FM * FM * 9 + FM)


class TrainDepthError(RuntimeError):
    """A libmctraindepth.so call returned non-zero."""


_loader = Loader("libmctraindepth.so", PREFIX, ABI_VERSION, TrainDepthError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check


class _Bound:
    """The loaded library with l1 as every function's first argument."""

    def __init__(self, lib, l1):
        self._lib, self._l1 = lib, l1

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        return lambda *args: fn(self._l1, *args)


class at_depth:
    """libmctraindepth.so at depth l1, as a library module: `load()` binds l1 to every function."""
    PREFIX, MAX_PAIRS, NPRM, LIB_PATH, check = PREFIX, MAX_PAIRS, NPRM, LIB_PATH, staticmethod(check)

    def __init__(self, l1):
        self.l1, self.WS, self.NPARAMS = l1, ws_of(l1), nparams_of(l1)

    def load(self):
        return _Bound(load(), self.l1)
