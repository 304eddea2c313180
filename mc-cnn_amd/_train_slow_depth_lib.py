"""libmctrainslowdepth.so (include/mc_train_slow_depth.h), the training kernels of the accurate net at -l2 1..7 on either image
store, as _train_loader.Loader binds it.  Imported lazily (by train_slow_depth.py), so inference users need only libmcadcensus.so.

The library's size, workspace and step_batch calls take (store, l2) first, its two run calls l2.  `at_depth(store, l2)` is the
library at one store and depth in the shape of the other libraries' modules (PREFIX, MAX_PAIRS, LIB_PATH, load, check), so that
train_common's TrainerBase, new_workspace and step_batch serve it as they serve those."""
from . import _train_mb_slow_lib as tmsl
from . import _train_slow_lib as tsl
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train_slow_depth.h
PREFIX = "mc_train_slow_depth"
ABI_VERSION = 1
KITTI, MB = 0, 1
MIN_L2, MAX_L2 = 1, 7
NH2 = 384
NPRM = 18
NFC1 = 86785
NFC_STEP = 147840
MAX_PAIRS = {KITTI: 1024, MB: 256}
EINVAL = -22
SIGNATURES = {
    "mc_train_slow_depth_version": (i, []),
    "mc_train_slow_depth_last_error": (text, []),
    "mc_train_slow_depth_nparams": (i, [i, i]),
    "mc_train_slow_depth_workspace_bytes": (sz, [i, i, i]),
    "mc_train_slow_depth_step_batch": (i, [i, i, vp, i, vp, vp, f, f, vp, vp, sz, vp]),
    "mc_train_slow_depth_run": (i, [i, vp, vp, i, i, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, f, f, vp, vp, sz, vp]),
    "mc_train_slow_depth_mb_run": (i, [i, vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)
TOWERS = {KITTI: tsl, MB: tmsl}       # the store's tower is its parent library's: WS, FM, L1, NCONV
STORE_OF = {"kitti": KITTI, "kitti2015": KITTI, "mb": MB}
TAKE_STORE = ("nparams", "workspace_bytes", "step_batch")   # the calls whose first argument is the store


def nfc_of(l2):
    """Floats of the FC stack: Linear 224 -> 384, l2 - 1 times 384 -> 384, 384 -> 1, each with its bias."""
    return NFC1 + (l2 - 1) * NFC_STEP


def nparams_of(store, l2):
    """Floats of the flat parameter buffer: the store's tower, then the FC stack of depth l2."""
    return TOWERS[store].NCONV + nfc_of(l2)


class TrainSlowDepthError(RuntimeError):
    """A libmctrainslowdepth.so call returned non-zero."""


_loader = Loader("libmctrainslowdepth.so", PREFIX, ABI_VERSION, TrainSlowDepthError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check


class _Bound:
    """The loaded library with (store, l2) or l2 as every function's first arguments."""

    def __init__(self, lib, store, l2):
        self._lib, self._store, self._l2 = lib, store, l2

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        lead = (self._store, self._l2) if name[len(PREFIX) + 1:] in TAKE_STORE else (self._l2,)
        return lambda *args: fn(*lead, *args)


class at_depth:
    """libmctrainslowdepth.so at one store and depth, as a library module: `load()` binds them to every function."""
    PREFIX, NPRM, LIB_PATH, check = PREFIX, NPRM, LIB_PATH, staticmethod(check)

    def __init__(self, store, l2):
        tower = TOWERS[store]
        self.store, self.l2, self.MAX_PAIRS = store, l2, MAX_PAIRS[store]
        self.WS, self.FM, self.L1, self.L2, self.NH2 = tower.WS, tower.FM, tower.L1, l2, NH2
        self.NCONV, self.NFC, self.NPARAMS = tower.NCONV, nfc_of(l2), nparams_of(store, l2)

    def load(self):
        return _Bound(load(), self.store, self.l2)
