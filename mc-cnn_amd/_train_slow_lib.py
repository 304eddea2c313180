"""libmctrainslow.so (include/mc_train_slow.h), the training kernels of the accurate architecture, as _train_loader.Loader
binds it.  Imported lazily (by train_slow.py), so inference users need only libmcadcensus.so."""
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train_slow.h
PREFIX = "mc_train_slow"
ABI_VERSION = 1
WS = 9
FM = 112
L1 = 4
L2 = 4
NH2 = 384
NPRM = 18
NCONV = 340144
NFC = 530305
NPARAMS = 870449
MAX_PAIRS = 1024
EINVAL = -22
SIGNATURES = {
    "mc_train_slow_version": (i, []),
    "mc_train_slow_last_error": (text, []),
    "mc_train_slow_workspace_bytes": (sz, [i]),
    "mc_train_slow_step_batch": (i, [vp, i, vp, vp, f, f, vp, vp, sz, vp]),
    "mc_train_slow_run": (i, [vp, vp, i, i, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, f, f, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


class TrainSlowError(RuntimeError):
    """A libmctrainslow.so call returned non-zero."""


_loader = Loader("libmctrainslow.so", PREFIX, ABI_VERSION, TrainSlowError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
