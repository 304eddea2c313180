"""libmctrainmbslow.so (include/mc_train_mb_slow.h), the training kernels of Middlebury's accurate net, as
_train_loader.Loader binds it.  Imported lazily (by train_mb_slow.py), so inference users need only libmcadcensus.so."""
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train_mb_slow.h
PREFIX = "mc_train_mb_slow"
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
SIGNATURES = {
    "mc_train_mb_slow_version": (i, []),
    "mc_train_mb_slow_last_error": (text, []),
    "mc_train_mb_slow_workspace_bytes": (sz, [i]),
    "mc_train_mb_slow_step_batch": (i, [vp, i, vp, vp, f, f, vp, vp, sz, vp]),
    "mc_train_mb_slow_run": (i, [vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


class TrainMbSlowError(RuntimeError):
    """A libmctrainmbslow.so call returned non-zero."""


_loader = Loader("libmctrainmbslow.so", PREFIX, ABI_VERSION, TrainMbSlowError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
