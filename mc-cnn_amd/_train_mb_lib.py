"""libmctrainmb.so (include/mc_train_mb.h), the training kernels of Middlebury's five-layer fast net, as
_train_loader.Loader binds it.  Imported lazily (by train_mb.py), so inference users need only libmcadcensus.so."""
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train_mb.h
PREFIX = "mc_train_mb"
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
SIGNATURES = {
    "mc_train_mb_version": (i, []),
    "mc_train_mb_last_error": (text, []),
    "mc_train_mb_workspace_bytes": (sz, [i]),
    "mc_train_mb_sample": (i, [vp, vp, i, vp, i64, vp, vp, vp, i, vp, vp]),
    "mc_train_mb_step_batch": (i, [vp, i, vp, vp, f, f, f, i, vp, vp, sz, vp]),
    "mc_train_mb_run": (i, [vp, vp, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


class TrainMbError(RuntimeError):
    """A libmctrainmb.so call returned non-zero."""


_loader = Loader("libmctrainmb.so", PREFIX, ABI_VERSION, TrainMbError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
