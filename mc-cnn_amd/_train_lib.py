"""libmctrain.so (include/mc_train.h), the training kernels of the fast architecture and the KITTI dataset preparation of
preprocess_kitti.py, as _train_loader.Loader binds it.  Imported lazily (by train.py and preprocess_kitti.py), so inference
users need only libmcadcensus.so."""
from ._train_loader import Loader, f, i, i64, sz, text, vp

# include/mc_train.h
PREFIX = "mc_train"
ABI_VERSION = 2
WS = 9
FM = 64
L1 = 4
NPRM = 18
NPARAMS = 111424
GT_MAX_W = 8192
SIGNATURES = {
    "mc_train_version": (i, []),
    "mc_train_last_error": (text, []),
    "mc_train_workspace_bytes": (sz, [i]),
    "mc_train_sample": (i, [vp, vp, i, i, i, vp, i64, vp, vp, i, vp, vp]),
    "mc_train_step_batch": (i, [vp, i, vp, vp, f, f, f, i, vp, vp, sz, vp]),
    "mc_train_run": (i, [vp, vp, i, i, i, vp, i64, vp, i64, i64, i, i, vp, vp, vp, f, f, f, i, vp, vp, sz, vp]),
    "mc_train_filter_gt": (i, [vp, vp, i, i, i, vp]),
    "mc_train_nnz_workspace_bytes": (sz, [i, i]),
    "mc_train_nnz_count": (i, [vp, i, i, i, vp, vp, sz, vp]),
    "mc_train_nnz_fill": (i, [vp, vp, i, i, i, vp, i64, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


class TrainError(RuntimeError):
    """A libmctrain.so call returned non-zero."""


_loader = Loader("libmctrain.so", PREFIX, ABI_VERSION, TrainError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
