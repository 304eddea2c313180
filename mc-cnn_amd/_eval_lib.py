"""libmceval.so (include/mc_eval.h), the test set's error count on the device, as _train_loader.Loader binds it.  Imported
lazily (by evalset.py), so inference users need only libmcadcensus.so."""
from ._train_loader import Loader, f, i, text, vp

# include/mc_eval.h
PREFIX = "mc_eval"
ABI_VERSION = 1
EINVAL = -22
SIGNATURES = {
    "mc_eval_version": (i, []),
    "mc_eval_last_error": (text, []),
    "mc_eval_error": (i, [vp, i, vp, i, i, i, f, vp, vp]),
}
SYMBOLS = list(SIGNATURES)


class EvalError(RuntimeError):
    """A libmceval.so call returned non-zero."""


_loader = Loader("libmceval.so", PREFIX, ABI_VERSION, EvalError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
