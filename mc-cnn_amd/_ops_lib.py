"""libmcops.so (include/mc_ops.h), the training and dataset operators of the reference's adcensus.* table, as
_train_loader.Loader binds it.  Loaded lazily (by adcensus.py's seven functions and modules.py), so importing the package needs
only libmcadcensus.so."""
from ._train_loader import Loader, f, i, i64, text, vp

# include/mc_ops.h
PREFIX = "mc_ops"
ABI_VERSION = 1
EINVAL = -22
MAX_C = 128
MAX_W = 8192
SUBSET_IMAGES = 200
SIGNATURES = {
    "mc_ops_version": (i, []),
    "mc_ops_last_error": (text, []),
    "mc_normalize_backward_input": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
    "mc_margin2": (i, [vp, vp, vp, i, f, i, vp]),
    "mc_remove_nonvisible": (i, [vp, i64, i, vp]),
    "mc_remove_occluded": (i, [vp, i64, i, vp]),
    "mc_remove_white": (i, [vp, vp, i64, vp]),
    "mc_make_dataset2": (i, [vp, i, i, vp, i64, i, i64, vp]),
    "mc_subset_dataset": (i, [vp, i64, vp, i64, vp, vp]),
}
SYMBOLS = list(SIGNATURES)


class OpsError(RuntimeError):
    """A libmcops.so call returned non-zero."""


_loader = Loader("libmcops.so", PREFIX, ABI_VERSION, OpsError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
