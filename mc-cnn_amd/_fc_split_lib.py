"""libmcfcsplit.so (include/mc_fc_split.h), the accurate net's FC stack as three bf16 MFMAs per product, as _train_loader.Loader
binds it.  Imported lazily (by fc.py, for mode "bf16x3" only), so the default path needs only libmcadcensus.so."""
import ctypes as C

from ._train_loader import Loader, i, sz, text, vp

# include/mc_fc_split.h
PREFIX = "mc_fc_split"
ABI_VERSION = 1
EINVAL = -22
NH = 384        # MC_FC_SPLIT_NH
VOXELS = 96     # MC_FC_SPLIT_VOXELS: voxels of one (y, d) per workgroup
SIGNATURES = {
    "mc_fc_split_version": (i, []),
    "mc_fc_split_last_error": (text, []),
    "mc_fc_split_workspace_bytes": (sz, [i, i, i, i]),
    "mc_fc_split_stack": (i, [vp, vp, i, i, i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(i), i, vp, vp, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


class FcSplitError(RuntimeError):
    """A libmcfcsplit.so call returned non-zero."""


_loader = Loader("libmcfcsplit.so", PREFIX, ABI_VERSION, FcSplitError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
