"""libmcconvsplit.so (include/mc_conv_split.h), the feature nets' 3x3 convolution as three bf16 MFMAs per product, as
_train_loader.Loader binds it.  Imported lazily (by adcensus.conv3x3, for mode "bf16x3" only), so the default path needs only
libmcadcensus.so."""
from ._train_loader import Loader, i, sz, text, vp

# include/mc_conv_split.h
PREFIX = "mc_conv_split"
ABI_VERSION = 1
EINVAL = -22
CIN_STEP = 16     # MC_CONV_SPLIT_CIN_STEP: Cin is a multiple of this
MAX_COUT = 128    # MC_CONV_SPLIT_MAX_COUT
SIGNATURES = {
    "mc_conv_split_version": (i, []),
    "mc_conv_split_last_error": (text, []),
    "mc_conv_split_workspace_bytes": (sz, [i, i]),
    "mc_conv_split": (i, [vp, vp, vp, vp, i, i, i, i, i, i, vp, sz, vp]),
}
SYMBOLS = list(SIGNATURES)


def eligible(Cin, Cout):
    """the layers mc_conv_split takes (the header's rule); adcensus.conv3x3 sends every other layer to mc_conv3x3"""
    return Cin >= CIN_STEP and Cin % CIN_STEP == 0 and 1 <= Cout <= MAX_COUT


class ConvSplitError(RuntimeError):
    """A libmcconvsplit.so call returned non-zero."""


_loader = Loader("libmcconvsplit.so", PREFIX, ABI_VERSION, ConvSplitError, SIGNATURES)
LIB_PATH, load, last_error, check = _loader.path, _loader.load, _loader.last_error, _loader.check
