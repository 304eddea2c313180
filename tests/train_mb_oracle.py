"""Middlebury's fast net (l1 5 on 11 x 11 patches, pairs from a ragged plane store) as a binding of
tests/train_fast_oracle.py: constants and the oracle's depth-taking functions with the depth filled in.  Nothing is computed
here.  The synthetic data.mb.* directory is tests/train_fixtures.py's."""
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_fast_oracle as fo  # noqa: E402
from train_fast_oracle import (FM, as_f64, features_of, flat, hinge_and_fragility, loss_of, mul32, robust_patches,  # noqa: E402,F401
                               sgd_steps, tail_parts)
from train_fixtures import NDISP, SCENE_TE, SCENES, write_synthetic_mb  # noqa: E402,F401

L1 = 5
WS = fo.ws_of(L1)
NPARAMS = fo.nparams_of(L1)
SHAPES = fo.shapes_of(L1)
assert WS == 11 and NPARAMS == 148352

warp_affine = partial(fo.warp_affine, size=WS)
make_patch_matrix = partial(fo.make_patch_matrix, WS)
make_patch = partial(fo.make_patch, WS)
sample_pair = partial(fo.sample_mb_pair, L1)
random_layers = partial(fo.random_layers, L1)
unflat = partial(fo.unflat, L1)
check_per_tensor = partial(fo.check_per_tensor, L1)
