"""KITTI's fast net (l1 4 on 9 x 9 patches) as a binding of tests/train_fast_oracle.py: constants and the oracle's
depth-taking functions with the depth filled in.  Nothing is computed here."""
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_fast_oracle as fo  # noqa: E402
from train_fast_oracle import (FM, as_f64, cubic, features_of, flat, hinge_and_fragility, loss_of, mul32,  # noqa: E402,F401
                               robust_patches, sgd_steps, tail_parts)

L1 = 4
WS = fo.ws_of(L1)
NPARAMS = fo.nparams_of(L1)
SHAPES = fo.shapes_of(L1)
assert WS == 9 and NPARAMS == 111424

warp_affine = partial(fo.warp_affine, size=WS)
make_patch_matrix = partial(fo.make_patch_matrix, WS)
make_patch = partial(fo.make_patch, WS)
sample_pair = partial(fo.sample_pair, L1)
random_layers = partial(fo.random_layers, L1)
unflat = partial(fo.unflat, L1)
check_per_tensor = partial(fo.check_per_tensor, L1)
