"""Middlebury's accurate net (main.lua:116-130, 663-677: five convolutions on 11 x 11 patches, three hidden Linears) as a
binding of tests/train_slow_oracle.py at WS, L1, L2 = 11, 5, 3.  Nothing is computed here."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_slow_oracle import EPS, FM, NH, Net, as_f64, bce2, bce2_grad, targets  # noqa: E402,F401

NET = Net(11, 5, 3)
WS, L1, L2, CONV_SHAPES, FC_SHAPES, NAMES = NET.WS, NET.L1, NET.L2, NET.CONV_SHAPES, NET.FC_SHAPES, NET.NAMES
NCONV, NPARAMS = NET.NCONV, NET.NPARAMS
assert NCONV == 453152 and NPARAMS == 835617 and len(NAMES) == 18
random_nets, wide_nets, flat, unflat, forward = NET.random_nets, NET.wide_nets, NET.flat, NET.unflat, NET.forward
loss_of, fragile, sgd_steps, check_per_tensor = NET.loss_of, NET.fragile, NET.sgd_steps, NET.check_per_tensor
