"""What tests/test_gpu_train_slow_depth.py and tests/test_train_slow_depth_host.py share (a plain module): the (store, l2, n_pairs)
cases of the float64 comparison, each case's oracle and wide initial nets, and the planned batch -- the parents' selector
(tests/test_gpu_train_slow.py, tests/test_gpu_train_mb_slow.py: `sturdy_pairs`) with their seeds and their bound on the share of
candidates it may drop.  The oracle alone decides; the host test runs the selector without a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_slow_oracle as so  # noqa: E402

TOWER = {"kitti": (9, 4), "mb": (11, 5)}                 # patch side, convolutions
SEED0 = {"kitti": 20, "mb": 40}                          # the parents' tests draw candidates from default_rng(SEED0 + n_pairs)
MAX_FRAGILE = 0.2                                        # the share of candidates the parents' tests let the selector drop
# n_pairs 1, 3, 17: R = 2, 6, 34 rows of the FC stack -- a lone partial 16-row tile, a partial tile, two full tiles and a partial one
ORACLE_CASES = [(d, l2, n) for d, depths in (("kitti", (1, 2, 7)), ("mb", (1, 5))) for l2 in depths for n in (1, 3, 17)]

_nets = {}


def net_of(dataset, l2):
    """(so.Net of the data set's tower at depth l2, its wide_nets(1)), made once."""
    if (dataset, l2) not in _nets:
        net = so.Net(TOWER[dataset][0], TOWER[dataset][1], l2)
        _nets[(dataset, l2)] = (net, net.wide_nets(1))
    return _nets[(dataset, l2)]


def sturdy_pairs(dataset, l2, n_pairs):
    """(the first n_pairs of 3 * n_pairs N(0, 1) candidates with no pre-activation within 3e-6 of 0 in float64, the share of
    candidates that have one)."""
    net, (conv, fc) = net_of(dataset, l2)
    rng = np.random.default_rng(SEED0[dataset] + n_pairs)
    cand = rng.standard_normal((3 * n_pairs, 3, net.WS, net.WS)).astype(np.float32)
    frag = net.fragile(conv, fc, cand)
    return cand[~frag][:n_pairs], float(frag.mean())
