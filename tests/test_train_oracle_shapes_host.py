"""CPU: the layout numbers of the training tests' oracles.  The shape-generic oracles (tests/train_fast_oracle.py,
tests/train_slow_oracle.py) give the parameter counts and patch sides of every shape the product trains, the binding modules
expose exactly those of their shape, and unflat inverts flat."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_fast_oracle as fo  # noqa: E402
import train_mb_oracle as mo  # noqa: E402
import train_mb_slow_oracle as mso  # noqa: E402
import train_oracle as to  # noqa: E402
import train_slow_oracle as so  # noqa: E402

FAST_NPARAMS = {1: 640, 2: 37568, 3: 74496, 4: 111424, 5: 148352}
SLOW = {(9, 4, 4): (so, 340144, 870449), (11, 5, 3): (mso, 453152, 835617)}      # module, convolutions' share, all


def same_layers(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and x.dtype == y.dtype for wa, wb in zip(a, b) for x, y in zip(wa, wb))


@pytest.mark.parametrize("l1", sorted(FAST_NPARAMS))
def test_the_fast_net_at_every_depth(l1):
    assert fo.nparams_of(l1) == FAST_NPARAMS[l1] and fo.ws_of(l1) == 2 * l1 + 1 == (3, 5, 7, 9, 11)[l1 - 1]
    assert fo.shapes_of(l1) == [(64, 1, 3, 3)] + [(64, 64, 3, 3)] * (l1 - 1)
    layers = fo.random_layers(l1, 3)
    v = fo.flat(layers)
    assert v.dtype == np.float32 and v.size == FAST_NPARAMS[l1]
    assert same_layers(fo.unflat(l1, v), layers)
    with pytest.raises(AssertionError):
        fo.unflat(l1, v[:-1])


@pytest.mark.parametrize("mod, l1", [(to, 4), (mo, 5)], ids=["train_oracle", "train_mb_oracle"])
def test_the_fast_bindings_expose_their_depth(mod, l1):
    assert (mod.L1, mod.WS, mod.FM, mod.NPARAMS) == (l1, fo.ws_of(l1), 64, FAST_NPARAMS[l1])
    assert mod.SHAPES == fo.shapes_of(l1)
    layers = mod.random_layers(3)
    assert same_layers(layers, fo.random_layers(l1, 3))
    assert same_layers(mod.unflat(mod.flat(layers)), layers)
    assert mod.make_patch(None, 0, 0, (1, 1), 0, (0, 0), 0, 0, 1).shape == (mod.WS, mod.WS)


@pytest.mark.parametrize("shape", sorted(SLOW), ids=["kitti", "mb"])
def test_the_accurate_net_of_both_shapes(shape):
    mod, nconv, nparams = SLOW[shape]
    net = so.Net(*shape)
    assert (net.NCONV, net.NPARAMS) == (nconv, nparams) and len(net.NAMES) == 18
    # the module of that shape exposes exactly these values
    assert (mod.WS, mod.L1, mod.L2, mod.FM, mod.NH, mod.NPARAMS) == shape + (112, 384, nparams)
    assert mod.CONV_SHAPES == net.CONV_SHAPES and mod.FC_SHAPES == net.FC_SHAPES and mod.NAMES == net.NAMES
    assert len(mod.CONV_SHAPES) == shape[1] and len(mod.FC_SHAPES) == shape[2] + 1
    conv, fc = mod.random_nets(3, 1.0)
    v = mod.flat(conv, fc)
    assert v.dtype == np.float32 and v.size == nparams
    c2, f2 = mod.unflat(v)
    assert same_layers(c2, conv) and same_layers(f2, fc)
    with pytest.raises(AssertionError):
        mod.unflat(v[:-1])
