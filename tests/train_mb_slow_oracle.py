"""Test oracle of `mb slow`'s training step (never imported by the product): float64 torch on the CPU of Middlebury's
accurate net (main.lua:116-130, 663-677: five convolutions on 11 x 11 patches, three hidden Linears) on the reference's
4-patch batch.  It is tests/train_slow_oracle.py for WS, L1, L2 = 11, 5, 3: BCECriterion2 with its eps, the targets and the
float64 conversion are that module's own functions; what depends on the net's shapes is restated here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_slow_oracle import EPS, as_f64, bce2, bce2_grad, targets  # noqa: E402,F401

WS, FM, NH, L1, L2 = 11, 112, 384, 5, 3
CONV_SHAPES = [(FM, 1 if i == 0 else FM, 3, 3) for i in range(L1)]
FC_SHAPES = [(NH, 2 * FM)] + [(NH, NH)] * (L2 - 1) + [(1, NH)]
NAMES = [n for i in range(L1) for n in ("w%d" % (i + 1), "b%d" % (i + 1))] + \
        [n for i in range(L2 + 1) for n in ("fw%d" % (i + 1), "fb%d" % (i + 1))]
NCONV = sum(int(np.prod(s)) + s[0] for s in CONV_SHAPES)
NPARAMS = sum(int(np.prod(s)) + s[0] for s in CONV_SHAPES + FC_SHAPES)
assert NCONV == 453152 and NPARAMS == 835617 and len(NAMES) == 18


def random_nets(seed, gain):
    """(conv_layers, fc_layers), float32, uniform in +-gain/sqrt(fan_in), drawn from default_rng(seed): the convolutions'
    shapes first, then the Linears', w before b.  gain 1 is the reference's reset(), gain sqrt(6) the wide initialisation
    the numeric tests use (few fragile pairs)."""
    rng = np.random.default_rng(seed)
    out = []
    for shapes in (CONV_SHAPES, FC_SHAPES):
        layers = []
        for s in shapes:
            b = gain / np.sqrt(np.prod(s[1:]))
            layers.append((rng.uniform(-b, b, s).astype(np.float32), rng.uniform(-b, b, s[0]).astype(np.float32)))
        out.append(layers)
    return out[0], out[1]


def wide_nets(seed):
    return random_nets(seed, np.sqrt(6.0))


def flat(conv, fc):
    return np.concatenate([np.asarray(a).ravel() for wb in list(conv) + list(fc) for a in wb])


def unflat(v):
    out, o = [], 0
    for s in CONV_SHAPES + FC_SHAPES:
        n = int(np.prod(s))
        out.append((np.array(v[o:o + n]).reshape(s), np.array(v[o + n:o + n + s[0]])))
        o += n + s[0]
    assert o == len(v) == NPARAMS
    return out[:L1], out[L1:]


def forward(conv, fc, patches, preacts=None):
    """patches (n, 3, 11, 11) torch float64 -> the Sigmoid's output (2n,): sample 2i is (left, positive), 2i+1 (left, negative).
    The batch is the reference's [L, P, L, N] per pair; Reshape(bs, 224) makes a row of two consecutive feature vectors.
    preacts: a list that receives every convolution's and Linear's pre-activation, each as (n, -1)."""
    import torch
    import torch.nn.functional as F
    n = patches.shape[0]
    h = torch.stack([patches[:, 0], patches[:, 1], patches[:, 0], patches[:, 2]], 1).reshape(4 * n, 1, WS, WS)
    assert len(conv) == L1 and len(fc) == L2 + 1
    for w, b in conv:
        h = F.conv2d(h, w, b)
        if preacts is not None:
            preacts.append(h.reshape(n, -1))
        h = F.relu(h)
    assert h.shape[2:] == (1, 1)
    h = h.reshape(2 * n, 2 * FM)
    for i, (w, b) in enumerate(fc):
        h = F.linear(h, w, b)
        if preacts is not None:
            preacts.append(h.reshape(n, -1))
        if i < len(fc) - 1:
            h = F.relu(h)
    return torch.sigmoid(h.reshape(2 * n))


def loss_of(conv, fc, patches):
    return bce2(forward(conv, fc, patches), targets(patches.shape[0]))


def fragile(conv, fc, patches, eps=3e-6):
    """Per pair: does any convolution or Linear pre-activation of the float64 forward pass lie within eps of 0, where fp32
    rounding can put it on the other side and flip a ReLU mask?  (The last Linear has no ReLU; a logit near 0 flips
    nothing.)  Uses the oracle only."""
    import torch
    with torch.no_grad():
        pre = []
        forward(as_f64(conv), as_f64(fc), torch.tensor(np.asarray(patches, np.float64)), pre)
        small = np.zeros(patches.shape[0], bool)
        for z in pre[:-1]:
            small |= (z.abs() < eps).any(1).numpy()
    return small


def sgd_steps(conv, fc, patches_list, lr, mom, fp32_state=False, moms=None):
    """One step per batch from (conv, fc) numpy nets; returns (flat params, flat momenta, losses).  Gradients in float64;
    fp32_state: parameters and momenta are stored in float32 after every update (the reference's and the product's
    state).  moms: flat initial momenta (default 0)."""
    import torch
    ps = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for wb in list(conv) + list(fc) for a in wb]
    vs = [torch.zeros_like(p) for p in ps]
    if moms is not None:
        o = 0
        for v in vs:
            v.copy_(torch.tensor(np.asarray(moms[o:o + v.numel()], np.float64)).reshape(v.shape))
            o += v.numel()
    losses = []
    for patches in patches_list:
        x = torch.tensor(np.asarray(patches, np.float64))
        for p in ps:
            p.grad = None
        layers = [(ps[2 * i], ps[2 * i + 1]) for i in range(len(ps) // 2)]
        loss = loss_of(layers[:L1], layers[L1:], x)
        loss.backward()
        losses.append(loss.item())
        with torch.no_grad():
            for p, v in zip(ps, vs):
                if fp32_state:
                    f = lambda t: t.float().double()
                    v.copy_(f(f(v * mom) - f(lr * p.grad)))
                    p.copy_(f(p + v))
                else:
                    v.mul_(mom).add_(p.grad, alpha=-lr)
                    p.add_(v)
    cat = lambda ts: np.concatenate([t.detach().numpy().ravel() for t in ts])
    return cat(ps), cat(vs), losses


def check_per_tensor(got, want, tol, what=""):
    """Flat 18-tensor vectors: each tensor of `got` within tol of that tensor's largest magnitude in `want`, so that no
    tensor's gradient is partly missing; a tensor that is exactly 0 in `want` has to be exactly 0.  Returns the errors."""
    o, errs = 0, {}
    shapes = CONV_SHAPES + FC_SHAPES
    for k, name in enumerate(NAMES):
        n = int(np.prod(shapes[k // 2])) if k % 2 == 0 else shapes[k // 2][0]
        g, x = got[o:o + n], want[o:o + n]
        top = np.abs(x).max()
        if top == 0:
            assert np.abs(g).max() == 0, "%s %s: float64 says exactly 0" % (what, name)
            errs[name] = 0.0
        else:
            errs[name] = float(np.abs(g - x).max() / top)
            print("%s %s: max error %.2e of its largest magnitude %.2e" % (what, name, errs[name], top))
            assert errs[name] <= tol, "%s %s: %.3e" % (what, name, errs[name])
        o += n
    assert o == got.size == want.size == NPARAMS
    return errs
