"""Test oracle of the accurate net's training step (never imported by the product): float64 torch on the CPU of the net
(main.lua:663-677) on the reference's 4-patch batch, BCECriterion2 restated with its eps (BCECriterion2.lua), momentum SGD
(main.lua:870-874), and the selector of pairs whose ReLU masks fp32 rounding can flip.  What depends on the net's shape is
`Net(WS, L1, L2)`: L1 convolutions of 112 maps on WS x WS patches, L2 hidden Linears of 384 units.  The module's own names
serve KITTI's shape (9, 4, 4); train_mb_slow_oracle.py binds Middlebury's (11, 5, 3; main.lua:116-130)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_fast_oracle import as_f64, momentum_sgd  # noqa: E402,F401

FM, NH = 112, 384
EPS = 1e-12


def targets(n_pairs):
    import torch
    return torch.tensor([0.0, 1.0] * n_pairs, dtype=torch.float64)


def bce2(o, t):
    """BCECriterion2:updateOutput: -sum( (log(o + eps) t + log((1 - o) + eps) (1 - t)) / n )."""
    import torch
    return -((torch.log(o + EPS) * t + torch.log((1 - o) + EPS) * (1 - t)) / t.numel()).sum()


def bce2_grad(o, t):
    """BCECriterion2:updateGradInput: -( t / (o + eps) - (1 - t) / ((1 - o) + eps) ) / n."""
    return -((t / (o + EPS) - (1 - t) / ((1 - o) + EPS)) / t.numel())


class Net:
    """The accurate net of one shape: its flat layout (w1 b1 .. fw1 fb1 ..) and its float64 step."""

    def __init__(self, ws, l1, l2):
        assert ws == 2 * l1 + 1
        self.WS, self.L1, self.L2 = ws, l1, l2
        self.CONV_SHAPES = [(FM, 1 if i == 0 else FM, 3, 3) for i in range(l1)]
        self.FC_SHAPES = [(NH, 2 * FM)] + [(NH, NH)] * (l2 - 1) + [(1, NH)]
        self.NAMES = [n for i in range(l1) for n in ("w%d" % (i + 1), "b%d" % (i + 1))] + \
                     [n for i in range(l2 + 1) for n in ("fw%d" % (i + 1), "fb%d" % (i + 1))]
        self.NCONV = sum(int(np.prod(s)) + s[0] for s in self.CONV_SHAPES)
        self.NPARAMS = sum(int(np.prod(s)) + s[0] for s in self.CONV_SHAPES + self.FC_SHAPES)

    def random_nets(self, seed, gain):
        """(conv_layers, fc_layers), float32, uniform in +-gain/sqrt(fan_in), drawn from default_rng(seed): the convolutions'
        shapes first, then the Linears', w before b.  gain 1 is the reference's reset(), gain sqrt(6) the wide initialisation
        the numeric tests use (few fragile pairs, logits spread over about +-2)."""
        rng = np.random.default_rng(seed)
        out = []
        for shapes in (self.CONV_SHAPES, self.FC_SHAPES):
            layers = []
            for s in shapes:
                b = gain / np.sqrt(np.prod(s[1:]))
                layers.append((rng.uniform(-b, b, s).astype(np.float32), rng.uniform(-b, b, s[0]).astype(np.float32)))
            out.append(layers)
        return out[0], out[1]

    def wide_nets(self, seed):
        return self.random_nets(seed, np.sqrt(6.0))

    def flat(self, conv, fc):
        return np.concatenate([np.asarray(a).ravel() for wb in list(conv) + list(fc) for a in wb])

    def unflat(self, v):
        out, o = [], 0
        for s in self.CONV_SHAPES + self.FC_SHAPES:
            n = int(np.prod(s))
            out.append((np.array(v[o:o + n]).reshape(s), np.array(v[o + n:o + n + s[0]])))
            o += n + s[0]
        assert o == len(v) == self.NPARAMS
        return out[:self.L1], out[self.L1:]

    def forward(self, conv, fc, patches, preacts=None):
        """patches (n, 3, WS, WS) torch float64 -> the Sigmoid's output (2n,): sample 2i is (left, positive), 2i+1 (left,
        negative).  The batch is the reference's [L, P, L, N] per pair; Reshape(bs, 224) makes a row of two consecutive
        feature vectors.  preacts: a list that receives every convolution's and Linear's pre-activation, each as (n, -1)."""
        import torch
        import torch.nn.functional as F
        n = patches.shape[0]
        h = torch.stack([patches[:, 0], patches[:, 1], patches[:, 0], patches[:, 2]], 1).reshape(4 * n, 1, self.WS, self.WS)
        assert len(conv) == self.L1 and len(fc) == self.L2 + 1
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

    def loss_of(self, conv, fc, patches):
        return bce2(self.forward(conv, fc, patches), targets(patches.shape[0]))

    def fragile(self, conv, fc, patches, eps=3e-6):
        """Per pair: does any convolution or Linear pre-activation of the float64 forward pass lie within eps of 0, where fp32
        rounding can put it on the other side and flip a ReLU mask?  (The last Linear has no ReLU; a logit near 0 flips
        nothing.)  Uses the oracle only."""
        import torch
        with torch.no_grad():
            pre = []
            self.forward(as_f64(conv), as_f64(fc), torch.tensor(np.asarray(patches, np.float64)), pre)
            small = np.zeros(patches.shape[0], bool)
            for z in pre[:-1]:
                small |= (z.abs() < eps).any(1).numpy()
        return small

    def sgd_steps(self, conv, fc, patches_list, lr, mom, fp32_state=False, moms=None):
        """One step per batch from (conv, fc) numpy nets, by train_fast_oracle.momentum_sgd (float64 gradients, fp32_state and
        moms as there); returns (flat params, flat momenta, losses)."""
        loss = lambda layers, x: self.loss_of(layers[:self.L1], layers[self.L1:], x)
        return momentum_sgd(list(conv) + list(fc), loss, patches_list, lr, mom, fp32_state, moms)

    def check_per_tensor(self, got, want, tol, what=""):
        """Flat 18-tensor vectors: each tensor of `got` within tol of that tensor's largest magnitude in `want`, so that no
        tensor's gradient is partly missing; a tensor that is exactly 0 in `want` has to be exactly 0.  Returns the errors."""
        o, errs = 0, {}
        shapes = self.CONV_SHAPES + self.FC_SHAPES
        for k, name in enumerate(self.NAMES):
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
        assert o == got.size == want.size == self.NPARAMS
        return errs


# ---- KITTI's shape ------------------------------------------------------------------------------------------------------------
NET = Net(9, 4, 4)
WS, L1, L2, CONV_SHAPES, FC_SHAPES, NAMES, NPARAMS = NET.WS, NET.L1, NET.L2, NET.CONV_SHAPES, NET.FC_SHAPES, NET.NAMES, NET.NPARAMS
assert NPARAMS == 870449 and len(NAMES) == 18
random_nets, wide_nets, flat, unflat, forward = NET.random_nets, NET.wide_nets, NET.flat, NET.unflat, NET.forward
loss_of, fragile, sgd_steps, check_per_tensor = NET.loss_of, NET.fragile, NET.sgd_steps, NET.check_per_tensor
