"""Test oracle of the fast net at any depth (never imported by the product): train_oracle.py's make_patch restatement and float64
torch autograd step with the depth l1 as a parameter -- l1 valid 3x3 convolutions of 64 maps on patches of side 2 l1 + 1
(main.lua:726-746 with -l1 l1 -fm 64) -- on train_oracle's size-generic warp, for a KITTI store (x0, x1) and a ragged plane store."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_oracle import as_f64, mul32, tail_parts, warp_affine  # noqa: E402

FM = 64


def ws_of(l1):
    return 2 * l1 + 1


def nparams_of(l1):
    return FM * 9 + FM + (l1 - 1) * (FM * FM * 9 + FM)


def shapes_of(l1):
    return [(FM, 1 if i == 0 else FM, 3, 3) for i in range(l1)]


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def make_patch_matrix(ws, dim3, dim4, scale, phi, trans, hshear):
    """The 2x3 matrix make_patch hands to cv.warp_affine, as float32, with the ws-pixel window's centre shift."""
    m = [1, 0, -dim4, 0, 1, -dim3]
    m = mul32([1, 0, trans[0], 0, 1, trans[1]], m)
    m = mul32([scale[0], 0, 0, 0, scale[1], 0], m)
    c, s = math.cos(phi), math.sin(phi)
    m = mul32([c, s, 0, -s, c, 0], m)
    m = mul32([1, hshear, 0, 0, 1, 0], m)
    m = mul32([1, 0, (ws - 1) / 2, 0, 1, (ws - 1) / 2], m)
    return np.array(m, np.float32)


def make_patch(ws, src, dim3, dim4, scale, phi, trans, hshear, brightness, contrast):
    """main.lua:607-619: warp into ws x ws, then dst:mul(contrast):add(brightness) in float32.  src None: a source that reads
    0 everywhere."""
    if src is None:
        dst = np.zeros((ws, ws), np.float32)
    else:
        dst = warp_affine(src, make_patch_matrix(ws, dim3, dim4, scale, phi, trans, hshear), size=ws)
    return (dst * np.float32(contrast)).astype(np.float32) + np.float32(brightness)


def _pair(ws, left_src, right_src, nnz_row, prm):
    prm = [float(np.float32(v)) for v in prm]
    _, dim3, dim4, d = [float(np.float32(v)) for v in nnz_row]
    left = make_patch(ws, left_src, dim3, dim4, prm[2:4], prm[4], prm[5:7], prm[7], prm[8], prm[9])
    r = dict(scale=prm[10:12], phi=prm[12], trans=prm[13:15], hshear=prm[15], brightness=prm[16], contrast=prm[17])
    return np.stack([left, make_patch(ws, right_src, dim3, dim4 - d + prm[0], **r), make_patch(ws, right_src, dim3, dim4 - d + prm[1], **r)])


def sample_pair(l1, x0, x1, nnz_row, prm):
    """The three patches (left, positive, negative) of a pair from a KITTI store, as include/mc_train.h lays them out."""
    i = int(np.float32(nnz_row[0])) - 1
    return _pair(ws_of(l1), x0[i], x1[i], nnz_row, prm)


def sample_mb_pair(l1, planes, nnz_row, src, prm):
    """The same from a ragged store: planes is a list of 2-D arrays, src the pair's two plane ids (left; both right patches).
    A plane id outside the list reads 0."""
    pick = lambda k: planes[k] if 0 <= k < len(planes) else None
    return _pair(ws_of(l1), pick(src[0]), pick(src[1]), nnz_row, prm)


# ---- the net of depth l1 and its step in float64 torch autograd -----------------------------------------------------------------
def random_layers(l1, seed):
    """nn.SpatialConvolution:reset's range, +-1/sqrt(fan_in), from numpy's generator."""
    rng = np.random.default_rng(seed)
    out = []
    for s in shapes_of(l1):
        bound = 1.0 / np.sqrt(s[1] * 9)
        out.append((rng.uniform(-bound, bound, s).astype(np.float32), rng.uniform(-bound, bound, (FM,)).astype(np.float32)))
    return out


def flat(layers):
    return np.concatenate([np.asarray(a, np.float32).ravel() for wb in layers for a in wb])


def unflat(l1, v):
    v, out, o = np.asarray(v), [], 0
    for s in shapes_of(l1):
        n = int(np.prod(s))
        out.append((v[o:o + n].reshape(s).copy(), v[o + n:o + n + FM].copy()))
        o += n + FM
    assert o == v.size == nparams_of(l1)
    return out


def features_of(layers, patches, preacts=None):
    """The net on the reference's 4-patch batch [L, P, L, N] per pair: patches (n, 3, ws, ws) -> (4n, 64, 1, 1), its depth that
    of `layers`.  preacts: a list that receives every layer's pre-activations."""
    import torch
    import torch.nn.functional as F
    n, ws = patches.shape[0], ws_of(len(layers))
    assert tuple(patches.shape[1:]) == (3, ws, ws)
    h = torch.stack([patches[:, 0], patches[:, 1], patches[:, 0], patches[:, 2]], 1).reshape(4 * n, 1, ws, ws)
    for i, (w, bias) in enumerate(layers):
        h = F.conv2d(h, w, bias)
        if preacts is not None:
            preacts.append(h)
        if i < len(layers) - 1:
            h = F.relu(h)
    assert h.shape[2:] == (1, 1)
    return h


def loss_of(layers, patches, margin, pow_):
    """Margin2(StereoJoin1(Normalize2(net(batch)))), the mean over the pairs."""
    return tail_parts(features_of(layers, patches), margin, pow_)[2].mean()


def hinge_and_fragility(layers, patches, margin, eps=3e-6):
    """train_oracle.hinge_and_fragility's rule and eps at the depth of `layers`: the hinge argument f = neg - pos + margin of each
    pair in float64, and whether some pre-activation before a ReLU, or f itself, lies within eps of 0."""
    import torch
    with torch.no_grad():
        pre = []
        h = features_of(as_f64(layers), torch.tensor(np.asarray(patches, np.float64)), pre)
        _, s, _ = tail_parts(h, margin, 1)
        f = (s[1::2] - s[0::2] + margin).numpy()
        n = patches.shape[0]
        small = np.zeros(n, bool)
        for z in pre[:-1]:
            small |= (z.abs().reshape(n, -1) < eps).any(1).numpy()
        small |= np.abs(f) < eps
    return f, small


def sgd_steps(params, patches_list, lr, mom, margin, pow_, fp32_state=False, moms=None):
    """train_oracle.sgd_steps for the depth of `params` ([(w, b)] numpy): one step per batch with float64 gradients,
    v = mom * v - lr * g, w += v.  Returns the flat parameters, momenta and the losses.  fp32_state: the state is rounded to
    float32 after every update.  moms: flat initial momenta (default 0)."""
    import torch
    ps = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for wb in params for a in wb]
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
        loss = loss_of([(ps[2 * i], ps[2 * i + 1]) for i in range(len(ps) // 2)], x, margin, pow_)
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


def check_per_tensor(l1, got, want, tol, what=""):
    """Flat w1 b1 .. w_l1 b_l1 vectors: each tensor of `got` within tol of that tensor's largest magnitude in `want`, so that no
    tensor's gradient is partly missing; a tensor that is exactly 0 in `want` has to be exactly 0."""
    o = 0
    for i, s in enumerate(shapes_of(l1), 1):
        for name, n in (("w%d" % i, int(np.prod(s))), ("b%d" % i, FM)):
            g, x = got[o:o + n], want[o:o + n]
            top = np.abs(x).max()
            if top == 0:
                assert np.abs(g).max() == 0, "%s %s: float64 says exactly 0" % (what, name)
            else:
                err = np.abs(g - x).max() / top
                print("%s %s: max error %.2e of its largest magnitude %.2e" % (what, name, err, top))
                assert err <= tol, "%s %s" % (what, name)
            o += n
    assert o == got.size == want.size == nparams_of(l1)
