"""Test oracle of Middlebury's training path (never imported by the product): make_patch (main.lua:603-619) restated for
11 x 11 patches on train_oracle's size-generic warp, the sampling of a pair from a ragged plane store, and float64 torch
autograd on the CPU of the five-layer fast net's training step (main.lua:726-746, 853-874 with -l1 5 -fm 64)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_oracle import as_f64, mul32, tail_parts, warp_affine  # noqa: E402

WS = 11
L1 = 5
FM = 64
NPARAMS = 148352
SHAPES = [(FM, 1 if i == 0 else FM, 3, 3) for i in range(L1)]
NAMES = [n for i in range(L1) for n in ("w%d" % (i + 1), "b%d" % (i + 1))]


def make_patch_matrix(dim3, dim4, scale, phi, trans, hshear):
    """The 2x3 matrix make_patch hands to cv.warp_affine, as float32, with the 11-pixel window's centre shift."""
    m = [1, 0, -dim4, 0, 1, -dim3]
    m = mul32([1, 0, trans[0], 0, 1, trans[1]], m)
    m = mul32([scale[0], 0, 0, 0, scale[1], 0], m)
    c, s = math.cos(phi), math.sin(phi)
    m = mul32([c, s, 0, -s, c, 0], m)
    m = mul32([1, hshear, 0, 0, 1, 0], m)
    m = mul32([1, 0, (WS - 1) / 2, 0, 1, (WS - 1) / 2], m)
    return np.array(m, np.float32)


def make_patch(src, dim3, dim4, scale, phi, trans, hshear, brightness, contrast):
    """main.lua:607-619: warp into 11 x 11, then dst:mul(contrast):add(brightness) in float32.  src None: a source that
    reads 0 everywhere."""
    if src is None:
        dst = np.zeros((WS, WS), np.float32)
    else:
        dst = warp_affine(src, make_patch_matrix(dim3, dim4, scale, phi, trans, hshear), size=WS)
    return (dst * np.float32(contrast)).astype(np.float32) + np.float32(brightness)


def sample_pair(planes, nnz_row, src, prm):
    """The three patches (left, positive, negative) of a pair: planes is a list of 2-D arrays, src the pair's two plane ids
    (left; both right patches), nnz_row (img, row, col, d) or None for a row outside the nnz.  A plane id outside the list
    and a missing row read 0."""
    prm = [float(np.float32(v)) for v in prm]
    pick = lambda k: planes[k] if nnz_row is not None and 0 <= k < len(planes) else None
    _, dim3, dim4, d = [float(np.float32(v)) for v in (nnz_row if nnz_row is not None else (0, 0, 0, 0))]
    left = make_patch(pick(src[0]), dim3, dim4, prm[2:4], prm[4], prm[5:7], prm[7], prm[8], prm[9])
    r = dict(scale=prm[10:12], phi=prm[12], trans=prm[13:15], hshear=prm[15], brightness=prm[16], contrast=prm[17])
    pos = make_patch(pick(src[1]), dim3, dim4 - d + prm[0], **r)
    neg = make_patch(pick(src[1]), dim3, dim4 - d + prm[1], **r)
    return np.stack([left, pos, neg])


# ---- the five-layer net and its step in float64 torch autograd -------------------------------------------------------------
def random_layers(seed):
    """nn.SpatialConvolution:reset's range, +-1/sqrt(fan_in), from numpy's generator."""
    rng = np.random.default_rng(seed)
    out = []
    for s in SHAPES:
        bound = 1.0 / np.sqrt(s[1] * 9)
        out.append((rng.uniform(-bound, bound, s).astype(np.float32), rng.uniform(-bound, bound, (FM,)).astype(np.float32)))
    return out


def flat(layers):
    return np.concatenate([np.asarray(a, np.float32).ravel() for wb in layers for a in wb])


def unflat(v):
    v, out, o = np.asarray(v), [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append((v[o:o + n].reshape(s).copy(), v[o + n:o + n + FM].copy()))
        o += n + FM
    assert o == v.size == NPARAMS
    return out


def features_of(layers, patches, preacts=None):
    """The net on the reference's 4-patch batch [L, P, L, N] per pair: patches (n, 3, 11, 11) -> (4n, 64, 1, 1).
    preacts: a list that receives every layer's pre-activations."""
    import torch
    import torch.nn.functional as F
    n = patches.shape[0]
    h = torch.stack([patches[:, 0], patches[:, 1], patches[:, 0], patches[:, 2]], 1).reshape(4 * n, 1, WS, WS)
    assert len(layers) == L1
    for i, (w, bias) in enumerate(layers):
        h = F.conv2d(h, w, bias)
        if preacts is not None:
            preacts.append(h)
        if i < L1 - 1:
            h = F.relu(h)
    assert h.shape[2:] == (1, 1)
    return h


def loss_of(layers, patches, margin, pow_):
    """Margin2(StereoJoin1(Normalize2(net(batch)))), the mean over the pairs."""
    return tail_parts(features_of(layers, patches), margin, pow_)[2].mean()


def hinge_and_fragility(layers, patches, margin, eps=3e-6):
    """Float64 forward pass of every pair: the hinge argument f = neg - pos + margin, and whether the pair is fragile: some
    pre-activation of layers 1-4, or f itself, lies within eps of 0, where fp32 rounding can flip a ReLU (or hinge) mask.
    Uses the oracle only (train_oracle.hinge_and_fragility's rule and eps)."""
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


def robust_patches(layers, candidates, n, margin):
    """The first n of the candidate pairs that the float64 oracle alone calls non-fragile (asserts that n survive)."""
    _, frag = hinge_and_fragility(layers, candidates, margin)
    keep = np.nonzero(~frag)[0]
    assert keep.size >= n, "only %d of %d candidate pairs are non-fragile, %d needed" % (keep.size, candidates.shape[0], n)
    return candidates[keep[:n]]


def sgd_steps(params, patches_list, lr, mom, margin, pow_, fp32_state=False, moms=None):
    """params: [(w, b)] numpy; one step per batch: float64 gradients, v = mom * v - lr * g, w += v.  Returns the flat
    parameters, momenta and the losses.  fp32_state: parameters and momenta are rounded to float32 after every update (the
    reference's and the product's state).  moms: flat initial momenta (default 0)."""
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
        loss = loss_of([(ps[2 * i], ps[2 * i + 1]) for i in range(L1)], x, margin, pow_)
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
    """Flat w1 b1 .. w5 b5 vectors: each of the 10 tensors of `got` within tol of that tensor's largest magnitude in `want`,
    so that no tensor's gradient is partly missing; a tensor that is exactly 0 in `want` has to be exactly 0."""
    o = 0
    for s in SHAPES:
        for name, n in (("w", int(np.prod(s))), ("b", FM)):
            g, x = got[o:o + n], want[o:o + n]
            top = np.abs(x).max()
            if top == 0:
                assert np.abs(g).max() == 0, "%s %s%s: float64 says exactly 0" % (what, name, s)
            else:
                err = np.abs(g - x).max() / top
                print("%s %s%s: max error %.2e of its largest magnitude %.2e" % (what, name, s, err, top))
                assert err <= tol, "%s %s%s" % (what, name, s)
            o += n
    assert o == got.size == want.size == NPARAMS


# ---- a synthetic data.mb.* directory (preprocess_mb.py's format) -------------------------------------------------------------
# (H, W, lights >= 2, exposures, test views) of six scenes: all sizes differ; image 5 has the four test views of the 2014
# scenes, image 1 the two of MiddEval3, the others the 0-element light-1 file of the older sets
SCENES = ((60, 90, 1, 1, 2), (66, 130, 2, 2, 0), (72, 101, 3, 3, 0), (90, 95, 1, 1, 0), (81, 118, 1, 3, 4), (75, 124, 3, 2, 0))
SCENE_TE = (1, 5)
NDISP = 24


def write_synthetic_mb(d, scenes=SCENES, te=SCENE_TE, seed=0, noise=1.5):
    """Textured scenes with piecewise-constant disparity (three bands of rows at different depths): the right view is the
    texture, the left view the texture shifted by d(y, x); dispnoc is d where the match lies inside the image, else 0.
    Exposures differ by a gain, lights by a smooth shading term; every right view carries independent noise of `noise`
    times the texture's std.  x_<n>_1.bin holds the test views (left, then right views), x_<n>_<light>.bin for light >= 2
    is (n_exp, 2, 1, H, W).  nnz_tr / nnz_te list every known pixel of the training / test images.  Returns
    {image number: {light: array}} of what was written."""
    from mc_cnn_amd import binio
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    k = np.ones(3) / 3
    gains = (1.0, 0.8, 1.25, 0.9)
    written, disps = {}, {}
    for n, (H, W, n_light, n_exp, n_test) in enumerate(scenes, 1):
        r = rng.standard_normal((H, W + 40))
        r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, r)
        r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 0, r)
        r = (r - r.mean()) / r.std()
        bands = rng.integers(4, NDISP - 4, 3)
        d_map = np.repeat(bands, -(-H // 3))[:H][:, None] * np.ones((1, W), np.int64)
        right = r[:, 40:]
        left = np.take_along_axis(r, 40 + np.arange(W)[None, :] - d_map, 1)
        disps[n] = np.where(np.arange(W)[None, :] - d_map >= 0, d_map, 0).astype(np.float32)
        ys, xs = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
        shade = lambda l: 0.3 * np.sin(1.3 * l + 2.0 * xs) * np.cos(0.7 * l - 1.5 * ys)
        view = lambda base, l, e: (base * gains[e % 4] + shade(l)).astype(np.float32)
        noisy = lambda a: a + noise * rng.standard_normal(a.shape)
        written[n] = {}
        if n_test:
            tv = [view(left, 1, 0)] + [view(noisy(right), 1 + (j == 3), int(j == 2)) for j in range(1, n_test)]   # same, exposure, light
            written[n][1] = np.stack(tv)[:, None].astype(np.float32)
        else:
            written[n][1] = np.zeros((0,), np.float32)
        for l in range(2, 2 + n_light):
            written[n][l] = np.stack([np.stack([view(left, l, e), view(noisy(right), l, e)])[:, None] for e in range(n_exp)]).astype(np.float32)
        for l, a in written[n].items():
            binio.tofile(os.path.join(d, "x_%d_%d.bin" % (n, l)), a)
        binio.tofile(os.path.join(d, "dispnoc%d.bin" % n), disps[n].reshape(1, 1, H, W))

    def nnz_of(ids):
        rows = []
        for i in ids:
            ys, xs = np.nonzero(disps[i] > 0.5)
            rows.append(np.stack([np.full(ys.size, i), ys, xs, disps[i][ys, xs]], 1))
        return np.concatenate(rows).astype(np.float32)
    tr = [n for n in range(1, len(scenes) + 1) if n not in te]
    binio.tofile(os.path.join(d, "meta.bin"), np.array([[s[0], s[1], NDISP] for s in scenes], np.int32))
    binio.tofile(os.path.join(d, "te.bin"), np.array(te, np.int32))
    binio.tofile(os.path.join(d, "nnz_tr.bin"), nnz_of(tr))
    binio.tofile(os.path.join(d, "nnz_te.bin"), nnz_of(te))
    return written
