"""Test oracle of the fast net's training path at any depth (never imported by the product): a float64 numpy restatement of
make_patch (main.lua:603-619) with OpenCV 2.4's cvWarpAffine(CV_INTER_CUBIC + CV_WARP_FILL_OUTLIERS) rules, the sampling of a
pair from a KITTI store (x0, x1) and from a ragged plane store, and float64 torch autograd on the CPU of the training step
(main.lua:726-746, 853-874 with -l1 l1 -fm 64): l1 valid 3x3 convolutions of 64 maps on patches of side 2 l1 + 1.  The depth
is a function's first argument, or that of the `layers` it is given.  train_oracle.py and train_mb_oracle.py bind it at KITTI's
l1 4 and Middlebury's l1 5."""
import math

import numpy as np

FM = 64


def ws_of(l1):
    return 2 * l1 + 1


def nparams_of(l1):
    return FM * 9 + FM + (l1 - 1) * (FM * FM * 9 + FM)


def shapes_of(l1):
    return [(FM, 1 if i == 0 else FM, 3, 3) for i in range(l1)]


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def mul32(a, b):
    """main.lua:603-605."""
    return [a[0] * b[0] + a[1] * b[3], a[0] * b[1] + a[1] * b[4], a[0] * b[2] + a[1] * b[5] + a[2],
            a[3] * b[0] + a[4] * b[3], a[3] * b[1] + a[4] * b[4], a[3] * b[2] + a[4] * b[5] + a[5]]


def make_patch_matrix(ws, dim3, dim4, scale, phi, trans, hshear):
    """The 2x3 matrix make_patch hands to cv.warp_affine, as float32 (torch.FloatTensor(m)), with the ws-pixel window's
    centre shift."""
    m = [1, 0, -dim4, 0, 1, -dim3]
    m = mul32([1, 0, trans[0], 0, 1, trans[1]], m)
    m = mul32([scale[0], 0, 0, 0, scale[1], 0], m)
    c, s = math.cos(phi), math.sin(phi)
    m = mul32([c, s, 0, -s, c, 0], m)
    m = mul32([1, hshear, 0, 0, 1, 0], m)
    m = mul32([1, 0, (ws - 1) / 2, 0, 1, (ws - 1) / 2], m)
    return np.array(m, np.float32)


def cubic(x):
    """interpolateCubic, A = -0.75, float32."""
    x = np.float32(x)
    A = np.float32(-0.75)
    one = np.float32(1)
    c0 = ((A * (x + one) - 5 * A) * (x + one) + 8 * A) * (x + one) - 4 * A
    c1 = ((A + 2) * x - (A + 3)) * x * x + one
    c2 = ((A + 2) * (one - x) - (A + 3)) * (one - x) * (one - x) + one
    c3 = one - c0 - c1 - c2
    return np.array([c0, c1, c2, c3], np.float32)


def warp_affine(src, mat, size):
    """cvWarpAffine(src, dst, mat, CV_INTER_CUBIC + CV_WARP_FILL_OUTLIERS) into a size x size float32 dst: the matrix is
    inverted in doubles, coordinates are fixed point with 1/32 pixel (AB_BITS 10, INTER_BITS 5), taps outside src read 0."""
    src = np.asarray(src, np.float32)
    H, W = src.shape
    M = [float(v) for v in np.asarray(mat, np.float32).ravel()[:6]]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0], M[1], M[3], M[4] = A11, M[1] * -D, M[3] * -D, A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    dst = np.zeros((size, size), np.float32)
    for dy in range(size):
        X0 = int(np.rint((M[1] * dy + M[2]) * 1024.0)) + 16
        Y0 = int(np.rint((M[4] * dy + M[5]) * 1024.0)) + 16
        for dx in range(size):
            X = (X0 + int(np.rint(M[0] * dx * 1024.0))) >> 5
            Y = (Y0 + int(np.rint(M[3] * dx * 1024.0))) >> 5
            sx, sy = (X >> 5) - 1, (Y >> 5) - 1
            wx, wy = cubic(np.float32(X & 31) * np.float32(1 / 32)), cubic(np.float32(Y & 31) * np.float32(1 / 32))
            acc = np.float32(0)
            if 0 <= sx < W - 3 and 0 <= sy < H - 3:
                for i in range(4):
                    S = src[sy + i, sx:sx + 4]
                    r = np.float32(0)
                    for j in range(4):
                        r = np.float32(r + S[j] * np.float32(wy[i] * wx[j])) if j else np.float32(S[0] * np.float32(wy[i] * wx[0]))
                    acc = r if i == 0 else np.float32(acc + r)
            elif sx >= W or sx + 4 <= 0 or sy >= H or sy + 4 <= 0:
                acc = np.float32(0)
            else:
                for i in range(4):
                    yi = sy + i
                    if not 0 <= yi < H:
                        continue
                    for j in range(4):
                        xj = sx + j
                        if 0 <= xj < W:
                            acc = np.float32(acc + src[yi, xj] * np.float32(wy[i] * wx[j]))
            dst[dy, dx] = acc
    return dst


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
    """The same from a ragged store: planes is a list of 2-D arrays, src the pair's two plane ids (left; both right patches),
    nnz_row (img, row, col, d) or None for a row outside the nnz.  A plane id outside the list and a missing row read 0."""
    pick = lambda k: planes[k] if nnz_row is not None and 0 <= k < len(planes) else None
    return _pair(ws_of(l1), pick(src[0]), pick(src[1]), nnz_row if nnz_row is not None else (0, 0, 0, 0), prm)


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


def tail_parts(h, margin, pow_):
    """Normalize2 -> StereoJoin1 -> Margin2 on features h (4n, C, 1, 1) [L, P, L, N per pair]: the normalised features,
    the scores (2n,) [pos, neg per pair] and each pair's loss."""
    import torch
    n = h.shape[0] // 4
    hn = h / torch.sqrt((h * h).sum(1, keepdim=True) + 1e-5)
    s = (hn[0::2] * hn[1::2]).sum(1).reshape(2 * n)
    f = s[1::2] - s[0::2] + margin
    d = torch.clamp(f, min=0)
    return hn, s, (d if pow_ == 1 else 0.5 * d * d)


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


def as_f64(layers):
    import torch
    return [(torch.tensor(np.asarray(w, np.float64)), torch.tensor(np.asarray(b, np.float64))) for w, b in layers]


def hinge_and_fragility(layers, patches, margin, eps=3e-6):
    """Float64 forward pass of every pair of patches (n, 3, ws, ws): the hinge argument f = neg - pos + margin of each pair,
    and whether the pair is fragile: some pre-activation before a ReLU, or f itself, lies within eps of 0, where fp32
    rounding can put it on the other side and flip a ReLU (or hinge) mask.  Uses the oracle only."""
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


def momentum_sgd(layers, loss_fn, patches_list, lr, mom, fp32_state=False, moms=None):
    """Momentum SGD (main.lua:870-874) on loss_fn([(w, b)] float64 tensors, patches) from [(w, b)] numpy: one step per batch
    with float64 gradients, v = mom * v - lr * g, w += v.  Returns the flat parameters, momenta and the losses.  fp32_state:
    parameters and momenta are rounded to float32 after every update (the reference's and the product's state).  moms: flat
    initial momenta (default 0).  The accurate net's oracle (train_slow_oracle.py) steps with it too."""
    import torch
    ps = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for wb in layers for a in wb]
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
        loss = loss_fn([(ps[2 * i], ps[2 * i + 1]) for i in range(len(ps) // 2)], x)
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


def sgd_steps(params, patches_list, lr, mom, margin, pow_, fp32_state=False, moms=None):
    """momentum_sgd on the fast net's loss at the depth of `params` ([(w, b)] numpy)."""
    return momentum_sgd(params, lambda layers, x: loss_of(layers, x, margin, pow_), patches_list, lr, mom, fp32_state, moms)


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
