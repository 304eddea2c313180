"""What the GPU training tests share besides the oracles (a plain module, imported as they are): moving arrays to the device,
bitwise and relative comparison, a small KITTI store, and synthetic data.kitti / data.mb.* directories."""
import os

import numpy as np


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Two float32 tensors of one shape and the same bit patterns (tests/util.py's same_bits, on numpy arrays, calls any two
    NaNs equal; this one does not)."""
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rel(g, w):
    return float(np.linalg.norm(g - w) / np.linalg.norm(w))


def small_images(seed, n_img=3, H=40, W=90, d=5, noise=0.1):
    """A KITTI store whose nnz lists every pixel, corners included, at disparity d: the right view is the left one shifted by d
    plus noise (1.5 is strong enough to leave most hinges of a random net active)."""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((n_img, H, W)).astype(np.float32)
    x1 = np.roll(x0, -d, axis=2) + noise * rng.standard_normal((n_img, H, W)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    nnz = np.stack([np.repeat(np.arange(1, n_img + 1), H * W), np.tile(ys.ravel(), n_img), np.tile(xs.ravel(), n_img),
                    np.full(n_img * H * W, d)], 1).astype(np.float32)
    return x0, x1, nnz


# ---- a synthetic data.kitti directory --------------------------------------------------------------------------------------------
def write_synthetic_kitti(d, n_img=6, H=48, W=160, seed=0, noise=2.0):
    """Textured scenes with known piecewise-constant disparity: x1 is x0 shifted by d(y, x) (bands of rows at
    different depths); dispnoc is d where the match lies inside the image, else 0.  nnz_tr / nnz_te list every known
    pixel of the training / test images (make_dataset2, adcensus.cu:1900-1929); the last two images are the test set.  x1
    carries independent noise of `noise` times the texture's std, so that matching is not trivial for an untrained net.
    Returns x0, x1."""
    from mc_cnn_amd import binio
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    x0 = np.zeros((n_img, 1, H, W), np.float32)
    x1 = np.zeros_like(x0)
    disp = np.zeros_like(x0)
    k = np.ones(3) / 3
    for i in range(n_img):
        r = rng.standard_normal((H, W + 40))
        r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, r)
        r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 0, r)
        r = (r - r.mean()) / r.std()
        bands = rng.integers(6, 30, 3)
        d_map = np.repeat(bands, -(-H // 3))[:H][:, None] * np.ones((1, W), np.int64)
        right = r[:, 40:]
        left = np.take_along_axis(r, 40 + np.arange(W)[None, :] - d_map, 1)
        x0[i, 0], x1[i, 0] = left, right + noise * rng.standard_normal(right.shape)
        disp[i, 0] = np.where(np.arange(W)[None, :] - d_map >= 0, d_map, 0)
    tr_ids, te_ids = np.arange(1, n_img - 1), np.array([n_img - 1, n_img])

    def nnz_of(ids):
        rows = []
        for i in ids:
            ys, xs = np.nonzero(disp[i - 1, 0] > 0.5)
            rows.append(np.stack([np.full(ys.size, i), ys, xs, disp[i - 1, 0, ys, xs]], 1))
        return np.concatenate(rows).astype(np.float32)
    for name, a in (("x0", x0), ("x1", x1), ("dispnoc", disp), ("metadata", np.array([[H, W, i] for i in range(n_img)], np.int32)),
                    ("tr", tr_ids.astype(np.int32)), ("te", te_ids.astype(np.int32)), ("nnz_tr", nnz_of(tr_ids)), ("nnz_te", nnz_of(te_ids))):
        binio.tofile(os.path.join(d, name + ".bin"), a)
    return x0, x1


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
