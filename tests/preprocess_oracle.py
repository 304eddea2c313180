"""Numpy restatement of the GPU stages of preprocess_kitti.lua:97-113 (test infrastructure), and writers of synthetic
KITTI archive trees (`data.kitti/unzip`, `data.kitti2015/unzip`) at the real image sizes.

`filter_gt` is the literal per-pixel rule of adcensus.cu:1723-1800 in float32, remove_occluded evaluated against the row as
remove_nonvisible left it; `make_dataset2` is adcensus.cu:1900-1929; `stages` has the signature of
`preprocess_kitti.gpu_stages`, so that a CPU test can run the whole preprocessing without a GPU."""
import os

import numpy as np

SIZES = [(375, 1242), (370, 1226), (376, 1241)]   # KITTI's image sizes


def filter_gt(disp, x0):
    """remove_nonvisible, remove_occluded, remove_white on maps (..., H, W) with their images x0 (..., H, W)."""
    d = np.array(disp, np.float32)
    W = d.shape[-1]
    d = np.where(d >= np.arange(W, dtype=np.float32), np.float32(0), d)           # y[id] >= x
    occ = np.zeros(d.shape, bool)
    for i in range(1, W):                                                           # i - y[id + i] < -y[id]
        occ[..., :W - i] |= (np.float32(i) - d[..., i:]) < -d[..., :W - i]
    d = np.where(occ, np.float32(0), d)
    return np.where(np.asarray(x0, np.float32) == 255, np.float32(0), d).astype(np.float32)


def make_dataset2(disp, ids):
    """Rows (id, row, col, d) of every d > 0.5 of the maps disp (n, H, W), map order then row-major."""
    rows = [np.zeros((0, 4), np.float32)]
    for k in range(disp.shape[0]):
        ys, xs = np.nonzero(disp[k] > 0.5)
        rows.append(np.stack([np.full(ys.size, ids[k]), ys, xs, disp[k][ys, xs]], 1).astype(np.float32))
    return np.concatenate(rows, 0)


def stages(dispnoc, x0, te):
    """preprocess_kitti.gpu_stages on the host."""
    n = dispnoc.shape[0]
    disp = filter_gt(dispnoc[:, 0], x0[:n, 0])
    ids = np.arange(1, n + 1)
    is_te = np.isin(ids, np.asarray(te))
    return make_dataset2(disp[~is_te], ids[~is_te]), make_dataset2(disp[is_te], ids[is_te]), {}


def png16_map(rng, h, w, d_max=100.0):
    """A PNG16-quantised ground-truth map with occlusions: per row, segments of random constant disparity (multiples of
    1/256 below d_max) with per-pixel jitter and holes (0)."""
    d = np.zeros((h, w), np.float32)
    for y in range(h):
        x = 0
        while x < w:
            n = int(rng.integers(3, 60))
            d[y, x:x + n] = rng.uniform(0, d_max)
            x += n
    d += rng.uniform(-0.5, 0.5, (h, w)).astype(np.float32)
    d[rng.uniform(0, 1, (h, w)) < 0.2] = 0
    return np.clip(np.round(d * 256), 0, 65535).astype(np.uint16)


def textured_pair(rng, h, w, noise, block=None):
    """Textured 8-bit pair with known disparities: x1 is x0 shifted by d(y, x), constant over blocks of block = (rows,
    columns) pixels (three bands of rows if None), plus independent noise of `noise` times the texture's std; ground truth
    is d where the match lies inside the image."""
    k = np.ones(3) / 3
    r = rng.standard_normal((h, w + 40))
    r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 1, r)
    r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), 0, r)
    r = (r - r.mean()) / r.std()
    bh, bw = block or (-(-h // 3), w)
    d_map = rng.integers(6, 30, (-(-h // bh), -(-w // bw))).repeat(bh, 0).repeat(bw, 1)[:h, :w]
    left = np.take_along_axis(r, 40 + np.arange(w)[None, :] - d_map, 1)
    right = r[:, 40:] + noise * rng.standard_normal((h, w))
    to8 = lambda a: np.clip(np.round(128 + 25 * a), 0, 254).astype(np.uint8)
    gt = np.where(np.arange(w)[None, :] - d_map >= 0, d_map * 256, 0).astype(np.uint16)
    return to8(left), to8(right), gt


def write_tree(root, year, n_tr, n_te, seed=0, textured=False, noise=2.0, block=None):
    """Write `<set>/unzip/{training,testing}/...` for preprocess_kitti.SETS[year]: n_tr training and n_te test pairs
    (8-bit grey for 2012, RGB for 2015) at the sizes of SIZES in turn, and PNG16 ground truth for the training pairs.
    Random images (0..255, 255 included) and png16_map ground truth, or textured_pair scenes."""
    from PIL import Image

    from mc_cnn_amd import preprocess_kitti as pk
    s = pk.SETS[year]
    rng = np.random.default_rng(seed)
    base = os.path.join(root, s["path"], "unzip")
    for d, n in (("training", n_tr), ("testing", n_te)):
        for sub in ("image_0", "image_1") + (("disp_noc",) if d == "training" else ()):
            os.makedirs(os.path.join(base, d, s[sub]), exist_ok=True)
        for cnt in range(n):
            h, w = SIZES[(cnt + (d == "testing")) % len(SIZES)]
            if textured:
                left, right, gt = textured_pair(rng, h, w, noise, block)
            else:
                left, right = (rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(2))
                gt = png16_map(rng, h, w)
            name = "%06d_10.png" % cnt
            for sub, img in (("image_0", left), ("image_1", right)):
                if s["nchannel"] == 3:
                    img = np.stack([img, np.roll(img, 1, 1), img[::-1]] if not textured else [img] * 3, -1)
                Image.fromarray(img).save(os.path.join(base, d, s[sub], name))
            if d == "training":
                Image.fromarray(gt).save(os.path.join(base, d, s["disp_noc"], name))
    return os.path.join(root, s["path"])
