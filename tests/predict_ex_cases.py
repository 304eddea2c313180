"""The pairs of tests/test_gpu_predict_ex.py, made on the CPU: a seeded random texture whose right view is the left one shifted by 3 pixels
in the upper half of the rows and by 5 in the lower half, plus N(0, 0.01) noise; 16 channel-normalised random feature maps shifted
the same way.  H = 12, W = 40 with D = 8 and D = 7: the smallest shapes that cover ds = D and ds = D + 1 (the (H,W,ds) volumes pad D
to a multiple of 4), rows shorter than a wave, and H * W no multiple of 256.

SEED was chosen here, on the CPU oracle alone, as the first seed at which the class map of every case (route x D, and the Middlebury
set) holds all three classes; the GPU tests assert that on the oracle's map before they compare anything."""
import numpy as np

H, W, C = 12, 40, 16
DS = (8, 7)
SEED = 0
SHIFTS = (3, 5)   # upper rows, lower rows


def shifted(left, rng, sigma=0.01):
    """right[..., y, x] = left[..., y, x + s(y)] + noise; fresh texture where x + s(y) leaves the image"""
    right = rng.standard_normal(left.shape).astype(np.float32)
    for rows, s in ((slice(0, H // 2), SHIFTS[0]), (slice(H // 2, H), SHIFTS[1])):
        right[..., rows, :W - s] = left[..., rows, s:]
    return (right + rng.normal(0, sigma, left.shape)).astype(np.float32)


def pair(seed=SEED):
    """(x0, x1) (H,W) float32, zero mean and unit deviation like the images main.py uploads"""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((H, W)).astype(np.float32)
    x1 = shifted(x0, rng)
    return x0, x1


def features(seed=SEED):
    """(2,C,H,W): unit length over the channels at every pixel (Normalize2), the right maps shifted like the right image"""
    rng = np.random.default_rng(seed + 1000)
    fl = rng.standard_normal((C, H, W)).astype(np.float32)
    fr = shifted(fl, rng)
    f = np.stack([fl, fr])
    return (f / np.sqrt((f * f).sum(1, keepdims=True))).astype(np.float32)


def slow_params(presets):
    """the (D,H,W) route: kitti_slow with a second aggregation block, so that the sub-pixel stage reads a (D,H,W) volume"""
    return dict(presets["kitti_slow"], cbca_i2=2)


def oracle_maps(oracle, presets, route, D, seed=SEED):
    """what the CPU oracle computes for a case: its stereo_predict dict, with `outlier` computed from the two arg-min maps where the
    parameter set has no LR check (route "mb")"""
    x0, x1 = pair(seed)
    if route == "fast":
        f = features(seed)
        o = oracle.stereo_predict(dict(presets["kitti_fast"]), x0, x1, D, featL=f[0], featR=f[1])
    else:
        prm = slow_params(presets) if route == "slow" else dict(presets["mb_slow"])
        o = oracle.stereo_predict(prm, x0, x1, D, rawL=oracle.ad(x0, x1, D, -1), rawR=oracle.ad(x1, x0, D, 1))
    if route == "mb":
        o["outlier"] = oracle.outlier_detection(o["dispL0"], o["dispR0"], D)
    return o


def has_all_classes(outlier):
    return set(np.unique(outlier)) == {0.0, 1.0, 2.0}
