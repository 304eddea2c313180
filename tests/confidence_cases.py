"""The cases of tests/test_confidence_host.py and tests/test_gpu_confidence.py, and what mc_cost_margins, confidence.sparsification and
confidence.keep_mask are, stated in numpy from their definitions (include/mc_adcensus.h, mc-cnn_amd/confidence.py) -- plain loops over
pixels and disparities and np.argsort(kind="stable"), nothing derived from the code under test.  Everything is made once per argument
tuple and handed out read-only."""
import functools

import numpy as np

INF = np.float32(np.inf)
NAN = np.float32(np.nan)

# (D, H, W) -> what it exercises
SHAPES = [
    (7, 3, 5),     # H*W = 15: the one-pixel kernel
    (9, 4, 6),     # H*W = 24: the four-pixel kernel
    (5, 33, 37),   # one-pixel kernel: five blocks of 256, the last partial
    (5, 32, 36),   # four-pixel kernel: two blocks of 256 x 4, the last partial
    (1, 4, 4),     # D = 1
    (2, 4, 4),     # D = 2
]


def margins_oracle(vol):
    """(d1, c1, c2, c2l) of a (D,H,W) float32 volume, (H,W) float32 each: a double loop over pixels and d with the plain float32
    comparisons of the definition (a NaN never wins a `<` and never blocks a negated comparison)."""
    vol = np.asarray(vol, np.float32)
    D, H, W = vol.shape
    d1, c1, c2, c2l = (np.zeros((H, W), np.float32) for _ in range(4))
    with np.errstate(invalid="ignore"):
        for y in range(H):
            for x in range(W):
                c = vol[:, y, x]
                best, arg = INF, 0
                for d in range(D):                       # the first strict minimum from +INF
                    if c[d] < best:
                        best, arg = c[d], d
                second = INF
                for d in range(D):                       # the smallest value below +INF at another d
                    if d != arg and c[d] < INF and c[d] < second:
                        second = c[d]
                second_local = INF
                for d in range(D):                       # ... among the local minima
                    before = c[d - 1] if d > 0 else NAN
                    after = c[d + 1] if d < D - 1 else NAN
                    local_min = c[d] < INF and not (before <= c[d]) and not (after < c[d])
                    if d != arg and local_min and c[d] < second_local:
                        second_local = c[d]
                d1[y, x], c1[y, x], c2[y, x], c2l[y, x] = arg, best, second, second_local
    return d1, c1, c2, c2l


# one curve per planted property (those that D is too short for are left out); values around the random costs' range
def _curves(D, rng):
    def base():
        return rng.uniform(-1.0, 1.0, D).astype(np.float32)

    out = []
    out.append(np.full(D, NAN, np.float32))                                   # an all-NaN curve
    c = np.full(D, NAN, np.float32); c[D // 2] = -0.25; out.append(c)         # a single finite value
    c = np.full(D, INF, np.float32); out.append(c)                            # nothing below +INF
    c = np.full(D, INF, np.float32); c[D - 1] = 0.5; out.append(c)            # +INF entries and one value, at the end
    if D >= 2:
        c = base(); c[0] = c[D - 1] = -2.0; out.append(c)                     # a tie of the minimum at two d
        c = np.arange(D, dtype=np.float32) * 0.125 - 0.5; out.append(c)       # strictly increasing: one local minimum, c2 finite
        out.append(c[::-1].copy())                                            # strictly decreasing
        c = base(); c[D // 2] = INF; out.append(c)                            # a +INF entry among finite ones
        c = -base() - 3.0; out.append(c)                                      # negative costs throughout
    if D >= 3:
        c = base(); c[1] = -2.0; c[0] = NAN; out.append(c)                    # a NaN in front of the minimum
        c = base(); c[D - 2] = -2.0; c[D - 1] = NAN; out.append(c)            # a NaN behind the minimum
    if D >= 5:
        c = np.array([1.0, 0.5, 0.5, 0.5, 1.0] + [2.0] * (D - 5), np.float32); out.append(c)      # a plateau: counts once
        c = np.array([1.0, 0.5, 0.5, 0.25, 1.0] + [2.0] * (D - 5), np.float32); out.append(c)     # a plateau followed by a descent
        c = np.array([0.0, -1.0, 0.5, -1.0, 0.75] + [2.0] * (D - 5), np.float32); out.append(c)   # two equal local minima
        c = np.array([0.5, -1.0, -0.5, 0.0, 0.25] + [2.0] * (D - 5), np.float32); out.append(c)   # runner-up that is no local minimum
    if D >= 7:
        c = np.array([3.0, 1.0, 2.0, NAN, 0.5, NAN, 0.75], np.float32)
        out.append(np.concatenate([c, np.full(D - 7, INF, np.float32)]))                          # local minima fenced by NaN, an INF tail
    return out


@functools.lru_cache(maxsize=None)
def volume(D, H, W, seed=0):
    """A (D,H,W) float32 volume of random finite costs in (-1, 1) with the curves of _curves planted at the first pixels and, where
    the image has room, at the last ones (so that every lane of a four-pixel group and the last partial block hold some), read-only."""
    rng = np.random.default_rng(1000 * seed + 100 * D + 10 * H + W)
    vol = rng.uniform(-1.0, 1.0, (D, H, W)).astype(np.float32)
    curves = _curves(D, rng)
    flat = vol.reshape(D, H * W)
    HW, n = H * W, len(curves)
    for k in range(min(n, HW)):                 # the first pixels: every lane of a four-pixel group, the first block
        flat[:, k] = curves[(k + seed) % n]     # (an image with fewer pixels than curves holds them all over two seeds)
    if HW >= 2 * n:
        for k in range(n):                      # ... and the last ones: the last, partial block
            flat[:, HW - 1 - k] = curves[(k + seed + 1) % n]
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def wanted(D, H, W, seed=0):
    out = margins_oracle(volume(D, H, W, seed))
    for a in out:
        a.setflags(write=False)
    return out


# ---- sparsification and keep_mask ---------------------------------------------------------------------------------------------------

def descending(conf):
    """flat indices by conf descending, ties by index ascending, a NaN ranking with -INF: np.argsort(kind="stable") of the negated key"""
    key = np.where(np.isnan(conf), -INF, conf).astype(np.float32)
    return np.argsort(-key, kind="stable")


def sparsification_oracle(conf, pred, actual, err_at, n=100):
    """(bad, bad_oracle, m), int64 arrays of n values, from the definition"""
    conf, pred, actual = (np.asarray(a, np.float32).reshape(-1) for a in (conf, pred, actual))
    at = np.flatnonzero(actual != 0)
    N = at.size
    with np.errstate(invalid="ignore"):
        err = np.abs(actual[at] - pred[at])
        wrong = (err > np.float32(err_at)).astype(np.int64)
    m = np.array([-((-k * N) // n) for k in range(1, n + 1)], np.int64)
    by_conf = wrong[descending(conf[at])]
    by_err = wrong[np.argsort(err, kind="stable")]
    bad = np.array([by_conf[:mk].sum() for mk in m], np.int64)
    bad_oracle = np.array([by_err[:mk].sum() for mk in m], np.int64)
    return bad, bad_oracle, m


def keep_mask_oracle(conf, fraction):
    conf = np.asarray(conf, np.float32)
    count = int(np.ceil(fraction * conf.size))
    mask = np.zeros(conf.size, bool)
    mask[descending(conf.reshape(-1))[:count]] = True
    return mask.reshape(conf.shape)


@functools.lru_cache(maxsize=None)
def ranking_case(name):
    """(conf, pred, actual, err_at, n) of a named case, (H,W) float32 maps, read-only.
      ties      confidences from four values only, N no multiple of n
      special   NaN, +INF and -INF confidences among heavy ties
      few       N < n: fewer ground-truth pixels than points on the curve
      exact     N a multiple of n, distinct confidences"""
    rng = np.random.default_rng(sum(map(ord, name)))
    H, W = (13, 17) if name != "exact" else (10, 20)
    actual = rng.uniform(1.0, 60.0, (H, W)).astype(np.float32)
    pred = (actual + rng.normal(0.0, 3.0, (H, W))).astype(np.float32)
    n, err_at = 100, 3.0
    if name == "ties":
        actual[rng.uniform(size=(H, W)) < 0.3] = 0
        conf = rng.integers(0, 4, (H, W)).astype(np.float32)
    elif name == "special":
        actual[rng.uniform(size=(H, W)) < 0.2] = 0
        conf = rng.integers(0, 3, (H, W)).astype(np.float32)
        kind = rng.integers(0, 8, (H, W))
        conf[kind == 0] = NAN
        conf[kind == 1] = INF
        conf[kind == 2] = -INF
    elif name == "few":
        keep = np.zeros(H * W, bool)
        keep[rng.permutation(H * W)[:37]] = True
        actual[~keep.reshape(H, W)] = 0
        conf = rng.integers(0, 5, (H, W)).astype(np.float32)
    else:
        conf = rng.permutation(H * W).reshape(H, W).astype(np.float32)
    N = int((actual != 0).sum())
    assert {"ties": N % n != 0, "special": N % n != 0, "few": N < n, "exact": N % n == 0}[name], (name, N)
    for a in (conf, pred, actual):
        a.setflags(write=False)
    return conf, pred, actual, err_at, n


RANKING_CASES = ("ties", "special", "few", "exact")
