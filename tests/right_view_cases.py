"""The cases of tests/test_gpu_right_view.py and the oracle's statement of what mc_predict_views' two maps are, made on the CPU.

The definition.  Let M mirror an array along x, M(a)[..., y, x] = a[..., y, W-1-x].  Mirroring the scene turns the right image into a left
one, so the right view's result is what the existing post-processing gives on the mirrored maps, mirrored back (oracle_right below):
classes from (M(dispR0), M(dispL0)), the two interpolations where the parameter set has an LR check, the sub-pixel stage on M(volR),
median, blur; stages dropped by sm_skip / sm_terminate exactly as on the left (stages()).  Every stage is the oracle's own operator.

The pairs are those of tests/predict_ex_cases.py, by import: H = 12, W = 40 with D = 8 and D = 7 (ds = D and ds = D + 1, rows shorter than
a wave, H * W no multiple of 256), routes fast / slow / mb.  One more case has W = 37 (route fast, D = 8), so that no row is a multiple of
4 pixels: made by the same recipe at that width (pair_w / features_w).

SEED was chosen here, on the CPU oracle alone, as the first seed at which the oracle's RIGHT-view class map of every case (route x D, and
the W = 37 case) holds all three classes (python tests/right_view_cases.py prints the search); the GPU tests assert that on the oracle's
map before they compare anything."""
import numpy as np

import predict_ex_cases as cases

H, W, C = cases.H, cases.W, cases.C
DS = cases.DS
W_ODD = 37
SEED = 0
ROUTES = ("fast", "slow", "mb")
CASES = [(route, D, W) for route in ROUTES for D in DS] + [("fast", 8, W_ODD)]   # (route, D, width)

TERMINATE = {"": 0, "cnn": 1, "cbca1": 2, "sgm": 3, "cbca2": 4, "occlusion": 5, "mismatch": 6, "subpixel_enchancement": 7, "median": 8,
             "bilateral": 9}
SKIP = {"": 0, "cbca": 1, "sgm": 2, "occlusion": 3, "subpixel_enchancement": 4, "median": 5, "bilateral": 6}


def M(a):
    return np.ascontiguousarray(np.asarray(a)[..., ::-1])


def shifted_w(left, rng, width, sigma=0.01):
    """predict_ex_cases.shifted at any width"""
    right = rng.standard_normal(left.shape).astype(np.float32)
    for rows, s in ((slice(0, H // 2), cases.SHIFTS[0]), (slice(H // 2, H), cases.SHIFTS[1])):
        right[..., rows, :width - s] = left[..., rows, s:]
    return (right + rng.normal(0, sigma, left.shape)).astype(np.float32)


def pair_w(seed, width):
    if width == W:
        return cases.pair(seed)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((H, width)).astype(np.float32)
    return x0, shifted_w(x0, rng, width)


def features_w(seed, width):
    if width == W:
        return cases.features(seed)
    rng = np.random.default_rng(seed + 1000)
    fl = rng.standard_normal((C, H, width)).astype(np.float32)
    f = np.stack([fl, shifted_w(fl, rng, width)])
    return (f / np.sqrt((f * f).sum(1, keepdims=True))).astype(np.float32)


def params(presets, route, over=None):
    prm = dict(presets["kitti_fast"]) if route == "fast" else cases.slow_params(presets) if route == "slow" else dict(presets["mb_slow"])
    return dict(prm, **(over or {}))


def oracle_maps(oracle, presets, route, D, width=W, seed=SEED, over=None):
    """(o, prm): the oracle's stereo_predict dict for a case, and the parameter set it ran with"""
    prm = params(presets, route, over)
    x0, x1 = pair_w(seed, width)
    if route == "fast":
        f = features_w(seed, width)
        return oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1]), prm
    return oracle.stereo_predict(prm, x0, x1, D, rawL=oracle.ad(x0, x1, D, -1), rawR=oracle.ad(x1, x0, D, 1)), prm


def stages(prm):
    """which stages of the tail run, main.lua:1054-1079: (occlusion, mismatch, subpixel, median, bilateral)"""
    term = prm.get("sm_terminate", 0)
    skip = prm.get("sm_skip", 0)
    term = TERMINATE[term] if isinstance(term, str) else term
    skip = SKIP[skip] if isinstance(skip, str) else skip
    active = term not in (1, 2, 3, 4)
    runs = []
    lr = bool(prm["lr_check"])
    for stage_skip, stage_term, exists in ((3, 5, lr), (3, 6, lr), (4, 7, True), (5, 8, True), (6, 9, True)):
        runs.append(exists and active and skip != stage_skip)
        if exists:
            active = active and term != stage_term
    return tuple(runs)


def oracle_right(oracle, o, prm, D):
    """(dispR_out, outlierR_out) of mc_predict_views from the oracle's dict o: the definition, composed from oracle.* and numpy"""
    occlusion, mismatch, subpixel, median, bilateral = stages(prm)
    oR = oracle.outlier_detection(M(o["dispR0"]), M(o["dispL0"]), D)
    t = M(o["dispR0"])
    if occlusion:
        t = oracle.interpolate_occlusion(t, oR)
    if mismatch:
        t = oracle.interpolate_mismatch(t, oR)
    if subpixel:
        t = oracle.subpixel_enchancement(t, M(o["volR"]))
    if median:
        t = oracle.median2d(t, prm["median_k"])
    if bilateral:
        t = oracle.mean2d(t, oracle.gaussian(prm["blur_sigma"]), prm["blur_t"])
    return M(t), M(oR)


def has_all_classes(outlier):
    return cases.has_all_classes(outlier)


def first_seed(oracle, presets, limit=64):
    for seed in range(limit):
        ok = True
        for route, D, width in CASES:
            o, prm = oracle_maps(oracle, presets, route, D, width, seed)
            ok = ok and has_all_classes(oracle_right(oracle, o, prm, D)[1])
        print("seed %d: %s" % (seed, "every case holds all three classes" if ok else "no"))
        if ok:
            return seed
    raise SystemExit("no seed below %d" % limit)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mc_cnn_amd
    from oracle import cpu_oracle
    cpu_oracle.build()
    assert first_seed(cpu_oracle, mc_cnn_amd.PRESETS) == SEED
