"""-m gpu: the post-processing tail of mc_predict against the CPU oracle, bit for bit: the mismatch ray walk on the bitmask that the
occlusion stage leaves (reachable through mc_predict only), the medians without a border path, the device-resident Gaussian table and
the single fix_border launch over both volumes."""
import numpy as np
import pytest

from util import diff_report, features, random_pair, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MASK_MAX_PIXELS = 524288   # MC_MIS_MASK_MAX_PIXELS: up to here the walk runs on the mask, beyond it on the marks themselves


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_same(got, want, name):
    assert same_bits(got, want), diff_report(got, want, name)


def fast(**over):
    import mc_cnn_amd
    return dict(mc_cnn_amd.PRESETS["kitti_fast"], **over)


def run_features(mc, oracle, prm, H, W, D, C, seed, name):
    x0, x1 = random_pair(H, W, seed=seed)
    f = features(C, H, W, seed=seed + 1)
    want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    got = mc.stereo_predict_fused(dev(np.stack([x0, x1]))[:, None], prm, D, feat=dev(f))
    torch.cuda.synchronize()
    assert_same(host(got["disp"]), want["disp"], name)
    return want


# ---- the ray walk on random features: mostly mismatches, long walks ----

@pytest.mark.parametrize("terminate", ["mismatch", ""])
@pytest.mark.parametrize("H,W,D", [(37, 150, 24), (9, 33, 8), (1, 70, 8)])   # W % 32 != 0: the mask's rows straddle words; 9 x 33 < one chunk
def test_ray_walk_on_random_features(mc, oracle, H, W, D, terminate):
    want = run_features(mc, oracle, fast(sm_terminate=terminate), H, W, D, 8, 100 + H, "disp %dx%dx%d %s" % (H, W, D, terminate))
    if H > 1:
        assert (want["outlier"] == 2).mean() > 0.25, "the case is meant to be rich in mismatches"


def test_ray_walk_with_a_part_chunk_after_a_whole_one(mc, oracle):
    """300 x 1000 pixels over one block per CU: every block's share is more than one chunk of 1024 pixels and no multiple of it"""
    H, W, D = 300, 1000, 8
    want = run_features(mc, oracle, fast(sm_terminate="mismatch"), H, W, D, 2, 7, "disp 300x1000")
    assert (want["outlier"] == 2).mean() > 0.25


@pytest.mark.parametrize("W", [MASK_MAX_PIXELS // 4, MASK_MAX_PIXELS // 4 + 1], ids=["at_the_cap", "one_past_the_cap"])
def test_ray_walk_at_the_mask_cap(mc, oracle, W):
    """4 x 131072 = 524288 pixels: the largest image that walks on the mask (64 KiB of LDS); one column more: the marks in global memory.
    blur_sigma = 1 keeps the oracle's last stage short."""
    want = run_features(mc, oracle, fast(blur_sigma=1.0), 4, W, 4, 2, 11, "disp 4x%d" % W)
    assert (want["outlier"] == 2).mean() > 0.1


# ---- the ray walk on prescribed arg-min maps (raw volumes with planted minima, -sm_skip sgm) ----
# Column 0 can never be a mismatch (outlier_detection: there d = 0 is the only candidate of the "some d matches" test, and it is the very
# test the pixel has just failed), so through mc_predict "all mismatches" means every column but the first, at least one ray of every pixel
# ends inside the image, and the corners' mismatches sit in column 1 and column W - 1.

def planted(d, D):
    H, W = d.shape
    vol = np.ones((D, H, W), np.float32)
    np.put_along_axis(vol, d[None].astype(np.int64), 0.0, axis=0)
    return vol


def maps_all_mismatch(H, W):
    # d1 = 2 everywhere: d0 = 0 and d0 >= 4 do not match it, d = 1 does for every x >= 1
    rng = np.random.default_rng(4)
    d0 = np.where(np.arange(W)[None, :] < 7, 0, rng.choice([0, 4, 5, 6, 7], (H, W))).astype(np.float32)
    return d0, np.full((H, W), 2, np.float32), lambda o: (o[:, 1:] == 2).all() and (o[:, 0] == 1).all()


def maps_no_mismatch(H, W):
    return np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), lambda o: (o == 0).all()


def maps_corners(H, W):
    d0, d1 = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for y in {0, H - 1}:
        d0[y, 1] = 1          # against d1[y, 0] = 3: no match; d = 0 matches d1[y, 1] = 0: a mismatch
        d1[y, 0] = 3
        d0[y, W - 1] = 3      # against d1[y, W - 4] = 0: no match; d = 0 matches: a mismatch
    want = np.zeros((H, W), np.float32)
    for y in {0, H - 1}:
        want[y, 0] = 1
        want[y, 1] = want[y, W - 1] = 2
    return d0, d1, lambda o: np.array_equal(o, want)


def maps_row_without_valid_pixel(H, W):
    rng = np.random.default_rng(5)
    d0 = rng.integers(0, 4, (H, W)).astype(np.float32)
    d1 = rng.integers(0, 4, (H, W)).astype(np.float32)
    y = H // 2
    d0[y] = 3                 # x < 3: occluded; else no match against d1 = 0, and d = 0 matches: mismatches
    d1[y] = 0
    return d0, d1, lambda o: (o[y] != 0).all() and (o[y, 3:] == 2).all()


@pytest.mark.parametrize("terminate", ["mismatch", ""])
@pytest.mark.parametrize("maps", [maps_all_mismatch, maps_no_mismatch, maps_corners, maps_row_without_valid_pixel],
                         ids=["all_mismatch", "no_mismatch", "corners", "row_without_valid_pixel"])
@pytest.mark.parametrize("H,W", [(37, 150), (9, 33), (1, 70)])
def test_ray_walk_on_prescribed_maps(mc, oracle, H, W, maps, terminate):
    D = 8
    d0, d1, classes_ok = maps(H, W)
    vl, vr = planted(d0, D), planted(d1, D)
    prm = fast(sm_skip="sgm", sm_terminate=terminate)
    x0, x1 = random_pair(H, W, seed=3)
    want = oracle.stereo_predict(prm, x0, x1, D, rawL=vl, rawR=vr)
    assert np.array_equal(want["dispL0"], d0) and np.array_equal(want["dispR0"], d1), "the planted minima are not the arg-min"
    assert classes_ok(want["outlier"]), "the maps do not give the outlier classes the case is about"
    got = mc.stereo_predict_fused(dev(np.stack([x0, x1]))[:, None], prm, D, raw=(dev(vl), dev(vr)))
    torch.cuda.synchronize()
    assert_same(host(got["disp"]), want["disp"], "disp %dx%d" % (H, W))


# ---- median 3 x 3 and 5 x 5: every edge and corner, images smaller than the window ----

@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (2, 7), (7, 2), (4, 64), (5, 65), (6, 129)])
def test_median_cut_windows(mc, oracle, H, W, k):
    rng = np.random.default_rng(H * 1000 + W)
    ties = rng.integers(0, 3, (H, W)).astype(np.float32)                    # three values: ties in every window
    huge = np.where(rng.random((H, W)) < 0.5, 3e38, -3e38).astype(np.float32)   # the padding may not count on small data
    mixed = np.where(rng.random((H, W)) < 0.3, huge, ties + rng.integers(0, 2, (H, W)).astype(np.float32) * 0.5).astype(np.float32)
    for name, img in (("ties", ties), ("huge", huge), ("mixed", mixed), ("all +3e38", np.full((H, W), 3e38, np.float32)),
                      ("all -3e38", np.full((H, W), -3e38, np.float32))):
        assert_same(host(mc.adcensus.median2d(dev(img)[None, None], k)), oracle.median2d(img, k), "median%d %s %dx%d" % (k, name, H, W))


# ---- the Gaussian table: cached on the device per sigma ----

def test_gaussian_table_alternating_sigmas_on_one_workspace(mc, oracle):
    from mc_cnn_amd.predict import Workspace
    H, W, D = 12, 70, 8
    x0, x1 = random_pair(H, W, seed=5)
    f = features(8, H, W, seed=6)
    prms = [fast(blur_sigma=s) for s in (7.74, 1.67)]
    want = [oracle.stereo_predict(p, x0, x1, D, featL=f[0], featR=f[1])["disp"] for p in prms]
    assert not same_bits(want[0], want[1])
    ws = Workspace(prms[0], D, H, W, "cuda")   # the larger table's workspace serves both
    xb, fd = dev(np.stack([x0, x1]))[:, None], dev(f)
    for rnd in range(3):
        for p, w in zip(prms, want):
            got = mc.stereo_predict_fused(xb, p, D, feat=fd, workspace=ws)
            torch.cuda.synchronize()
            assert_same(host(got["disp"]), w, "round %d sigma %g" % (rnd, p["blur_sigma"]))


def test_gaussian_table_on_two_streams(mc, oracle):
    from mc_cnn_amd.predict import Workspace
    H, W, D = 12, 70, 8
    x0, x1 = random_pair(H, W, seed=8)
    f = features(8, H, W, seed=9)
    prms = [fast(blur_sigma=s) for s in (2.78, 4.64)]   # sigmas no other test of this file has uploaded
    want = [oracle.stereo_predict(p, x0, x1, D, featL=f[0], featR=f[1])["disp"] for p in prms]
    xb, fd = dev(np.stack([x0, x1]))[:, None], dev(f)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [Workspace(prms[1], D, H, W, "cuda") for _ in prms]   # the larger table's workspace serves both
    got = [[], []]
    for rnd in range(4):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                # both sigmas on both streams: stream i runs prms[i], then prms[1 - i], ...
                j = (i + rnd) % 2
                got[i].append((j, mc.stereo_predict_fused(xb, prms[j], D, feat=fd, workspace=wss[i])["disp"].clone()))
    torch.cuda.synchronize()
    for i in (0, 1):
        for rnd, (j, g) in enumerate(got[i]):
            assert_same(host(g), want[j], "stream %d round %d sigma %g" % (i, rnd, prms[j]["blur_sigma"]))


# ---- fix_border on both (H,W,D) volumes in one launch ----

@pytest.mark.parametrize("border_n", [0, 1, 4])
def test_fix_border_of_both_volumes(mc, oracle, border_n):
    H, W, D = 6, 40, 8
    prm = fast(border_n=border_n)
    x0, x1 = random_pair(H, W, seed=2)
    f = features(8, H, W, seed=3)
    want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    got = mc.stereo_predict_fused(dev(np.stack([x0, x1]))[:, None], prm, D, feat=dev(f), want_volumes=True)
    torch.cuda.synchronize()
    for k in ("volL", "volR", "disp"):
        assert_same(host(got[k]), want[k], "%s border_n=%d" % (k, border_n))
