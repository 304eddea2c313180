"""-m gpu: mc_predict_ex, mc_predict with three more optional outputs per pixel -- `outlier`, what outlier_detection writes for the two
arg-min maps (0 match, 1 occlusion, 2 mismatch), and `cost` / `curvature`, the final left volume at the disparity d the sub-pixel stage
reads and 2 (c(d+1) + c(d-1) - 2 c(d)) there (0 where d < 1 or d >= D - 1).

Every comparison is exact (np.array_equal with equal_nan): each quantity is a copy or one fixed fp32 expression.  The pairs
(tests/predict_ex_cases.py) are 12 x 40 with D = 8 and D = 7 (ds = D and ds = D + 1, rows shorter than a wave, H * W no multiple of 256);
D = 6 is added where the maps are gathered, so that the lower rows' disparity 5 is the range's last one and takes the curvature's edge
branch, like d = 0 does at the left border of the arg-min maps."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import predict_ex_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = cases.H, cases.W
EXTRAS = ("outlier", "cost", "curvature")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, what):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert np.array_equal(got, want, equal_nan=True), "%s: %d of %d differ, first at %d: %r != %r" % (
        what, bad.sum(), bad.size, bad.argmax(), got[bad.argmax()], want[bad.argmax()])


def params(mc, route):
    return dict(mc.PRESETS["kitti_fast"]) if route == "fast" else cases.slow_params(mc.PRESETS) if route == "slow" else dict(mc.PRESETS["mb_slow"])


@functools.lru_cache(maxsize=None)
def inputs(route, D, seed=cases.SEED):
    """(xb, kw) on the device: the pair, and its features (route fast) or its mc_ad volumes (routes slow and mb); made once, never written"""
    from mc_cnn_amd import adcensus
    x0, x1 = cases.pair(seed)
    xb = dev(np.stack([x0, x1]))[:, None].contiguous()
    if route == "fast":
        return xb, dict(feat=dev(cases.features(seed)))
    volL = adcensus.fill_nan(torch.empty((1, D, H, W), dtype=torch.float32, device="cuda"))
    volR = adcensus.fill_nan(torch.empty((1, D, H, W), dtype=torch.float32, device="cuda"))
    adcensus.ad(xb[0:1], xb[1:2], volL, -1)
    adcensus.ad(xb[1:2], xb[0:1], volR, 1)
    torch.cuda.synchronize()
    return xb, dict(raw=(volL, volR))


def require_all_classes(oracle, mc, route, D, seed=cases.SEED):
    """the precondition of every comparison, on the CPU oracle's own class map; for the volume routes also that the oracle's ad volumes,
    which that map was computed from, are the ones the GPU run reads"""
    o = cases.oracle_maps(oracle, mc.PRESETS, route, D, seed)
    assert cases.has_all_classes(o["outlier"]), "the case is meant to hold matches, occlusions and mismatches"
    if route != "fast":
        x0, x1 = cases.pair(seed)
        raw = inputs(route, D, seed)[1]["raw"]
        same(host(raw[0]), oracle.ad(x0, x1, D, -1), "mc_ad, left")
        same(host(raw[1]), oracle.ad(x1, x0, D, 1), "mc_ad, right")
    return o


def fused(mc, route, D, over=None, **want):
    xb, kw = inputs(route, D)
    res = mc.stereo_predict_fused(xb, dict(params(mc, route), **(over or {})), D, **kw, **want)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in res.items()}


def gather(volL, d, D):
    """cost and curvature from the (D,H,W) left volume at the (H,W) disparity map d, in float32 in the kernel's order"""
    vol = volL.reshape(D, H, W)
    di = d.reshape(H, W).astype(np.int64)
    assert (di >= 0).all() and (di < D).all()
    cz = np.take_along_axis(vol, di[None], 0)[0]
    cn = np.take_along_axis(vol, np.clip(di - 1, 0, D - 1)[None], 0)[0]
    cp = np.take_along_axis(vol, np.clip(di + 1, 0, D - 1)[None], 0)[0]
    assert cz.dtype == cn.dtype == cp.dtype == np.float32
    with np.errstate(invalid="ignore"):
        curv = np.float32(2) * ((cp + cn) - np.float32(2) * cz)
    curv[(di < 1) | (di >= D - 1)] = 0
    assert curv.dtype == np.float32
    return cz, curv


@pytest.mark.parametrize("D", cases.DS + (6,))
@pytest.mark.parametrize("route", ["fast", "slow"])
def test_routes(mc, oracle, route, D):
    """the (H,W,ds) route (kitti_fast from features) and the (D,H,W) route (kitti_slow with a CBCA-2 block, from raw volumes)"""
    o = require_all_classes(oracle, mc, route, D)
    res = fused(mc, route, D, want_volumes=True, want_disp0=True, want_outlier=True, want_confidence=True)
    for k in EXTRAS:
        assert res[k].shape == (1, 1, H, W) and res[k].dtype == np.float32
    op = torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")
    mc.adcensus.outlier_detection(dev(res["dispL0"]), dev(res["dispR0"]), op, D)
    same(res["outlier"], host(op), "outlier against the operator")
    same(res["outlier"], oracle.outlier_detection(res["dispL0"].reshape(H, W), res["dispR0"].reshape(H, W), D), "outlier against the oracle's operator")
    same(res["outlier"], o["outlier"], "outlier against the oracle's pipeline")
    d = fused(mc, route, D, over=dict(sm_terminate="mismatch"))["disp"]   # what the sub-pixel stage reads
    cost, curv = gather(res["volL"], d, D)
    di = d.astype(np.int64).reshape(-1)
    assert np.isnan(cost).any(), "the case is meant to hold filled-in pixels whose cost lies in the NaN triangle"
    assert ((di >= 1) & (di < D - 1)).any() and (curv != 0).any()
    if D == 6:
        assert (di == D - 1).sum() > 100, "the lower rows' disparity is meant to be the range's last"
    same(res["cost"], cost, "cost")
    same(res["curvature"], curv, "curvature")


@pytest.mark.parametrize("D", cases.DS)
def test_middlebury(mc, oracle, D):
    """lr_check = 0, left_only = 1: the class map runs the check for itself (and the right volume for it); disp is what it was"""
    require_all_classes(oracle, mc, "mb", D)
    left = dict(left_only=1)
    plain = fused(mc, "mb", D, over=left)
    res = fused(mc, "mb", D, over=left, want_outlier=True)
    maps = fused(mc, "mb", D, over=left, want_disp0=True)
    op = torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")
    mc.adcensus.outlier_detection(dev(maps["dispL0"]), dev(maps["dispR0"]), op, D)
    assert cases.has_all_classes(host(op))
    same(res["outlier"], host(op), "outlier against the operator on the two arg-min maps")
    same(res["disp"], plain["disp"], "disp with the class map against mc_predict's, left_only = 1")
    # and with the confidence maps: the stage reads the arg-min, whose left border holds d = 0
    full = fused(mc, "mb", D, over=left, want_volumes=True, want_disp0=True, want_outlier=True, want_confidence=True)
    assert (full["dispL0"] == 0).any()
    cost, curv = gather(full["volL"], full["dispL0"], D)
    same(full["cost"], cost, "cost at the arg-min")
    same(full["curvature"], curv, "curvature at the arg-min")
    same(full["outlier"], host(op), "outlier, all outputs asked for")
    same(full["disp"], plain["disp"], "disp, all outputs asked for")


def predict_ex(mc, route, D, subset, ex=True):
    """mc_predict_ex (ex = False: mc_predict) through ctypes with every optional output of mc_predict and the given subset of the extras"""
    from mc_cnn_amd.predict import Workspace
    lib = mc._lib.lib
    xb, kw = inputs(route, D)
    p = mc.make_params(params(mc, route))
    ws = Workspace(p, D, H, W, xb.device)
    out = {k: torch.full((1, D if k.startswith("vol") else 1, H, W), -7.0, dtype=torch.float32, device="cuda")
           for k in ("volL", "volR", "dispL0", "dispR0", "disp") + tuple(subset)}
    fl, fr = (kw["feat"][0].data_ptr(), kw["feat"][1].data_ptr()) if "feat" in kw else (None, None)
    rl, rr = (kw["raw"][0].data_ptr(), kw["raw"][1].data_ptr()) if "raw" in kw else (None, None)
    head = (C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), fl, fr, cases.C if fl else 0, rl, rr, D, H, W, ws.ptr, ws.nbytes_full,
            out["volL"].data_ptr(), out["volR"].data_ptr(), out["dispL0"].data_ptr(), out["dispR0"].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    if ex:
        rc = lib.mc_predict_ex(*head, *(out[k].data_ptr() if k in out else None for k in EXTRAS), out["disp"].data_ptr(), st)
    else:
        rc = lib.mc_predict(*head, out["disp"].data_ptr(), st)
    mc._lib.check(rc, "mc_predict_ex")
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("route,D", [("fast", 8), ("fast", 7), ("slow", 7), ("mb", 8)])
def test_no_subset_of_the_extras_perturbs_the_other_outputs(mc, oracle, route, D):
    require_all_classes(oracle, mc, route, D)
    want = predict_ex(mc, route, D, (), ex=False)
    every = predict_ex(mc, route, D, EXTRAS)
    for n in range(len(EXTRAS) + 1):
        for subset in itertools.combinations(EXTRAS, n):
            got = predict_ex(mc, route, D, subset)
            for k in ("disp", "volL", "volR", "dispL0", "dispR0"):
                same(got[k], want[k], "%s with %s" % (k, subset or "no extras"))
            for k in subset:
                assert not (got[k] == -7.0).all()
                same(got[k], every[k], "%s alone in %s against all three" % (k, subset))


@pytest.mark.parametrize("route,D", [("fast", 7), ("slow", 8)])
def test_skipped_and_terminated_stages(mc, oracle, route, D):
    require_all_classes(oracle, mc, route, D)
    every = dict(want_outlier=True, want_confidence=True)
    full = fused(mc, route, D, want_volumes=True, want_disp0=True, **every)
    # without the two interpolations the sub-pixel stage reads the arg-min, d = 0 at the left border included
    skip = fused(mc, route, D, over=dict(sm_skip="occlusion"), want_volumes=True, want_disp0=True, **every)
    assert (skip["dispL0"] == 0).any()
    cost, curv = gather(skip["volL"], skip["dispL0"], D)
    same(skip["cost"], cost, "cost at the arg-min")
    same(skip["curvature"], curv, "curvature at the arg-min")
    same(skip["outlier"], full["outlier"], "outlier with the interpolations skipped")
    assert not np.array_equal(skip["cost"], full["cost"], equal_nan=True), "the interpolations are meant to move some disparities"
    # a method that ends behind the sub-pixel stage: the maps are what they were
    med = fused(mc, route, D, over=dict(sm_terminate="median"), **every)
    for k in EXTRAS:
        same(med[k], full[k], "%s with sm_terminate = median" % k)
    same(med["disp"], fused(mc, route, D, over=dict(sm_terminate="median"))["disp"], "disp with sm_terminate = median")
    # a method that ends at the SGM: the classes are still written, the confidence maps refused
    sgm = fused(mc, route, D, over=dict(sm_terminate="sgm"), want_disp0=True, want_outlier=True)
    op = torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")
    mc.adcensus.outlier_detection(dev(sgm["dispL0"]), dev(sgm["dispR0"]), op, D)
    same(sgm["outlier"], host(op), "outlier with sm_terminate = sgm")
    assert cases.has_all_classes(sgm["outlier"])
    same(sgm["disp"], fused(mc, route, D, over=dict(sm_terminate="sgm"))["disp"], "disp with sm_terminate = sgm")
    with pytest.raises(mc._lib.McError, match="cost_out is written by the sub-pixel stage"):
        fused(mc, route, D, over=dict(sm_terminate="sgm"), **every)


def test_two_streams(mc, oracle):
    """two calls with the extras on two streams, a workspace each: each gives what it gives alone"""
    from mc_cnn_amd.predict import Workspace
    jobs = [("fast", 8), ("slow", 7)]
    alone = []
    for route, D in jobs:
        require_all_classes(oracle, mc, route, D)
        alone.append(fused(mc, route, D, want_outlier=True, want_confidence=True))
    slots = []
    for route, D in jobs:
        xb, kw = inputs(route, D)
        slots.append(dict(route=route, D=D, xb=xb, kw=kw, ws=Workspace(params(mc, route), D, H, W, xb.device), stream=torch.cuda.Stream()))
    torch.cuda.synchronize()
    for rnd in range(3):   # queued back to back, nothing waits in between
        for sl in slots:
            with torch.cuda.stream(sl["stream"]):
                sl["res"] = mc.stereo_predict_fused(sl["xb"], params(mc, sl["route"]), sl["D"], workspace=sl["ws"], want_outlier=True,
                                                    want_confidence=True, **sl["kw"])
    torch.cuda.synchronize()
    for sl, want in zip(slots, alone):
        for k in ("disp",) + EXTRAS:
            same(host(sl["res"][k]), want[k], "%s of the %s call on its own stream" % (k, sl["route"]))


@pytest.mark.parametrize("D", cases.DS)
@pytest.mark.parametrize("route", ["fast", "slow", "mb"])
def test_fused_against_op_by_op(mc, oracle, route, D):
    require_all_classes(oracle, mc, route, D)
    xb, kw = inputs(route, D)
    ops = mc.stereo_predict(xb, params(mc, route), D, return_all=True, **kw)
    torch.cuda.synchronize()
    res = fused(mc, route, D, want_outlier=True, want_confidence=True)
    for k in EXTRAS:
        assert tuple(ops[k].shape) == (1, 1, H, W)
        same(res[k], host(ops[k]), "%s, fused against op by op" % k)
    same(res["disp"], host(ops["disp"]), "disp, fused against op by op")
    assert cases.has_all_classes(res["outlier"]) and np.isnan(res["cost"]).any() == (route != "mb")


def test_main_extras(mc, tmp_path, monkeypatch, capsys):
    """`main.py kitti fast -a predict -extras`: the three files next to disp.bin, (1,1,H,W) float32, announced like the others"""
    from PIL import Image
    from mc_cnn_amd import main as mcmain
    D = 8
    x0, x1 = cases.pair()
    for name, x in (("L.png", x0), ("R.png", x1)):
        Image.fromarray(np.clip(128 + 48 * x, 0, 255).astype(np.uint8)).save(tmp_path / name)
    monkeypatch.chdir(tmp_path)
    argv = ["kitti", "fast", "-a", "predict", "-net_fname", "random:3", "-left", "L.png", "-right", "R.png", "-disp_max", str(D)]
    assert mcmain.main(argv) == 0
    assert capsys.readouterr().out.splitlines() == ["Writing right.bin, 1 x %d x %d x %d" % (D, H, W), "Writing left.bin, 1 x %d x %d x %d" % (D, H, W),
                                                    "Writing disp.bin, 1 x 1 x %d x %d" % (H, W)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["L.png", "R.png", "disp.bin", "left.bin", "right.bin"]
    plain = {k: (tmp_path / k).read_bytes() for k in ("disp.bin", "left.bin", "right.bin")}
    assert mcmain.main(argv + ["-extras"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3:] == ["Writing %s.bin, 1 x 1 x %d x %d" % (k, H, W) for k in EXTRAS] and len(lines) == 6
    for k, blob in plain.items():
        assert (tmp_path / k).read_bytes() == blob, "%s changes with -extras" % k
    got = {}
    for k in EXTRAS:
        assert (tmp_path / ("%s.bin" % k)).stat().st_size == 4 * H * W
        got[k] = mc.read_bin("%s.bin" % k, (1, 1, H, W))
    # the same host path by hand
    xb = dev(np.stack([mcmain.normalize(mcmain.load_image("L.png")), mcmain.normalize(mcmain.load_image("R.png"))]))
    layers = mcmain.load_net("random:3", "kitti", "fast")
    prm = dict(mc.TABLES[("kitti", "fast")], border_n=len(layers))
    want = mc.stereo_predict_fused(xb, prm, D, feat=mcmain.features_fast(xb, layers), want_outlier=True, want_confidence=True)
    torch.cuda.synchronize()
    for k in EXTRAS:
        same(got[k], host(want[k]), "%s.bin" % k)
    assert set(np.unique(got["outlier"])) <= {0.0, 1.0, 2.0}
