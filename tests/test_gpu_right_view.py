"""-m gpu: mc_predict_views, mc_predict_ex with the RIGHT view's finished disparity map (`disp_right`) and class map (`outlier_right`).

What the two maps are is stated in tests/right_view_cases.py (oracle_right): the existing post-processing on the x-mirrored arg-min maps
and right volume, mirrored back.  Every comparison is exact (util.same_bits): each stage is the left view's operator, which the suite
already holds to the oracle bit for bit, and the mirror is a copy.  The cases are 12 x 40 with D = 8 and D = 7 on the three routes
(ds = D and ds = D + 1, rows shorter than a wave, H * W no multiple of 256) and one 12 x 37 pair (no row a multiple of 4 pixels).  Every
test first asserts, on the oracle's own right-view class map, that the case holds matches, occlusions and mismatches."""
import ctypes as C
import functools

import numpy as np
import pytest

import right_view_cases as rv
from util import diff_report, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H = rv.H
LEFT = ("disp", "volL", "volR", "dispL0", "dispR0", "outlier", "cost", "curvature")
RIGHT = ("disp_right", "outlier_right")
EVERYTHING = dict(want_volumes=True, want_disp0=True, want_outlier=True, want_confidence=True)
IDS = ["%s-D%d-W%d" % c for c in rv.CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, what):
    assert same_bits(got, want), diff_report(got, want, what)


@functools.lru_cache(maxsize=None)
def inputs(route, D, width):
    """(xb, kw) on the device: the pair, and its features (route fast) or its mc_ad volumes (routes slow and mb); made once, never written"""
    from mc_cnn_amd import adcensus
    x0, x1 = rv.pair_w(rv.SEED, width)
    xb = dev(np.stack([x0, x1]))[:, None].contiguous()
    if route == "fast":
        return xb, dict(feat=dev(rv.features_w(rv.SEED, width)))
    volL = adcensus.fill_nan(torch.empty((1, D, H, width), dtype=torch.float32, device="cuda"))
    volR = adcensus.fill_nan(torch.empty((1, D, H, width), dtype=torch.float32, device="cuda"))
    adcensus.ad(xb[0:1], xb[1:2], volL, -1)
    adcensus.ad(xb[1:2], xb[0:1], volR, 1)
    torch.cuda.synchronize()
    return xb, dict(raw=(volL, volR))


_wanted = {}


def wanted(oracle, mc, route, D, width, over=None):
    """the oracle's dict for a case and its two right-view maps, computed once per (case, overrides) and never written; for the volume
    routes also the check that the oracle's ad volumes are the ones the GPU run reads"""
    key = (route, D, width, tuple(sorted((over or {}).items())))
    if key not in _wanted:
        o, prm = rv.oracle_maps(oracle, mc.PRESETS, route, D, width, over=over)
        o["disp_right"], o["outlier_right"] = rv.oracle_right(oracle, o, prm, D)
        if route != "fast" and not over:
            x0, x1 = rv.pair_w(rv.SEED, width)
            raw = inputs(route, D, width)[1]["raw"]
            same(host(raw[0]), oracle.ad(x0, x1, D, -1), "mc_ad, left")
            same(host(raw[1]), oracle.ad(x1, x0, D, 1), "mc_ad, right")
        _wanted[key] = o
    return _wanted[key]


def require_all_classes(oracle, mc, route, D, width):
    """the precondition of every comparison, on the CPU oracle's own right-view class map"""
    o = wanted(oracle, mc, route, D, width)
    assert rv.has_all_classes(o["outlier_right"]), "the case is meant to hold matches, occlusions and mismatches in the right view"
    return o


def fused(mc, route, D, width, over=None, **want):
    xb, kw = inputs(route, D, width)
    res = mc.stereo_predict_fused(xb, rv.params(mc.PRESETS, route, over), D, **kw, **want)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in res.items()}


@pytest.mark.parametrize("route,D,width", rv.CASES, ids=IDS)
def test_both_maps_equal_the_oracles(mc, oracle, route, D, width):
    o = require_all_classes(oracle, mc, route, D, width)
    res = fused(mc, route, D, width, want_right=True, **EVERYTHING)
    for k in RIGHT:
        assert res[k].shape == (1, 1, H, width) and res[k].dtype == np.float32
        same(res[k], o[k], "%s against the oracle's composition" % k)
    assert rv.has_all_classes(res["outlier_right"])
    # the maps it was composed from are the ones this call exports
    for k in ("volR", "dispL0", "dispR0", "disp"):
        same(res[k], o[k], k)
    # asked for alone: the same maps
    alone = fused(mc, route, D, width, want_right=True)
    assert sorted(alone) == ["disp", "disp_right", "outlier_right"]
    for k in RIGHT + ("disp",):
        same(alone[k], res[k], "%s, asked for alone" % k)


@pytest.mark.parametrize("route,D,width", rv.CASES, ids=IDS)
def test_fused_against_op_by_op(mc, oracle, route, D, width):
    require_all_classes(oracle, mc, route, D, width)
    xb, kw = inputs(route, D, width)
    ops = mc.stereo_predict(xb, rv.params(mc.PRESETS, route), D, return_all=True, **kw)
    torch.cuda.synchronize()
    res = fused(mc, route, D, width, want_right=True)
    for k in RIGHT:
        assert tuple(ops[k].shape) == (1, 1, H, width)
        same(res[k], host(ops[k]), "%s, fused against op by op" % k)


@pytest.mark.parametrize("route,D,width", rv.CASES, ids=IDS)
def test_left_side_outputs_do_not_change(mc, oracle, route, D, width):
    require_all_classes(oracle, mc, route, D, width)
    without = fused(mc, route, D, width, **EVERYTHING)
    with_right = fused(mc, route, D, width, want_right=True, **EVERYTHING)
    assert sorted(with_right) == sorted(LEFT + RIGHT) and sorted(without) == sorted(LEFT)
    for k in LEFT:
        same(with_right[k], without[k], "%s with the right view's maps against without" % k)


def views(mc, route, D, width, entry, right=(), over=None, lanes=0):
    """mc_predict_views / mc_predict_ex through ctypes with every optional output of mc_predict_ex and the given subset of RIGHT"""
    from mc_cnn_amd.predict import Workspace
    lib = mc._lib.lib
    xb, kw = inputs(route, D, width)
    p = mc.make_params(rv.params(mc.PRESETS, route, over))
    ws = Workspace(p, D, H, width, xb.device)
    out = {k: torch.full((1, D if k.startswith("vol") else 1, H, width), -7.0, dtype=torch.float32, device="cuda") for k in LEFT + tuple(right)}
    fl, fr = (kw["feat"][0].data_ptr(), kw["feat"][1].data_ptr()) if "feat" in kw else (None, None)
    rl, rr = (kw["raw"][0].data_ptr(), kw["raw"][1].data_ptr()) if "raw" in kw else (None, None)
    head = (C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), fl, fr, rv.C if fl else 0, rl, rr, D, H, width, ws.ptr, ws.nbytes_full,
            out["volL"].data_ptr(), out["volR"].data_ptr(), out["dispL0"].data_ptr(), out["dispR0"].data_ptr(),
            out["outlier"].data_ptr(), out["cost"].data_ptr(), out["curvature"].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    hook = C.CDLL(mc._lib.LIB_PATH).mc_test_predict_lanes
    hook(lanes)
    try:
        if entry == "views":
            rc = lib.mc_predict_views(*head, *(out[k].data_ptr() if k in out else None for k in RIGHT), out["disp"].data_ptr(), st)
        else:
            rc = lib.mc_predict_ex(*head, out["disp"].data_ptr(), st)
        mc._lib.check(rc, "mc_predict_%s" % entry)
        torch.cuda.synchronize()
    finally:
        hook(0)
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("route,D,width", [("fast", 8, rv.W), ("fast", 8, rv.W_ODD), ("slow", 7, rv.W), ("mb", 8, rv.W)])
def test_with_both_pointers_null_it_is_mc_predict_ex(mc, oracle, route, D, width):
    o = require_all_classes(oracle, mc, route, D, width)
    ex = views(mc, route, D, width, "ex")
    null = views(mc, route, D, width, "views")
    for k in LEFT:
        assert not (ex[k] == -7.0).all()
        same(null[k], ex[k], "%s, mc_predict_views with both maps NULL against mc_predict_ex" % k)
    # either map alone, and on either schedule of the fast path: the same bits
    for right in (("disp_right",), ("outlier_right",), RIGHT):
        for lanes in ((1, 2) if route == "fast" else (0,)):
            got = views(mc, route, D, width, "views", right, lanes=lanes)
            for k in LEFT:
                same(got[k], ex[k], "%s with %s, lanes %d" % (k, right, lanes))
            for k in right:
                same(got[k], o[k], "%s asked for as %s, lanes %d" % (k, right, lanes))


DROPS = [dict(sm_skip=s) for s in ("cbca", "sgm", "occlusion", "subpixel_enchancement", "median", "bilateral")] + \
        [dict(sm_terminate=t) for t in ("occlusion", "mismatch", "subpixel_enchancement", "median")]


@pytest.mark.parametrize("over", DROPS, ids=lambda d: "%s=%s" % tuple(d.items())[0])
@pytest.mark.parametrize("route,D", [("slow", 7)])
def test_skipped_and_terminated_stages(mc, oracle, route, D, over):
    """the (D,H,W) route with both aggregation blocks, so that every -sm_skip value drops something: the right map follows the same drops"""
    require_all_classes(oracle, mc, route, D, rv.W)
    o = wanted(oracle, mc, route, D, rv.W, over)
    res = fused(mc, route, D, rv.W, over=over, want_right=True, want_disp0=True)
    for k in ("dispL0", "dispR0", "disp") + RIGHT:
        same(res[k], o[k], "%s with %s" % (k, over))


@pytest.mark.parametrize("over", [dict(sm_skip="occlusion"), dict(sm_skip="subpixel_enchancement"), dict(sm_terminate="mismatch"),
                                  dict(sm_terminate="median")], ids=lambda d: "%s=%s" % tuple(d.items())[0])
def test_stage_drops_on_the_fast_route(mc, oracle, over):
    """... and on the (H,W,ds) route, where the sub-pixel stage reads the padded volume at the mirrored pixel (D = 7: ds = 8)"""
    require_all_classes(oracle, mc, "fast", 7, rv.W)
    o = wanted(oracle, mc, "fast", 7, rv.W, over)
    res = fused(mc, "fast", 7, rv.W, over=over, want_right=True)
    for k in ("disp",) + RIGHT:
        same(res[k], o[k], "%s with %s" % (k, over))
    full = wanted(oracle, mc, "fast", 7, rv.W)
    assert not same_bits(o["disp_right"], full["disp_right"]), "the dropped stage is meant to change the map"


@pytest.mark.parametrize("D", rv.DS)
def test_left_only_is_ignored_where_a_right_view_map_is_asked_for(mc, oracle, D):
    """lr_check = 0, left_only = 1 (Middlebury outside -a predict): both volumes are computed, no interpolation runs"""
    o = require_all_classes(oracle, mc, "mb", D, rv.W)
    plain = fused(mc, "mb", D, rv.W, over=dict(left_only=1))
    from mc_cnn_amd.predict import Workspace
    xb, kw = inputs("mb", D, rv.W)
    p = mc.make_params(rv.params(mc.PRESETS, "mb", dict(left_only=1)))
    ws = Workspace(p, D, H, rv.W, xb.device)
    disp = torch.full((1, 1, H, rv.W), -7.0, dtype=torch.float32, device="cuda")
    dispR = torch.full_like(disp, -7.0)
    rc = mc._lib.lib.mc_predict_views(C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), None, None, 0, kw["raw"][0].data_ptr(), kw["raw"][1].data_ptr(),
                                      D, H, rv.W, ws.ptr, ws.nbytes_full, None, None, None, None, None, None, None, dispR.data_ptr(), None,
                                      disp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    mc._lib.check(rc, "mc_predict_views")
    torch.cuda.synchronize()
    same(host(dispR), o["disp_right"], "disp_right with left_only = 1")
    same(host(disp), plain["disp"], "disp with left_only = 1")
    same(host(disp), o["disp"], "disp against the oracle")


def test_main_right_view(mc, tmp_path, monkeypatch, capsys):
    """`main.py kitti fast -a predict -right_view`: disp_right.bin next to disp.bin, (1,1,H,W) float32; with -extras also outlier_right.bin"""
    from PIL import Image
    from mc_cnn_amd import main as mcmain
    D, W = 8, rv.W
    x0, x1 = rv.pair_w(rv.SEED, W)
    for name, x in (("L.png", x0), ("R.png", x1)):
        Image.fromarray(np.clip(128 + 48 * x, 0, 255).astype(np.uint8)).save(tmp_path / name)
    monkeypatch.chdir(tmp_path)
    argv = ["kitti", "fast", "-a", "predict", "-net_fname", "random:1", "-left", "L.png", "-right", "R.png", "-disp_max", str(D)]
    assert mcmain.main(argv) == 0
    capsys.readouterr()
    plain = {k: (tmp_path / k).read_bytes() for k in ("disp.bin", "left.bin", "right.bin")}
    assert mcmain.main(argv + ["-right_view"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3:] == ["Writing disp_right.bin, 1 x 1 x %d x %d" % (H, W)] and len(lines) == 4
    assert sorted(p.name for p in tmp_path.iterdir()) == ["L.png", "R.png", "disp.bin", "disp_right.bin", "left.bin", "right.bin"]
    for k, blob in plain.items():
        assert (tmp_path / k).read_bytes() == blob, "%s changes with -right_view" % k
    assert (tmp_path / "disp_right.bin").stat().st_size == 4 * H * W
    got = mc.read_bin("disp_right.bin", (1, 1, H, W))
    # the same host path by hand
    xb = dev(np.stack([mcmain.normalize(mcmain.load_image("L.png")), mcmain.normalize(mcmain.load_image("R.png"))]))
    layers = mcmain.load_net("random:1", "kitti", "fast")
    prm = dict(mc.TABLES[("kitti", "fast")], border_n=len(layers))
    want = mc.stereo_predict_fused(xb, prm, D, feat=mcmain.features_fast(xb, layers), want_right=True, want_outlier=True)
    torch.cuda.synchronize()
    same(got, host(want["disp_right"]), "disp_right.bin")
    assert not same_bits(got, host(want["disp"])), "the two views' maps are meant to differ"
    assert mcmain.main(argv + ["-right_view", "-extras"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[-2:] == ["Writing %s.bin, 1 x 1 x %d x %d" % (k, H, W) for k in RIGHT] and len(lines) == 8
    same(mc.read_bin("outlier_right.bin", (1, 1, H, W)), host(want["outlier_right"]), "outlier_right.bin")
    same(mc.read_bin("disp_right.bin", (1, 1, H, W)), got, "disp_right.bin with -extras")
